"""PLY files, numpy only: the reconstruction script's three ASCII writers (one header / columns scheme) and a reader of ASCII and binary
little-endian meshes."""
import numpy as np

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
_XYZ = ("float", "%f", ("x", "y", "z"))                 # (ply type, % format, property names) of the writers' three vertex blocks
_NORMAL = ("float", "%f", ("nx", "ny", "nz"))
_RGB = ("uchar", "%d", ("red", "green", "blue"))


def _columns(formats, columns):
    """Rows of space-separated, %-formatted columns, each ending in a newline: one string, built without a Python loop
    over the rows (np.char formats each column element with the same % operator a per-row write uses)."""
    if len(columns[0]) == 0:
        return ""
    line = np.char.mod(formats[0], columns[0])
    for fmt, col in zip(formats[1:], columns[1:]):
        line = np.char.add(np.char.add(line, " "), np.char.mod(fmt, col))
    return "\n".join(line.tolist()) + "\n"


def _write(filename, vertex, faces=None):
    """The one writer: ``vertex`` is a list of ``((ply type, % format, three property names), array [N,3])`` blocks, written as the
    columns of the vertex element in that order; ``faces`` [F,3], when given, follows as the face element."""
    header = "ply\nformat ascii 1.0\nelement vertex %d\n" % len(vertex[0][1])
    header += "".join(f"property {kind} {name}\n" for (kind, _, names), _ in vertex for name in names)
    if faces is not None:
        header += "element face %d\nproperty list uchar int vertex_index\n" % len(faces)
    body = _columns([fmt for (_, fmt, _), _ in vertex for _ in range(3)], [block[:, i] for _, block in vertex for i in range(3)])
    if faces is not None:
        body += _columns(["3 %d", "%d", "%d"], [faces[:, 0], faces[:, 1], faces[:, 2]])
    with open(filename, "w") as f:
        f.write(header + "end_header\n" + body)


def meshwrite(filename, verts, faces, norms, colors):
    """ASCII .ply of a coloured mesh with normals, byte for byte the reconstruction script's format (:379-415)."""
    verts, faces, norms, colors = (np.asarray(a) for a in (verts, faces, norms, colors))
    _write(filename, [(_XYZ, verts), (_NORMAL, norms), (_RGB, colors)], faces)


def pcwrite(filename, xyzrgb):
    """ASCII .ply of a coloured point cloud [N,6] (xyz, rgb), byte for byte the reconstruction script's format (:417-439)."""
    xyzrgb = np.asarray(xyzrgb)
    _write(filename, [(_XYZ, xyzrgb[:, :3]), (_RGB, xyzrgb[:, 3:].astype(np.uint8))])


def pcwrite_normals(filename, xyzrgb, normals):
    """ASCII .ply of a coloured point cloud [N,6] (xyz, rgb) with a normal [N,3] for every point: ``pcwrite``'s format with ``property float
    nx/ny/nz`` between z and red, the vertex layout of ``meshwrite`` (what MeshLab, Open3D and ``meshread`` read)."""
    xyzrgb, normals = np.asarray(xyzrgb), np.asarray(normals)
    if normals.shape != (len(xyzrgb), 3):
        raise ValueError(f"pcwrite_normals: normals {normals.shape} do not belong to {len(xyzrgb)} points")
    _write(filename, [(_XYZ, xyzrgb[:, :3]), (_NORMAL, normals), (_RGB, xyzrgb[:, 3:].astype(np.uint8))])


def _header(filename, data):
    """``(format, elements, offset of the body)`` of a PLY file's bytes; elements: [name, count, [(kind, name, type or (count type, item
    type)), ...]] with numpy type codes."""
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"meshread: {filename} is not a PLY file")
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        words = line.split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "format":
            fmt = words[1]
        elif words[0] == "element":
            elements.append([words[1], int(words[2]), []])
        elif words[0] == "property" and elements:
            if words[1] == "list":
                elements[-1][2].append(("list", words[4], (_PLY_TYPES.get(words[2]), _PLY_TYPES.get(words[3]))))
            else:
                elements[-1][2].append(("scalar", words[2], _PLY_TYPES.get(words[1])))
    if fmt == "binary_big_endian":
        raise ValueError(f"meshread: {filename} is a binary_big_endian PLY file; only ascii and binary_little_endian are read")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"meshread: {filename} has the unknown format {fmt!r}")
    for name, _, properties in elements:
        for kind, prop, t in properties:
            if (t if kind == "scalar" else t[0] and t[1]) is None:
                raise ValueError(f"meshread: property {prop} of element {name} has an unknown type")
    return fmt, elements, data.find(b"\n", end) + 1


def _ascii_element(tokens, pos, count, properties):
    """One element of an ASCII body from token ``pos`` on: ``(scalar columns, lists, next token)``.  A table of scalars, and a table of
    polygons that all have the corners of the first (the usual case), are read without a loop over the rows."""
    width = len(properties)
    if all(kind == "scalar" for kind, _, _ in properties):
        rows = np.array(tokens[pos:pos + count * width], dtype=np.float64).reshape(count, width)
        return {prop: rows[:, i] for i, (_, prop, _) in enumerate(properties)}, {}, pos + count * width
    if count and width == 1:
        n = int(tokens[pos])
        if len(tokens) >= pos + count * (n + 1):
            table = np.array(tokens[pos:pos + count * (n + 1)], dtype=np.float64).reshape(count, n + 1)
            if np.all(table[:, 0] == n):
                return {}, {properties[0][1]: table[:, 1:].astype(np.int64)}, pos + count * (n + 1)
    lists = {prop: [] for kind, prop, _ in properties if kind == "list"}
    for _ in range(count):
        for kind, prop, _ in properties:
            if kind == "list":
                n = int(tokens[pos])
                lists[prop].append(np.array(tokens[pos + 1:pos + 1 + n], dtype=np.int64))
                pos += 1 + n
            else:
                pos += 1
    return {}, lists, pos


def _binary_element(data, pos, count, properties):
    """One element of a binary little-endian body from byte ``pos`` on: ``(scalar columns, lists, next byte)``, with the fast paths of
    ``_ascii_element``."""
    if all(kind == "scalar" for kind, _, _ in properties):
        dtype = np.dtype([(prop, "<" + t) for _, prop, t in properties])
        table = np.frombuffer(data, dtype=dtype, count=count, offset=pos)
        return {prop: table[prop] for _, prop, _ in properties}, {}, pos + count * dtype.itemsize
    if count and len(properties) == 1:
        ct, it = (np.dtype("<" + t) for t in properties[0][2])
        n = int(np.frombuffer(data, dtype=ct, count=1, offset=pos)[0])
        dtype = np.dtype([("n", ct), ("v", it, (n,))])
        if pos + count * dtype.itemsize <= len(data):
            table = np.frombuffer(data, dtype=dtype, count=count, offset=pos)
            if np.all(table["n"] == n):
                return {}, {properties[0][1]: table["v"].astype(np.int64).reshape(count, n)}, pos + count * dtype.itemsize
    lists = {prop: [] for kind, prop, _ in properties if kind == "list"}
    for _ in range(count):
        for kind, prop, t in properties:
            if kind == "list":
                ct, it = (np.dtype("<" + x) for x in t)
                n = int(np.frombuffer(data, dtype=ct, count=1, offset=pos)[0])
                pos += ct.itemsize
                lists[prop].append(np.frombuffer(data, dtype=it, count=n, offset=pos).astype(np.int64))
                pos += n * it.itemsize
            else:
                pos += np.dtype(t).itemsize
    return {}, lists, pos


def meshread(filename):
    """``(verts float32 [V,3], faces int32 [F,3])`` of a .ply mesh, numpy only: ``format ascii 1.0`` or ``binary_little_endian 1.0``;
    the vertex element needs the scalar properties x, y, z, in any order and of any scalar type, and its other properties are
    skipped; the face element is ``property list uchar|int int|uint vertex_index|vertex_indices`` (other face properties are
    skipped), a polygon of n corners becoming the fan (0, i, i + 1) of n - 2 triangles; other elements are skipped.  Reads what
    ``meshwrite`` writes.  Raises ``ValueError`` for a ``binary_big_endian`` file and for anything else it cannot read."""
    with open(filename, "rb") as f:
        data = f.read()
    fmt, elements, body = _header(filename, data)
    verts, faces = None, np.zeros((0, 3), dtype=np.int32)
    tokens, pos = (data[body:].split(), 0) if fmt == "ascii" else (None, body)
    for name, count, properties in elements:
        if fmt == "ascii":
            columns, lists, pos = _ascii_element(tokens, pos, count, properties)
        else:
            columns, lists, pos = _binary_element(data, pos, count, properties)
        if name == "vertex":
            if not all(axis in columns for axis in "xyz"):
                raise ValueError(f"meshread: the vertex element of {filename} lacks x, y or z")
            verts = np.stack([np.asarray(columns[axis], dtype=np.float32) for axis in "xyz"], axis=1).reshape(-1, 3)
        elif name == "face":
            polygons = lists.get("vertex_index", lists.get("vertex_indices"))
            if polygons is None:
                raise ValueError(f"meshread: the face element of {filename} has no vertex_index list")
            if isinstance(polygons, np.ndarray):
                n = polygons.shape[1]
                fans = [polygons[:, [0, i, i + 1]] for i in range(1, n - 1)]
                triangles = np.stack(fans, axis=1).reshape(-1, 3) if fans else np.zeros((0, 3), np.int64)
            else:
                triangles = [(p[0], p[i], p[i + 1]) for p in polygons for i in range(1, len(p) - 1)]
            faces = np.asarray(triangles, dtype=np.int64).reshape(-1, 3).astype(np.int32)
    if verts is None:
        raise ValueError(f"meshread: {filename} has no vertex element")
    return verts, faces
