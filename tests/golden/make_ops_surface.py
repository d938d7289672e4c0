"""Records the public surface of ``dvmvs.hip.ops`` into ops_surface.json (next to this file): every public name, the signature of every
callable the package defines, the public constants, ``__all__``, which names carry a docstring, and the schema of every registered
``torch.ops.dvmvs`` op.  tests/test_ops_surface.py holds the package to it; re-record only when the surface changes on purpose.

    python tests/golden/make_ops_surface.py [output.json]
"""
import inspect
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.normpath(os.path.join(HERE, "..", "..", "deep-video-mvs_amd")))

CONSTANTS = ("ACTIVATIONS", "RESIDUAL_NONE", "RESIDUAL_SAME", "RESIDUAL_NEAREST_UP2", "ACTIVATION_SIGMOID_TO_DEPTH", "EUNSUPPORTED",
             "TSDF_FUSE_TILE", "CONSISTENCY_MAX_SOURCES")


def surface():
    import torch
    from torch._library.custom_ops import CustomOpDef
    from dvmvs.hip import ops
    # (the modules of the package itself are how it is organised, not what it offers)
    names = sorted(n for n in dir(ops) if not n.startswith("_")
                   and not (isinstance(getattr(ops, n), types.ModuleType) and getattr(ops, n).__name__.startswith(ops.__name__ + ".")))
    signatures, documented = {}, []
    for n in names:
        v = getattr(ops, n)
        fn = v._init_fn if isinstance(v, CustomOpDef) else v
        if inspect.isfunction(fn) and fn.__module__.startswith(ops.__name__):
            signatures[n] = str(inspect.signature(fn))
            if fn.__doc__:
                documented.append(n)
    schemas = {name: str(getattr(torch.ops.dvmvs, name.split("::")[1]).default._schema)
               for name in sorted(torch._C._dispatch_get_all_op_names()) if name.startswith("dvmvs::") and "." not in name}
    return {"names": names, "signatures": signatures, "documented": documented, "all": list(ops.__all__),
            "constants": {n: getattr(ops, n) for n in CONSTANTS}, "schemas": schemas}


def normalised(record):
    """As it reads back from JSON (tuples are lists there)."""
    return json.loads(json.dumps(record))


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ops_surface.json")
    with open(path, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(path)
