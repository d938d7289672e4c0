"""The plumbing every op shares: the no-CPU error, the tensor check, pointers, the launch and the custom-op registration."""
import torch

from dvmvs.hip import _capi

EUNSUPPORTED = -2     # include/dvmvs_hip.h


def no_cpu(op):
    raise RuntimeError(f"dvmvs::{op} only runs as a HIP kernel on an MI355X; move the tensors to the GPU. "
                       f"There is deliberately no CPU fallback (the CPU oracle under oracle/ is for tests).")


def _dtype_names(dtype):
    return " or ".join(str(d).replace("torch.", "") for d in (dtype if type(dtype) is tuple else (dtype,)))


def _shape_text(shape):
    return "" if shape is None else " [" + ",".join("*" if d is None else str(d) for d in shape) + "]"


def _shape_fits(got, want):
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if w is not None and g != w:
            return False
    return True


def check_tensors(name, *tensors, dtype=torch.float32, label=None, shape=None, device=None, contiguous=False, on_gpu=True):
    """The one device / dtype / layout check of the ops.  Every tensor must be on the GPU (else the no-CPU RuntimeError) and of ``dtype``
    (one dtype or a tuple of them).  Without ``label`` that is all, and a wrong dtype is a TypeError.

    With ``label`` (the argument's name, for the message) a tensor must also have ``shape`` (None entries are free; None: any shape), be
    on ``device`` (None: any GPU) and, with ``contiguous``, be dense.  Something that is no tensor is a TypeError; anything else that is
    wrong, the dtype included, is one ValueError that says what was expected and what came.  Dtype and shape are judged before the
    device; ``on_gpu=False`` leaves out the GPU requirement, for ops that report every malformed argument before a misplaced one and
    check the devices in a second call."""
    for t in tensors:
        if label is None:
            if on_gpu and t.device.type != "cuda":
                no_cpu(name)
            if t.dtype != dtype and (type(dtype) is not tuple or t.dtype not in dtype):
                raise TypeError(f"dvmvs::{name}: expected {_dtype_names(dtype)} tensors, got {t.dtype}")
            continue
        if not torch.is_tensor(t):
            raise TypeError(f"dvmvs::{name}: {label} must be a tensor, got {type(t).__name__}")
        if (t.dtype == dtype or (type(dtype) is tuple and t.dtype in dtype)) and (shape is None or _shape_fits(t.shape, shape)):
            if on_gpu and t.device.type != "cuda":
                no_cpu(name)
            if (device is None or t.device == device) and (not contiguous or t.is_contiguous()):
                continue
        raise ValueError(f"dvmvs::{name}: {label} must be a {'contiguous ' if contiguous else ''}{_dtype_names(dtype)}{_shape_text(shape)} tensor"
                         f"{'' if device is None else f' on {device}'}, got {t.dtype} {tuple(t.shape)} on {t.device}"
                         f"{'' if t.is_contiguous() else ', not contiguous'}")


def device_index(device):
    """The index of ``device`` (a torch.device or what makes one); the current device's where it names none."""
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def ptr(t):
    return t.data_ptr()


def opt_ptr(t):
    """Device pointer of an optional tensor: NULL for None."""
    return None if t is None else t.data_ptr()


def channel_ptr(name, label, t, C):
    """Pointer of a per-channel vector (a bias, a pre-bias) that may be absent: ``t`` has 0 or ``C`` entries, or is None; NULL unless it has C."""
    if t is None:
        return None
    n = t.numel()
    if n != C and n != 0:
        raise ValueError(f"dvmvs::{name}: {label} has {n} entries for {C} channels")
    return t.data_ptr() if n else None


def out_or_new(name, out, shape, dtype, device, label="out"):
    """An optional destination: a new ``dtype`` tensor of ``shape`` on ``device``, or ``out`` when it is exactly that and contiguous."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    check_tensors(name, out, dtype=dtype, label=label, shape=shape, device=device, contiguous=True)
    return out


def launch(entry, device, *args):
    """Calls the C entry ``entry`` of the library with ``device`` current and that device's current stream as its last argument, and
    raises the library's error under the entry's name when it returns non-zero.  Nothing else: no synchronisation, no host read, no
    allocation, so every op stays capturable into a hipGraph."""
    with torch.cuda.device(device):
        rc = getattr(_capi.lib(), entry)(*args, torch.cuda.current_stream(device).cuda_stream)
    if rc != 0:
        _capi.check(rc, entry)


def custom_op(name, mutates_args=(), fake=None):
    """Decorator: registers the implementation as ``torch.ops.dvmvs.<name>`` for HIP tensors, with ``fake`` as its shape inference where
    there is one and a CPU kernel that raises the no-CPU error."""
    def register(impl):
        op = torch.library.custom_op(f"dvmvs::{name}", impl, mutates_args=mutates_args, device_types="cuda")
        if fake is not None:
            op.register_fake(fake)
        op.register_kernel("cpu")(lambda *args, **kwargs: no_cpu(name))
        return op
    return register
