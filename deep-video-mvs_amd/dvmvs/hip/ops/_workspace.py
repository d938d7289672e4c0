"""The persistent device buffers of the ops, two kinds and no more.  Both are made outside any graph capture, when the first (eager /
warm-up) call that needs one happens, and both assume what the package assumes everywhere: one process per GPU and one stream per
process, so that the calls sharing a buffer are ordered with respect to each other."""
import torch

from dvmvs.hip.ops._common import device_index

_zeroed = {}
_grown = {}


def _elements(nbytes, dtype):
    return -(-int(nbytes) // dtype.itemsize)


def zeroed(purpose, device, shape_key, nbytes, dtype):
    """The buffer of (purpose, device, shape_key): at least ``nbytes`` of ``dtype``, zero-filled once when it is created.  For kernels
    whose contract is that every call finds their words zero and leaves them zero; a caller whose kernel call FAILED must ``drop`` the
    entry, since that contract may then be broken."""
    key = (purpose, device_index(device), shape_key)
    workspace = _zeroed.get(key)
    if workspace is None:
        workspace = _zeroed[key] = torch.zeros(_elements(nbytes, dtype), dtype=dtype, device=device)
    return workspace


def drop(purpose, device, shape_key):
    """Forgets the zeroed buffer of (purpose, device, shape_key); the next request makes a fresh, zero-filled one."""
    _zeroed.pop((purpose, device_index(device), shape_key), None)


def grown(purpose, device, nbytes, dtype):
    """The buffer of (purpose, device): at least ``nbytes`` of ``dtype``, grown to the largest request seen and never initialised (for
    kernels that write it before they read it).  A buffer that is replaced is marked as in use on the current stream, so the allocator
    does not hand its memory out again before the work enqueued there has finished with it."""
    key = (purpose, device_index(device))
    workspace = _grown.get(key)
    if workspace is None or workspace.numel() * dtype.itemsize < nbytes:
        if workspace is not None:
            workspace.record_stream(torch.cuda.current_stream(device))
        workspace = _grown[key] = torch.empty(_elements(nbytes, dtype), dtype=dtype, device=device)
    return workspace
