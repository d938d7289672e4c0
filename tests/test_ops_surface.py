"""CPU: ``dvmvs.hip.ops`` offers exactly the surface recorded in tests/golden/ops_surface.json (tests/golden/make_ops_surface.py): its
public names, the signatures of its callables, its constants, ``__all__``, the docstrings and the schemas of the registered ops.  The
package is organised in family modules over shared plumbing; none of that may change what a caller sees."""
import importlib.util
import json
import os


def _recorder(golden_dir):
    spec = importlib.util.spec_from_file_location("make_ops_surface", os.path.join(golden_dir, "make_ops_surface.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_ops_surface_is_the_recorded_one(golden_dir):
    recorder = _recorder(golden_dir)
    with open(os.path.join(golden_dir, "ops_surface.json")) as f:
        want = json.load(f)
    got = recorder.normalised(recorder.surface())
    assert len(want["names"]) == 81 and "direct_conv_shape" in want["names"] and len(want["schemas"]) == 17
    for part in ("names", "all", "constants", "documented", "signatures", "schemas"):
        assert got[part] == want[part], part
    assert got == want


def test_every_op_is_registered_by_importing_the_package(golden_dir):
    import torch
    from dvmvs.hip import ops  # noqa: F401
    with open(os.path.join(golden_dir, "ops_surface.json")) as f:
        want = json.load(f)
    for name in want["schemas"]:
        op = getattr(torch.ops.dvmvs, name.split("::")[1])
        assert torch._C._dispatch_has_kernel_for_dispatch_key(op.default.name(), "CPU"), name      # the stub that refuses CPU tensors
