"""Accuracy criteria shared by the GPU test modules (a plain helper module, so that no test module imports another)."""
import torch


def as_accurate_as_reference(got, ref32, ref64, slack=3.0, floor=2e-6):
    """Principled fp32 criterion: measured against the SAME algebra evaluated in float64, the kernel may be at most
    ``slack`` times as far away as the float32 reference/oracle itself is (plus a small floor).  This separates
    "different rounding" (allowed: the fp32 result is only defined up to its own round-off, which for the sweep is
    dominated by ~1e-5 px of sample-position error times the feature gradient) from "different algorithm"."""
    got, ref32, ref64 = got.detach().cpu().double(), ref32.detach().cpu().double(), ref64.detach().cpu().double()
    err_kernel, err_ref = (got - ref64).abs(), (ref32 - ref64).abs()
    assert err_kernel.max().item() <= slack * err_ref.max().item() + floor, (err_kernel.max().item(), err_ref.max().item())
    assert err_kernel.mean().item() <= slack * err_ref.mean().item() + floor / 10, (err_kernel.mean().item(), err_ref.mean().item())


def f64(*ts):
    return [t.double() if isinstance(t, torch.Tensor) else [x.double() for x in t] for t in ts]
