"""GPU: the one workspace cache of the ops (dvmvs/hip/ops/_workspace.py) -- a grown buffer is replaced only by a larger one and kept per
purpose, a zeroed buffer is made once and made afresh after ``drop``, and an op whose C call fails forgets the zeroed workspace it handed
to that call.  The failing calls are Python stand-ins for the C entries that only return an error code: nothing is launched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL = -1      # DVMVS_EINVAL, include/dvmvs_hip.h


@pytest.fixture
def workspace():
    from dvmvs.hip.ops import _workspace
    return _workspace


def test_grown_buffer_is_replaced_only_by_a_larger_one(workspace, hip_device):
    first = workspace.grown("test_grown", hip_device, 256, torch.uint8)
    second = workspace.grown("test_grown", hip_device, 1024, torch.uint8)
    third = workspace.grown("test_grown", hip_device, 256, torch.uint8)
    assert first.numel() >= 256 and first.dtype == torch.uint8 and first.device == hip_device
    assert second is not first and second.numel() >= 1024 and second.data_ptr() != first.data_ptr()
    assert third is second
    other = workspace.grown("test_grown_other", hip_device, 256, torch.uint8)
    assert other is not second and other.data_ptr() != second.data_ptr()
    assert workspace.grown("test_grown", hip_device, 1024, torch.uint8) is second          # ... and the other purpose did not disturb it
    words = workspace.grown("test_grown_words", hip_device, 10, torch.float32)             # sizes are bytes, rounded up to whole elements
    assert words.dtype == torch.float32 and words.numel() == 3


def test_zeroed_buffer_is_made_once_and_afresh_after_drop(workspace, hip_device):
    key = ("test_zeroed", hip_device, (3, 5))
    first = workspace.zeroed(*key, 64, torch.float64)
    assert first.dtype == torch.float64 and first.numel() == 8 and not first.any()
    assert workspace.zeroed(*key, 64, torch.float64) is first
    assert workspace.zeroed("test_zeroed", hip_device, (3, 6), 64, torch.float64) is not first     # another shape key, another buffer
    first.fill_(7.0)                                                                              # a contract broken by a failed call
    workspace.drop(*key)
    fresh = workspace.zeroed(*key, 64, torch.float64)
    assert fresh is not first and fresh.data_ptr() != first.data_ptr() and not fresh.any()
    workspace.drop(*key)
    workspace.drop(*key)                                                                          # forgetting twice is fine


def test_failed_depth_errors_call_forgets_its_workspace(monkeypatch, hip_device):
    from dvmvs.hip import _capi, ops
    gt = torch.tensor([[1.0, 2.0], [3.0, 4.0]], device=hip_device)
    pred = gt + 0.5
    assert ops.depth_errors(gt, pred).shape == (1, 8)
    before = ops.depth_errors_workspace(hip_device, 1, 4)
    assert ops.depth_errors_workspace(hip_device, 1, 4) is before and before.dtype == torch.float64
    monkeypatch.setattr(_capi.lib(), "dvmvs_depth_errors_fwd", lambda *args: EINVAL)
    with pytest.raises(RuntimeError, match="dvmvs_depth_errors_fwd"):
        ops.depth_errors(gt, pred)
    after = ops.depth_errors_workspace(hip_device, 1, 4)
    assert after is not before and after.data_ptr() != before.data_ptr() and not after.any()


def test_failed_sweep_call_forgets_its_workspace(monkeypatch, hip_device):
    from dvmvs.hip import _capi, ops
    B, M, C, H, W, D = 1, 1, 4, 8, 8, 4
    assert ops.sweep.COST_VOLUME_TWO_PASS
    image1, image2 = torch.rand(B, C, H, W, device=hip_device), torch.rand(B, C, H, W, device=hip_device)
    Hm = torch.eye(3, device=hip_device).reshape(1, 1, 9).contiguous()
    kt = torch.tensor([[[0.1, 0.0, 0.0]]], device=hip_device)
    before, nbytes = ops.sweep_workspace(hip_device, B, M, H, W, D)
    assert ops.sweep_workspace(hip_device, B, M, H, W, D)[0] is before and before.dtype == torch.float32 and before.numel() * 4 >= nbytes
    monkeypatch.setattr(_capi.lib(), "dvmvs_cost_volume_planned_fwd", lambda *args: EINVAL)
    with pytest.raises(RuntimeError, match="dvmvs_cost_volume_planned_fwd"):
        ops.cost_volume(image1, [image2], Hm, kt, 0.25, 20.0, D, True, 0)
    middle = ops.sweep_workspace(hip_device, B, M, H, W, D)[0]
    assert middle is not before and middle.data_ptr() != before.data_ptr() and not middle.any()
    with pytest.raises(RuntimeError, match="dvmvs_cost_volume_planned_fwd"):
        ops.cost_volume_into(image1, [image2], Hm, kt, 0.25, 20.0, torch.empty(B, D, H, W, device=hip_device))
    assert ops.sweep_workspace(hip_device, B, M, H, W, D)[0] is not middle
