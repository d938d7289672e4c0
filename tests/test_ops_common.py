"""CPU: the shared checks of the op bindings (dvmvs/hip/ops/_common.py), as far as host tensors reach them: which exception a wrong
argument gets, in which order the properties are judged, and what the small pointer helpers return."""
import pytest
import torch


@pytest.fixture
def common():
    from dvmvs.hip.ops import _common
    return _common


def test_unlabelled_check_is_device_then_dtype(common):
    with pytest.raises(RuntimeError, match="MI355X.*no CPU fallback"):
        common.check_tensors("some_op", torch.zeros(2))
    with pytest.raises(RuntimeError, match="dvmvs::some_op"):
        common.check_tensors("some_op", torch.zeros(2, dtype=torch.float64))                  # misplaced is reported before mistyped
    with pytest.raises(TypeError, match="expected float32 tensors, got torch.float64"):
        common.check_tensors("some_op", torch.zeros(2), torch.zeros(2, dtype=torch.float64), on_gpu=False)
    with pytest.raises(TypeError, match="expected uint8 or int16 tensors"):
        common.check_tensors("some_op", torch.zeros(2), dtype=(torch.uint8, torch.int16), on_gpu=False)
    common.check_tensors("some_op", torch.zeros(2, dtype=torch.int16), dtype=(torch.uint8, torch.int16), on_gpu=False)


def test_labelled_check_is_type_then_dtype_and_shape_then_device_then_layout(common):
    good = torch.zeros(3, 4, 5)
    with pytest.raises(TypeError, match="poses must be a tensor, got ndarray"):
        common.check_tensors("some_op", good.numpy(), label="poses")
    for bad in (good.double(), good[0], good[:, :3]):
        with pytest.raises(ValueError, match=r"poses must be a float32 \[3,4,\*\] tensor, got"):
            common.check_tensors("some_op", bad, label="poses", shape=(3, 4, None))              # malformed before misplaced
    with pytest.raises(RuntimeError, match="MI355X"):
        common.check_tensors("some_op", good, label="poses", shape=(3, 4, None))
    common.check_tensors("some_op", good, label="poses", shape=(3, 4, None), on_gpu=False)
    common.check_tensors("some_op", good, label="poses", on_gpu=False, device=torch.device("cpu"), contiguous=True)
    with pytest.raises(ValueError, match="poses must be a contiguous float32 tensor.*not contiguous"):
        common.check_tensors("some_op", good.transpose(0, 1), label="poses", on_gpu=False, contiguous=True)
    with pytest.raises(ValueError, match="poses must be a float32 tensor on meta, got .* on cpu"):
        common.check_tensors("some_op", good, label="poses", on_gpu=False, device=torch.device("meta"))


def test_pointer_helpers(common):
    t = torch.zeros(6)
    assert common.opt_ptr(None) is None and common.opt_ptr(t) == t.data_ptr() == common.ptr(t)
    assert common.channel_ptr("some_op", "bias", None, 6) is None and common.channel_ptr("some_op", "bias", t[:0], 6) is None
    assert common.channel_ptr("some_op", "bias", t, 6) == t.data_ptr()
    with pytest.raises(ValueError, match="bias has 6 entries for 5 channels"):
        common.channel_ptr("some_op", "bias", t, 5)


def test_optional_destination(common):
    new = common.out_or_new("some_op", None, (2, 3), torch.int32, torch.device("cpu"))
    assert new.shape == (2, 3) and new.dtype == torch.int32
    with pytest.raises(ValueError, match=r"out must be a contiguous int32 \[2,3\] tensor on cpu"):
        common.out_or_new("some_op", new.float(), (2, 3), torch.int32, torch.device("cpu"))
    with pytest.raises(ValueError, match=r"counts must be a contiguous int32 \[2,4\] tensor"):
        common.out_or_new("some_op", new, (2, 4), torch.int32, torch.device("cpu"), label="counts")
    with pytest.raises(RuntimeError, match="MI355X"):                                            # well-formed, but a host tensor
        common.out_or_new("some_op", new, (2, 3), torch.int32, torch.device("cpu"))


def test_device_index(common):
    assert common.device_index("cuda:3") == 3 and common.device_index(torch.device("cuda", 1)) == 1
