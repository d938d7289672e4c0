"""DepthEngine at frame sizes other than 320x256 (tests/engine_size_cases.py: 96x64, 160x128, 256x256, 320x256 as calibration, 640x512).
The size is ``Config.test_image_width / height`` when the engine is built; every layer then asks the kernels' shape rules anew, the sweep, the
ConvLSTM path and the buffers follow the size.  Checked per size against the float64 CPU pipeline of tests/golden/engine_sizes_<W>x<H>.npz:

* the criterion: a stage's distance from float64 is at most SLACK = 3 times the float32 CPU pipeline's own (the fixture's yardstick, the
  largest over the size's frames; never computed from the engine), depth as rel-L1, h / c / bottom / cost volume as mean |x - x64| / mean |x64|.
  The depth is read on the whole map (small frames) or on 49 152 pixels drawn uniformly, on its whole two-pixel border and as the means of all
  8x8 blocks; the other stages on samples; and every stage's whole-tensor sums lie within the bound the criterion implies for them;
* the condition: the engine's low-resolution depth estimate takes every pixel from the source point the float64 pipeline takes it from;
* the dispatch: which problems reach which kernel (engine_size_cases.EXPECTED);
* the product path (graphs, look-ahead): two engines agree bit for bit, meet the criterion, and repeat frame 1 after a reset;
* sizes that are no multiple of 32 are refused before anything is allocated.
Every frame after the first starts from the fixture's installed state (teacher forcing), so a ratio belongs to its frame alone.

Measured on an MI355X (engine's distance / yardstick, "depth" per frame; then the range over all stages -- the border and block-mean depth
among them -- and frames), the same for the eager and the graph engines, which hold the same bits: 96x64 1.19 0.96 0.63 (0.42 .. 1.25); 160x128
1.02 0.81 0.52 (0.40 .. 1.13); 256x256 1.09 1.04 0.66 (0.53 .. 1.12); 320x256 1.03 0.94 0.49 (0.39 .. 1.11); 640x512 1.10 1.08 (0.86 .. 1.15);
0 flipped estimate pixels everywhere; whole-tensor sums off by 1e-9 .. 1e-5 of the sum of magnitudes.  For scale: one output channel of one 1x1
layer scaled by 1.001 reads 4 .. 12 at 96x64; at 640x512 the last column of the full-resolution head shifted by a row reads 175 on the border,
the last row of one channel of the second refinement layer zeroed 86."""
import functools

import pytest
import torch

import engine_size_cases as cases
import synthetic as syn

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _modules():
    from dvmvs.fusionnet.model import CostVolumeDecoder, CostVolumeEncoder, FeatureExtractor, FeatureShrinker, LSTMFusion
    return tuple(syn.build_e2e_modules((FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder)))


@functools.lru_cache(maxsize=None)
def _fixture(size):
    return cases.load_fixture(*size)


def build_engine(patch, size, dev, **kw):
    """A DepthEngine for frames of ``size`` = (W, H): the documented setting, set before the engine is built."""
    from dvmvs.config import Config
    from dvmvs.engine import DepthEngine
    patch.setattr(Config, "test_image_width", size[0])
    patch.setattr(Config, "test_image_height", size[1])
    engine = DepthEngine(*_modules(), device=dev, **kw)
    assert (engine.width, engine.height) == size
    return engine


@functools.lru_cache(maxsize=None)
def _inputs(size, dev):
    W, H = size
    indices = sorted({i for r, ms in cases.frames(W, H) for i in (r,) + tuple(ms)})
    return {i: cases.image(i, W, H).to(dev) for i in indices}


def run_frames(engine, size, dev, announce=False, only=None):
    """The size's frames, each after the first from the fixture's installed state.  ``announce``: the next frame is announced to ``step`` as a
    caller that knows its keyframes does (look-ahead).  Returns per frame the clones of what the criterion reads."""
    W, H = size
    z, K, images, frames = _fixture(size), cases.full_K(W, H), _inputs(size, dev), cases.frames(W, H)
    out = []
    for n, (r, ms) in enumerate(frames[:only]):
        if n == 0:
            engine.reset()
        else:
            h, c, depth = cases.unpack_state(z, f"f{n}_state")
            engine.load_state(h.to(dev), c.to(dev), depth.to(dev), torch.from_numpy(z[f"f{n}_state_pose"]))
        ahead = {}
        if announce and n + 1 < len(frames):
            r1, ms1 = frames[n + 1]
            ahead = dict(next_reference_image=images[r1], next_frame_id=r1, next_reference_pose=syn.pose(r1),
                         next_measurement_poses=[syn.pose(i) for i in ms1], next_measurement_ids=list(ms1))
        depth = engine.step(images[r], syn.pose(r), [images[i] for i in ms], [syn.pose(i) for i in ms], K, frame_id=r, measurement_ids=list(ms), **ahead)
        cur = engine._direct_buffers["sets"][1 - engine._parity]      # the buffer set the frame ran on (step has already turned to the other)
        s = engine._static
        out.append(dict(depth=depth.clone(), h=s["h"].clone(), c=s["c"].clone(), bottom=cur["lstm_cat"][:, :512].clone(),
                        cost_volume=cur["enc_cat"][0][:, 32:].clone(), feat_half=cur["enc_cat"][0][:, :32].clone(),
                        estimate=engine._direct_buffers["estimate"].clone()))
    torch.cuda.synchronize(dev)
    return out


def check_results(results, size, what):
    """Prints every ratio, then asserts the condition and the criterion on every frame."""
    W, H = size
    z = _fixture(size)
    yard = cases.yardsticks(z, W, H)
    failures = []
    for n, res in enumerate(results):
        assert tuple(res["depth"].shape) == (1, H, W) and bool(torch.isfinite(res["depth"]).all())
        flips = cases.flipped_pixels(res["estimate"].cpu().numpy(), z[f"f{n}_depth_estimation"])
        tensors = {k: res[k] for k in cases.SAMPLED}
        got = cases.result_distances(z, n, W, H, res["depth"], **tensors)
        print(f"{what} {W}x{H} frame {n}: estimate flips {flips}; distance from float64 / float32 CPU pipeline's (ratio): " +
              ", ".join(f"{s} {got[s]:.2e} / {yard[s]:.2e} ({got[s] / yard[s]:.2f})" for s in cases.STAGES))
        if flips:
            failures.append((n, "estimate flips", flips))
        failures += [(n, s, got[s] / yard[s]) for s in cases.CRITERION_STAGES if not got[s] <= cases.SLACK * yard[s]]
        # the whole tensors: |sum - sum64| and |sum |x| - sum |x64|| are at most sum |x - x64| (engine_size_cases.sum_distances)
        sums = cases.sum_distances(z, n, W, H, res["depth"], **tensors)
        print(f"{what} {W}x{H} frame {n}: whole-tensor sums off by (of the sum of magnitudes): " +
              ", ".join(f"{s} {sums[s][0]:.1e} {sums[s][1]:.1e}" for s in sums))
        failures += [(n, s + " sums", sums[s]) for s in sums if s in cases.CRITERION_STAGES and not max(sums[s]) <= cases.SLACK * yard[s]]
    assert not failures, (size, failures)


# ---- eager, stage by stage; the dispatch is recorded on the same run ---------------------------------------------------------------------
def _spies(patch, log):
    """Wrappers around the convolution entries, the gates, the up-sampler, the sweep and the library convolution that record their problems."""
    from dvmvs.hip import ops

    def spy(owner, name, describe):
        real = getattr(owner, name)

        def wrapper(*args, **kw):
            log.setdefault(name, []).append(describe(*args, **kw))
            return real(*args, **kw)

        patch.setattr(owner, name, wrapper)

    spy(ops, "bottleneck_conv_into", lambda x, packed, C_out, stride, partials, upsample=False:
        (x.shape[1], int(C_out), x.shape[2] * (2 if upsample else 1), x.shape[3] * (2 if upsample else 1), int(stride), bool(upsample)))
    spy(ops, "direct_conv_into", lambda x, packed, n_tile, bias, dst, C_out, k, stride, act, dst_nhwc=None:
        (x.shape[1], x.shape[2], x.shape[3], int(C_out), int(k), int(stride)))
    spy(ops, "conv_head_into", lambda x, *a, **kw: (x.shape[1], x.shape[2], x.shape[3]))
    spy(ops, "pointwise_conv_into", lambda x, packed, bias, dst, C_out, *a, **kw: (x.shape[1], int(C_out), x.shape[2], x.shape[3]))
    spy(ops, "lstm_gates_partials_into", lambda partials, n, c, h: (int(n), c.shape[2], c.shape[3]))
    spy(ops, "lstm_gates_into", lambda combined, c, h: (c.shape[2], c.shape[3]))
    spy(ops, "upsample2x", lambda x: tuple(x.shape[1:]))
    spy(ops, "cost_volume_into", lambda image1, image2s, Hm, kt, lo, hi, dst, variant=0, work_list=None:
        (int(variant), image1.shape[2], image1.shape[3], work_list is not None))
    # (the library convolution; the input images are smoothed with one on the CPU: only what runs on the device counts)
    spy(torch.nn.functional, "conv2d", lambda x, w, bias=None, stride=1, padding=0, dilation=1, groups=1:
        (x.shape[1], w.shape[0], x.shape[2], x.shape[3], w.shape[2], int(stride[0] if isinstance(stride, (tuple, list)) else stride), int(groups), x.is_cuda))


def recorded_problems(log):
    """The spies' log in engine_size_cases.EXPECTED's form."""
    convs = [p for p in log.get("conv2d", []) if p[7] and p[6] == 1]
    bottleneck = {p[:5] for p in log.get("bottleneck_conv_into", []) if p[:2] != cases.LSTM_PROBLEM}
    lstm = {"bottleneck" for p in log.get("bottleneck_conv_into", []) if p[:2] == cases.LSTM_PROBLEM} | {"library" for p in convs if p[:2] == cases.LSTM_PROBLEM}
    return {"bottleneck": sorted(bottleneck), "up2x": sorted({p[:5] for p in log.get("bottleneck_conv_into", []) if p[5]}),
            "lstm": sorted(lstm), "direct": sorted(set(log.get("direct_conv_into", []))), "head": sorted(set(log.get("conv_head_into", []))),
            "pointwise": sorted(set(log.get("pointwise_conv_into", []))),
            "library": sorted({p[:6] for p in convs if p[:2] != cases.LSTM_PROBLEM}),
            "sweep": sorted({p[0] for p in log.get("cost_volume_into", [])}),
            "gates_on_partials": sorted(set(log.get("lstm_gates_partials_into", []))), "gates": sorted(set(log.get("lstm_gates_into", []))),
            "upsample2x": sorted(set(log.get("upsample2x", [])))}


@functools.lru_cache(maxsize=None)
def eager_run(size, dev):
    """(results per frame, recorded problems, the engine's sweep_mfma) of one eager engine with the default kernels over the size's frames."""
    log = {}
    with pytest.MonkeyPatch.context() as patch:
        engine = build_engine(patch, size, dev, use_graphs=False)
        assert engine.direct and engine.bottleneck_convs and engine.direct_convs and engine.pointwise_convs
        _spies(patch, log)
        results = run_frames(engine, size, dev)
    return results, recorded_problems(log), engine.sweep_mfma


@pytest.mark.parametrize("size", cases.SIZES, ids=cases.size_id)
def test_eager_engine_stage_by_stage(hip_device, size):
    results, _, _ = eager_run(size, hip_device)
    assert len(results) == len(cases.frames(*size))
    check_results(results, size, "eager")


@pytest.mark.parametrize("size", cases.SIZES, ids=cases.size_id)
def test_dispatch(hip_device, size):
    """The problems the size sends to each kernel are the cases module's list, and the facts that tell the sizes apart hold."""
    W, H = size
    _, got, sweep_mfma = eager_run(size, hip_device)
    print(f"{W}x{H}: " + "; ".join(f"{k} {v}" for k, v in got.items()))
    expected = cases.EXPECTED[size]
    for kind in ("bottleneck", "up2x", "lstm", "direct", "head", "pointwise", "library"):
        assert got[kind] == sorted(expected[kind]), (size, kind, got[kind])
    assert got["sweep"] and set(got["sweep"]) <= set(expected["sweep"]), (size, got["sweep"])
    h, w = H // 32, W // 32
    # the ConvLSTM convolution: through the bottleneck kernel (WINDOW staging, gates on its K-split partial sums) at 640x512 as at 320x256, through the
    # library at the other sizes
    assert got["lstm"] == (["bottleneck"] if size in ((320, 256), (640, 512)) else ["library"])
    if got["lstm"] == ["bottleneck"]:
        from dvmvs.hip import ops
        assert got["gates_on_partials"] == [(ops.bottleneck_conv_splits(1, 2048, 1024, h, w, 1), h, w)] and got["gates"] == []
    else:
        assert got["gates"] == [(h, w)] and got["gates_on_partials"] == []
    # the decoder's first up-sampling inside its convolution's staging: where the ConvLSTM's map is 8x10.  (160x128 has an 8x10 map too, its 1/16 one:
    # that level's up-sampling goes with its depth head's in the paired launch, and its convolution takes the up-sampled map)
    assert got["up2x"] == ([(512, 256, 16, 20, 1)] if size == (320, 256) else [])
    assert got["upsample2x"] == ([] if size == (320, 256) else [(512, h, w)])
    if size in ((256, 256), (96, 64)):      # no output width is a multiple of 40: every dense 3x3 / 5x5 layer is the library's
        assert got["bottleneck"] == [] and got["direct"] == [] and len(got["library"]) >= len(cases.DENSE_LAYERS)
    assert len(got["head"]) == 5 and len(got["pointwise"]) >= 18      # the depth heads and the 1x1 layers stay HIP at every size
    # the correlate-then-interpolate sweep (variant 6) from 64x64 cells on; below, the tiled variants from their host-made work lists
    assert sweep_mfma == (size != (96, 64)) and (got["sweep"] == [6]) == sweep_mfma


# ---- the product path -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.SIZES, ids=cases.size_id)
def test_product_path(hip_device, monkeypatch, size):
    """Default engines (hipGraph replay, look-ahead as the keyframe-index runners announce it): two of them agree bit for bit on every stage of
    every frame and hold the eager engine's bits, so they meet the criterion (checked on one); after a reset frame 1 returns the bits of the first
    time, and so do the frames behind it -- by then every kind of frame is a replayed graph, at the first pass its first occurrence ran eagerly."""
    dev = hip_device
    first, second = build_engine(monkeypatch, size, dev), build_engine(monkeypatch, size, dev)
    assert first.use_graphs and first.direct and first.max_lookahead >= 1
    a, b = run_frames(first, size, dev, announce=True), run_frames(second, size, dev, announce=True)
    for n, (ra, rb) in enumerate(zip(a, b)):
        for key in ra:
            assert torch.equal(ra[key], rb[key]), (size, n, key)
    check_results(a, size, "graphs + look-ahead")
    # (the eager engine of this process: every launch is a pure function of its inputs, and the library picks a convolution's algorithm once per
    # problem and process and keeps it, so engines of one process run the same kernels; between processes the library's choice may differ)
    eager, _, _ = eager_run(size, dev)
    for n, (ra, re) in enumerate(zip(a, eager)):
        for key in ra:
            assert torch.equal(ra[key], re[key]), (size, n, key, "eager")
    again = run_frames(first, size, dev, announce=True)
    assert first._graphs and len(again) == len(a)
    for n, (ra, rg) in enumerate(zip(a, again)):
        for key in ra:
            assert torch.equal(rg[key], ra[key]), (size, n, key, "after reset")
    first.close()
    second.close()


# ---- refused sizes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.REFUSED_SIZES, ids=cases.size_id)
def test_sizes_that_are_no_multiple_of_32_are_refused(hip_device, monkeypatch, size):
    """The network's 1/32 map and its x2 skip connections cannot be formed: ValueError from DepthEngine.__init__, before anything is allocated."""
    modules = _modules()
    torch.cuda.synchronize(hip_device)
    before = torch.cuda.memory_allocated(hip_device)
    with pytest.raises(ValueError, match="multiple of 32"):
        build_engine(monkeypatch, size, hip_device)
    assert torch.cuda.memory_allocated(hip_device) == before
    assert modules is _modules()
