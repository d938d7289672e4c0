"""CPU: the MVDepthNet / GP-MVS baseline modules (dvmvs.baselines) against the reference's module surface and the GP-MVS filter
algebra against the fixture of the reference run (tests/golden/baselines_e2e.npz, make_baseline_goldens.py)."""
import json
import os

import numpy as np
import pytest
import torch

import synthetic as syn
from gp_filter_cpu import gp_filter_step

from dvmvs.baselines import runner
from dvmvs.baselines.gpmvs.decoder import Decoder as GPDecoder
from dvmvs.baselines.gpmvs.encoder import Encoder as GPEncoder
from dvmvs.baselines.gpmvs.gplayer import GPlayer
from dvmvs.baselines.mvdepthnet.decoder import Decoder
from dvmvs.baselines.mvdepthnet.encoder import Encoder

CLASSES = {"mvdepthnet_encoder": Encoder, "mvdepthnet_decoder": Decoder, "gpmvs_encoder": GPEncoder, "gpmvs_decoder": GPDecoder,
           "gpmvs_gplayer": lambda: GPlayer(device="cpu")}
SEEDS = {"mvdepthnet_encoder": 10, "mvdepthnet_decoder": 11, "gpmvs_encoder": 12, "gpmvs_decoder": 13}
GP_PARAMS = {"gamma2": 0.5, "ell": 0.3, "sigma2": 0.1}


def seeded(name):
    """The module with the weights make_baseline_goldens.py gave the reference's module of the same name."""
    mod = CLASSES[name]()
    if name == "gpmvs_gplayer":
        with torch.no_grad():
            for k, v in GP_PARAMS.items():
                getattr(mod, k).fill_(v)
        return mod.eval()
    syn.deterministic_init(mod, seed=SEEDS[name])
    syn.apply_bn_stats([(name, mod)], os.path.join(syn.GOLDEN_DIR, "baselines_bn_stats.npz"))
    return mod.eval()


@pytest.fixture(scope="module")
def e2e():
    return np.load(os.path.join(syn.GOLDEN_DIR, "baselines_e2e.npz"))


def test_state_dict_keys_and_shapes_match_the_reference():
    with open(os.path.join(syn.GOLDEN_DIR, "baseline_state_dict_keys.json")) as f:
        expected = json.load(f)
    assert sorted(expected) == sorted(CLASSES)
    for name, ctor in CLASSES.items():
        got = {k: list(v.shape) for k, v in ctor().state_dict().items()}
        assert got == expected[name], name


def test_train_keeps_batchnorm_frozen():
    enc = Encoder().train()
    bns = [m for m in enc.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert enc.training and bns and all(not m.training and not m.weight.requires_grad for m in bns)


def test_three_checkpoint_layouts_load(tmp_path):
    enc, dec = seeded("mvdepthnet_encoder"), seeded("mvdepthnet_decoder")
    # plain state dicts (fine-tuned MVDepthNet)
    plain = tmp_path / "plain"
    plain.mkdir()
    torch.save(enc.state_dict(), plain / "finetuned_mvdepthnet_encoder")
    torch.save(dec.state_dict(), plain / "finetuned_mvdepthnet_decoder")
    # DataParallel-prefixed (GP-MVS) with a GP layer
    prefixed = tmp_path / "prefixed"
    prefixed.mkdir()
    torch.save({"module." + k: v for k, v in enc.state_dict().items()}, prefixed / "gpmvs_encoder")
    torch.save({"module." + k: v for k, v in dec.state_dict().items()}, prefixed / "gpmvs_decoder")
    torch.save(seeded("gpmvs_gplayer").state_dict(), prefixed / "gpmvs_gplayer")
    # MVDepthNet's combined file: both modules' keys (and others) under 'state_dict'
    combined = tmp_path / "combined"
    combined.mkdir()
    both = dict(enc.state_dict())
    both.update(dec.state_dict())
    both["unrelated.weight"] = torch.zeros(1)
    torch.save({"state_dict": both, "epoch": 3}, combined / "pretrained_mvdepthnet_combined")

    def same(a, b):
        return all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in a.state_dict())

    for folder in (plain, combined):
        e, d = runner.build_mvdepthnet(folder, device="cpu", seed=5)
        assert same(e, enc) and same(d, dec)
    e, d, g = runner.build_gpmvs(prefixed, device="cpu", seed=5)
    assert same(e, enc) and same(d, dec) and g.gamma2.item() == pytest.approx(0.5)


def test_closed_form_transition_matches_expm():
    scipy_linalg = pytest.importorskip("scipy.linalg")
    for ell, dt in ((0.7, 0.0), (1.3, 0.11), (0.35, 0.26), (2.0, 4.7), (0.9, 12.0)):
        lam = np.sqrt(3) / ell
        F = np.array([[0, 1], [-lam ** 2, -2 * lam]])
        got, want = runner.gp_transition(lam, dt), scipy_linalg.expm(F * dt)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_host_filter_algebra_matches_the_reference_run(e2e):
    gp = runner.GPFilter(*(np.float32(v).item() for v in e2e["gp_params"]))
    for n in range(int(e2e["n_frames"])):
        A, k, reset = gp.step(float(e2e[f"gp_f{n}_dt"]))
        assert reset == (n == 0)
        np.testing.assert_allclose(np.reshape(A, (2, 2)), e2e[f"gp_f{n}_A"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(k, e2e[f"gp_f{n}_k"], rtol=1e-12, atol=1e-14)


def test_numpy_filter_reproduces_the_reference_state(e2e):
    """gp_filter_cpu fed the fixture's conv5 (at the pinned columns) reproduces the reference's float64 state and Z there."""
    state = np.zeros((2, e2e["gp_f0_conv5_samples"].size))
    for n in range(int(e2e["n_frames"])):
        state, Z = gp_filter_step(state, e2e[f"gp_f{n}_conv5_samples"], e2e[f"gp_f{n}_A"], e2e[f"gp_f{n}_k"], reset=(n == 0))
        want = e2e[f"gp_f{n}_state_samples"]
        assert np.abs(state - want).max() <= 1e-12 * np.abs(want).max()
        np.testing.assert_array_equal(Z, e2e[f"gp_f{n}_Z_samples"])


def test_system_names():
    f = "keyframe+hololens-dataset+000+nmeas+2"
    assert runner.system_name("mvdepthnet", f) == "keyframe_hololens-dataset_320_256_2_mvdepthnet_finetuned"
    assert runner.system_name("gpmvs", "/x/" + f, finetuned=False) == "keyframe_hololens-dataset_320_256_2_gpmvs_without_ft"


def rel_l1(got, pins):
    idx = syn.sample_indices(got.numel())
    g = got.reshape(-1)[idx].double()
    w = torch.from_numpy(pins).double()
    return ((g - w).abs().sum() / w.abs().sum()).item()


def test_cpu_forward_of_mvdepthnet_matches_frame0(e2e):
    """Encoder / decoder of this package on the CPU, fed the reference's own cost volume for frame 0 (the CPU has no sweep kernel:
    the volume comes from the reference's function restated by oracle/dvmvs_oracle.py)."""
    import dvmvs_oracle as orc
    enc, dec = seeded("mvdepthnet_encoder"), seeded("mvdepthnet_decoder")
    r, m0, m1 = (int(v) for v in e2e["f0_frames"])
    image = syn.e2e_image
    cv = orc.cost_volume_fusion(image(r), [image(m0), image(m1)], syn.pose(r), [syn.pose(m0), syn.pose(m1)], syn.full_K(),
                                0.5, 50.0, 64, False)
    with torch.no_grad():
        disp = dec(*enc(image(r), cv))[0]
    depth = 1.0 / torch.clamp(disp, 0.02, 2.0)
    assert rel_l1(depth, e2e["mv_f0_depth_samples"]) <= 1e-5
