"""The frame engine's module surface (CPU): ``dvmvs.engine`` is split by concern into flat modules beside it -- the fused layers, the module
surface for the reference's own loop, the device-free host parts, the frame's parameter block and the destination-passing frame body --, still
exports every name that was ever imported from it, and the lower modules do not import it back.  The parameter block's host half runs
without a device, and the experiment switches whose code was removed are not read any more."""
import ast
import os
import subprocess
import sys

import torch

import synthetic as syn

PACKAGE = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "deep-video-mvs_amd"))


def test_engine_exports_the_names_of_its_parts():
    from dvmvs import engine, frame_direct, frame_host, fused_layers, module_surface, parameter_block
    homes = {fused_layers: ("FusedConv2d", "fold_batchnorm", "fuse_epilogues", "_graph_microseconds", "_KERNEL_SWITCHES", "set_kernel_families"),
             module_surface: ("GraphedModule", "accelerate"),
             frame_host: ("CopyQueue", "FeatureCache", "FrameBody"),
             parameter_block: ("ParameterBlock",),
             frame_direct: ("DirectFrameBody",)}
    for module, names in homes.items():
        for name in names:
            assert getattr(engine, name) is getattr(module, name), name
            assert getattr(getattr(module, name), "__module__", module.__name__) == module.__name__, name      # defined there, not passed on
    assert engine.DepthEngine.__module__ == "dvmvs.engine" and engine._fork_point.__module__ == "dvmvs.engine"
    assert {"_FORK_AFTER", "_GRAPH_QUEUE_FILLERS"} <= set(vars(engine))      # (read from this namespace at use time: bench.py assigns them)
    assert callable(fused_layers.FusedConv2d.repack) and callable(frame_host._store_measurement_map)


def _imports(path):
    found = set()
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Import):
            found |= {alias.name for alias in node.names}
        if isinstance(node, ast.ImportFrom):
            found |= {node.module or ""} | {f"{node.module}.{alias.name}" for alias in node.names}
    return found


def test_the_parts_depend_on_each_other_one_way():
    folder = os.path.join(PACKAGE, "dvmvs")
    parts = {"dvmvs.fused_layers", "dvmvs.module_surface", "dvmvs.frame_host", "dvmvs.parameter_block", "dvmvs.frame_direct", "dvmvs.engine"}
    allowed = {"fused_layers": set(), "frame_host": set(), "module_surface": {"dvmvs.fused_layers"}, "parameter_block": {"dvmvs.frame_host"},
               "frame_direct": {"dvmvs.fused_layers"}}
    for name, may in allowed.items():
        used = {p for p in parts for i in _imports(os.path.join(folder, name + ".py")) if i == p or i.startswith(p + ".")}
        assert used == may, (name, used)
    # and at run time, in a fresh interpreter: importing the layers, the host parts or the parameter block loads neither the engine nor another part
    for name in ("fused_layers", "frame_host", "parameter_block"):
        code = f"import sys; import dvmvs.{name}; print(sorted(m for m in sys.modules if m.startswith('dvmvs.') and m.split('.')[1] in {sorted(p.split('.')[1] for p in parts)!r}))"
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=PACKAGE), capture_output=True, text=True, check=True).stdout
        loaded = set(ast.literal_eval(out.strip().splitlines()[-1]))
        assert loaded == {f"dvmvs.{name}"} | allowed[name], (name, loaded)


def test_parameter_block_host_half_needs_no_device():
    from dvmvs.parameter_block import ParameterBlock
    block = ParameterBlock(sequences=1, height=256, width=320, n_depth_levels=64, min_depth=0.25, max_depth=20.0, pose_algebra="reference",
                           sweep_work_list=True, sweep_mfma=True, is_fusionnet=True)
    assert block.params is None and block.views == {} and block.mirror.device.type == "cpu" and block.mirror.numel() == block.total and block.total % 4 == 0
    assert {"Hm", "kt", "reproject_T", "lstm_T", "full_K", "half_K", "lstm_K", "pose", "prev_pose", "meas_pose", "sweep_items", "Hm1", "kt1",
            "sweep_items1"} == set(block.offsets)
    poses = torch.from_numpy(syn.sample_poses()).float()
    reference, measurements = syn.keyframe_index_lines(2)[0]
    pose, full_K = poses[reference:reference + 1], syn.full_K()
    previous = poses[measurements[0]:measurements[0] + 1]
    committed, variant, next_variant = block.evaluate(block.mirror, 2, pose, [poses[m:m + 1] for m in measurements], full_K, previous,
                                                      torch.zeros(1, dtype=torch.bool), 0, True, None)
    assert variant == 6 and next_variant is None and torch.equal(committed, pose.reshape(1, 4, 4))
    region = lambda name, n: block.mirror[block.offsets[name][0]:block.offsets[name][0] + n]
    assert torch.equal(region("pose", 16), pose.reshape(-1)) and torch.equal(region("prev_pose", 16), previous.reshape(-1))
    assert torch.equal(region("full_K", 9), torch.as_tensor(full_K).float().reshape(-1))
    assert bool(region("Hm", 18).abs().sum() > 0) and not bool(region("Hm1", 18).abs().sum() > 0)      # (buffer set 0 was planned, set 1 untouched)


WORDS = ("aux_stream", "paired_upsampling", "up2x_in_conv", "batch_copies", "upload_in_copy_batch", "gates_on_partials", "staging_slots", "beside")


def test_removed_experiment_switches_are_not_read():
    """A removed variable, when set, is not read: no attribute of the engine's modules or of their classes is named after a removed experiment,
    and no source file of the package or the tools spells one of their words (in either case) any more."""
    code = ("import sys, dvmvs.engine\n"
            f"words = {WORDS!r}\n"
            "parts = [m for n, m in sys.modules.items() if n == 'dvmvs.engine' or n.split('.')[:2] in (['dvmvs', p] for p in\n"
            "         ('fused_layers', 'module_surface', 'frame_host', 'parameter_block', 'frame_direct'))]\n"
            "assert len(parts) == 6, parts\n"
            "owners = parts + [v for m in parts for v in vars(m).values() if isinstance(v, type) and v.__module__ == m.__name__]\n"
            "print([(getattr(o, '__name__', o), a) for o in owners for a in vars(o) if any(w in a.lower() for w in words)])\n")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=PACKAGE, DVMVS_AUX_STREAM="1"), capture_output=True, text=True,
                         check=True).stdout
    assert out.strip().splitlines()[-1] == "[]", out
    root = os.path.dirname(PACKAGE)
    for folder in (os.path.join(PACKAGE, "dvmvs"), os.path.join(root, "tools")):
        for where, _, files in os.walk(folder):
            for file in files:
                if file.endswith((".py", ".sh")):
                    source = open(os.path.join(where, file)).read().lower()
                    assert not any(word in source for word in WORDS[:-1]), (file, [w for w in WORDS if w in source])
