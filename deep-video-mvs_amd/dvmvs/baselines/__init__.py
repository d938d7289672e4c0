"""The MVDepthNet, GP-MVS and DPSNet baselines of the reference's dvmvs/baselines/, at the same import paths.

Both sweep the full-resolution normalised RGB images with the SAD cost volume (dvmvs::rgb_sweep, csrc/sweep_rgb.hip, which
also writes the encoder's 67-channel input) and run an encoder / decoder pair; GP-MVS filters the encoder bottleneck across
frames with a Gaussian-process Kalman filter on the device (dvmvs::gp_filter_step, csrc/gp_filter.hip).  Runners:
dvmvs.baselines.runner, ``python -m dvmvs.baselines.mvdepthnet`` and ``python -m dvmvs.baselines.gpmvs``.

DPSNet (dvmvs.baselines.dpsnet) builds its plane volumes with dvmvs::dps_volume (csrc/dps_volume.hip) and regresses depth with
dvmvs::dps_regress (csrc/dps_regress.hip); runner: ``python -m dvmvs.baselines.dpsnet``.
"""
