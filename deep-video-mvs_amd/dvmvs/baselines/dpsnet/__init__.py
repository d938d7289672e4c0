"""DPSNet baseline: ``dvmvs.baselines.dpsnet.dpsnet.PSNet`` (the reference's module surface) on the fused plane volume and
soft-argmin kernels; runner ``dvmvs.baselines.runner.predict_dpsnet`` / ``python -m dvmvs.baselines.dpsnet``."""
