from dvmvs.baselines.networks import Encoder  # noqa: F401
