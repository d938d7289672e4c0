from dvmvs.baselines.networks import Decoder  # noqa: F401
