"""MVDepthNet: Encoder (mvdepthnet.encoder), Decoder (mvdepthnet.decoder)."""
