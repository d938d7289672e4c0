"""GP-MVS: Encoder (gpmvs.encoder), Decoder (gpmvs.decoder), GPlayer (gpmvs.gplayer)."""
