"""Training on the device: mirrors Payne/train (``trainphot``: the photometric LayerNorm + SiLU networks; ``trainspec``: the spectral networks SMLP and LinNet)."""
