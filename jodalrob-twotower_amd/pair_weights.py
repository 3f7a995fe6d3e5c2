"""Per-pair sample weights for the weighted in-batch softmax (TFRS sample_weight; include/twotower.h *_pw entries).

A batch may carry batch["pair_weight"], f32 [B]: the train task then takes the weighted mean of the pairs' loss terms.  The helper
here builds the weights that make every notice (or company) count once however many pairs it has -- the natural partner of the
repeated-entity mask on a table where one notice has many bidders.
"""
from __future__ import annotations

import numpy as np
import torch


def inverse_count_weights(pairs, side: str = "notice") -> torch.Tensor:
    """f32 [P]: 1 / (number of rows of the pair table `pairs` [P, 2] that share this row's notice (side="notice", column 0) or
    company (side="company", column 1)).  Returned on pairs' device (a numpy array gives a CPU tensor); a tensor on a device is
    counted on the host, as sampling_bias.log_sampling_probs counts."""
    if side not in ("notice", "company"):
        raise ValueError(f"side must be 'notice' or 'company', got {side!r}")
    dev = pairs.device if isinstance(pairs, torch.Tensor) else torch.device("cpu")
    idx = pairs.detach().to("cpu").numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    if idx.ndim != 2 or idx.shape[1] != 2:
        raise ValueError(f"pairs must have shape [P, 2], got {list(idx.shape)}")
    if not np.issubdtype(idx.dtype, np.integer):
        raise TypeError(f"pairs must hold integers, got {idx.dtype}")
    col = idx[:, 0 if side == "notice" else 1]
    if col.size and col.min() < 0:
        raise ValueError("pairs holds a negative index")
    _, inverse, counts = np.unique(col, return_inverse=True, return_counts=True)
    w = 1.0 / counts[inverse.reshape(-1)].astype(np.float64)
    return torch.from_numpy(w.astype(np.float32)).to(dev)
