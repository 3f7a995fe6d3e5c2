"""Log sampling probabilities for the logQ-corrected in-batch softmax (Yi et al., RecSys 2019; include/twotower.h *_lq entries).

A training batch is a uniform draw from a fixed pair list, so the probability that entity j enters a batch as one of its B
slots is exactly its share of the pairs, q_j = count_j / P: the marginal below is the exact sampling probability here, not an
estimate.  (The paper's streaming, hashed frequency estimator is for unbounded streams whose counts are not known up front; it is
not needed and not provided.)
"""
from __future__ import annotations

import numpy as np
import torch


def log_sampling_probs(entity_idx, n_entities: int) -> torch.Tensor:
    """f32 [n_entities]: log(count_j / P) for the P training pairs' entity indices `entity_idx` (one side of the pair list:
    notices or companies).  An entity with no pair gets log(1 / P), as if it had one.  Returned on entity_idx's device (a
    numpy array gives a CPU tensor)."""
    n_entities = int(n_entities)
    if n_entities < 1:
        raise ValueError(f"n_entities must be >= 1, got {n_entities}")
    dev = entity_idx.device if isinstance(entity_idx, torch.Tensor) else torch.device("cpu")
    idx = entity_idx.detach().to("cpu").numpy() if isinstance(entity_idx, torch.Tensor) else np.asarray(entity_idx)
    idx = idx.reshape(-1)
    if idx.size == 0:
        raise ValueError("log_sampling_probs needs at least one pair")
    if not np.issubdtype(idx.dtype, np.integer):
        raise TypeError(f"entity_idx must hold integers, got {idx.dtype}")
    if idx.min() < 0 or idx.max() >= n_entities:
        raise ValueError(f"entity index out of range [0, {n_entities})")
    counts = np.bincount(idx.astype(np.int64), minlength=n_entities).astype(np.float64)
    lq = np.log(np.maximum(counts, 1.0) / float(idx.size))
    return torch.from_numpy(lq.astype(np.float32)).to(dev)
