"""Minimal id container with the slice of the torchrec.KeyedJaggedTensor interface the reference's
hot path uses (src/towers/cat_embed.py:92-94, src/towers/tower/base_tower.py:130,
scripts/train.py:269-272): keys() / values() / lengths() / to() / device() / pin_memory(), and the KJT's third tensor,
weights() / weights_or_none(): one float per id, read by the pooled lookup of a bag-mode embedder alone.

values(): int64 [B*K], SAMPLE-major (categorical_data.flatten() of a [B,K] matrix --
src/towers/pairs/unified_bid_data_loader.py:834); lengths(): ones [B*K] (:835).
A real torchrec KJT is accepted everywhere this class is: only these methods are called.
"""
from __future__ import annotations

import math
from typing import List

import torch


class KeyedJaggedTensor:
    def __init__(self, keys: List[str], values: torch.Tensor, lengths: torch.Tensor | None = None,
                 weights: torch.Tensor | None = None):
        self._keys = list(keys)
        self._values = values
        self._lengths = lengths
        self._weights = weights        # f32 [nnz], one per id in the order of values(), or None: every id weighs 1
        # a captured bag-mode step's static KJT (graph.GraphedTrainStep(bag_capacity=...)): values() is an id buffer of a fixed capacity
        # and bag_count the int32 device word with the number of ids handed over -- the towers then run the pooled lookup's
        # capacity form (ops.BagSide.capacity).  None everywhere else.
        self.bag_count = None

    @classmethod
    def from_lengths_sync(cls, keys, values, lengths):
        return cls(keys, values, lengths)

    def keys(self) -> List[str]:
        return self._keys

    def values(self) -> torch.Tensor:
        return self._values

    def lengths(self) -> torch.Tensor:
        if self._lengths is None:      # all bags have length 1 on this path
            self._lengths = torch.ones(self._values.numel(), dtype=torch.long, device=self._values.device)
        return self._lengths

    def weights(self) -> torch.Tensor:
        if self._weights is None:      # (as torchrec: asking for weights a KJT does not carry is an error)
            raise ValueError("this KeyedJaggedTensor carries no weights (weights_or_none() returns None then)")
        return self._weights

    def weights_or_none(self) -> torch.Tensor | None:
        return self._weights

    def to(self, device, non_blocking: bool = False) -> "KeyedJaggedTensor":
        lengths = None if self._lengths is None else self._lengths.to(device, non_blocking=non_blocking)
        weights = None if self._weights is None else self._weights.to(device, non_blocking=non_blocking)
        out = KeyedJaggedTensor(self._keys, self._values.to(device, non_blocking=non_blocking), lengths, weights)
        out.bag_count = None if self.bag_count is None else self.bag_count.to(device, non_blocking=non_blocking)
        return out

    def device(self) -> torch.device:
        return self._values.device

    def pin_memory(self) -> "KeyedJaggedTensor":
        lengths = None if self._lengths is None else self._lengths.pin_memory()
        weights = None if self._weights is None else self._weights.pin_memory()
        return KeyedJaggedTensor(self._keys, self._values.pin_memory(), lengths, weights)

    def __repr__(self):
        return f"KeyedJaggedTensor(keys={len(self._keys)}, values={tuple(self._values.shape)}, device={self._values.device})"


def build_bag_kjt(categorical_keys: List[str], bags=None, values: torch.Tensor | None = None,
                  lengths: torch.Tensor | None = None, device=None, weights=None) -> KeyedJaggedTensor:
    """A KJT of multi-valued features in the sample-major wire format: lengths()[b*K + k] = length of bag (b, k) (0 allowed),
    values() = all bags' ids concatenated in that slot order.  Either `bags` -- per sample, per key, the list of ids
    (bags[b][k]) -- or a (values [nnz], lengths [B*K]) pair.  With every length 1 this is build_batch_kjt's format.
    weights: one float per id -- a tensor [nnz], or with `bags` per sample, per key, the list of the bag's weights
    (weights[b][k][i] belongs to bags[b][k][i]).  ValueError for another count or shape and for a non-finite value in a list."""
    K = len(categorical_keys)
    if (bags is None) == (values is None or lengths is None):
        raise ValueError("build_bag_kjt takes either `bags` or both `values` and `lengths`")
    if bags is not None:
        if any(len(row) != K for row in bags):
            raise ValueError(f"every sample needs one id list per key ({K} keys)")
        lengths = torch.tensor([len(bag) for row in bags for bag in row], dtype=torch.long)
        values = torch.tensor([int(i) for row in bags for bag in row for i in bag], dtype=torch.long)
        if weights is not None and not isinstance(weights, torch.Tensor):
            if len(weights) != len(bags) or any(not isinstance(wr, (list, tuple)) or len(wr) != K for wr in weights):
                raise ValueError(f"weights must list, per sample, one weight list per key ({len(bags)} samples, {K} keys)")
            for row, wr in zip(bags, weights):
                for bag, wb in zip(row, wr):
                    if not isinstance(wb, (list, tuple)) or len(wb) != len(bag):
                        raise ValueError("every bag needs one weight per id: a weight list does not have its bag's length")
            flat = [float(w) for wr in weights for wb in wr for w in wb]
            if any(not math.isfinite(w) for w in flat):
                raise ValueError("non-finite bag weight")
            weights = torch.tensor(flat, dtype=torch.float32)
    else:
        values, lengths = values.reshape(-1).to(torch.long), lengths.reshape(-1).to(torch.long)
        if K == 0 or lengths.numel() % K != 0:
            raise ValueError(f"{lengths.numel()} bag lengths do not divide into {K} keys")
    if weights is not None:
        if not isinstance(weights, torch.Tensor):
            raise ValueError("with `values` and `lengths` the weights are a tensor [nnz]")
        weights = weights.reshape(-1).to(torch.float32)
        if weights.numel() != values.numel():
            raise ValueError(f"{weights.numel()} weights for {values.numel()} ids")
    if device is not None:
        values, lengths = values.to(device), lengths.to(device)
        weights = None if weights is None else weights.to(device)
    return KeyedJaggedTensor(categorical_keys, values, lengths, weights)


def concat_kjt(a: KeyedJaggedTensor, b: KeyedJaggedTensor) -> KeyedJaggedTensor:
    """The samples of `a` followed by the samples of `b` (same keys): values, lengths and weights are all sample-major, so they
    concatenate as they are.  Where only one operand carries weights the other's ids weigh 1."""
    if list(a.keys()) != list(b.keys()):
        raise ValueError("concat_kjt needs two KJTs over the same keys")
    dev = a.values().device
    wa, wb = (getattr(x, "weights_or_none", lambda: None)() for x in (a, b))
    weights = None
    if wa is not None or wb is not None:
        ones = lambda x: torch.ones(x.values().numel(), dtype=torch.float32, device=dev)
        weights = torch.cat([ones(a) if wa is None else wa.to(device=dev, dtype=torch.float32),
                             ones(b) if wb is None else wb.to(device=dev, dtype=torch.float32)])
    return KeyedJaggedTensor(list(a.keys()), torch.cat([a.values(), b.values().to(dev)]),
                             torch.cat([a.lengths(), b.lengths().to(a.lengths().device)]), weights)


def build_batch_kjt(categorical_data: torch.Tensor, categorical_keys: List[str]) -> KeyedJaggedTensor:
    """[B,K] ids -> KJT, the wire format of _build_batch_kjt (unified_bid_data_loader.py:827-841)."""
    b, k = categorical_data.shape
    values = categorical_data.reshape(-1).to(torch.long)
    return KeyedJaggedTensor(categorical_keys, values,
                             torch.ones(b * k, dtype=torch.long, device=categorical_data.device))
