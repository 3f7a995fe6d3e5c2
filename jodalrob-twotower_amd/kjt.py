"""Minimal id container with the slice of the torchrec.KeyedJaggedTensor interface the reference's
hot path uses (src/towers/cat_embed.py:92-94, src/towers/tower/base_tower.py:130,
scripts/train.py:269-272): keys() / values() / lengths() / to() / device() / pin_memory().

values(): int64 [B*K], SAMPLE-major (categorical_data.flatten() of a [B,K] matrix --
src/towers/pairs/unified_bid_data_loader.py:834); lengths(): ones [B*K] (:835).
A real torchrec KJT is accepted everywhere this class is: only these methods are called.
"""
from __future__ import annotations

from typing import List

import torch


class KeyedJaggedTensor:
    def __init__(self, keys: List[str], values: torch.Tensor, lengths: torch.Tensor | None = None):
        self._keys = list(keys)
        self._values = values
        self._lengths = lengths
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

    def to(self, device, non_blocking: bool = False) -> "KeyedJaggedTensor":
        lengths = None if self._lengths is None else self._lengths.to(device, non_blocking=non_blocking)
        out = KeyedJaggedTensor(self._keys, self._values.to(device, non_blocking=non_blocking), lengths)
        out.bag_count = None if self.bag_count is None else self.bag_count.to(device, non_blocking=non_blocking)
        return out

    def device(self) -> torch.device:
        return self._values.device

    def pin_memory(self) -> "KeyedJaggedTensor":
        lengths = None if self._lengths is None else self._lengths.pin_memory()
        return KeyedJaggedTensor(self._keys, self._values.pin_memory(), lengths)

    def __repr__(self):
        return f"KeyedJaggedTensor(keys={len(self._keys)}, values={tuple(self._values.shape)}, device={self._values.device})"


def build_bag_kjt(categorical_keys: List[str], bags=None, values: torch.Tensor | None = None,
                  lengths: torch.Tensor | None = None, device=None) -> KeyedJaggedTensor:
    """A KJT of multi-valued features in the sample-major wire format: lengths()[b*K + k] = length of bag (b, k) (0 allowed),
    values() = all bags' ids concatenated in that slot order.  Either `bags` -- per sample, per key, the list of ids
    (bags[b][k]) -- or a (values [nnz], lengths [B*K]) pair.  With every length 1 this is build_batch_kjt's format."""
    K = len(categorical_keys)
    if (bags is None) == (values is None or lengths is None):
        raise ValueError("build_bag_kjt takes either `bags` or both `values` and `lengths`")
    if bags is not None:
        if any(len(row) != K for row in bags):
            raise ValueError(f"every sample needs one id list per key ({K} keys)")
        lengths = torch.tensor([len(bag) for row in bags for bag in row], dtype=torch.long)
        values = torch.tensor([int(i) for row in bags for bag in row for i in bag], dtype=torch.long)
    else:
        values, lengths = values.reshape(-1).to(torch.long), lengths.reshape(-1).to(torch.long)
        if K == 0 or lengths.numel() % K != 0:
            raise ValueError(f"{lengths.numel()} bag lengths do not divide into {K} keys")
    if device is not None:
        values, lengths = values.to(device), lengths.to(device)
    return KeyedJaggedTensor(categorical_keys, values, lengths)


def concat_kjt(a: KeyedJaggedTensor, b: KeyedJaggedTensor) -> KeyedJaggedTensor:
    """The samples of `a` followed by the samples of `b` (same keys): values and lengths are both sample-major, so both
    concatenate as they are."""
    if list(a.keys()) != list(b.keys()):
        raise ValueError("concat_kjt needs two KJTs over the same keys")
    return KeyedJaggedTensor(list(a.keys()), torch.cat([a.values(), b.values().to(a.values().device)]),
                             torch.cat([a.lengths(), b.lengths().to(a.lengths().device)]))


def build_batch_kjt(categorical_data: torch.Tensor, categorical_keys: List[str]) -> KeyedJaggedTensor:
    """[B,K] ids -> KJT, the wire format of _build_batch_kjt (unified_bid_data_loader.py:827-841)."""
    b, k = categorical_data.shape
    values = categorical_data.reshape(-1).to(torch.long)
    return KeyedJaggedTensor(categorical_keys, values,
                             torch.ones(b * k, dtype=torch.long, device=categorical_data.device))
