"""The optional batch entries that change the loss -- ONE table: what the score node has a form of and what combines (the node decides
with it), and per batch entry where it lives, what it is called in a refusal and what its arrays look like (the task's validator
`TwoTowerTrainTask._batch_terms` and the captured step `graph.GraphedTrainStep` walk it).  A new term is a row here."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import torch

# ---- what combines ------------------------------------------------------------------------------------------------------------------
_TERM_FORMS = {"cells": ("bf16",), "extras": ("fp32", "bf16"), "ent": ("fp32", "bf16"), "pw": ("fp32", "bf16"),
               "lq": ("fp32", "bf16", "bf16x3")}                      # term -> the score_dtypes that have a form of it
_TERM_CLASHES = frozenset({frozenset({"cells", "ent"}), frozenset({"cells", "pw"}), frozenset({"extras", "pw"})})
_CLASH_WHY = {frozenset({"cells", "ent"}): ": cells built from the pair table already hold every repeat"}


def _terms_clash(a, b):
    return frozenset({a, b}) in _TERM_CLASHES


# ---- the batch entries, in the order they are decided -------------------------------------------------------------------------------
SIDES = ("notice", "company")


class Term(NamedTuple):
    key: str                       # the batch key
    where: str                     # "side": batch[side][key], either or both; "top": batch[key]; "nested": batch[key] is a dict
    term: str                      # its name in _TERM_FORMS
    noun: str                      # "<noun> (a batch with '<key>') <verb> not supported ..."
    verb: str
    thing: str                     # "... mismatch: the step was captured with <thing>, the batch carries <pron>"
    pron: str
    store_says: tuple              # step_from_store's words for ("... none", "... <pron>")
    dtype: Optional[torch.dtype]   # of its arrays (None: no array of its own)
    shape: tuple                   # "B": the batch size; another name: a free length
    missing: Optional[str]         # a side the batch does not carry stands for "zeros", its "rows" (row indices), or nothing
    eval_why: Optional[str]        # why forward_with_ranks refuses it (None: it does not)

    @property
    def phrase(self):
        return f"{self.noun} (a batch with '{self.key}')"

    @functools.lru_cache(maxsize=None)
    def names(self, owner):
        """what the array check calls its arrays: in the task's batch, or as a captured step's arguments (formed once)"""
        if self.where == "side":
            return tuple(f"batch['{s}']['{self.key}']" if owner == "the batch" else f"{s} {self.key}" for s in SIDES)
        return (f"batch['{self.key}']" if owner == "the batch" else self.key,)

    def of(self, batch):
        """the batch's entry (per side: the (notice, company) pair), or None when the batch carries none"""
        if self.where != "side":
            return batch.get(self.key)
        v = tuple(batch[s].get(self.key) for s in SIDES)
        return None if v[0] is None and v[1] is None else v

    def dims(self, B):
        return tuple(B if d == "B" else d for d in self.shape)

    def fill(self, B, dev):
        """what a missing side stands for, as a [B] array"""
        return (torch.zeros if self.missing == "zeros" else torch.arange)(B, dtype=self.dtype, device=dev)


_GOT, _HAS = ("got", "got"), ("has", "carries")
TABLE = (
    Term("log_q", "side", "lq", "the logQ correction", "is", "a log_q", "one", _GOT, torch.float32, ("B",), "zeros", None),
    Term("entity", "side", "ent", "the repeated-entity mask", "is", "entity ids", "them", _GOT, torch.int32, ("B",), "rows", None),
    Term("pair_weight", "top", "pw", "pair weights", "are", "pair weights", "them", _HAS, torch.float32, ("B",), None,
         "evaluation is unweighted"),
    Term("negatives", "nested", "extras", "extra negatives", "are", "extra negatives", "them", _HAS, None, ("M",), None,
         "evaluation ranks the batch's own companies"),
    Term("masked_cells", "top", "cells", "masked cells", "are", "masked cells", "them", _HAS, torch.int32, ("L", 2), None,
         "evaluation filters with exclusion lists"),
)
ROWS = {row.key: row for row in TABLE}
B_TERMS = tuple(row for row in TABLE if row.shape == ("B",))          # one [B] array per side, or one


def present(batch):
    """the keys of the entries `batch` carries"""
    return frozenset(row.key for row in TABLE if row.of(batch) is not None)


def check(t, name, dtype, shape, dev, owner, a=None):
    """t is a `dtype` tensor of `shape` (a name in it: any length) on `dev`, or ValueError; owner: whose device that is.  (a: the
    article, where a text has its own)"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != len(shape) or \
            any(not isinstance(d, str) and t.shape[i] != d for i, d in enumerate(shape)):
        word = str(dtype).replace("torch.", "")
        raise ValueError(f"{name} must be {a or ('an' if word[0] in 'aeiou' else 'a')} {word} tensor of shape [{', '.join(map(str, shape))}], got "
                         f"{getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', []))}")
    if t.device != dev:
        raise ValueError(f"{name} is on {t.device}, {owner} on {dev}")
    return t


def mismatch(row, captured, who="the batch"):
    """a step captured with (captured) / without the entry was handed the opposite by `who` ("the batch" or "step_from_store")"""
    none, some = _HAS if who == "the batch" else row.store_says
    return (f"{row.key} mismatch: the step was captured " + ("with" if captured else "without") + f" {row.thing}, {who} "
            + (f"{none} none" if captured else f"{some} {row.pron}"))


def segment(dst, src):
    """[(dst, src)] for the hand-over's copy launch, which moves 16-byte pieces -- or, where either is not 16-byte aligned (a slice
    of an epoch's array), the copy at once and no segment"""
    src = src.contiguous()
    if src.data_ptr() % 16 or dst.data_ptr() % 16:
        dst.copy_(src, non_blocking=True)
        return []
    return [(dst, src)]
