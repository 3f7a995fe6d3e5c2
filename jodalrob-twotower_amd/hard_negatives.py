"""Hard-negative mining under a positive-aware score ceiling -- the loop that joins the catalogue sweep to the shared extra negatives.

The rows that outscore a notice's known company are mostly unlabelled positives (companies that would have been right and that the
data does not record), and a shared extra negative enters the row softmax of every notice of its batch.  So the miner does not
take a notice's top-k: it takes the k best rows BELOW a ceiling formed from the notice's own positives ("TopK-PercPos" of the
NV-Retriever study), with every known company of the notice excluded, and keeps `per_notice` of them -- the first ones, or a
uniform draw among them (the ANCE rule).

    mined = mine_hard_negatives(task, notice_store, company_store, pairs, k=64, per_notice=8, ceiling=(0.95, 0.0))
    loader = DevicePairLoader(notice_store, company_store, pairs, B, shuffle=True, extra_negatives=1024, mined=mined)

The ceiling is applied inside the sweep (CatalogIndex.search(max_score=), tt_ceil_retrieve_topk_*), so all k slots go to rows under
it, and it is formed from CatalogIndex.pair_scores: the positives' scores bit for bit as the sweep computes them.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from .retrieval import MAX_K, CatalogIndex, exclusions_from_pairs


@dataclass
class MinedNegatives:
    """table int32 [len(notice_store), per_notice]: row i holds the company rows mined for notice i, -1 for a notice without pairs
    and for the slots the sweep could not fill; beside it the parameters of the mining pass."""
    table: torch.Tensor
    k: int
    per_notice: int
    ceiling: Optional[Tuple[float, float]]
    select: str
    seed: int


def select_mined(idx: torch.Tensor, per_notice: int, select: str, generator=None) -> torch.Tensor:
    """per_notice of a search's k slots idx int64 [n, k] (-1: empty, only at the end of a row) -> int32 [n, per_notice].  'top': the
    first per_notice.  'uniform': a uniform draw without replacement among the row's valid slots (one random key per slot from
    `generator`, the per_notice smallest win), -1 beyond the number of valid slots."""
    if select == "top":
        return idx[:, :per_notice].to(torch.int32)
    key = torch.rand(idx.shape, generator=generator, device=idx.device)
    key = torch.where(idx >= 0, key, torch.full_like(key, 2.0))
    pick = torch.argsort(key, dim=1, stable=True)[:, :per_notice]
    return idx.gather(1, pick).to(torch.int32)


@torch.no_grad()
def mine_hard_negatives(model, notice_store, company_store, pairs, k: int = 64, per_notice: int = 8,
                        ceiling: Optional[Tuple[float, float]] = (0.95, 0.0), select: str = "top", chunk: int = 8192, seed: int = 0,
                        index: Optional[CatalogIndex] = None) -> MinedNegatives:
    """Mines per_notice hard negatives for every notice of `pairs` [P, 2] (notice row, company row) with the current weights.

    The unique notices are embedded in eval mode, `chunk` at a time (the modules' train / eval state is restored), and searched
    against `index` (default: CatalogIndex.from_store(model, company_store)).  Per notice: every known company of it is excluded;
    s_min is the lowest score of its positives (pair_scores: the sweep's own bits); the k best rows with a score below
        ceil = alpha * s_min + beta,      ceiling = (alpha, beta)
    are searched (ceiling=None: no ceiling), and per_notice of them kept -- select='top': the best ones; 'uniform': a uniform draw
    without replacement among the valid ones, from a generator seeded with `seed`.
    alpha < 1 lowers the ceiling only for a positive score: for s_min < 0, alpha * s_min lies ABOVE s_min, and rows that outscore
    the positive pass.  Scores here are cosines / T of trained towers, where a known positive below zero is rare; a margin that
    holds for either sign is beta < 0 with alpha = 1.
    `model` is a TwoTowerTrainTask or a TwoTowerModel, as in CatalogIndex.from_store.  One host synchronisation per chunk, inside
    exclusions_from_pairs."""
    k, per_notice, chunk, seed = int(k), int(per_notice), int(chunk), int(seed)
    if select not in ("top", "uniform"):
        raise ValueError(f"select must be 'top' or 'uniform', got {select!r}")
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    nC = len(company_store) if index is None else len(index)
    if not 1 <= k <= min(MAX_K, nC):
        raise ValueError(f"k must be in [1, min({MAX_K}, catalogue size {nC})], got {k}")
    if not 1 <= per_notice <= k:
        raise ValueError(f"per_notice must be in [1, k = {k}], got {per_notice}")
    if ceiling is not None:
        if not isinstance(ceiling, (tuple, list)) or len(ceiling) != 2:
            raise ValueError("ceiling must be None or an (alpha, beta) pair")
        ceiling = (float(ceiling[0]), float(ceiling[1]))
    dev = torch.device(notice_store.device)
    pairs = torch.as_tensor(pairs).to(device=dev, dtype=torch.int64)
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs must be a [P, 2] array of (notice row, company row) rows")
    if pairs.shape[0] and (int(pairs[:, 0].min()) < 0 or int(pairs[:, 0].max()) >= len(notice_store)):
        raise KeyError("pair refers to a notice that is not in the feature store")
    if index is None:
        index = CatalogIndex.from_store(model, company_store, chunk)
    table = torch.full((len(notice_store), per_notice), -1, dtype=torch.int32, device=dev)
    out = MinedNegatives(table, k, per_notice, ceiling, select, seed)
    if pairs.shape[0] == 0:
        return out
    up = torch.unique(pairs, dim=0)                                         # sorted by (notice, company)
    notices = torch.unique(up[:, 0])
    starts = list(range(0, notices.numel(), chunk))
    # the chunks' slices of the sorted pair list, found once for the whole pass
    cut = torch.searchsorted(up[:, 0].contiguous(), notices[torch.tensor(starts, device=dev)]).tolist() + [up.shape[0]]
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    tower_model = model.two_tower_model if hasattr(model, "two_tower_model") else model
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        for j, s in enumerate(starts):
            keys = notices[s:s + chunk]
            Q = tower_model.get_notice_embeddings(notice_store.gather(keys.contiguous())).detach().float()
            off, rows = exclusions_from_pairs(keys, up[cut[j]:cut[j + 1]], len(index))
            ceil = None
            if ceiling is not None:
                n = rows.numel()                                            # entry e of the lists is a pair of notice q_of[e]
                q_of = torch.searchsorted(off[1:], torch.arange(n, dtype=torch.int64, device=dev), right=True)
                s_pos = index.pair_scores(Q[q_of], rows)
                s_min = torch.full((keys.numel(),), float("inf"), dtype=torch.float32, device=dev)
                s_min.scatter_reduce_(0, q_of, s_pos, "amin")
                ceil = ceiling[0] * s_min + ceiling[1]
            _, idx = index.search(Q, k, exclude=(off, rows), max_score=ceil)
            table[keys] = select_mined(idx, per_notice, select, gen)
    finally:
        for m, was in modes:
            m.training = was
    return out
