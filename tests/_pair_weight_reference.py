"""float64 reference of the per-pair sample weights of the in-batch softmax (include/twotower.h *_pw entries), on the kernels' operands.

Raw weights w [B]; w' = w with every entry that is not a positive finite number replaced by 0; g_a = w'_a B / sum(w') (all 0 when the
sum is 0).  With R / C the row- / column-direction logits (S, or the logQ-corrected ones) and M the repeated-entity mask (empty
without ids), R' = R.masked_fill(M, -inf), C' likewise:

    l_a  = 0.5 * [(lse_b R'[a, :] - R[a, a]) + (lse_a' C'[:, a] - C[a, a])]
    loss = (1 / B) sum_a g_a l_a                        (= sum w' l / sum w')
    W    = diag(g) softmax(R', 1) + softmax(C', 0) diag(g) - 2 diag(g)
    dN   = inv_t / (2B) * W C,   dC = inv_t / (2B) * W^T N

Operands, mask and logits are tests/_mask_reference.py's; bf16: W is rounded to bf16 after the -2 g term, as the kernels round it.
Works on whatever device its inputs are on.
"""
import numpy as np
import torch

from _mask_reference import L_CLAMP, _bf16, logits, mask_matrix, operands

PATTERNS = ["ones", "random", "edge_zeros", "one_hot", "all_zero", "dirty"]


def clamp_weights(w):
    """w' in f64: the positive finite entries of w, 0 elsewhere"""
    w = w.double()
    return torch.where(torch.isfinite(w) & (w > 0), w, torch.zeros_like(w))


def normalise(w):
    """g = w' B / sum(w') in f64 (all 0 when the sum is 0)"""
    wp = clamp_weights(w)
    s = wp.sum()
    return wp * (wp.shape[0] / s) if s.item() > 0 else torch.zeros_like(wp)


def _mask(B, ent_n, ent_c, device):
    if ent_n is None and ent_c is None:
        return torch.zeros((B, B), dtype=torch.bool, device=device)
    return mask_matrix(ent_n, ent_c)


def row_terms(S, M, lq_n=None, lq_c=None):
    """l [B]: each pair's two softmax terms, halved (differentiable in S)"""
    R, C = logits(S, lq_n, lq_c)
    Rm, Cm = R.masked_fill(M, -float("inf")), C.masked_fill(M, -float("inf"))
    return 0.5 * ((torch.logsumexp(Rm, 1) - R.diagonal()) + (torch.logsumexp(Cm, 0) - C.diagonal()))


def weighted_mean_loss(S, M, w, lq_n=None, lq_c=None):
    """sum(w' l) / sum(w') as autograd sees it (0 when every weight is 0)"""
    wp = clamp_weights(w)
    l = row_terms(S, M, lq_n, lq_c)
    return (wp * l).sum() / wp.sum() if wp.sum().item() > 0 else (0.0 * l).sum()


def reference(n, c, inv_t, w, mode, ent_n=None, ent_c=None, lq_n=None, lq_c=None):
    """f64 weighted loss and (dN, dC) for d_loss = 1 on the kernels' operands, by the closed form"""
    A, Bm, k = operands(n, c, inv_t, mode)
    B = A.shape[0]
    S = (A @ Bm.T) * k
    M = _mask(B, ent_n, ent_c, A.device)
    g = normalise(w.to(A.device))
    loss = (g * row_terms(S, M, lq_n, lq_c)).sum() / B
    R, C = logits(S, lq_n, lq_c)
    W = g[:, None] * torch.softmax(R.masked_fill(M, -float("inf")), 1) + torch.softmax(C.masked_fill(M, -float("inf")), 0) * g[None, :] \
        - 2.0 * torch.diag(g)
    if mode == "bf16":
        W = _bf16(W.float())
    s = inv_t / (2.0 * B)
    An = A * (k / inv_t) if mode == "bf16" else A           # bf16: the notice image carries the unit scale, dC divides it out
    return loss.item(), s * (W @ Bm), s * (W.T @ An)


def ref_sums(n, c, inv_t, mode, ent_n=None, ent_c=None, lq_n=None, lq_c=None):
    """f64 per-row sums as the entries return them -- UNWEIGHTED: rowsum[a] = sum over the unmasked b of exp(s_ab - 1/T) w_b, colsum
    likewise (w = exp(-40 - lq) with the logQ correction, else 1)"""
    A, Bm, k = operands(n, c, inv_t, mode)
    E = torch.exp((A @ Bm.T) * k - abs(inv_t)).masked_fill(_mask(A.shape[0], ent_n, ent_c, A.device), 0.0)
    if lq_n is None:
        return E.sum(1), E.sum(0)
    wn = torch.exp(-L_CLAMP - lq_n.double().clamp(-L_CLAMP, 0.0))
    wc = torch.exp(-L_CLAMP - lq_c.double().clamp(-L_CLAMP, 0.0))
    return E @ wc, E.T @ wn


def weights(B, pattern, seed=0, device="cpu"):
    """f32 [B] raw weights of the named pattern"""
    r = np.random.default_rng(1000 + seed)
    rnd = r.uniform(0.25, 4.0, B)
    if pattern == "ones":
        w = np.ones(B)
    elif pattern == "random":
        w = rnd
    elif pattern == "edge_zeros":                            # zero at the tile edges and the batch's two ends
        w = rnd
        for i in (0, 31, 32, 63, 64, B - 1):
            if 0 <= i < B:
                w[i] = 0.0
    elif pattern == "one_hot":
        w = np.zeros(B)
        w[(2 * B) // 3] = 3.0
    elif pattern == "all_zero":
        w = np.zeros(B)
    elif pattern == "dirty":                                 # negative, NaN and +inf entries act as zeros
        w = rnd
        for i, v in ((0, -1.5), (1, float("nan")), (2, float("inf")), (B - 1, -float("inf")), (B // 2, -0.0)):
            if 0 <= i < B and (B > 3 or i == 0):
                w[i] = v
        if B > 3:
            w[3] = 2.0                                       # (at least one positive weight)
    else:
        raise ValueError(pattern)
    return torch.tensor(w, dtype=torch.float32, device=device)
