"""float64 reference of the repeated-entity mask of the in-batch softmax (include/twotower.h *_mask entries), on the kernels' operands.

A pair (a, b), a != b, is masked iff ent_n[a] == ent_n[b] or ent_c[a] == ent_c[b]; with M the mask and R / C the row- / column-direction
logits (S = N C^T / T, or S - lqC[b] / S - lqN[a] with the logQ correction, lq clamped to [-40, 0]):

    loss = 0.5 * [mean_a(lse_b R'[a, :] - R[a, a]) + mean_b(lse_a C'[:, b] - C[b, b])],   R' = R.masked_fill(M, -inf), C' likewise
    W    = softmax(R', 1) + softmax(C', 0) - 2 I,   dN = inv_t / (2B) * W C,   dC = inv_t / (2B) * W^T N

Operand rounding as tests/test_gpu_logq.py's _operands / _reference (restated here so that the file runs without a GPU): bf16 -- the
notice image holds bf16(unit_scale * n), unit_scale = f32(inv_t) * f32(log2 e), the company image bf16(c), the softmax weights are
rounded to bf16 and the gradient products run on the images; fp32 -- the f32 values themselves.  Works on whatever device its inputs
are on.
"""
import numpy as np
import torch

L_CLAMP = 40.0


def unit_scale(inv_t):
    """tt_score_unit_scale: inv_t * log2(e) in f32"""
    return float(np.float32(inv_t) * np.float32(1.4426950408889634))


def _bf16(x):
    return x.to(torch.bfloat16).to(torch.float64)


def operands(n, c, inv_t, mode):
    """(A, Bm, k): the f64 operands the kernels multiply and the factor that turns A Bm^T into s = <n, c> / T"""
    if mode == "bf16":
        sn = unit_scale(inv_t)
        return _bf16(torch.tensor(sn, dtype=torch.float32, device=n.device) * n), _bf16(c), inv_t / sn
    assert mode == "fp32", mode
    return n.double(), c.double(), inv_t


def mask_matrix(ent_n, ent_c):
    """bool [B, B]: True where the pair is masked (never on the diagonal); a side given as None is all-distinct"""
    B = (ent_n if ent_n is not None else ent_c).shape[0]
    dev = (ent_n if ent_n is not None else ent_c).device
    M = torch.zeros((B, B), dtype=torch.bool, device=dev)
    for e in (ent_n, ent_c):
        if e is not None:
            M |= e[:, None] == e[None, :]
    M.fill_diagonal_(False)
    return M


def logits(S, lq_n, lq_c):
    """(R, C): the row- and column-direction logits"""
    if lq_n is None:
        return S, S
    qn = lq_n.double().clamp(-L_CLAMP, 0.0)
    qc = lq_c.double().clamp(-L_CLAMP, 0.0)
    return S - qc[None, :], S - qn[:, None]


def masked_loss(S, M, lq_n=None, lq_c=None):
    """the loss as autograd sees it: masked_fill(-inf) + logsumexp (differentiable in S)"""
    R, C = logits(S, lq_n, lq_c)
    Rm, Cm = R.masked_fill(M, -float("inf")), C.masked_fill(M, -float("inf"))
    return 0.5 * ((torch.logsumexp(Rm, 1) - R.diagonal()).mean() + (torch.logsumexp(Cm, 0) - C.diagonal()).mean())


def reference(n, c, inv_t, ent_n, ent_c, mode, lq_n=None, lq_c=None):
    """f64 masked loss and (dN, dC) for d_loss = 1 on the kernels' operands, by the closed form"""
    A, Bm, k = operands(n, c, inv_t, mode)
    B = A.shape[0]
    S = (A @ Bm.T) * k
    M = mask_matrix(ent_n, ent_c)
    loss = masked_loss(S, M, lq_n, lq_c)
    R, C = logits(S, lq_n, lq_c)
    W = torch.softmax(R.masked_fill(M, -float("inf")), 1) + torch.softmax(C.masked_fill(M, -float("inf")), 0) \
        - 2.0 * torch.eye(B, dtype=torch.float64, device=A.device)
    if mode == "bf16":
        W = _bf16(W.float())
    g = inv_t / (2.0 * B)
    if mode == "bf16":
        Ag = A * (k / inv_t)                                 # the notice image carries the unit scale: dC divides it out
        return loss.item(), g * (W @ Bm), g * (W.T @ Ag)
    return loss.item(), g * (W @ Bm), g * (W.T @ A)


def ref_sums(n, c, inv_t, ent_n, ent_c, mode, lq_n=None, lq_c=None):
    """f64 per-row masked sums as the entries return them: rowsum[a] = sum over the unmasked b of exp(s_ab - 1/T) w_b, colsum likewise
    (w = exp(-40 - lq) with the logQ correction, else 1)"""
    A, Bm, k = operands(n, c, inv_t, mode)
    E = torch.exp((A @ Bm.T) * k - abs(inv_t)).masked_fill(mask_matrix(ent_n, ent_c), 0.0)
    if lq_n is None:
        return E.sum(1), E.sum(0)
    wn = torch.exp(-L_CLAMP - lq_n.double().clamp(-L_CLAMP, 0.0))
    wc = torch.exp(-L_CLAMP - lq_c.double().clamp(-L_CLAMP, 0.0))
    return E @ wc, E.T @ wn


def ids(B, pattern, seed=0, device="cpu"):
    """(ent_n, ent_c) int32 [B] of the named pattern"""
    g = np.random.default_rng(seed)
    en, ec = np.arange(B, dtype=np.int64), np.arange(B, dtype=np.int64) + 7 * B
    if pattern == "distinct":
        pass
    elif pattern == "one_notice":                            # every off-diagonal pair masked
        en[:] = 5
    elif pattern == "tile_edge":                             # pairs across the 32-row tile edges and the batch's two ends
        for a, b in ((31, 32), (63, 64)):
            if b < B:
                en[b] = en[a]
        if B > 1:
            en[0] = en[B - 1]                                # (row 0 joins the last row's notice: B - 1 may be 32 or 64 itself)
        if B > 33:
            ec[33] = ec[32]
    elif pattern == "groups":
        en = g.integers(0, max(B // 4, 1), B)
        ec = g.integers(0, max(B // 3, 1), B)
    elif pattern == "heavy":                                 # half the rows share one notice
        en[g.permutation(B)[:B // 2]] = -3
    else:
        raise ValueError(pattern)
    return (torch.tensor(en, dtype=torch.int32, device=device), torch.tensor(ec, dtype=torch.int32, device=device))
