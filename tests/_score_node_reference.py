"""float64 reference of the WHOLE score node (two_tower_train_task._ScoreCEFn): every optional term of the in-batch softmax at once, on
the kernels' operands.  Built from the pieces the term references share (tests/_mask_reference.py, _xneg_reference.py,
_known_mask_reference.py, _pair_weight_reference.py); works on whatever device its inputs are on.

N [B, D], C [B, D] and the extras X [M, D] are unit rows.  S = N C^T / T, Z = N X^T / T; q = log q clamped to [-40, 0] (0 where a vector
is missing while the batch is corrected); row logits R[a, b] = S[a, b] - qc[b] and Rx[a, m] = Z[a, m] - qx[m], column logits
C[a, b] = S[a, b] - qn[a].  Masks: Min = the repeated-entity mask (a side without ids is all-distinct) or-ed with the cells (a, j), j < B;
Mx = (ent_x[m] == ent_c[a]) or-ed with the cells (a, B + m).  g = the normalised pair weights, or ones.  R', Rx', C' = the logits with the
masked entries at -inf, P = the row softmax over the B + M entries:

    loss = (1/B) sum_a g_a * 0.5 * [(lse(R'[a, :] u Rx'[a, :]) - R[a, a]) + (lse C'[:, a] - C[a, a])]
    W    = diag(g) P[:, :B] + softmax(C', 0) diag(g) - 2 diag(g),   Wx = diag(g) P[:, B:]
    dN   = y (W Bm + Wx Xm),   dC = y W^T A,   dX = y Wx^T A,   y = (1/T) / (2B)
    rowsum[a] = sum over the unmasked b and m of exp(s - 1/T) w,   colsum[b] = sum over the unmasked a of exp(s_ab - 1/T) w_a
                (w = exp(-40 - q) with the logQ correction, else 1: the entries' convention -- never weighted by g)

Modes: "fp32" -- the f32 values themselves; "bf16" -- the notice image holds bf16(unit_scale * n), the others bf16(c) / bf16(x), W and Wx
are rounded to bf16 after the -2 g term, the products run on the images and dC / dX divide the notice image's unit scale out; "bf16x3" --
every operand is hi + lo, hi = bf16(v), lo = bf16(v - hi) (tests/test_gpu_logq.py's split), weights unrounded.
"""
import torch

from _known_mask_reference import cell_masks
from _mask_reference import L_CLAMP, _bf16, logits, mask_matrix, operands
from _pair_weight_reference import normalise
from _xneg_reference import x_mask, x_operand

NINF = -float("inf")


def _split(v):
    hi = v.to(torch.bfloat16).float()
    return hi.double() + (v - hi).to(torch.bfloat16).double()


def node_operands(n, c, x, inv_t, mode):
    """(A, Bm, Xm, k): the f64 operands the kernels multiply and the factor that turns A Bm^T into s = <n, c> / T; Xm [0, D] without x"""
    if mode == "bf16x3":
        A, Bm, k = _split(n.float()), _split(c.float()), inv_t
        Xm = _split(x.float()) if x is not None else None
    else:
        A, Bm, k = operands(n, c, inv_t, mode)
        Xm = x_operand(x, mode) if x is not None else None
    if Xm is None:
        Xm = torch.zeros((0, A.shape[1]), dtype=torch.float64, device=A.device)
    return A, Bm, Xm, k


def node_masks(B, M, device, ent_n=None, ent_c=None, ent_x=None, cells=None):
    """(Min bool [B, B], Mx bool [B, M])"""
    Min = mask_matrix(ent_n, ent_c) if (ent_n is not None or ent_c is not None) else torch.zeros((B, B), dtype=torch.bool, device=device)
    Mx = x_mask(ent_c, ent_x, B, M, device)
    if cells is not None:
        cin, cx = cell_masks(cells, B, M, device)
        Min, Mx = Min | cin, Mx | cx
    return Min, Mx


def _q(v, R, device):
    return torch.zeros(R, dtype=torch.float64, device=device) if v is None else v.double().clamp(-L_CLAMP, 0.0)


def reference(n, c, inv_t, mode, lq_n=None, lq_c=None, ent_n=None, ent_c=None, pair_w=None, x=None, lq_x=None, ent_x=None, cells=None):
    """(loss, dN, dC, dX, rowsum, colsum) for d_loss = 1 by the closed form; dX None without x"""
    A, Bm, Xm, k = node_operands(n, c, x, inv_t, mode)
    B, M, dev = A.shape[0], Xm.shape[0], A.device
    S, Z = (A @ Bm.T) * k, (A @ Xm.T) * k
    R, C = logits(S, lq_n, lq_c)
    lq = lq_n is not None
    Rx = Z - _q(lq_x, M, dev)[None, :] if lq else Z
    Min, Mx = node_masks(B, M, dev, ent_n, ent_c, ent_x, cells)
    g = normalise(pair_w.to(dev)) if pair_w is not None else torch.ones(B, dtype=torch.float64, device=dev)
    rows = torch.cat([R.masked_fill(Min, NINF), Rx.masked_fill(Mx, NINF)], 1)
    Cm = C.masked_fill(Min, NINF)
    l = 0.5 * ((torch.logsumexp(rows, 1) - R.diagonal()) + (torch.logsumexp(Cm, 0) - C.diagonal()))
    loss = (g * l).sum() / B
    P = torch.softmax(rows, 1)
    W = g[:, None] * P[:, :B] + torch.softmax(Cm, 0) * g[None, :] - 2.0 * torch.diag(g)
    Wx = g[:, None] * P[:, B:]
    if mode == "bf16":
        W, Wx = _bf16(W.float()), _bf16(Wx.float())
    y = inv_t / (2.0 * B)
    Ag = A * (k / inv_t) if mode == "bf16" else A            # the notice image carries the unit scale: dC and dX divide it out
    dN, dC = y * (W @ Bm + Wx @ Xm), y * (W.T @ Ag)
    dX = y * (Wx.T @ Ag) if x is not None else None
    # the entries' sums
    off = abs(inv_t) + (L_CLAMP if lq else 0.0)
    rowsum = torch.exp(R - off).masked_fill(Min, 0.0).sum(1) + torch.exp(Rx - off).masked_fill(Mx, 0.0).sum(1)
    colsum = torch.exp(C - off).masked_fill(Min, 0.0).sum(0)
    return loss.item(), dN, dC, dX, rowsum, colsum


def autograd_reference(n, c, inv_t, lq_n=None, lq_c=None, ent_n=None, ent_c=None, pair_w=None, x=None, lq_x=None, ent_x=None, cells=None):
    """The same six quantities by f64 autograd of masked_fill + logsumexp on the concatenated logits, written out on its own: f32-exact
    operands (mode "fp32" of `reference`), the masks by loops over the ids and the cell list, the weighted mean as sum(w' l) / sum(w')."""
    B, D = n.shape
    dev = n.device
    nd, cd = n.double().clone().requires_grad_(True), c.double().clone().requires_grad_(True)
    xd = (x.double().clone() if x is not None else torch.zeros((0, D), dtype=torch.float64, device=dev)).requires_grad_(True)
    M = xd.shape[0]
    full = torch.zeros((B, B + M), dtype=torch.bool)
    en = None if ent_n is None else ent_n.cpu().tolist()
    ec = None if ent_c is None else ent_c.cpu().tolist()
    ex = None if ent_x is None else ent_x.cpu().tolist()
    for a in range(B):
        for b in range(B):
            if a != b and ((en is not None and en[a] == en[b]) or (ec is not None and ec[a] == ec[b])):
                full[a, b] = True
        if ec is not None and ex is not None:
            for m in range(M):
                if ex[m] == ec[a]:
                    full[a, B + m] = True
    if cells is not None:
        for a, j in (cells.cpu().tolist() if isinstance(cells, torch.Tensor) else [tuple(map(int, r)) for r in cells]):
            if 0 <= a < B and 0 <= j < B + M and j != a:
                full[a, j] = True
    full = full.to(dev)
    Min = full[:, :B]
    on = lq_n is not None
    zero = lambda R: torch.zeros(R, dtype=torch.float64, device=dev)
    qn = lq_n.double().clamp(-40.0, 0.0) if on else zero(B)
    qc = lq_c.double().clamp(-40.0, 0.0) if on else zero(B)
    qx = lq_x.double().clamp(-40.0, 0.0) if (on and lq_x is not None) else zero(M)
    S, Z = (nd @ cd.T) * inv_t, (nd @ xd.T) * inv_t
    rows = torch.cat([S - qc[None, :], Z - qx[None, :]], 1)
    cols = S - qn[:, None]
    l = 0.5 * ((torch.logsumexp(rows.masked_fill(full, NINF), 1) - rows.diagonal()) + (torch.logsumexp(cols.masked_fill(Min, NINF), 0) - cols.diagonal()))
    if pair_w is None:
        loss = l.mean()
    else:
        w = pair_w.double().to(dev)
        w = torch.where(torch.isfinite(w) & (w > 0), w, torch.zeros_like(w))
        loss = (w * l).sum() / w.sum() if w.sum().item() > 0 else (0.0 * l).sum()
    loss.backward()
    with torch.no_grad():
        off = abs(inv_t) + (40.0 if on else 0.0)
        rowsum = torch.exp(rows - off).masked_fill(full, 0.0).sum(1)
        colsum = torch.exp(cols - off).masked_fill(Min, 0.0).sum(0)
    return loss.item(), nd.grad, cd.grad, xd.grad if x is not None else None, rowsum, colsum


def accuracy(n, c, inv_t, mode, x=None, columns=False):
    """the row top-1 rate on the raw scores of the kernels' operands, over the B + M columns (no term moves it: ties count as hits);
    columns: the column top-1 rate of the in-batch scores"""
    A, Bm, Xm, k = node_operands(n, c, None if columns else x, inv_t, mode)
    S = torch.cat([A @ Bm.T, A @ Xm.T], 1) * k
    S = S.T if columns else S
    return float(((S > S.diagonal()[:, None]).sum(1) == 0).double().mean())
