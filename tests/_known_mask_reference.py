"""float64 reference of the in-batch softmax with masked cells (include/twotower.h *_cells entries), on the kernels' operands.

cells: int [L, 2] rows (a, j), a in [0, B), j in [0, B + M): j < B in-batch column j, j >= B extra j - B.  Cleaning: cells on the
diagonal (j == a) and cells outside the ranges are dropped, duplicates collapse.  With Omega the cleaned set and R, Rx, C the row,
extras and column logits of tests/_xneg_reference.py:

    R', Rx' = R, Rx with Omega's cells at -inf;   C' = C with the cells (a, b) of Omega, b < B, at -inf
    loss = 0.5 * [mean_a(lse(R'[a, :] u Rx'[a, :]) - R[a, a]) + mean_b(lse_a C'[:, b] - C[b, b])]
    W  = softmax over the B + M row entries (first B columns) + softmax(C', 0) - 2 I,   Wx = that row softmax's last M columns
    dN = g (W C + Wx X),   dC = g W^T N,   dX = g Wx^T N,   g = (1/T) / (2B)

The positive is never masked, so no sum is empty.  `mode` as tests/_xneg_reference.py: "bf16" rounds the operands and the weights the
kernels' way.  M = 0: x is None (or an empty [0, D] tensor) and dX comes back as None.
"""
import numpy as np
import torch

import _xneg_reference as XR
from _mask_reference import L_CLAMP, _bf16  # noqa: F401


def clean_cells(cells, B, M):
    """Omega as a sorted int64 numpy array [K, 2] of distinct in-range off-diagonal cells"""
    c = np.asarray(cells.cpu() if isinstance(cells, torch.Tensor) else cells, dtype=np.int64).reshape(-1, 2)
    ok = (c[:, 0] >= 0) & (c[:, 0] < B) & (c[:, 1] >= 0) & (c[:, 1] < B + M) & (c[:, 1] != c[:, 0])
    c = c[ok]
    return np.unique(c, axis=0) if len(c) else c


def cell_masks(cells, B, M, device):
    """(Min bool [B, B], Mx bool [B, M]) of Omega"""
    om = clean_cells(cells, B, M)
    full = torch.zeros((B, B + M), dtype=torch.bool)
    if len(om):
        full[torch.as_tensor(om[:, 0]), torch.as_tensor(om[:, 1])] = True
    full = full.to(device)
    return full[:, :B].contiguous(), full[:, B:].contiguous()


def _x(n, x):
    return x if x is not None else torch.zeros((0, n.shape[1]), dtype=n.dtype, device=n.device)


def _parts(n, c, x, cells, inv_t, mode, lq_n, lq_c, lq_x):
    S, Z, R, C, Rx, _, _, A, Bm, Xm, k = XR.parts(n, c, _x(n, x), inv_t, mode, None, None, None, lq_n, lq_c, lq_x)
    Min, Mx = cell_masks(cells, A.shape[0], Xm.shape[0], A.device)
    return S, Z, R, C, Rx, Min, Mx, A, Bm, Xm, k


def reference(n, c, x, cells, inv_t, mode, lq_n=None, lq_c=None, lq_x=None):
    """f64 loss and (dN, dC, dX) for d_loss = 1 by the closed form; dX None when x is None"""
    S, Z, R, C, Rx, Min, Mx, A, Bm, Xm, k = _parts(n, c, x, cells, inv_t, mode, lq_n, lq_c, lq_x)
    B = A.shape[0]
    loss = XR.xneg_loss(S, Z, Min, Mx, lq_n, lq_c, lq_x)
    W, Wx = XR.weights(R, C, Rx, Min, Mx)
    if mode == "bf16":
        W, Wx = _bf16(W.float()), _bf16(Wx.float())
    g = inv_t / (2.0 * B)
    Ag = A * (k / inv_t) if mode == "bf16" else A            # the notice image carries the unit scale: dC and dX divide it out
    return loss.item(), g * (W @ Bm + Wx @ Xm), g * (W.T @ Ag), (g * (Wx.T @ Ag)) if x is not None else None


def ref_rowsum(n, c, x, cells, inv_t, mode, lq_n=None, lq_c=None, lq_x=None):
    """f64 row sums as the entries return them: sum over the unmasked b and m of exp(s - 1/T) w (w = exp(-40 - q) with logQ, else 1)"""
    S, Z, R, C, Rx, Min, Mx, A, Bm, Xm, k = _parts(n, c, x, cells, inv_t, mode, lq_n, lq_c, lq_x)
    off = abs(inv_t) + (L_CLAMP if lq_n is not None else 0.0)
    return torch.exp(R - off).masked_fill(Min, 0.0).sum(1) + torch.exp(Rx - off).masked_fill(Mx, 0.0).sum(1)


def autograd_reference(n, c, x, cells, inv_t, lq_n=None, lq_c=None, lq_x=None):
    """(loss, dN, dC, dX) by f64 autograd of masked_fill + logsumexp on the concatenated logits, written out on its own (f32-exact
    operands: mode "fp32" of `reference`)"""
    B, D = n.shape
    nd, cd = n.double().clone().requires_grad_(True), c.double().clone().requires_grad_(True)
    xd = _x(n, x).double().clone().requires_grad_(True)
    M = xd.shape[0]
    Min, Mx = cell_masks(cells, B, M, n.device)
    q = lambda t, m: torch.zeros(m, dtype=torch.float64, device=n.device) if t is None else t.double().clamp(-40.0, 0.0)
    on = lq_n is not None
    S, Z = (nd @ cd.T) * inv_t, (nd @ xd.T) * inv_t
    R = S - (q(lq_c, B)[None, :] if on else 0.0)
    Cc = S - (q(lq_n, B)[:, None] if on else 0.0)
    Rx = Z - (q(lq_x, M)[None, :] if on else 0.0)
    ninf = -float("inf")
    rows = torch.cat([R.masked_fill(Min, ninf), Rx.masked_fill(Mx, ninf)], 1)
    loss = 0.5 * ((torch.logsumexp(rows, 1) - R.diagonal()).mean() + (torch.logsumexp(Cc.masked_fill(Min, ninf), 0) - Cc.diagonal()).mean())
    loss.backward()
    return loss.item(), nd.grad, cd.grad, xd.grad if x is not None else None


def entity_cells(ent_n, ent_c, ent_x=None):
    """the cells the repeated-entity mask stands for: (a, b), a != b, rows sharing a notice or a company id; (a, B + m) where extra
    m carries row a's company id"""
    en, ec = np.asarray(ent_n.cpu()), np.asarray(ent_c.cpu())
    B = len(en)
    m = (en[:, None] == en[None, :]) | (ec[:, None] == ec[None, :])
    np.fill_diagonal(m, False)
    out = [np.argwhere(m)]
    if ent_x is not None:
        mx = ec[:, None] == np.asarray(ent_x.cpu())[None, :]
        ax = np.argwhere(mx)
        ax[:, 1] += B
        out.append(ax)
    return np.concatenate(out, 0).astype(np.int64)


def brute_cells(sel, extras, known, m):
    """the loader's cells of one batch by set membership: sel int [m, 2] the batch's (notice, company) rows, extras int [M] company rows
    (or None), known a set of (notice, company) tuples -> sorted list of (a, j), j != a"""
    cols = [int(v) for v in sel[:, 1]] + ([int(v) for v in extras] if extras is not None else [])
    out = []
    for a in range(m):
        for j, comp in enumerate(cols):
            if j != a and (int(sel[a, 0]), comp) in known:
                out.append((a, j))
    return sorted(out)
