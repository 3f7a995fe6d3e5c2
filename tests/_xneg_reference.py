"""float64 reference of the in-batch softmax with shared extra negatives (include/twotower.h *_xneg entries), on the kernels' operands.

N [B, D], C [B, D] and the extras X [M, D] are unit rows.  S = N C^T / T, Z = N X^T / T; row-direction logits R[a, b] = S[a, b] - qc[b]
and Rx[a, m] = Z[a, m] - qx[m], column-direction logits C[a, b] = S[a, b] - qn[a] (q = log q clamped to [-40, 0], or 0).  The extras have
no positive and stand in no column sum.  Mask: the in-batch pairs as tests/_mask_reference.py; extra m is masked for row a iff
ent_x[m] == ent_c[a].

    loss = 0.5 * [mean_a(lse(R'[a, :] u Rx'[a, :]) - R[a, a]) + mean_b(lse_a C'[:, b] - C[b, b])]
    W  = softmax over the B + M row entries (first B columns) + softmax(C', 0) - 2 I,   Wx = that row softmax's last M columns
    dN = g (W C + Wx X),   dC = g W^T N,   dX = g Wx^T N,   g = (1/T) / (2B)

bf16 mode: W and Wx are rounded to bf16 before the products (the kernels round their second MFMA operand), the products run on the
images, and dC / dX divide the notice image's unit scale out.  The extras' image is bf16(x), unscaled.
"""
import torch

from _mask_reference import L_CLAMP, _bf16, logits, mask_matrix, operands


def x_operand(x, mode):
    return _bf16(x) if mode == "bf16" else x.double()


def x_mask(ent_c, ent_x, B, M, device):
    """bool [B, M]: True where extra m is masked for row a; no ids on either side: nothing is"""
    if ent_c is None or ent_x is None:
        return torch.zeros((B, M), dtype=torch.bool, device=device)
    return ent_c[:, None] == ent_x[None, :]


def parts(n, c, x, inv_t, mode, ent_n=None, ent_c=None, ent_x=None, lq_n=None, lq_c=None, lq_x=None):
    """(S, Z, R, C, Rx, Min, Mx, A, Bm, Xm, k): scores, logits and masks on the kernels' operands"""
    A, Bm, k = operands(n, c, inv_t, mode)
    Xm = x_operand(x, mode)
    B, M = A.shape[0], Xm.shape[0]
    S, Z = (A @ Bm.T) * k, (A @ Xm.T) * k
    R, C = logits(S, lq_n, lq_c)
    Rx = Z if lq_n is None else Z - (lq_x.double().clamp(-L_CLAMP, 0.0) if lq_x is not None else torch.zeros(M, dtype=torch.float64, device=A.device))[None, :]
    Min = mask_matrix(ent_n, ent_c) if (ent_n is not None or ent_c is not None) else torch.zeros((B, B), dtype=torch.bool, device=A.device)
    Mx = x_mask(ent_c, ent_x, B, M, A.device)
    return S, Z, R, C, Rx, Min, Mx, A, Bm, Xm, k


def xneg_loss(S, Z, Min, Mx, lq_n=None, lq_c=None, lq_x=None):
    """the loss as autograd sees it: masked_fill(-inf) + logsumexp on the concatenated row logits (differentiable in S and Z)"""
    R, C = logits(S, lq_n, lq_c)
    Rx = Z if lq_n is None else Z - (lq_x.double().clamp(-L_CLAMP, 0.0) if lq_x is not None else 0.0 * Z[0])[None, :]
    ninf = -float("inf")
    rows = torch.cat([R.masked_fill(Min, ninf), Rx.masked_fill(Mx, ninf)], 1)
    return 0.5 * ((torch.logsumexp(rows, 1) - R.diagonal()).mean() + (torch.logsumexp(C.masked_fill(Min, ninf), 0) - C.diagonal()).mean())


def weights(R, C, Rx, Min, Mx):
    """(W [B, B], Wx [B, M]) of the closed form"""
    B = R.shape[0]
    ninf = -float("inf")
    P = torch.softmax(torch.cat([R.masked_fill(Min, ninf), Rx.masked_fill(Mx, ninf)], 1), 1)
    W = P[:, :B] + torch.softmax(C.masked_fill(Min, ninf), 0) - 2.0 * torch.eye(B, dtype=torch.float64, device=R.device)
    return W, P[:, B:]


def reference(n, c, x, inv_t, mode, ent_n=None, ent_c=None, ent_x=None, lq_n=None, lq_c=None, lq_x=None, with_wx=True):
    """f64 loss and (dN, dC, dX) for d_loss = 1 by the closed form.  with_wx=False drops Wx from the gradients and the extras from the
    loss: the form then is tests/_mask_reference.reference."""
    S, Z, R, C, Rx, Min, Mx, A, Bm, Xm, k = parts(n, c, x, inv_t, mode, ent_n, ent_c, ent_x, lq_n, lq_c, lq_x)
    B = A.shape[0]
    if not with_wx:
        Mx = torch.ones_like(Mx)                             # every extra masked: the rows' softmax is the in-batch one
    loss = xneg_loss(S, Z, Min, Mx, lq_n, lq_c, lq_x)
    W, Wx = weights(R, C, Rx, Min, Mx)
    if mode == "bf16":
        W, Wx = _bf16(W.float()), _bf16(Wx.float())
    g = inv_t / (2.0 * B)
    Ag = A * (k / inv_t) if mode == "bf16" else A            # the notice image carries the unit scale: dC and dX divide it out
    return loss.item(), g * (W @ Bm + Wx @ Xm), g * (W.T @ Ag), g * (Wx.T @ Ag)


def ref_rowsum(n, c, x, inv_t, mode, ent_n=None, ent_c=None, ent_x=None, lq_n=None, lq_c=None, lq_x=None):
    """f64 row sums as the entries return them: sum over the unmasked b and m of exp(s - 1/T) w (w = exp(-40 - q) with logQ, else 1)"""
    S, Z, R, C, Rx, Min, Mx, A, Bm, Xm, k = parts(n, c, x, inv_t, mode, ent_n, ent_c, ent_x, lq_n, lq_c, lq_x)
    off = abs(inv_t) + (L_CLAMP if lq_n is not None else 0.0)
    return torch.exp(R - off).masked_fill(Min, 0.0).sum(1) + torch.exp(Rx - off).masked_fill(Mx, 0.0).sum(1)
