"""Float64 numpy transcription of the Hadamard-MLP pair decoder (pgcn_link_mlp_fwd / _bwd), shared
by the tests of its kernels.  Not a test file.

With z_e = H[src_e] * H[dst_e] (element-wise, width d) and the packed tensor P [d + 3][>= h] --
rows 0 .. d - 1: W1 [d][h], row d: b1, row d + 1: w2, row d + 2: {b2, 0, ...}:

    pre_e[u] = b1[u] + sum_i z_e[i] W1[i][u]
    score_e  = b2 + sum_u w2[u] max(pre_e[u], 0)

    dhid_e[u] = g_e w2[u] [pre_e[u] > 0]        dz_e = dhid_e W1^T
    dW1 = z^T dhid    db1 = sum_e dhid_e    dw2 = sum_e g_e hid_e    db2 = sum_e g_e
    dH_i = sum over the selected pairs e of dz_e * (1[src_e == i] H[dst_e] + 1[dst_e == i] H[src_e])

g is read for every pair; only dH is restricted to the selected ones (select None or >= 0).
"""
import numpy as np


def pack(W1, b1, w2, b2, ld_p, fill=0.0):
    d, h = W1.shape
    P = np.full((d + 3, ld_p), fill, np.float32)
    P[:d, :h], P[d, :h], P[d + 1, :h], P[d + 2, 0] = W1, b1, w2, b2
    return P


def unpack(P, d, h):
    P = np.asarray(P, np.float64)
    return P[:d, :h], P[d, :h], P[d + 1, :h], P[d + 2, 0]


def forward(src, dst, H, P, d, h):
    """(scores [E], the per-pair error bound's two sums A = sum_u |w2 hid| and
    B = sum_u |w2| (|b1| + sum_i |z_i W1_iu|), pre [E][h])."""
    H = np.asarray(H, np.float64)[:, :d]
    W1, b1, w2, b2 = unpack(P, d, h)
    z = H[np.asarray(src)] * H[np.asarray(dst)]
    pre = z @ W1 + b1
    hid = np.maximum(pre, 0.0)
    A = (np.abs(w2) * hid).sum(axis=1)
    B = ((np.abs(b1) + np.abs(z) @ np.abs(W1)) * np.abs(w2)).sum(axis=1)
    return hid @ w2 + b2, A, B, pre


def backward(src, dst, H, P, g, d, h, select=None):
    """(dH [n][d], dP [d + 3][h], |terms| sums of the same shapes, entries m_i [n])."""
    H = np.asarray(H, np.float64)[:, :d]
    src, dst = np.asarray(src), np.asarray(dst)
    W1, b1, w2, b2 = unpack(P, d, h)
    g = np.asarray(g, np.float64)
    z = H[src] * H[dst]
    pre = z @ W1 + b1
    hid, on = np.maximum(pre, 0.0), pre > 0
    dhid = g[:, None] * w2 * on
    dP, mP = np.zeros((d + 3, h)), np.zeros((d + 3, h))
    dP[:d], mP[:d] = z.T @ dhid, np.abs(z).T @ np.abs(dhid)
    dP[d], mP[d] = dhid.sum(axis=0), np.abs(dhid).sum(axis=0)
    dP[d + 1], mP[d + 1] = (g[:, None] * hid).sum(axis=0), np.abs(g[:, None] * hid).sum(axis=0)
    dP[d + 2, 0], mP[d + 2, 0] = g.sum(), np.abs(g).sum()
    dz, mz = dhid @ W1.T, np.abs(dhid) @ np.abs(W1).T
    sel = np.ones(len(src), bool) if select is None else np.asarray(select) >= 0
    dH, mH = np.zeros_like(H), np.zeros_like(H)
    for out, coef, rows in ((dH, dz, H), (mH, mz, np.abs(H))):
        np.add.at(out, src[sel], coef[sel] * rows[dst[sel]])
        np.add.at(out, dst[sel], coef[sel] * rows[src[sel]])
    m = np.bincount(src[sel], minlength=len(H)) + np.bincount(dst[sel], minlength=len(H))
    return dH, dP, mH, mP, m
