"""float64 numpy restatements of BatchNorm (pgcn_params.batch_norm, include/pgcn.h): the kernel
formulas, and the engine's model with it (the conventions of test_gpu_layernorm's NumpyNormGCN:
dense algebra on scipy CSR matrices, no dropout, starting from the engine's weights).
"""
import numpy as np

from test_gpu_layernorm import WD, NumpyNormGCN

BN_EPS = 1e-5


def fwd(x, gamma, beta):
    """(y, xhat, mean, rstd) with the biased column statistics over the rows of x."""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=0)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=0) + BN_EPS)
    xhat = (x - mean) * rstd
    return np.asarray(gamma, np.float64) * xhat + np.asarray(beta, np.float64), xhat, mean, rstd


def bwd(dy, xhat, rstd, gamma):
    """(dx, dgamma, dbeta)."""
    dy, xhat = np.asarray(dy, np.float64), np.asarray(xhat, np.float64)
    n = len(dy)
    dbeta, dgamma = dy.sum(axis=0), (dy * xhat).sum(axis=0)
    dx = np.asarray(gamma, np.float64) * rstd * (dy - dbeta / n - xhat * dgamma / n)
    return dx, dgamma, dbeta


class Model(NumpyNormGCN):
    """test_gpu_layernorm's float64 engine model (same weights, Adam and loss) with a BatchNorm
    where it has a LayerNorm: Z = Â (H W_l) -> BatchNorm -> ReLU [+ H on a residual layer]."""

    def forward(self, split):
        A, L = self.A, self.L
        self.Y, self.H, self.xhat, self.rstd = [], [], [], []
        h = None
        for l in range(L - 1):
            z = A @ ((self.X @ self.W[0]) if l == 0 else (h @ self.W[l]))
            y, xhat, _, rstd = fwd(z, self.gamma[l], self.beta[l])
            hn = np.maximum(y, 0.0) + (h if self.res[l] else 0.0)
            self.Y.append(y)
            self.H.append(hn)
            self.xhat.append(xhat)
            self.rstd.append(rstd)
            h = hn
        self.last_in = A @ h if self.re else h
        logits = self.last_in @ self.W[L - 1] if self.re else A @ (h @ self.W[L - 1])
        rows = np.nonzero((self.split == split) & (self.label >= 0))[0]
        zr = logits[rows] - logits[rows].max(axis=1, keepdims=True)
        lse = np.log(np.exp(zr).sum(axis=1))
        loss = float((lse - zr[np.arange(len(rows)), self.label[rows]]).mean())
        self.rows, self.shifted, self.lse, self.logits = rows, zr, lse, logits
        return loss + WD * float((self.W[0] ** 2).sum()) / 2.0

    def backward(self):
        A, L, rows = self.A, self.L, self.rows
        d_out = np.zeros_like(self.logits)
        p = np.exp(self.shifted - self.lse[:, None])
        p[np.arange(len(rows)), self.label[rows]] -= 1.0
        d_out[rows] = p / len(rows)
        self.dW = [None] * L
        self.dgamma, self.dbeta = [None] * (L - 1), [None] * (L - 1)
        if self.re:
            self.dW[L - 1] = self.last_in.T @ d_out
            g = A @ (d_out @ self.W[L - 1].T)
        else:
            self.dW[L - 1] = self.H[L - 2].T @ (A @ d_out)
            g = (A @ d_out) @ self.W[L - 1].T
        for l in range(L - 2, -1, -1):
            dz, self.dgamma[l], self.dbeta[l] = bwd(g * (self.Y[l] > 0), self.xhat[l],
                                                    self.rstd[l], self.gamma[l])
            dvar1 = A @ dz
            if l == 0:
                self.dW[0] = np.asarray(self.X.T @ dvar1)
                break
            self.dW[l] = self.H[l - 1].T @ dvar1
            g = dvar1 @ self.W[l].T + (g if self.res[l] else 0.0)
