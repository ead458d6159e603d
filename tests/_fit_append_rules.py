"""NumPy fp64 rules for appending training points to a fitted posterior (FittedPosterior.append, smn_fit_append*).

Two statements of the same posterior:
  * one shot: oracle.nngp_oracle.predict on ALL the points with the ABSOLUTE ridge lambda, lambda = ridge_rel tr(K_00) / n0
    taken from the first n0 points (the ridge a state freezes at creation);
  * the block append: from the factor L of K_00 + lambda I and beta = L^-1 Y, per chunk of new points
        V = K(x+, X) L^-T,  S = K(x+, x+) + lambda I - V V^T,  L22 = chol(S),  z = L22^-1 (y+ - V beta)
        L <- [[L, 0], [V, L22]],  beta <- [beta; z],  logdet += 2 sum log diag L22,  quad_c += |z_c|^2.
Constants and model builders restate the scheme of test_gpu_fit.py (TOL, RIDGE, 2 layers, (w_std, b_std, last_w_std) =
(1.1, 0.4, 1.0)); d is 6 (below the 16 / 32-element padding of the feature dimension) or 40 (above it)."""
import functools

import numpy as np
import scipy.linalg as sla

from oracle import nngp_oracle as O

LAYERS, W, B, LW = 2, 1.1, 0.4, 1.0
DEPTH = {"mlp": LAYERS, "resnet": 1}
TOL = {np.float64: 1e-7, np.float32: 1e-2}
RIDGE = {np.float64: 1e-3, np.float32: 1e-2}
NETS = {"mlp": 0, "resnet": 1}
OFN = {"mlp": O.mlp_kernel, "resnet": O.dense_resnet_kernel}
T = 37   # test points of every case (not a multiple of anything)


def kernel(net, kind, x1, x2=None):
    return OFN[net](x1, x2, DEPTH[net], "relu", W, B, LW, kind)


def frozen_ridge(k00, ridge_rel, ridge_abs=0.0):
    """lambda of a state made on the points of k00."""
    return ridge_abs + ridge_rel * np.trace(k00) / k00.shape[0]


def one_shot(k_dd, k_td, k_tt, y, lam):
    """dict(mean, cov, quad [c], logdet) of the posterior of all points under K + lam I."""
    mean, cov = O.predict(k_dd, k_td, k_tt, y, diag_reg=lam, diag_reg_absolute_scale=True)
    kt = k_dd + lam * np.eye(k_dd.shape[0])
    y2 = y[:, None] if y.ndim == 1 else y
    quad = np.array([float(y2[:, k] @ np.linalg.solve(kt, y2[:, k])) for k in range(y2.shape[1])])
    return dict(mean=mean, cov=cov, quad=quad, logdet=float(np.linalg.slogdet(kt)[1]))


class BlockState:
    """The factor, beta and the totals, grown by the block formulas."""

    def __init__(self, k00, y0, lam):
        y0 = y0[:, None] if y0.ndim == 1 else y0
        self.lam = float(lam)
        self.L = np.linalg.cholesky(k00 + lam * np.eye(k00.shape[0]))
        self.beta = sla.solve_triangular(self.L, y0, lower=True)
        self.quad = np.sum(self.beta ** 2, axis=0)
        self.logdet = 2.0 * float(np.sum(np.log(np.diag(self.L))))

    @property
    def n(self):
        return self.L.shape[0]

    def append(self, k_new_old, k_new_new, y_new):
        """k_new_old [k, n] against the points held so far, k_new_new [k, k]."""
        y_new = y_new[:, None] if y_new.ndim == 1 else y_new
        k, n = k_new_old.shape
        v = sla.solve_triangular(self.L, k_new_old.T, lower=True).T
        s = k_new_new + self.lam * np.eye(k) - v @ v.T
        l22 = np.linalg.cholesky(s)            # LinAlgError when S is not positive definite: the state is untouched
        z = sla.solve_triangular(l22, y_new - v @ self.beta, lower=True)
        self.L = np.block([[self.L, np.zeros((n, k))], [v, l22]])
        self.beta = np.vstack([self.beta, z])
        self.quad = self.quad + np.sum(z ** 2, axis=0)
        self.logdet += 2.0 * float(np.sum(np.log(np.diag(l22))))
        return v

    def predict(self, k_td, k_tt):
        v = sla.solve_triangular(self.L, k_td.T, lower=True).T
        return v @ self.beta, k_tt - v @ v.T


@functools.lru_cache(maxsize=None)
def data(n, c, d, f32, seed=0):
    """(x [n, d], xt [T, d], y [n, c]) as the device will see them, in fp64."""
    rng = np.random.default_rng(1000 * n + 10 * d + c + 7919 * seed)
    dt = np.float32 if f32 else np.float64
    return tuple(rng.standard_normal(s).astype(dt).astype(np.float64) for s in ((n, d), (T, d), (n, c)))


@functools.lru_cache(maxsize=None)
def reference(net, kind, n0, n, c, d, f32):
    """The one-shot posterior of n points at the ridge frozen on the first n0, with lam and the kernels it came from."""
    x, xt, y = data(n, c, d, f32)
    kdd, ktd, ktt = kernel(net, kind, x), kernel(net, kind, xt, x), kernel(net, kind, xt)
    lam = frozen_ridge(kdd[:n0, :n0], RIDGE[np.float32 if f32 else np.float64])
    ref = one_shot(kdd, ktd, ktt, y, lam)
    ref.update(lam=lam, kdd=kdd, ktd=ktd, ktt=ktt)
    return ref


def constant_norm_rows(x):
    """Rows rescaled to |x|^2 / d = 1: the MLP kernel's diagonal is then the same for every point, tr K / N does not move
    when points are added, and the frozen ridge equals the relative ridge of the fit on all the points."""
    x = np.asarray(x, dtype=np.float64)
    return x / np.sqrt(np.sum(x * x, axis=1, keepdims=True) / x.shape[1])
