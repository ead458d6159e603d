"""NumPy fp64 restatement of the cross, multi-seed reverse mode of the conv-NNGP kernel (smn_kernel_cnn_input_grad_cross in
csrc/cnn_input_grad.hip) and of FittedPosterior.predict_grad over get_cnn_kernel (shared by test_cnn_cross_grad_host.py and
test_gpu_cnn_cross_grad.py; not a test module).

The rules are _cnn_input_grad_rules.input_grad on the union [x1; x2] with n_grad = n1.  A cross seed s [n1, n2] becomes the
union seed with lower block g[n1 + j, r] = s[r, j] / 2 (the symmetric rules count a pair twice, a cross entry occurs once),
zero among the x1 images, and g[r, r] = gdiag[r] for the variance seed only.
    gmean[r, k] = sum_j alpha[j, k] dK(x1_r, x2_j)/dx1_r
    gvar[r]     = gdiag[r] dK(x1_r, x1_r)/dx1_r + sum_j gbar[r, j] dK(x1_r, x2_j)/dx1_r
Every gradient comes with S, the same sum over absolute values: the scale a rounding-error bound is relative to.
"""
import numpy as np

import _cnn_input_grad_rules as G


def _union_seed(seed, gdiag, n1, n2):
    g = np.zeros((n1 + n2, n1 + n2))
    g[n1:, :n1] = np.asarray(seed, dtype=np.float64).T / 2.0
    if gdiag is not None:
        g[np.arange(n1), np.arange(n1)] = np.asarray(gdiag, dtype=np.float64)
    return g


def cross_input_grad(x1, x2, layers, act, w_std, b_std, last_w_std, alpha=None, gbar=None, gdiag=None):
    """{"gmean": [n1,c,H,W,C], "smean": the same shape, "gvar": [n1,H,W,C], "svar": ...}; gmean needs alpha [n2, c], gvar
    gbar [n1, n2] and / or gdiag [n1] (a missing one is absent from the sum)."""
    x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    n1, n2 = x1.shape[0], x2.shape[0]
    u = np.concatenate([x1, x2], axis=0)
    run = lambda seed, gd: G.input_grad(_union_seed(seed, gd, n1, n2), u, layers, act, w_std, b_std, last_w_std, n_grad=n1)  # noqa: E731
    out = {}
    if alpha is not None:
        alpha = np.asarray(alpha, dtype=np.float64)
        parts = [run(np.broadcast_to(alpha[:, k], (n1, n2)), None) for k in range(alpha.shape[1])]
        out["gmean"] = np.stack([p[0] for p in parts], axis=1)
        out["smean"] = np.stack([p[1] for p in parts], axis=1)
    if gbar is not None or gdiag is not None:
        out["gvar"], out["svar"] = run(np.zeros((n1, n2)) if gbar is None else gbar, gdiag)
    return out


def posterior_seeds(k_dd, k_td, y, ridge, dtype=np.float64):
    """(alpha [n, c], gbar = -2 K_td K~^-1 [t, n]) for K~ = K_dd + ridge I (ridge absolute), solved by NumPy in `dtype` on the
    operands rounded to `dtype`; returned as float64."""
    kt = (np.asarray(k_dd, dtype=np.float64) + ridge * np.eye(k_dd.shape[0])).astype(dtype)
    y = np.asarray(y, dtype=dtype).reshape(k_dd.shape[0], -1)
    alpha = np.linalg.solve(kt, y)
    u = np.linalg.solve(kt, np.asarray(k_td, dtype=dtype).T).T
    return np.asarray(alpha, dtype=np.float64), -2.0 * np.asarray(u, dtype=np.float64)


def predict_grad(kernel, x, y, xt, ridge, layers, act, w_std, b_std, last_w_std, dtype=np.float64):
    """(dmean [T,C,H,W,Cin], dvar [T,H,W,Cin], S of each) of the posterior of K~ = kernel(x, x) + ridge I at the test images:
    mean = K_td K~^-1 Y, var = K_tt - K_td K~^-1 K_dt.  `kernel(a, b)` is the fp64 kernel (oracle.cnn_kernel with the same
    hyper-parameters); `dtype` is the precision the seeds are solved in."""
    alpha, gbar = posterior_seeds(kernel(x, None), kernel(xt, x), y, ridge, dtype)
    r = cross_input_grad(xt, x, layers, act, w_std, b_std, last_w_std, alpha=alpha, gbar=gbar, gdiag=np.ones(len(xt)))
    return r["gmean"], r["gvar"], r["smean"], r["svar"]
