"""Finite-time gradient-descent predictions restated in NumPy (test infrastructure, not a test module).

Gradient flow on 0.5 * mean((f - y)^2) over all N*C outputs of the linearised infinite ensemble, neural_tangents'
normalisation.  K is the NNGP kernel and Theta the NTK over [x_train; x_test]; G is Theta for get="ntk" and K for get="nngp":

    G~ = G_dd + rho I = V diag(lam) V^T   (numpy.linalg.eigh; rho = diag_reg tr(G_dd)/N, or diag_reg itself when absolute)
    s = learning_rate t / (N C),  d = -expm1(-lam s) / lam,  e = -expm1(-2 lam s) / lam   (t = inf: both 1 / lam), lam clamped at 0
    P = G_*d V,  z = V^T y,  mean_t = (P . d) z
    nngp: cov_t = K_** - (P . e) P^T
    ntk:  A_t = (P . d) V^T,  cov_t = K_** + A_t K_dd A_t^T - (A_t K_d* + K_*d A_t^T)        (K_dd without the ridge)

Every function takes `dtype` and keeps ALL its arithmetic, the kernel build included, in that dtype: the float32 evaluation
against the float64 one is the yardstick of the device tests.
"""
import numpy as np

from oracle import nngp_oracle as O


def joint_kernels(kind, xa, get, dtype=np.float64, **hyp):
    """(K, Theta or None) over the rows of xa, built by the oracle in `dtype`."""
    xa = np.asarray(xa, dtype=dtype)
    if kind == "cnn":
        if get != "nngp":
            raise ValueError("the conv kernel has no NTK here")
        return O.cnn_kernel(xa, None, dtype=dtype, **hyp), None
    fn = {"mlp": O.mlp_kernel, "dense_resnet": O.dense_resnet_kernel}[kind]
    if get == "nngp":
        return np.asarray(fn(xa, None, get="nngp", dtype=dtype, **hyp), dtype=dtype), None
    k, th = fn(xa, None, get=("nngp", "ntk"), dtype=dtype, **hyp)
    return np.asarray(k, dtype=dtype), np.asarray(th, dtype=dtype)


def regularised(g_dd, diag_reg, absolute=False):
    n = g_dd.shape[0]
    dt = g_dd.dtype.type
    rho = dt(diag_reg) * (dt(1.0) if absolute else np.trace(g_dd) / dt(n))
    return g_dd + rho * np.eye(n, dtype=g_dd.dtype)


def time_factors(lam, s):
    """d(lam), e(lam) at scaled time s (a scalar of lam's dtype, or inf)."""
    if np.isinf(s):
        return 1.0 / lam, 1.0 / lam
    return -np.expm1(-lam * s) / lam, -np.expm1(-2.0 * lam * s) / lam


def gd_predict(k, theta, n, y, times, diag_reg=0.0, absolute=False, learning_rate=1.0, dtype=np.float64, with_evals=False):
    """means [len(times), T, C] and covs [len(times), T, T] in `dtype`."""
    dt = np.dtype(dtype).type
    k = np.asarray(k, dtype=dtype)
    g = k if theta is None else np.asarray(theta, dtype=dtype)
    y = np.asarray(y, dtype=dtype).reshape(n, -1)
    c = y.shape[1]
    lam, v = np.linalg.eigh(regularised(g[:n, :n], diag_reg, absolute))
    lam = np.maximum(lam, dt(0.0))
    p = g[n:, :n] @ v
    z = v.T @ y
    k_ss, k_sd, k_dd = k[n:, n:], k[n:, :n], k[:n, :n]
    means, covs = [], []
    for t in np.atleast_1d(np.asarray(times, dtype=np.float64)):
        s = dt(np.inf) if np.isinf(t) else dt(learning_rate * t / (n * c))
        d, e = time_factors(lam, s)
        means.append((p * d) @ z)
        if theta is None:
            covs.append(k_ss - (p * e) @ p.T)
        else:
            a = (p * d) @ v.T
            cross = a @ k_sd.T
            covs.append(k_ss + a @ k_dd @ a.T - (cross + cross.T))
    out = np.stack(means).astype(dtype), np.stack(covs).astype(dtype)
    return out + (lam,) if with_evals else out
