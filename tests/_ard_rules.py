"""The log-marginal likelihood of the exact models differentiated in the INPUTS of an MLP / dense-ResNet kernel, restated in
NumPy (test infrastructure, not a test module): the yardstick of per-feature input scales (ARD) and of d loss / d X.

x~ = the inputs as the kernel sees them (x * s under input scales), Lambda = log p(Y | x~), K~ = K(x~, x~) + eps I, A = K~^-1 Y
[N, C], G = coef A A^T - C K~^-1 (coef = 1: Gaussian; (nu + N C) / ((nu + Q / s) s): Student-t, nu = 2a, s = b/a), so that
d Lambda = 1/2 sum_nm G_nm dK~_nm.  For n != m, K_nm = F(u_nm, v_n, v_m), u = x~_n . x~_m / d, v_n = |x~_n|^2 / d; the diagonal is
the closed form K_nn = F_d(v_n).  With F_1 = dF/du, F_2[n, m] = dK_nm/dv_n and ddiag_n = F_d'(v_n) -- what
_input_grad_rules.factors(kind, x~, x~, get, ...) returns, the diagonal entries of F_1 and F_2 discarded --

    W_nm   = G_nm F_1[n, m]                 (n != m; W_nn = 0)
    r_n    = sum_{m != n} G_nm F_2[n, m]
    gx_n   = dLambda/dx~_n = (sum_m W_nm x~_m + (2 r_n + G_nn ddiag_n) x~_n) / d
    feat_j = sum_n gx[n, j] x~[n, j]        (dLambda/ds_j = feat_j / s_j,  dLambda/dx_n = s o gx_n)

Every function takes `dtype` and keeps ALL its arithmetic in it: the float32 evaluation against the float64 one is the yardstick
of the device tests.
"""
import numpy as np
from scipy.special import gammaln

import _input_grad_rules as IR
from oracle import nngp_oracle as O


def g_matrix(neg_kinv, alpha, coef, dtype=np.float64):
    """G = coef A A^T + C (-K~^-1) in `dtype` (A = alpha [N, C])."""
    dt = np.dtype(dtype).type
    a = np.asarray(alpha, dtype=dtype).reshape(len(alpha), -1)
    return (dt(coef) * (a @ a.T) + dt(a.shape[1]) * np.asarray(neg_kinv, dtype=dtype)).astype(dtype)


def seed_input_grad(kind, xs, g, get="nngp", dtype=np.float64, **hyp):
    """(gx [N, d], feat [d]) for a symmetric seed G [N, N]: 1/2 sum_nm G_nm dK_nm differentiated in x~."""
    dt = np.dtype(dtype).type
    xs, g = np.asarray(xs, dtype=dtype), np.asarray(g, dtype=dtype)
    n, d = xs.shape
    f1, f2, ddiag = IR.factors(kind, xs, xs, get, dtype=dtype, **hyp)
    off = ~np.eye(n, dtype=bool)
    w = np.where(off, g * f1, dt(0))
    r = np.where(off, g * f2, dt(0)).sum(axis=1)
    gx = ((w @ xs + (dt(2) * r + np.diag(g) * ddiag)[:, None] * xs) / dt(d)).astype(dtype)
    return gx, (gx * xs).sum(axis=0).astype(dtype)


def posterior_parts(kind, xs, y, get, eps, method, a, b, dtype=np.float64, **hyp):
    """(-K~^-1, A, coef, Q, logdet K~) in `dtype` (the scalars as Python floats of values computed in `dtype`)."""
    dt = np.dtype(dtype).type
    xs = np.asarray(xs, dtype=dtype)
    y2 = np.asarray(y, dtype=dtype).reshape(len(xs), -1)
    n, c = y2.shape
    k = np.asarray(IR.KERNELS[kind](xs, None, get=get, dtype=dtype, **hyp), dtype=dtype)
    kt = k + dt(eps) * np.eye(n, dtype=dtype)
    kinv = np.linalg.inv(kt).astype(dtype)
    kinv = dt(0.5) * (kinv + kinv.T)
    alpha = (kinv @ y2).astype(dtype)
    q = np.sum(y2 * alpha, dtype=dtype)
    ld = dt(2) * np.log(np.diag(np.linalg.cholesky(kt))).sum(dtype=dtype)
    if method == "gp":
        coef = dt(1)
    else:
        nu, s = dt(2) * dt(a), dt(b) / dt(a)
        coef = (nu + dt(n * c)) / ((nu + q / s) * s)
    return -kinv, alpha, float(coef), float(q), float(ld)


def lml_input_grad(kind, xs, y, get="nngp", eps=1e-3, method="gp", a=2.0, b=2.0, dtype=np.float64, **hyp):
    """(gx, feat) = (dLambda/dx~ [N, d], sum_n gx o x~ [d]) of Lambda = log p(Y | x~), Y [N] or [N, C]."""
    ninv, alpha, coef, _, _ = posterior_parts(kind, xs, y, get, eps, method, a, b, dtype=dtype, **hyp)
    return seed_input_grad(kind, xs, g_matrix(ninv, alpha, coef, dtype), get, dtype=dtype, **hyp)


def logpdf(kind, xs, y, get="nngp", eps=1e-3, method="gp", a=2.0, b=2.0, **hyp):
    """Lambda = log p(Y | x~) from the oracle's kernel, fp64: Gaussian, or the joint multivariate t of all N C outputs."""
    xs = np.asarray(xs, dtype=np.float64)
    y2 = np.asarray(y, dtype=np.float64).reshape(len(xs), -1)
    n, c = y2.shape
    kt = np.asarray(IR.KERNELS[kind](xs, None, get=get, **hyp), dtype=np.float64) + eps * np.eye(n)
    l = np.linalg.cholesky(kt)
    z = np.linalg.solve(l, y2)
    q, ld = float(np.sum(z * z)), 2.0 * float(np.log(np.diag(l)).sum())
    if method == "gp":
        return -0.5 * q - 0.5 * n * c * np.log(2.0 * np.pi) - 0.5 * c * ld
    nu, s = 2.0 * a, b / a
    t = 0.5 * (nu + n * c)
    return float(-t * np.log1p(q / (s * nu)) - 0.5 * n * c * np.log(nu * np.pi) + gammaln(t) - gammaln(0.5 * nu)
                 - 0.5 * (c * ld + n * c * np.log(s)))


def loss(kind, x, s, y, get="nngp", **kw):
    """The exact models' loss -Lambda / N on x * s."""
    x = np.asarray(x, dtype=np.float64)
    return -logpdf(kind, x * np.asarray(s, dtype=np.float64), y, get, **kw) / len(x)


def loss_scale_grad_fd(kind, x, s, y, get="nngp", h=1e-6, **kw):
    """Central differences of `loss` in every scale, step h s_j."""
    s = np.asarray(s, dtype=np.float64)
    out = np.empty_like(s)
    for j in range(len(s)):
        up, dn = s.copy(), s.copy()
        up[j] += h * s[j]
        dn[j] -= h * s[j]
        out[j] = (loss(kind, x, up, y, get, **kw) - loss(kind, x, dn, y, get, **kw)) / (2.0 * h * s[j])
    return out


def loss_input_grad_fd(kind, x, s, y, get="nngp", h=1e-6, **kw):
    """Central differences of `loss` in every entry of x [N, d] (the inputs as handed in), step h."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    for i in range(x.shape[0]):
        for j in range(x.shape[1]):
            up, dn = x.copy(), x.copy()
            up[i, j] += h
            dn[i, j] -= h
            out[i, j] = (loss(kind, up, s, y, get, **kw) - loss(kind, dn, s, y, get, **kw)) / (2.0 * h)
    return out
