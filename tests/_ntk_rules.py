"""NumPy / SciPy fp64 restatement of the exact GP / Student-t process whose covariance function is the neural tangent kernel
Theta of the MLP / dense-ResNet architectures (spax.kernels.NTKKernel, SMN_NET_NTK): the kernel, its tangents with respect to
w_std^2 and b_std^2, the log-marginal likelihood with its analytic gradient, central differences of it, predictions and
leave-one-out.  Shared by test_ntk_host.py and test_gpu_ntk_gp.py; not a test module.

Theta is the oracle's (oracle.mlp_kernel / dense_resnet_kernel(get="ntk")), the log-pdfs are oracle.mvn_logpdf / mvt_logpdf,
predictions oracle.predict on Theta blocks, leave-one-out tests/_loo_rules.from_matrix on Theta~.  The tangents restate the
six-state forward-mode rules of csrc/grad.hip: per Dense + activation, with q the pre-activation variances,
    A = w2 K + b2,  A_w = K + w2 K_w,  A_b = 1 + w2 K_b;    T = A + w2 Theta,  T_w = A_w + Theta + w2 Theta_w,  T_b = A_b + w2 Theta_b
    K <- phi(A),  K_t = phi_A A_t + phi_1 q_i,t + phi_2 q_j,t;    D = phi_A,  D_t = D_A A_t + D_1 q_i,t + D_2 q_j,t
    Theta <- T D,  Theta_t = T_t D + T D_t;    Theta_out = lw2 (K + Theta)
    ReLU (c = A / sqrt(q_i q_j)):  D_A = 1 / (2 pi sqrt(1-c^2) sqrt(q_i q_j)),  D_i = -c / (4 pi q_i sqrt(1-c^2)),
                                   both 0 where (1-c)(1+c) <= 0 after clamping and on the diagonal (D = 1/2 there)
    erf (R = (1+2q_i)(1+2q_j) - 4A^2):  D_A = 16 A / (pi R^(3/2)),  D_i = -4 (1+2q_j) / (pi R^(3/2))
"""
import functools

import numpy as np

import _loo_rules as LR
import _multi_rules as M
from oracle import nngp_oracle as O

KEYS = M.KEYS
HYP = dict(w_std=1.3, b_std=0.4, last_w_std=0.9, eps=5e-2, alpha=1.7, beta=2.4)   # the existing gradient test's


def theta(family, x1, x2, layers, act, w_std, b_std, last_w_std):
    """Theta(x1, x2) (x2 None: symmetric), fp64, from the oracle."""
    fn = {"mlp": O.mlp_kernel, "resnet": O.dense_resnet_kernel}[family]
    x1 = np.asarray(x1, dtype=np.float64)
    x2 = None if x2 is None else np.asarray(x2, dtype=np.float64)
    return fn(x1, x2, layers, act, w_std, b_std, last_w_std, get="ntk")


# ---------------------------------------------------------------------------------------------------------- tangents
def _act(act, a, qi, qj):
    """phi, phi_A (= D), phi_1, phi_2, D_A, D_1, D_2 of the activation map at pre-activation A with variances q_i, q_j."""
    pi = np.pi
    if act == "relu":
        sp = np.sqrt(np.outer(qi, qj))
        c = np.clip(a / sp, -1.0, 1.0)
        s1 = np.sqrt(np.maximum((1.0 - c) * (1.0 + c), 0.0))
        pm = pi - np.arccos(c)
        phi = sp * (s1 + pm * c) / (2 * pi)
        d = pm / (2 * pi)
        p1 = s1 * sp / (4 * pi * qi[:, None])
        p2 = s1 * sp / (4 * pi * qj[None, :])
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(s1 > 0, 1.0 / (2 * pi * s1), 0.0)
        da, d1, d2 = inv / sp, -inv * c / (2 * qi[:, None]), -inv * c / (2 * qj[None, :])
    elif act == "erf":
        ti, tj = 1.0 + 2.0 * qi, 1.0 + 2.0 * qj
        p = np.outer(ti, tj)
        r = p - 4.0 * a * a
        s = 2.0 * a / np.sqrt(p)
        phi = 2 / pi * np.arcsin(np.clip(s, -1.0, 1.0))
        d = 4.0 / (pi * np.sqrt(r))
        p1 = -(2 / pi) * s / (np.sqrt(r / p) * ti[:, None])
        p2 = -(2 / pi) * s / (np.sqrt(r / p) * tj[None, :])
        da = 16.0 * a / (pi * r ** 1.5)
        d1 = -4.0 * tj[None, :] / (pi * r ** 1.5)
        d2 = -4.0 * ti[:, None] / (pi * r ** 1.5)
    else:
        raise KeyError(act)
    return phi, d, p1, p2, da, d1, d2


def tangents(family, x, layers, act, w_std, b_std, last_w_std):
    """(Theta_out, dTheta_out/dw_std, dTheta_out/db_std, dTheta_out/dlast_w_std) [N,N] by the six-state rules, fp64."""
    x = np.asarray(x, dtype=np.float64)
    w2, b2, lw2 = w_std ** 2, b_std ** 2, last_w_std ** 2
    n, d = x.shape
    k = x @ x.T / d
    q = np.einsum("ij,ij->i", x, x) / d
    np.fill_diagonal(k, q)
    z = np.zeros_like(k)
    state = (k, z.copy(), z.copy(), z.copy(), z.copy(), z.copy(), q, np.zeros(n), np.zeros(n))

    def dense(k, kw, kb, th, tw, tb, q, qw, qb):
        a, aw, ab = w2 * k + b2, k + w2 * kw, 1.0 + w2 * kb
        return a, aw, ab, a + w2 * th, aw + th + w2 * tw, ab + w2 * tb, w2 * q + b2, q + w2 * qw, 1.0 + w2 * qb

    def activ(a, aw, ab, t, tw, tb, q, qw, qb):
        phi, dd, p1, p2, da, d1, d2 = _act(act, a, q, q)
        kw_ = dd * aw + p1 * qw[:, None] + p2 * qw[None, :]
        kb_ = dd * ab + p1 * qb[:, None] + p2 * qb[None, :]
        dw = da * aw + d1 * qw[:, None] + d2 * qw[None, :]
        db = da * ab + d1 * qb[:, None] + d2 * qb[None, :]
        if act == "relu":                                   # c = 1 identically on the diagonal: D = 1/2, no derivative
            np.fill_diagonal(dw, 0.0)
            np.fill_diagonal(db, 0.0)
        return (phi, kw_, kb_, t * dd, tw * dd + t * dw, tb * dd + t * db, np.diag(phi).copy(), np.diag(kw_).copy(),
                np.diag(kb_).copy())

    if family == "mlp":
        for _ in range(layers):
            state = activ(*dense(*state))
    elif family == "resnet":                                # between blocks the Theta slots hold T
        state = dense(*state)
        for _ in range(layers):
            block = dense(*activ(*state))
            state = tuple(u + v for u, v in zip(block, state))
        state = activ(*state)
    else:
        raise KeyError(family)
    k, kw, kb, th, tw, tb = state[:6]
    return lw2 * (k + th), lw2 * (kw + tw) * 2 * w_std, lw2 * (kb + tb) * 2 * b_std, 2 * last_w_std * (k + th)


# ------------------------------------------------------------------------------------------------------------- heads
def logpdf(kt, y, method, alpha, beta):
    """log p(Y) of Y [N,C] (or [N]) under the joint head with matrix K~: the C columns share K~; Gaussian: independent columns;
    Student-t: ONE multivariate t over vec(Y) with shape (b/a) (I_C x K~) (MultiSPR's model; SPR at C = 1)."""
    y = np.asarray(y, dtype=np.float64)
    y2 = y[:, None] if y.ndim == 1 else y
    c = y2.shape[1]
    if method == "gp":
        return float(sum(O.mvn_logpdf(y2[:, j], kt) for j in range(c)))
    return float(O.mvt_logpdf(y2.T.reshape(-1), (beta / alpha) * np.kron(np.eye(c), kt), 2.0 * alpha))


def loss(family, x, y, layers, act, method, w_std, b_std, last_w_std, eps, alpha=2.0, beta=2.0):
    """SPR / MultiSPR.loss under NTKKernel: -log p(Y) / N with K~ = Theta + eps I."""
    th = theta(family, x, None, layers, act, w_std, b_std, last_w_std)
    n = th.shape[0]
    return -logpdf(th + eps * np.eye(n), y, method, alpha, beta) / n


def loss_fd(family, x, y, layers, act, method, keys, h=1e-5, **hyp):
    """Central differences of `loss` in the constrained values, relative step h (oracle.spr_loss_grad_fd's)."""
    out = {}
    for k in keys:
        v = float(hyp[k])
        step = h * abs(v) if v != 0.0 else h
        up = dict(hyp); up[k] = v + step
        dn = dict(hyp); dn[k] = v - step
        out[k] = (loss(family, x, y, layers, act, method, **up) - loss(family, x, y, layers, act, method, **dn)) / (2.0 * step)
    return out


def loss_grad(family, x, y, layers, act, method, w_std, b_std, last_w_std, eps, alpha=2.0, beta=2.0):
    """(loss, {key: d loss / d constrained value}) analytically: 1/2 sum G dTheta~/d theta over the six-state tangents, the
    (a, b) part from _multi_rules.loss_grad's closed form fed Theta."""
    y = np.asarray(y, dtype=np.float64)
    y2 = y[:, None] if y.ndim == 1 else y
    n, c = y2.shape
    th, dw, db, dl = tangents(family, x, layers, act, w_std, b_std, last_w_std)
    g, _, _, _, q, ld = M.g_parts(th, y2, eps, method, alpha, beta)
    lp = M.head(th + eps * np.eye(n), y2, method, alpha, beta)[0]
    dlp = {"w_std": 0.5 * np.sum(g * dw), "b_std": 0.5 * np.sum(g * db), "last_w_std": 0.5 * np.sum(g * dl), "eps": 0.5 * np.trace(g)}
    if method == "tp":
        from scipy.special import digamma
        nu, s, nc = 2.0 * alpha, beta / alpha, n * c
        t = 0.5 * (nu + nc)
        u = q / (s * nu)
        d_s = t * (u / s) / (1.0 + u) - 0.5 * nc / s
        d_nu = -0.5 * np.log1p(u) + t * (u / nu) / (1.0 + u) - 0.5 * nc / nu + 0.5 * digamma(t) - 0.5 * digamma(0.5 * nu)
        dlp["alpha"] = 2.0 * d_nu - d_s * beta / alpha ** 2
        dlp["beta"] = d_s / alpha
    return -lp / n, {key: -float(v) / n for key, v in dlp.items()}


def predict(family, x, y, xt, layers, act, w_std, b_std, last_w_std, eps):
    """NTKKernel.predict: oracle.predict on Theta blocks (relative ridge eps tr(Theta_dd)/N)."""
    args = (layers, act, w_std, b_std, last_w_std)
    return O.predict(theta(family, x, None, *args), theta(family, xt, x, *args), theta(family, xt, None, *args),
                     np.asarray(y, dtype=np.float64), diag_reg=eps)


def predictive_nll(family, x, y, xt, yt, layers, act, method, w_std, b_std, last_w_std, eps, alpha=2.0, beta=2.0):
    """SPR.test_nll under NTKKernel (y_mean = 0, y_std = 1): the marginals of `predict`; Student-t with nu + N degrees of
    freedom and d = nu + y^T ((b/a) Theta + 1e-6 I)^-1 y (Theta WITHOUT eps, as the NNGP head has K)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y.shape[0]
    mean, cov = predict(family, x, y, xt, layers, act, w_std, b_std, last_w_std, eps)
    ys, ms, var = np.asarray(yt, dtype=np.float64).reshape(-1), mean.ravel(), np.diag(cov)
    if method == "gp":
        lp = O.normal_logpdf(ys, ms, np.sqrt(var))
    else:
        nu, s = 2.0 * alpha, beta / alpha
        khat = s * theta(family, x, None, layers, act, w_std, b_std, last_w_std) + 1e-6 * np.eye(n)
        d = nu + float(y @ np.linalg.solve(khat, y))
        lp = O.student_t_logpdf(ys, nu + n, ms, np.sqrt(d / (nu + n) * s * var))
    return -float(np.mean(lp))


def loo(family, x, y, layers, act, method, w_std, b_std, last_w_std, eps, alpha=2.0, beta=2.0):
    """_loo_rules.from_matrix on Theta~ = Theta + eps I."""
    th = theta(family, x, None, layers, act, w_std, b_std, last_w_std)
    y = np.asarray(y, dtype=np.float64)
    return LR.from_matrix(th + eps * np.eye(th.shape[0]), y[:, None] if y.ndim == 1 else y, method, alpha, beta)


def loo_loss(family, x, y, layers, act, method, **hyp):
    return -loo(family, x, y, layers, act, method, **hyp)["lam"] / np.asarray(y).shape[0]


def loo_loss_fd(family, x, y, layers, act, method, keys, h=1e-5, **hyp):
    out = {}
    for k in keys:
        v = float(hyp[k])
        step = h * abs(v) if v != 0.0 else h
        up = dict(hyp); up[k] = v + step
        dn = dict(hyp); dn[k] = v - step
        out[k] = (loo_loss(family, x, y, layers, act, method, **up) - loo_loss(family, x, y, layers, act, method, **dn)) / (2.0 * step)
    return out


def loo_loss_grad(family, x, y, layers, act, method, w_std, b_std, last_w_std, eps, alpha=2.0, beta=2.0):
    """(loo loss, {key: d / d constrained value}): d Lambda = sum_ij G_ij dTheta~_ij with the seed G of _loo_rules."""
    y = np.asarray(y, dtype=np.float64)
    y2 = y[:, None] if y.ndim == 1 else y
    n = y2.shape[0]
    th, dw, db, dl = tangents(family, x, layers, act, w_std, b_std, last_w_std)
    r = LR.from_matrix(th + eps * np.eye(n), y2, method, alpha, beta)
    g = r["g"]
    grads = {"w_std": -np.sum(g * dw) / n, "b_std": -np.sum(g * db) / n, "last_w_std": -np.sum(g * dl) / n, "eps": -np.trace(g) / n}
    if method == "tp":
        grads.update(LR.head_grads(r["dhead"], n, alpha, beta))
    return -r["lam"] / n, {k: float(v) for k, v in grads.items()}


# ------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def reg_data(n, d=6, seed=17, dup=False):
    """(x [n,d], y [n]) of the existing gradient test (seed 17, n = 150, d = 6); dup: x[7] = x[3] exactly."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    if dup:
        x[7] = x[3]
    y = np.sin(x[:, 0]) + 0.3 * rng.standard_normal(n)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def ref_loss_and_fd(family, act, layers, method, n, dup=False, seed=17, d=6):
    """(loss, central differences h = 1e-5) of a regression case at HYP, computed once per session."""
    x, y = reg_data(n, d, seed, dup)
    keys = KEYS if method == "tp" else KEYS[:4]
    return loss(family, x, y, layers, act, method, **HYP), loss_fd(family, x, y, layers, act, method, keys, **HYP)
