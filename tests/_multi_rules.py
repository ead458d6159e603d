"""NumPy / SciPy fp64 restatement of the exact C-output GP / Student-t process (MultiSPR): the joint log-pdf, its
analytic gradient, the predictive heads and the classification read-out.  Shared by test_multi_host.py and
test_gpu_multi.py; not a test module.

Y [N,C], K~ = K(x,x) + eps I, A = K~^-1 Y, Q = tr(Y^T K~^-1 Y), ld = logdet K~:
    Gaussian:   log p = -Q/2 - (N C / 2) log 2 pi - (C/2) ld
    Student-t:  vec(Y) ~ MVT_{NC}(nu = 2a, 0, s (I_C x K~)), s = b/a, t = (nu + N C)/2:
                log p = -t log1p(Q/(s nu)) - (N C/2) log(nu pi) + lgamma(t) - lgamma(nu/2) - (C ld + N C log s)/2
    d log p / d theta = 1/2 sum_ij G_ij dK~_ij/d theta,   G = coef A A^T - C K~^-1,
    coef = 1 (Gaussian) or (nu + N C)/((nu + Q/s) s) (Student-t)
The kernels are the oracle's; the tangents dK/dw^2, dK/db^2 are the forward-mode rules of csrc/grad.hip restated here
for the MLP family and those of tests/_cnn_grad_rules.py for get_cnn_kernel.
"""
import functools

import numpy as np
from scipy.special import digamma, gammaln

import _cnn_grad_rules as R
from oracle import nngp_oracle as O

FAMILIES = ("mlp", "resnet", "cnn", "conv_resnet")
KEYS = ("w_std", "b_std", "last_w_std", "eps", "alpha", "beta")


def kernel(family, x1, x2, layers, act, w_std, b_std, last_w_std):
    """K(x1, x2) (x2 None: symmetric) of one of the four kernel families, fp64."""
    x1 = np.asarray(x1, dtype=np.float64)
    x2 = None if x2 is None else np.asarray(x2, dtype=np.float64)
    if family == "mlp":
        return O.mlp_kernel(x1, x2, layers, act, w_std, b_std, last_w_std)
    if family == "resnet":
        return O.dense_resnet_kernel(x1, x2, layers, act, w_std, b_std, last_w_std)
    if family == "cnn":
        return O.cnn_kernel(x1, x2, layers, act, w_std, b_std, last_w_std)
    if family == "conv_resnet":
        return O.conv_resnet_kernel(x1, x2, layers, act, w_std, b_std, last_w_std)
    raise KeyError(family)


def label_targets(labels, c):
    y = np.full((len(labels), c), -1.0 / c)
    y[np.arange(len(labels)), np.asarray(labels)] += 1.0
    return y


# ----------------------------------------------------------------------------------------------------------- log-pdf
def head(kt, y, method, alpha, beta):
    """(log p, Q, ld, A, K~^-1, coef) of Y [N,C] under the joint head with matrix K~ (jitter included)."""
    n, c = y.shape
    l = np.linalg.cholesky(kt)                     # raises LinAlgError when K~ is not positive definite
    kinv = np.linalg.inv(kt)
    kinv = 0.5 * (kinv + kinv.T)
    a = kinv @ y
    z = np.linalg.solve(l, y)
    q = float(np.sum(z * z))
    ld = 2.0 * float(np.log(np.diag(l)).sum())
    if method == "gp":
        lp = -0.5 * q - 0.5 * n * c * np.log(2.0 * np.pi) - 0.5 * c * ld
        coef = 1.0
    else:
        nu, s = 2.0 * alpha, beta / alpha
        t = 0.5 * (nu + n * c)
        lp = (-t * np.log1p(q / (s * nu)) - 0.5 * n * c * np.log(nu * np.pi) + gammaln(t) - gammaln(0.5 * nu)
              - 0.5 * (c * ld + n * c * np.log(s)))
        coef = (nu + n * c) / ((nu + q / s) * s)
    return float(lp), q, ld, a, kinv, coef


def loss(family, x, y, layers, act, method, w_std, b_std, last_w_std, eps, alpha=2.0, beta=2.0):
    """MultiSPR.loss: -log p(Y) / N."""
    k = kernel(family, x, None, layers, act, w_std, b_std, last_w_std)
    n = k.shape[0]
    return -head(k + eps * np.eye(n), np.asarray(y, dtype=np.float64), method, alpha, beta)[0] / n


def loss_fd(family, x, y, layers, act, method, keys, h=1e-5, **hyp):
    """Central differences of `loss` with respect to the constrained values, relative step h."""
    out = {}
    for k in keys:
        v = float(hyp[k])
        step = h * abs(v) if v != 0.0 else h
        up = dict(hyp); up[k] = v + step
        dn = dict(hyp); dn[k] = v - step
        out[k] = (loss(family, x, y, layers, act, method, **up) - loss(family, x, y, layers, act, method, **dn)) / (2.0 * step)
    return out


# ---------------------------------------------------------------------------------------------------------- tangents
def dense_tangents(family, x, layers, act, w_std, b_std, last_w_std):
    """(K, dK/dw^2, dK/db^2) [N,N] of the MLP / dense-ResNet kernel: csrc/grad.hip's forward-mode rules, fp64."""
    x = np.asarray(x, dtype=np.float64)
    w2, b2, lw2 = w_std ** 2, b_std ** 2, last_w_std ** 2
    k = x @ x.T / x.shape[1]
    q = np.einsum("ij,ij->i", x, x) / x.shape[1]
    np.fill_diagonal(k, q)
    kw, kb, qw, qb = np.zeros_like(k), np.zeros_like(k), np.zeros_like(q), np.zeros_like(q)
    resnet = family == "resnet"
    nsets = layers + 1 if resnet else layers

    def dense(k, kw, kb):
        return w2 * k + b2, k + w2 * kw, 1.0 + w2 * kb

    if resnet:
        k, kw, kb = dense(k, kw, kb)
        q, qw, qb = dense(q, qw, qb)
    for s in range(nsets):
        if not resnet:
            k, kw, kb = dense(k, kw, kb)
            q, qw, qb = dense(q, qw, qb)
        o, da, d1, d2 = R.act_d(k, q[:, None], q[None, :], act)
        ow = da * kw + d1 * qw[:, None] + d2 * qw[None, :]
        ob = da * kb + d1 * qb[:, None] + d2 * qb[None, :]
        if act == "relu":
            dq, qo = 0.5, q / 2.0
        else:
            dq = (4 / np.pi) / ((1.0 + 2.0 * q) * np.sqrt(1.0 + 4.0 * q))
            qo = (2 / np.pi) * np.arcsin(2.0 * q / (1.0 + 2.0 * q))
        qow, qob = dq * qw, dq * qb
        if resnet and s != nsets - 1:          # K <- [Dense o act](K) + K
            ka, kaw, kab = dense(o, ow, ob)
            qa, qaw, qab = dense(qo, qow, qob)
            k, kw, kb = k + ka, kw + kaw, kb + kab
            q, qw, qb = q + qa, qw + qaw, qb + qab
        else:
            k, kw, kb, q, qw, qb = o, ow, ob, qo, qow, qob
        for m, dg in ((k, q), (kw, qw), (kb, qb)):
            np.fill_diagonal(m, dg)
    return lw2 * k, lw2 * kw, lw2 * kb


def tangents(family, x, layers, act, w_std, b_std, last_w_std):
    if family in ("mlp", "resnet"):
        return dense_tangents(family, x, layers, act, w_std, b_std, last_w_std)
    if family == "cnn":
        return R.tangent_matrices(x, layers, act, w_std, b_std, last_w_std)
    raise NotImplementedError(family)


def g_parts(k, y, eps, method, alpha, beta):
    """(G, A, -K~^-1, coef, Q, ld) for the kernel matrix k (no jitter) and Y [N,C]."""
    n, c = y.shape
    _, q, ld, a, kinv, coef = head(k + eps * np.eye(n), y, method, alpha, beta)
    return coef * (a @ a.T) - c * kinv, a, -kinv, coef, q, ld


def loss_grad(family, x, y, layers, act, method, w_std, b_std, last_w_std, eps, alpha=2.0, beta=2.0):
    """(loss, {key: d loss / d constrained value}) analytically: 1/2 sum G dK~/d theta and the closed-form (a, b) part."""
    y = np.asarray(y, dtype=np.float64)
    n, c = y.shape
    k, kw, kb = tangents(family, x, layers, act, w_std, b_std, last_w_std)
    g, _, _, _, q, ld = g_parts(k, y, eps, method, alpha, beta)
    terms, _ = R.terms_from(g, k, kw, kb, w_std, b_std, last_w_std)
    lp = head(k + eps * np.eye(n), y, method, alpha, beta)[0]
    dlp = {key: 0.5 * t for key, t in zip(("w_std", "b_std", "last_w_std", "eps"), terms)}
    if method == "tp":
        nu, s, nc = 2.0 * alpha, beta / alpha, n * c
        t = 0.5 * (nu + nc)
        u = q / (s * nu)
        d_s = t * (u / s) / (1.0 + u) - 0.5 * nc / s
        d_nu = -0.5 * np.log1p(u) + t * (u / nu) / (1.0 + u) - 0.5 * nc / nu + 0.5 * digamma(t) - 0.5 * digamma(0.5 * nu)
        dlp["alpha"] = 2.0 * d_nu - d_s * beta / alpha ** 2
        dlp["beta"] = d_s / alpha
    return -lp / n, {key: -v / n for key, v in dlp.items()}


# -------------------------------------------------------------------------------------------------------- prediction
def predict(family, x, y, xt, layers, act, w_std, b_std, last_w_std, eps):
    """NNGPKernel.predict: mean [T,C] and covariance [T,T] under the RELATIVE ridge eps tr(K)/N."""
    args = (layers, act, w_std, b_std, last_w_std)
    return O.predict(kernel(family, x, None, *args), kernel(family, xt, x, *args), kernel(family, xt, None, *args),
                     np.asarray(y, dtype=np.float64), diag_reg=eps)


def predictive_nll(family, x, y, xt, yt, layers, act, method, w_std, b_std, last_w_std, eps, alpha=2.0, beta=2.0,
             y_mean=0.0, y_std=1.0):
    """MultiSPR.test_nll: -mean_t sum_c log p(y_tc) in de-normalised units."""
    y = np.asarray(y, dtype=np.float64)
    n, c = y.shape
    mean, cov = predict(family, x, y, xt, layers, act, w_std, b_std, last_w_std, eps)
    ys = np.asarray(yt, dtype=np.float64) * y_std + y_mean
    ms = mean * y_std + y_mean
    var = np.diag(cov) * y_std ** 2
    if method == "gp":
        lp = O.normal_logpdf(ys, ms, np.sqrt(var)[:, None])
    else:
        nu, s = 2.0 * alpha, beta / alpha
        khat = s * kernel(family, x, None, layers, act, w_std, b_std, last_w_std) + 1e-6 * np.eye(n)   # K WITHOUT eps
        d = nu + float(np.sum(y * np.linalg.solve(khat, y)))
        sigma = np.sqrt(d / (nu + n * c) * s * var)
        lp = O.student_t_logpdf(ys, nu + n * c, ms, sigma[:, None])
    return -float(np.mean(np.sum(lp, axis=1)))


# ------------------------------------------------------------------------------------------------------------- cases
HYP = dict(w_std=1.3, b_std=0.4, last_w_std=0.9, eps=1e-3, alpha=1.7, beta=2.4)
DENSE_NC = [(37, 3), (100, 48), (128, 10), (130, 10)]        # n + C crosses a 128-tile that n + 1 does not; n on / past an edge
DENSE_NETS = [("mlp", "relu"), ("mlp", "erf"), ("resnet", "relu"), ("resnet", "erf")]
DENSE_D, DENSE_LAYERS = 7, 2
CONV_IMAGES = [(6, 6, 2), (8, 8, 3)]
CONV_NC = [(20, 3), (36, 10)]
CONV_LAYERS = 2


def as_seen(a, dtype):
    """The values the device sees when `a` is stored in `dtype`, as fp64."""
    return np.asarray(a).astype(dtype).astype(np.float64)


@functools.lru_cache(maxsize=None)
def dense_data(n, c, f32=False, t=9):
    """(x [n,7], Y [n,c], labels, x_test [t,7], Y_test, labels_test): labels from a random linear read-out of x."""
    rng = np.random.default_rng(1000 * n + c)
    proj = rng.standard_normal((DENSE_D, c))
    xa = rng.standard_normal((n + t, DENSE_D))
    lab = np.argmax(xa @ proj + 0.3 * rng.standard_normal((n + t, c)), axis=1)
    ya = label_targets(lab, c) + 0.05 * rng.standard_normal((n + t, c))
    if f32:
        xa, ya = as_seen(xa, np.float32), as_seen(ya, np.float32)
    for a in (xa, ya, lab):
        a.setflags(write=False)
    return xa[:n], ya[:n], lab[:n], xa[n:], ya[n:], lab[n:]


@functools.lru_cache(maxsize=None)
def conv_data(n, c, h, w, ch, f32=False, t=7):
    rng = np.random.default_rng(100 * n + 10 * h + c)
    proto = rng.standard_normal((c, h, w, ch))
    lab = rng.integers(0, c, size=n + t)
    xa = proto[lab] + 0.7 * rng.standard_normal((n + t, h, w, ch))
    ya = label_targets(lab, c) + 0.05 * rng.standard_normal((n + t, c))
    if f32:
        xa, ya = as_seen(xa, np.float32), as_seen(ya, np.float32)
    for a in (xa, ya, lab):
        a.setflags(write=False)
    return xa[:n], ya[:n], lab[:n], xa[n:], ya[n:], lab[n:]


def _freeze(d):
    return tuple(sorted(d.items()))


@functools.lru_cache(maxsize=None)
def _cached_loss(family, data_key, layers, act, method, hyp):
    x, y = DATA[data_key[0]](*data_key[1:])[:2]
    return loss(family, x, y, layers, act, method, **dict(hyp))


@functools.lru_cache(maxsize=None)
def _cached_grad(family, data_key, layers, act, method, hyp):
    x, y = DATA[data_key[0]](*data_key[1:])[:2]
    return loss_grad(family, x, y, layers, act, method, **dict(hyp))


@functools.lru_cache(maxsize=None)
def _cached_fd(family, data_key, layers, act, method, hyp):
    x, y = DATA[data_key[0]](*data_key[1:])[:2]
    keys = KEYS if method == "tp" else KEYS[:4]
    return loss_fd(family, x, y, layers, act, method, keys, **dict(hyp))


DATA = {"dense": dense_data, "conv": conv_data}


def ref_loss(family, data_key, layers, act, method, hyp=HYP):
    """loss of a named data set (("dense", n, c, f32) or ("conv", n, c, h, w, ch, f32)), computed once per session."""
    return _cached_loss(family, tuple(data_key), layers, act, method, _freeze(hyp))


def ref_grad(family, data_key, layers, act, method, hyp=HYP):
    return _cached_grad(family, tuple(data_key), layers, act, method, _freeze(hyp))


def ref_fd(family, data_key, layers, act, method, hyp=HYP):
    return _cached_fd(family, tuple(data_key), layers, act, method, _freeze(hyp))


# (family, act, layers, data key without the f32 flag): the prediction / classification cases
PRED_CASES = [("mlp", "relu", DENSE_LAYERS, ("dense", 37, 3)), ("resnet", "erf", DENSE_LAYERS, ("dense", 130, 10)),
              ("cnn", "relu", CONV_LAYERS, ("conv", 20, 3, 6, 6, 2))]


@functools.lru_cache(maxsize=None)
def ref_prediction(family, act, layers, data_key, f32=False):
    """dict(mean [T,C], var [T], nll_gp, nll_tp, labels, margin) of a prediction case; margin = the smallest gap between
    the two largest posterior means of a test point, relative to max |mean|."""
    x, y, _, xt, yt, _ = DATA[data_key[0]](*data_key[1:], f32)
    hyp = {k: HYP[k] for k in ("w_std", "b_std", "last_w_std", "eps")}
    mean, cov = predict(family, x, y, xt, layers, act, **hyp)
    top = np.sort(mean, axis=1)
    out = dict(mean=mean, var=np.diag(cov).copy(), labels=np.argmax(mean, axis=1),
               margin=float(np.min(top[:, -1] - top[:, -2])) / float(np.max(np.abs(mean))))
    for method in ("gp", "tp"):
        out["nll_" + method] = predictive_nll(family, x, y, xt, yt, layers, act, method, **HYP)
    return out
