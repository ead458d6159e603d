"""NumPy / SciPy fp64 restatement of leave-one-out cross-validation for the exact C-output GP / Student-t process (SPR at
C = 1, MultiSPR): the log-pdf of every point given all the others, its sum Lambda, the leave-one-out mean and scale, the seed G
(d Lambda = sum_ij G_ij dK~_ij) and the gradient of the loss -Lambda / N with respect to all six trainables.  Shared by
test_loo_host.py and test_gpu_loo.py; not a test module.

Y [N,C], K~ = K + eps I, P = K~^-1, A = P Y, p_i = P_ii, Q = sum_ic Y_ic A_ic, e_i = sum_c A_ic^2 / p_i; leaving out point i
leaves out all C outputs of that point:
    mean       mu_ic = Y_ic - A_ic / p_i
    Gaussian   variance 1 / p_i,  log p_i = -(C/2) log 2 pi + (C/2) log p_i - e_i / 2
    Student-t  vec(Y) ~ MVT_NC(nu = 2a, 0, s (I_C x K~)), s = b/a: a C-variate t with nu + (N-1) C degrees of freedom,
               shape sigma_i^2 I_C, sigma_i^2 = (nu + (Q - e_i)/s) / (nu + (N-1) C) * s / p_i
    G = -1/2 (U A^T + A U^T) - P diag(d) P - lQ A A^T,  U = P a,  a_ic = 2 le_i A_ic / p_i,  d_i = C/(2 p_i) - le_i e_i / p_i
`brute` is the definition itself (the joint density over the marginal density of the other N - 1 points, scipy.stats): when the
closed forms and it disagree, it decides.
"""
import functools

import numpy as np
from scipy.special import digamma, gammaln

import _cnn_grad_rules as R
import _multi_rules as M

KEYS = M.KEYS


def parts(p_mat, a, y, method, alpha=2.0, beta=2.0, rows=None):
    """Everything the head returns, from P = K~^-1 (symmetric), A = P Y and Y, in fp64.  rows: G (and its scale g_abs) for
    those rows only, [len(rows), N] -- O(len(rows) N^2) instead of O(N^3).  lam_abs / dhead_abs: the sums of the magnitudes
    of the terms that make up Lambda and d Lambda / d(df, scale), the scale their rounding errors are relative to."""
    p_mat, a, y = (np.asarray(v, dtype=np.float64) for v in (p_mat, a, y))
    n, c = y.shape
    p = np.diag(p_mat).copy()
    q = float(np.sum(y * a))
    e = np.sum(a * a, axis=1) / p
    mean = y - a / p[:, None]
    if method == "gp":
        lp = -0.5 * c * np.log(2.0 * np.pi) + 0.5 * c * np.log(p) - 0.5 * e
        lam_abs = float(np.sum(0.5 * c * np.log(2.0 * np.pi) + 0.5 * c * np.abs(np.log(p)) + 0.5 * e))
        scale2 = 1.0 / p
        le = np.full(n, -0.5)
        lq = 0.0
        dhead, dhead_abs = np.zeros(2), np.zeros(2)
        df_out = None
    else:
        nu, s = 2.0 * alpha, beta / alpha
        m1, m2 = 0.5 * (nu + (n - 1) * c), 0.5 * (nu + n * c)
        # Q - e_i cancels completely at n = 1 and largely at small n: the difference is taken in extended precision
        al, yl = a.astype(np.longdouble), y.astype(np.longdouble)
        qme = (np.sum(yl * al) - np.sum(al * al, axis=1) / p.astype(np.longdouble)).astype(np.float64)
        ti, tq = nu + qme / s, nu + q / s
        lp = (gammaln(m2) - gammaln(m1) - 0.5 * c * np.log(np.pi) - 0.5 * c * np.log(s) + 0.5 * c * np.log(p)
              + m1 * np.log(ti) - m2 * np.log(tq))
        scale2 = ti / (nu + (n - 1) * c) * s / p
        le = -m1 / (s * ti)
        lq = float(np.sum(m1 / (s * ti)) - n * m2 / (s * tq))
        d_nu = np.sum(0.5 * digamma(m2) - 0.5 * digamma(m1) + 0.5 * np.log(ti) + m1 / ti - 0.5 * np.log(tq) - m2 / tq)
        d_s = np.sum(-0.5 * c / s - m1 * qme / (s * s * ti) + m2 * q / (s * s * tq))
        dhead = np.array([d_nu, d_s])
        lam_abs = float(np.sum(abs(gammaln(m2)) + abs(gammaln(m1)) + 0.5 * c * abs(np.log(np.pi)) + 0.5 * c * abs(np.log(s))
                               + 0.5 * c * np.abs(np.log(p)) + m1 * np.abs(np.log(ti)) + m2 * abs(np.log(tq))))
        dhead_abs = np.array([np.sum(0.5 * abs(digamma(m2)) + 0.5 * abs(digamma(m1)) + 0.5 * np.abs(np.log(ti)) + m1 / ti
                                     + 0.5 * abs(np.log(tq)) + m2 / tq),
                              np.sum(0.5 * c / s + m1 * np.abs(q - e) / (s * s * ti) + m2 * abs(q) / (s * s * tq))])
        df_out = nu + (n - 1) * c
    acoef = 2.0 * le[:, None] * a / p[:, None]
    d = 0.5 * c / p - le * e / p
    u = p_mat @ acoef
    sel = slice(None) if rows is None else np.asarray(rows)
    g = -0.5 * (u[sel] @ a.T + a[sel] @ u.T) - (p_mat[sel] * d[None, :]) @ p_mat - lq * (a[sel] @ a.T)
    # the scale of a rounding bound on G: |P| |D| |P| + |U| |A|^T + |A| |U|^T + |lQ| |A| |A|^T
    ap, aa, au = np.abs(p_mat), np.abs(a), np.abs(u)
    g_abs = (ap[sel] * np.abs(d)[None, :]) @ ap + au[sel] @ aa.T + aa[sel] @ au.T + abs(lq) * (aa[sel] @ aa.T)
    return dict(lp=lp, lam=float(np.sum(lp)), lam_abs=lam_abs, mean=mean, scale2=scale2, df=df_out, g=g, g_abs=g_abs,
                dhead=dhead, dhead_abs=dhead_abs, p=p, e=e, q=q, q_abs=float(np.sum(np.abs(y * a))), d=d, u=u, lq=lq)


def from_matrix(kt, y, method, alpha=2.0, beta=2.0):
    """parts() for the matrix K~ (jitter included); raises LinAlgError when it is not positive definite."""
    np.linalg.cholesky(kt)
    p_mat = np.linalg.inv(kt)
    p_mat = 0.5 * (p_mat + p_mat.T)
    y = np.asarray(y, dtype=np.float64)
    return parts(p_mat, p_mat @ y, y, method, alpha, beta)


def brute(kt, y, method, alpha=2.0, beta=2.0):
    """log p(Y_i | Y_-i) for every i by literally deleting point i: log p(Y) - log p(Y_-i) under the joint prior."""
    from scipy.stats import multivariate_normal, multivariate_t
    kt, y = np.asarray(kt, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, c = y.shape

    def joint(k, yy):
        if yy.shape[0] == 0:
            return 0.0
        cov = np.kron(np.eye(c), k)
        v = yy.T.reshape(-1)
        if method == "gp":
            return float(multivariate_normal(np.zeros(v.size), cov).logpdf(v))
        return float(multivariate_t(np.zeros(v.size), (beta / alpha) * cov, df=2.0 * alpha).logpdf(v))

    full = joint(kt, y)
    out = np.zeros(n)
    for i in range(n):
        keep = np.arange(n) != i
        out[i] = full - joint(kt[np.ix_(keep, keep)], y[keep])
    return out


def brute_moments(kt, y, i):
    """Mean [C] and variance factor of the Gaussian conditional of point i given the others (the Student-t location is the
    same; its shape rescales this variance)."""
    n = kt.shape[0]
    keep = np.arange(n) != i
    if n == 1:
        return np.zeros(y.shape[1]), float(kt[0, 0])
    sol = np.linalg.solve(kt[np.ix_(keep, keep)], np.column_stack([y[keep], kt[keep, i]]))
    return kt[i, keep] @ sol[:, :-1], float(kt[i, i] - kt[i, keep] @ sol[:, -1])


def loss(family, x, y, layers, act, method, w_std, b_std, last_w_std, eps, alpha=2.0, beta=2.0):
    """loo_loss: -Lambda / N."""
    k = M.kernel(family, x, None, layers, act, w_std, b_std, last_w_std)
    n = k.shape[0]
    return -from_matrix(k + eps * np.eye(n), y, method, alpha, beta)["lam"] / n


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


def head_grads(dhead, n, alpha, beta):
    """d loss / d(alpha, beta) from d Lambda / d(df, scale): df = 2 alpha, scale = beta / alpha."""
    return {"alpha": -(2.0 * dhead[0] - dhead[1] * beta / alpha ** 2) / n, "beta": -(dhead[1] / alpha) / n}


def loss_grad(family, x, y, layers, act, method, w_std, b_std, last_w_std, eps, alpha=2.0, beta=2.0):
    """(loss, {key: d loss / d constrained value}, terms, terms_abs): d Lambda / d theta = sum_ij G_ij dK~_ij / d theta."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    k, kw, kb = M.tangents(family, x, layers, act, w_std, b_std, last_w_std)
    r = from_matrix(k + eps * np.eye(n), y, method, alpha, beta)
    terms, terms_abs = R.terms_from(r["g"], k, kw, kb, w_std, b_std, last_w_std)
    grads = {key: -t / n for key, t in zip(("w_std", "b_std", "last_w_std", "eps"), terms)}
    if method == "tp":
        grads.update(head_grads(r["dhead"], n, alpha, beta))
    return -r["lam"] / n, grads, terms, terms_abs


def as_seen(a, dtype):
    return M.as_seen(a, dtype)


def spd_case(n, c, seed=0):
    """A well-conditioned SPD matrix K~ [n,n] (cond <= ~30) with its inverse P, targets Y [n,c] and A = P Y, fp64."""
    rng = np.random.default_rng(7000 + 31 * n + c + seed)
    b = rng.standard_normal((n, n + 3)) / np.sqrt(n + 3)
    kt = b @ b.T + 0.5 * np.eye(n)
    p_mat = np.linalg.inv(kt)
    p_mat = 0.5 * (p_mat + p_mat.T)
    y = rng.standard_normal((n, c))
    return kt, p_mat, y, p_mat @ y


@functools.lru_cache(maxsize=None)
def head_case(n, c, f32):
    """(-P, A, Y) as the device sees them in the storage type (fp64 values), read-only; the rules are fed exactly these."""
    _, p_mat, y, a = spd_case(n, c)
    dt = np.float32 if f32 else np.float64
    out = tuple(as_seen(v, dt) for v in (-p_mat, a, y))
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def head_ref(n, c, f32, method, alpha=1.7, beta=2.4):
    nk, a, y = head_case(n, c, f32)
    return parts(-nk, a, y, method, alpha, beta)
