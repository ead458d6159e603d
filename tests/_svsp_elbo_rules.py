"""NumPy fp64 restatement of the negative ELBO of the sparse variational classifier (SVSP.loss, spax/models.py:30-56 of the
reference) and of its analytic gradient, written from the mathematics (shared by test_svsp_elbo_host.py and
test_gpu_svsp_elbo.py; not a test module).

Z = I inducing images, x = B batch images, K = K([Z; x], [Z; x]), C classes, q_var = diag(q_sqrt) as the reference uses it:

    K_abs = K_ZZ + eps I      K_rel = K_ZZ + eps tr(K_ZZ)/I I      Kinv = K_abs^-1      A = K_xZ Kinv      P = K_rel^-1 K_Zx
    mean[c] = A q_mu[c]       cov[c] = A diag(q_var[c]) A^T + K_xx - K_xZ P            L_c = chol(scale cov[c])
    f[c,b,s] = mean[c,b] + sum_k L_c[b,k] xi[c,k,s]            ll = mean_{b,s} log_softmax_c(f)[y_b,b,s]
    kl = 1/2 (C logdet K_ZZ - sum log q_var - I C + sum_c sum_i Kinv_ii q_var[c,i] + s sum_c q_mu[c]^T Kinv q_mu[c])
    loss = -ll + kl / N

xi[c,k,s] is the variate of (seed, point0 + k, class c, draw s) of the library's Philox layout (include/smnngp.h).  The
closed-form inverse-gamma terms of the KL and everything that maps (a, b) to (df, scale, s) are in `prior_terms`.
The gradient Gbar = d loss / d K is returned symmetric: a symmetric perturbation of K_ij = K_ji changes the loss by
(Gbar_ij + Gbar_ji) dK_ij, so sum_ij Gbar_ij dK_ij/d theta is the derivative with respect to a kernel hyper-parameter.
"""
import math

import numpy as np
import scipy.linalg as sla
from scipy.special import digamma, gammaln, logsumexp, polygamma

from _svsp_rules import philox4x32_10

STUDENT_STREAM = 0x80000000


# ---------------------------------------------------------------- variates (fp64 layout of include/smnngp.h)
def bailey(seed, point, cls, draw, df):
    """(t, dt/d df) of Bailey's polar method at the first accepted try; (0, 0) if none of the 64 tries is accepted."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    for blk in range(32):
        r = philox4x32_10((draw, point, cls, STUDENT_STREAM | blk), key)
        for a, b in ((r[0], r[1]), (r[2], r[3])):
            u, v = (a + 0.5) * 2.0 ** -31 - 1.0, (b + 0.5) * 2.0 ** -31 - 1.0
            w = u * u + v * v
            if 0.0 < w <= 1.0:
                lw = math.log(w)
                e = math.expm1(-2.0 / df * lw)                  # w^(-2/df) - 1
                t = u * math.sqrt(df * e / w)
                br = 0.0 if e == 0.0 else 0.5 * (1.0 / df + (2.0 * lw / (df * df)) * (e + 1.0) / e)
                return t, t * br
    return 0.0, 0.0


def normal(seed, point, cls, draw):
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    r = philox4x32_10((draw, point, cls >> 2, 0), key)
    a, b = (r[0], r[1]) if (cls & 3) < 2 else (r[2], r[3])
    rad = math.sqrt(-2.0 * math.log((a + 0.5) * 2.0 ** -32))
    ang = 2.0 * math.pi * (b + 0.5) * 2.0 ** -32
    return rad * (math.cos(ang) if (cls & 1) == 0 else math.sin(ang))


def variates(seed, df, point0, num_batch, num_class, num_samples):
    """xi [C,B,S] and d xi / d df [C,B,S] (zeros for the normal stream, df <= 0)."""
    xi = np.zeros((num_class, num_batch, num_samples))
    dxi = np.zeros_like(xi)
    for c in range(num_class):
        for k in range(num_batch):
            for s in range(num_samples):
                if df > 0:
                    xi[c, k, s], dxi[c, k, s] = bailey(seed, point0 + k, c, s, df)
                else:
                    xi[c, k, s] = normal(seed, point0 + k, c, s)
    return xi, dxi


# ---------------------------------------------------------------- reverse-mode Cholesky
def cholesky_reverse(L, gL):
    """gS = d loss / d S (symmetric) for S = L L^T from gL = d loss / d L (lower): Phi = tril(L^T gL) with the diagonal
    halved, gS = sym(L^-T Phi L^-1) (Murray, arXiv:1602.07527)."""
    phi = np.tril(L.T @ np.tril(gL))
    phi[np.diag_indices_from(phi)] *= 0.5
    y = sla.solve_triangular(L, phi, lower=True, trans="T")               # L^-T Phi
    z = sla.solve_triangular(L, y.T, lower=True, trans="T").T             # (L^-T Phi) L^-1
    return 0.5 * (z + z.T)


# ---------------------------------------------------------------- the correlated softmax head
def head_loss(mean, cov, labels, xi, scale):
    C, B, S = xi.shape
    f = np.empty((C, B, S))
    for c in range(C):
        f[c] = mean[c][:, None] + np.linalg.cholesky(scale * cov[c]) @ xi[c]
    lsm = f - logsumexp(f, axis=0, keepdims=True)
    return float(np.mean(lsm[np.asarray(labels), np.arange(B), :]))


def head(mean, cov, labels, xi, scale, dxi=None):
    """mean [C,B], cov [C,B,B], xi [C,B,S] -> dict(ll, gmean [C,B], gcov [C,B,B], gscale, dfterm) of the loss -ll:
    gmean = d(-ll)/d mean, gcov = d(-ll)/d cov (symmetric), gscale = d(-ll)/d scale, dfterm = sum gf L d xi/d df."""
    mean, cov, xi = (np.asarray(v, dtype=np.float64) for v in (mean, cov, xi))
    C, B, S = xi.shape
    labels = np.asarray(labels)
    Ls = [np.linalg.cholesky(scale * cov[c]) for c in range(C)]
    f = np.stack([mean[c][:, None] + Ls[c] @ xi[c] for c in range(C)])
    lsm = f - logsumexp(f, axis=0, keepdims=True)
    ll = float(np.mean(lsm[labels, np.arange(B), :]))
    gf = np.exp(lsm)
    gf[labels, np.arange(B), :] -= 1.0
    gf /= B * S
    gmean = gf.sum(axis=2)
    gcov = np.empty((C, B, B))
    gscale, dfterm = 0.0, 0.0
    for c in range(C):
        gS = cholesky_reverse(Ls[c], np.tril(gf[c] @ xi[c].T))
        gcov[c] = scale * gS
        gscale += float(np.sum(gS * cov[c]))
        if dxi is not None:
            dfterm += float(np.sum(gf[c] * (Ls[c] @ dxi[c])))
    return dict(ll=ll, gmean=gmean, gcov=gcov, gscale=gscale, dfterm=dfterm)


# ---------------------------------------------------------------- the ELBO
def _blocks(K, I):
    return K[:I, :I], K[:I, I:], K[I:, I:]


def forward(K, I, q_mu, q_var, eps, s, N, labels, xi, scale):
    """(-ll, kl / N) without the closed-form inverse-gamma terms."""
    K = np.asarray(K, dtype=np.float64)
    kzz, kzx, kxx = _blocks(K, I)
    C = q_mu.shape[0]
    eye = np.eye(I)
    kinv = np.linalg.inv(kzz + eps * eye)
    A = kzx.T @ kinv
    P = np.linalg.solve(kzz + eps * np.trace(kzz) / I * eye, kzx)
    bb = kxx - kzx.T @ P
    mean = q_mu @ A.T
    cov = np.einsum("bi,ci,di->cbd", A, q_var, A) + bb[None]
    ll = head_loss(mean, cov, labels, xi, scale)
    kl = 0.5 * (C * np.linalg.slogdet(kzz)[1] - np.sum(np.log(q_var)) - I * C + np.sum(np.diag(kinv)[None, :] * q_var)
                + s * np.einsum("ci,ij,cj->", q_mu, kinv, q_mu))
    return -ll, kl / N


def elbo(K, I, q_mu, q_var, eps, s, N, labels, xi, scale, dxi=None):
    """Everything the device entry returns: nll, kl_n, g_q_mu, g_q_var [C,I], g_eps, gscale, g_s, dfterm, gbar [U,U],
    cond (of K_abs)."""
    K = np.asarray(K, dtype=np.float64)
    q_mu, q_var = np.asarray(q_mu, dtype=np.float64), np.asarray(q_var, dtype=np.float64)
    kzz, kzx, kxx = _blocks(K, I)
    C = q_mu.shape[0]
    eye = np.eye(I)
    k_abs = kzz + eps * eye
    kinv = np.linalg.inv(k_abs)
    kinv = 0.5 * (kinv + kinv.T)
    k_rel = kzz + eps * np.trace(kzz) / I * eye
    A = kzx.T @ kinv
    P = np.linalg.solve(k_rel, kzx)
    bb = kxx - kzx.T @ P
    mean = q_mu @ A.T
    cov = np.einsum("bi,ci,di->cbd", A, q_var, A) + bb[None]
    h = head(mean, cov, labels, xi, scale, dxi)
    quad = float(np.einsum("ci,ij,cj->", q_mu, kinv, q_mu))
    kd = np.diag(kinv)
    kl = 0.5 * (C * np.linalg.slogdet(kzz)[1] - np.sum(np.log(q_var)) - I * C + np.sum(kd[None, :] * q_var) + s * quad)
    gmean, gcov = h["gmean"], h["gcov"]
    g_q_mu = gmean @ A + s * (q_mu @ kinv) / N
    g_q_var = np.einsum("bi,cbd,di->ci", A, gcov, A) + (kd[None, :] - 1.0 / q_var) / (2.0 * N)
    gA = gmean.T @ q_mu + 2.0 * np.einsum("cbd,di,ci->bi", gcov, A, q_var)
    gbb = gcov.sum(axis=0)
    m = kzx @ gA
    g_kinv = 0.5 * (m + m.T) + (np.diag(q_var.sum(axis=0)) + s * q_mu.T @ q_mu) / (2.0 * N)
    gk_abs = -kinv @ g_kinv @ kinv
    gk_rel = P @ gbb @ P.T
    g_zz = gk_abs + gk_rel + eps / I * np.trace(gk_rel) * eye + C * np.linalg.inv(kzz) / (2.0 * N)
    g_xz = gA @ kinv - 2.0 * gbb @ P.T                                    # total derivative w.r.t. the [B,I] block
    U = K.shape[0]
    gbar = np.zeros((U, U))
    gbar[:I, :I] = 0.5 * (g_zz + g_zz.T)
    gbar[I:, I:] = 0.5 * (gbb + gbb.T)
    gbar[I:, :I] = 0.5 * g_xz
    gbar[:I, I:] = 0.5 * g_xz.T
    g_eps = np.trace(gk_abs) + np.trace(kzz) / I * np.trace(gk_rel)
    return dict(nll=-h["ll"], kl_n=kl / N, g_q_mu=g_q_mu, g_q_var=g_q_var, g_eps=float(g_eps), gscale=h["gscale"],
                g_s=0.5 * quad / N, dfterm=h["dfterm"], gbar=gbar, cond=float(np.linalg.cond(k_abs)),
                mean=mean, cov=cov)


# ---------------------------------------------------------------- the mixing prior
def prior_terms(a=None, b=None, alpha=None, beta=None):
    """GaussianPrior (a is None) or InverseGammaPrior -> dict(df, scale, s, kl_extra, d_extra_a, d_extra_b): the
    closed-form terms of priors.py:78-81 and their derivatives with respect to the constrained a and b."""
    if a is None:
        return dict(df=0.0, scale=1.0, s=1.0, kl_extra=0.0, d_extra_a=0.0, d_extra_b=0.0)
    extra = (alpha * math.log(b / beta) - gammaln(a) + gammaln(alpha) + (a - alpha) * digamma(a) + (beta - b) * a / b)
    return dict(df=2.0 * a, scale=b / a, s=a / b, kl_extra=float(extra),
                d_extra_a=float((a - alpha) * polygamma(1, a) + (beta - b) / b),
                d_extra_b=float(alpha / b - a * beta / (b * b)))


def prior_grads(res, pt, a, b, N):
    """d loss / d (a, b) from an `elbo` result and `prior_terms`."""
    g_a = 2.0 * res["dfterm"] - res["gscale"] * b / (a * a) + res["g_s"] / b + pt["d_extra_a"] / N
    g_b = res["gscale"] / a - res["g_s"] * a / (b * b) + pt["d_extra_b"] / N
    return g_a, g_b


def relerr_norm(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), np.finfo(np.float64).tiny))
