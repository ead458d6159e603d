"""NumPy fp64 restatement of SVSP.test_acc_nll (shared by test_svsp_host.py and test_gpu_svsp.py; not a test module),
written from the mathematics, on the fp64 reference kernels of oracle/nngp_oracle.py:

    K_rel = K_ZZ + eps tr(K_ZZ)/I I          K_abs = K_ZZ + eps I
    mean  = K_tZ K_rel^-1 q_mu^T             cov = K_tt - K_tZ K_rel^-1 K_Zt            A = K_tZ K_abs^-1
    test_cov[c] = A diag(q_var[c]) A^T + cov ;  only its diagonal is sampled from:  var[t,c] = cov[t,t] + sum_j A[t,j]^2 q_var[c,j]
    f[c,t,s] = mean[t,c] + sigma[t,c] xi[c,t,s],  sigma = sqrt(scale var)   (scale = 1 Gaussian, b/a inverse-gamma: t_{2a} variates)
    lsm = f - logsumexp_c f ;  ll[t] = logsumexp_s lsm[y_t,t,s] - log S ;  score[t,c] = logsumexp_s lsm[c,t,s] ;  pred = argmax_c
Also a pure-Python Philox4x32-10, the generator the device head uses, for the published known-answer vectors.
"""
import numpy as np
from scipy.special import logsumexp

from oracle import nngp_oracle as O


def kernel_fn(network="cnn", **kw):
    base = O.cnn_kernel if network == "cnn" else O.conv_resnet_kernel
    return lambda x1, x2=None: base(x1, x2, **kw)


def moments_literal(kfn, z, x, q_mu, q_var, eps):
    """The reference's own sequence of operations: the full [B,B] covariance, einsum("ij,cjk,kl->cil"), then the diagonal.
    Returns mean [T,C], var [T,C]."""
    k_ii, k_bi, k_bb = kfn(z), kfn(x, z), kfn(x)
    n_i = k_ii.shape[0]
    k_ii_inv = np.linalg.inv(k_ii + eps * np.eye(n_i))
    mean, cov = O.predict(k_ii, k_bi, k_bb, q_mu.T, diag_reg=eps)                     # [B,C], [B,B]
    a_b = k_bi @ k_ii_inv
    q_sigma = np.einsum("ci,ij->cij", q_var, np.eye(n_i))
    test_cov = np.einsum("ij,cjk,kl->cil", a_b, q_sigma, a_b.T) + cov[None]          # [C,B,B]
    return mean, np.diagonal(test_cov, axis1=-2, axis2=-1).T.copy()


def moments(k_zz, k_zt, ktt_diag, q_mu, q_var, eps):
    """The diagonal-only form from kernel blocks: k_zz [I,I], k_zt [I,T], ktt_diag [T] -> mean [T,C], var [T,C], cond(K_rel)."""
    import scipy.linalg as sla
    k_zz, k_zt = np.asarray(k_zz, dtype=np.float64), np.asarray(k_zt, dtype=np.float64)
    n_i = k_zz.shape[0]
    k_rel = k_zz + eps * np.trace(k_zz) / n_i * np.eye(n_i)
    k_abs = k_zz + eps * np.eye(n_i)
    cf = sla.cho_factor(k_rel, lower=True)
    b = sla.cho_solve(cf, k_zt)                                                        # [I,T]
    mean = b.T @ np.asarray(q_mu, dtype=np.float64).T
    v0 = np.asarray(ktt_diag, dtype=np.float64) - np.einsum("jt,jt->t", k_zt, b)
    a = sla.cho_solve(sla.cho_factor(k_abs, lower=True), k_zt).T                       # [T,I]
    var = v0[:, None] + (a * a) @ np.asarray(q_var, dtype=np.float64).T
    return mean, var, float(np.linalg.cond(k_rel))


def moments_diag(kfn, z, x, q_mu, q_var, eps):
    k_tt = np.array([kfn(x[i:i + 1])[0, 0] for i in range(len(x))])
    mean, var, _ = moments(kfn(z), kfn(z, x), k_tt, q_mu, q_var, eps)
    return mean, var


def head(mean, sigma, labels, noise):
    """mean, sigma [T,C]; noise [T,C,S] standard variates -> ll [T], score [T,C], pred [T], all fp64."""
    mean, sigma, noise = (np.asarray(v, dtype=np.float64) for v in (mean, sigma, noise))
    f = mean[:, :, None] + sigma[:, :, None] * noise
    lsm = f - logsumexp(f, axis=1, keepdims=True)
    score = logsumexp(lsm, axis=2)
    ll = score[np.arange(len(labels)), np.asarray(labels)] - np.log(noise.shape[2])
    return ll, score, np.argmax(score, axis=1)


def head_statistics(mean, sigma, labels, noise):
    """The reference head at S_ref draws, with what a comparison at fewer draws needs: per point and class
    p = mean_s exp(lsm) and sd = std_s exp(lsm); the standard error of log mean_S p at S draws is sd / (p sqrt(S))
    (delta method)."""
    mean, sigma, noise = (np.asarray(v, dtype=np.float64) for v in (mean, sigma, noise))
    f = mean[:, :, None] + sigma[:, :, None] * noise
    p_draw = np.exp(f - logsumexp(f, axis=1, keepdims=True))
    p, sd = p_draw.mean(axis=2), p_draw.std(axis=2)
    score = np.log(p) + np.log(noise.shape[2])
    ll = np.log(p[np.arange(len(labels)), np.asarray(labels)])
    return ll, score, p, sd


# ---------------------------------------------------------------- Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11)
def philox4x32_10(ctr, key):
    c, k, m = [int(v) for v in ctr], [int(v) for v in key], 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & m, (p0 >> 32) ^ c[3] ^ k[1], p0 & m]
        k = [(k[0] + 0x9E3779B9) & m, (k[1] + 0xBB67AE85) & m]
    return c


PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


# ---------------------------------------------------------------- the fixture of the GPU tests
def fixture(num_inducing=40, num_test=256, num_class=4, hw=8, seed=5):
    rng = np.random.default_rng(seed)
    templates = rng.standard_normal((num_class, hw, hw, 1))

    def images(n):
        lab = rng.integers(0, num_class, n)
        return templates[lab] + 1.6 * rng.standard_normal((n, hw, hw, 1)), lab

    z, zl = images(num_inducing)
    x, y = images(num_test)
    q_mu = 2.0 * np.eye(num_class)[zl].T + 0.1 * rng.standard_normal((num_class, num_inducing))
    q_var = 0.01 + 0.05 * np.abs(rng.standard_normal((num_class, num_inducing)))
    kw = dict(num_hiddens=3, act="relu", w_std=1.2, b_std=0.1, last_w_std=1.0)
    return dict(z=z, x=x, y=y.astype(np.int32), q_mu=q_mu, q_var=q_var, kernel=kw)


# ---------------------------------------------------------------- statistics of a block of variates
def variate_statistics(xi, df):
    """xi [P,C,S] standard variates (df <= 0: normal, else Student-t(df)) -> (N, Kolmogorov-Smirnov D, {name: |correlation|}).
    Correlations: lag 1 along the draws, adjacent classes, adjacent points -- of the probability-integral transform
    u = F(xi) ("u_*": defined for every df), and of the raw variates where their fourth moment is finite (normal,
    df > 4; a Pearson correlation of Cauchy or t_4 samples does not concentrate like 1/sqrt(N))."""
    from scipy import stats
    dist = stats.norm() if df <= 0 else stats.t(df)
    xi = np.asarray(xi, dtype=np.float64)
    n = xi.size
    d = stats.kstest(xi.ravel(), dist.cdf).statistic

    def corr(a, b):
        a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
        return abs(float(a @ b / np.sqrt((a @ a) * (b @ b))))

    def three(v, tag):
        return {tag + "lag1": corr(v[:, :, :-1], v[:, :, 1:]), tag + "class": corr(v[:, :-1], v[:, 1:]),
                tag + "point": corr(v[:-1], v[1:])}

    out = three(dist.cdf(xi), "u_")
    if df <= 0 or df > 4:
        out.update(three(xi, ""))
    return n, d, out
