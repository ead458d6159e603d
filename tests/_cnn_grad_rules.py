"""NumPy fp64 restatement of the forward-mode rules of csrc/cnn_grad.hip (shared by test_cnn_grad_abi.py and
test_gpu_cnn_grad.py; not a test module), and the conv SPR loss composed from the fp64 reference kernel.

For an image pair the state is three H x W maps (K, Kw = dK/dw^2, Kb = dK/db^2); per image the diagonal has (q, qw, qb).
    Conv:  Kw <- box(K)/9 + w^2 box(Kw)/9    Kb <- 1 + w^2 box(Kb)/9    K <- w^2 box(K)/9 + b^2
    Act:   Kw <- phi_A Kw + phi_qi qw_n + phi_qj qw_m   (Kb likewise);   K <- phi(K, q_n, q_m)
    Flatten + Dense:  lw^2 * mean over pixels
"""
import numpy as np

from oracle import nngp_oracle as O


def box3(a):
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)])
    h, w = a.shape[-2:]
    out = np.zeros_like(a)
    for dh in range(3):
        for dw in range(3):
            out += p[..., dh:dh + h, dw:dw + w]
    return out


def act_d(k, qi, qj, act):
    """(phi, phi_A, phi_qi, phi_qj) per pixel; qi / qj broadcast against k."""
    if act == "relu":
        sp = np.sqrt(qi * qj)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(sp > 0, k / sp, 0.0)
        c = np.clip(c, -1.0, 1.0)
        s1 = np.sqrt(np.maximum((1.0 - c) * (1.0 + c), 0.0))
        pm = np.pi - np.arccos(c)
        o = sp * (s1 + pm * c) / (2 * np.pi)
        da = pm / (2 * np.pi) + 0.0 * sp
        with np.errstate(divide="ignore", invalid="ignore"):   # zero variance: not differentiable, no variance-side term
            d1 = np.where(qi > 0, s1 * sp / (4 * np.pi * qi), 0.0)
            d2 = np.where(qj > 0, s1 * sp / (4 * np.pi * qj), 0.0)
        return o, da, d1, d2
    ti, tj = 1.0 + 2.0 * qi, 1.0 + 2.0 * qj
    sp = np.sqrt(ti * tj)
    s = np.clip(2.0 * k / sp, -1.0, 1.0)
    den = np.sqrt(np.maximum((1.0 - s) * (1.0 + s), 1e-300))
    o = (2 / np.pi) * np.arcsin(s)
    return o, 4.0 / (np.pi * sp * den), -(2 / np.pi) * s / (den * ti), -(2 / np.pi) * s / (den * tj)


def cnn_tangents(x, layers, act, w_std, b_std, last_w_std, rows=None):
    """(K, dK/dw^2, dK/db^2), each [len(rows), n], for image rows `rows` (default: all) against all images; the entries
    with row == column hold the exact per-image values, as the device code does."""
    x = np.asarray(x, dtype=np.float64)
    n, c = x.shape[0], x.shape[-1]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    w2, b2, lw2 = w_std ** 2, b_std ** 2, last_w_std ** 2
    k = np.einsum("nhwc,mhwc->nmhw", x[rows], x) / c
    kw, kb = np.zeros_like(k), np.zeros_like(k)
    q = np.einsum("nhwc,nhwc->nhw", x, x) / c
    qw, qb = np.zeros_like(q), np.zeros_like(q)
    for _ in range(layers):
        bk = box3(k)
        kw = bk / 9.0 + w2 * box3(kw) / 9.0
        kb = 1.0 + w2 * box3(kb) / 9.0
        k = w2 * bk / 9.0 + b2
        bq = box3(q)
        qw = bq / 9.0 + w2 * box3(qw) / 9.0
        qb = 1.0 + w2 * box3(qb) / 9.0
        q = w2 * bq / 9.0 + b2
        o, da, d1, d2 = act_d(k, q[rows][:, None], q[None, :], act)
        kw = da * kw + d1 * qw[rows][:, None] + d2 * qw[None, :]
        kb = da * kb + d1 * qb[rows][:, None] + d2 * qb[None, :]
        k = o
        if act == "relu":
            dq, q = 0.5, q / 2.0
        else:
            dq = (4 / np.pi) / ((1.0 + 2.0 * q) * np.sqrt(1.0 + 4.0 * q))
            q = (2 / np.pi) * np.arcsin(2.0 * q / (1.0 + 2.0 * q))
        qw, qb = dq * qw, dq * qb
    out = [lw2 * a.mean(axis=(2, 3)) for a in (k, kw, kb)]
    ri = np.arange(len(rows))
    for a, d in zip(out, (q, qw, qb)):
        a[ri, rows] = lw2 * d.mean(axis=(1, 2))[rows]
    return out


def tangent_matrices(x, layers, act, w_std, b_std, last_w_std, block=None):
    """cnn_tangents for all rows, evaluated `block` rows at a time (the per-pixel arrays are [block, n, H, W])."""
    n = np.asarray(x).shape[0]
    block = block or n
    parts = [cnn_tangents(x, layers, act, w_std, b_std, last_w_std, np.arange(r0, min(n, r0 + block)))
             for r0 in range(0, n, block)]
    return [np.concatenate([p[i] for p in parts], axis=0) for i in range(3)]


def terms_from(g, k, kw, kb, w_std, b_std, last_w_std):
    """terms[0..3] = sum_nm G_nm dK~_nm/d(w_std, b_std, last_w_std, eps), and the same sums over |G| |dK~/d theta| (the
    scale a rounding-error bound has to be relative to: the terms of the sum may cancel)."""
    t, ta = np.zeros(4), np.zeros(4)
    for i, (f, d) in enumerate(((2.0 * w_std, kw), (2.0 * b_std, kb), (2.0 / last_w_std, k))):
        t[i] = f * np.sum(g * d)
        ta[i] = abs(f) * np.sum(np.abs(g) * np.abs(d))
    t[3], ta[3] = np.trace(g), np.abs(np.diag(g)).sum()
    return t, ta


def contract(g, x, layers, act, w_std, b_std, last_w_std, block=None):
    k, kw, kb = tangent_matrices(x, layers, act, w_std, b_std, last_w_std, block)
    return terms_from(g, k, kw, kb, w_std, b_std, last_w_std)


def g_matrix(k, y, eps, method, alpha, beta):
    """(G = coef alpha alpha^T - K~^-1, K~^-1 y, -K~^-1, coef, quad, logdet, df, scale) in NumPy fp64."""
    n = k.shape[0]
    kt = k + eps * np.eye(n)
    kinv = np.linalg.inv(kt)
    kinv = 0.5 * (kinv + kinv.T)
    al = kinv @ y
    quad = float(y @ al)
    logdet = float(np.linalg.slogdet(kt)[1])
    df, scale = (0.0, 1.0) if method == "gp" else (2.0 * alpha, beta / alpha)
    coef = 1.0 if method == "gp" else (df + n) / ((df + quad / scale) * scale)
    return coef * np.outer(al, al) - kinv, al, -kinv, coef, quad, logdet, df, scale


def ref_loss(x, y, layers, act, method, w_std, b_std, last_w_std, eps, alpha=2.0, beta=2.0):
    """SPR.loss of a conv model from the fp64 reference pieces: -logpdf / N with cov = K + eps I."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    k = O.cnn_kernel(x, None, layers, act, w_std, b_std, last_w_std)
    n = k.shape[0]
    cov = k + O.jitter(n, eps)
    lp = O.mvn_logpdf(y, cov) if method == "gp" else O.mvt_logpdf(y, (beta / alpha) * cov, 2.0 * alpha)
    return -lp / n


def ref_grad_fd(x, y, layers, act, method, keys, h=1e-5, **hyp):
    """Central differences of ref_loss with respect to the constrained values, relative step h (as spr_loss_grad_fd)."""
    out = {}
    for k in keys:
        v = float(hyp[k])
        step = h * abs(v) if v != 0.0 else h
        up = dict(hyp); up[k] = v + step
        dn = dict(hyp); dn[k] = v - step
        out[k] = (ref_loss(x, y, layers, act, method, **up) - ref_loss(x, y, layers, act, method, **dn)) / (2.0 * step)
    return out
