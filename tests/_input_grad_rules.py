"""The derivative of an MLP / dense-ResNet kernel entry in its FIRST argument, and the predictive gradients built on it, restated
in NumPy (test infrastructure, not a test module).

K(x1_r, x2_j) = F(u, v) with u = x1_r . x2_j / d and v = |x1_r|^2 / d (x2 a constant):

    dK_rj/dx1_r = (F_1 x2_j + 2 F_2 x1_r) / d,      F_1 = dF/du,  F_2 = dF/dv

F_1, F_2 by forward mode through the layer stack, seeds k_u = 1, k_v = 0, dq_r/dv = p_r, every column-side tangent 0.  With
phi, D = phi_A, phi_1 = dphi/dq_r, D_A, D_1 of the activation map and t in {u, v}:

    Dense(w2, b2):  A = w2 k + b2,  A_t = w2 k_t;   NTK: T = A + w2 Theta,  T_t = A_t + w2 Theta_t
    activation:     k <- phi(A),  k_u <- D A_u,  k_v <- D A_v + phi_1 p_r
                    NTK: Theta <- T D,  Theta_u <- T_u D + T D_A A_u,  Theta_v <- T_v D + T (D_A A_v + D_1 p_r)
    last Dense:     K = lw2 k,  Theta_out = lw2 (k + Theta)

in the order of oracle.mlp_kernel / oracle.dense_resnet_kernel.  Guards at the singular points (the conventions of the device
code): ReLU where (1 - c)(1 + c) <= 0 after clamping has D_A = D_1 = 0; a zero-variance row (ReLU, q = 0) has c = 0, as
oracle.relu_map defines it, and no variance-side term.

Every function takes `dtype` and keeps ALL its arithmetic in it: the float32 evaluation against the float64 one is the yardstick
of the device tests.
"""
import numpy as np
import scipy.linalg as sla

from oracle import nngp_oracle as O

KERNELS = {"mlp": O.mlp_kernel, "resnet": O.dense_resnet_kernel}


def _act(act, a, qi, qj):
    """(phi, D, phi_1, D_A, D_1) of the activation map at pre-activation covariance a [n1, n2], row variances qi [n1] and column
    variances qj [n2]; derivatives with respect to a and to q_i (the row side)."""
    dt = a.dtype.type
    pi = dt(np.pi)
    qi_c = qi[:, None]
    if act == "relu":
        sp = np.sqrt(np.outer(qi, qj))
        ok = sp > 0
        spg = np.where(ok, sp, dt(1))
        qig = np.where(qi_c > 0, qi_c, dt(1))
        c = np.clip(np.where(ok, a / spg, dt(0)), dt(-1), dt(1))
        om = (dt(1) - c) * (dt(1) + c)
        flat = ~(om > 0)
        s1 = np.sqrt(np.maximum(om, dt(0)))
        s1g = np.where(flat, dt(1), s1)
        pm = pi - np.arccos(c)
        phi = sp * (s1 + pm * c) / (dt(2) * pi)
        big_d = pm / (dt(2) * pi)
        phi1 = np.where(qi_c > 0, s1 * sp / (dt(4) * pi * qig), dt(0))
        d_a = np.where(flat | ~ok, dt(0), dt(1) / (dt(2) * pi * s1g * spg))
        d_1 = np.where(flat | ~(qi_c > 0), dt(0), -c / (dt(4) * pi * qig * s1g))
        return phi, big_d, phi1, d_a, d_1
    if act == "erf":
        ti, tj = dt(1) + dt(2) * qi_c, dt(1) + dt(2) * qj[None, :]
        sp = np.sqrt(ti * tj)
        s = np.clip(dt(2) * a / sp, dt(-1), dt(1))
        den = np.sqrt(np.maximum(dt(1) - s * s, dt(1e-300 if a.dtype == np.float64 else 1e-30)))
        phi = (dt(2) / pi) * np.arcsin(s)
        big_d = dt(4) / (pi * sp * den)
        phi1 = -(dt(2) / pi) * s / (den * ti)
        r32 = (sp * den) ** 3
        d_a = dt(16) * a / (pi * r32)
        d_1 = -dt(4) * tj / (pi * r32)
        return phi, big_d, phi1, d_a, d_1
    raise KeyError(act)


def _act_diag(act, q):
    """(phi, phi', D, D') on the diagonal, as functions of the variance q entering the activation."""
    dt = q.dtype.type
    pi = dt(np.pi)
    if act == "relu":
        return q / dt(2), np.full_like(q, 0.5), np.full_like(q, 0.5), np.zeros_like(q)
    t1, t2 = dt(1) + dt(2) * q, dt(1) + dt(4) * q
    r2 = np.sqrt(t2)
    return ((dt(2) / pi) * np.arcsin(dt(2) * q / t1), (dt(4) / pi) / (t1 * r2), (dt(4) / pi) / r2, -(dt(8) / pi) / (t2 * r2))


def _diag_chain(kind, act, q0, num_hiddens, w2, b2):
    """The per-row diagonal recursion: the list of (q, p = dq/dq0) entering each activation, and the final (q, q', theta,
    theta') behind the last activation (theta: the tangent kernel's diagonal, T for the ResNet's blocks)."""
    q, qt = q0.copy(), np.ones_like(q0)
    th, tht = np.zeros_like(q0), np.zeros_like(q0)
    nsets = num_hiddens if kind == "mlp" else num_hiddens + 1
    if kind == "resnet":
        q, qt = w2 * q + b2, w2 * qt
        th, tht = q.copy(), qt.copy()
    sets = []
    for s in range(nsets):
        if kind == "mlp":
            q, qt = w2 * q + b2, w2 * qt
            th, tht = q + w2 * th, qt + w2 * tht
        sets.append((q, qt))
        o, oq, dd, ddq = _act_diag(act, q)
        ot, to, tot = oq * qt, th * dd, tht * dd + th * ddq * qt
        if kind == "resnet" and s != nsets - 1:
            a2, a2t = w2 * o + b2, w2 * ot
            q, qt = q + a2, qt + a2t
            th, tht = th + a2 + w2 * to, tht + a2t + w2 * tot
        else:
            q, qt, th, tht = o, ot, to, tot
    return sets, (q, qt, th, tht)


def factors(kind, x1, x2, get="nngp", num_hiddens=1, act="relu", w_std=1.0, b_std=0.0, last_w_std=1.0, dtype=np.float64):
    """F_1, F_2 [n1, n2] and the diagonal derivative dk_rr/dq0 [n1] of K (get="nngp") or Theta (get="ntk")."""
    dt = np.dtype(dtype).type
    x1, x2 = np.asarray(x1, dtype=dtype), np.asarray(x2, dtype=dtype)
    d = dt(x1.shape[1])
    w2, b2, lw2 = dt(w_std) * dt(w_std), dt(b_std) * dt(b_std), dt(last_w_std) * dt(last_w_std)
    ntk = get == "ntk"
    k = (x1 @ x2.T) / d
    q1 = np.einsum("ij,ij->i", x1, x1) / d
    q2 = np.einsum("ij,ij->i", x2, x2) / d
    rows, (_, qt_f, _, tht_f) = _diag_chain(kind, act, q1, num_hiddens, w2, b2)
    cols, _ = _diag_chain(kind, act, q2, num_hiddens, w2, b2)
    ku, kv = np.ones_like(k), np.zeros_like(k)
    th, thu, thv = np.zeros_like(k), np.zeros_like(k), np.zeros_like(k)
    nsets = len(rows)
    if kind == "resnet":
        k, ku = w2 * k + b2, w2 * ku
        th, thu = k.copy(), ku.copy()
    for s in range(nsets):
        a, au, av, tt, tu, tv = k, ku, kv, th, thu, thv
        if kind == "mlp":
            a, au, av = w2 * k + b2, w2 * ku, w2 * kv
            tt, tu, tv = a + w2 * th, au + w2 * thu, av + w2 * thv
        (qi, p), (qj, _) = rows[s], cols[s]
        phi, big_d, phi1, d_a, d_1 = _act(act, a, qi, qj)
        pr = p[:, None]
        o, ou, ov = phi, big_d * au, big_d * av + phi1 * pr
        du, dv = d_a * au, d_a * av + d_1 * pr
        to, tou, tov = tt * big_d, tu * big_d + tt * du, tv * big_d + tt * dv
        if kind == "resnet" and s != nsets - 1:
            a2, a2u, a2v = w2 * o + b2, w2 * ou, w2 * ov
            o, ou, ov = a + a2, au + a2u, av + a2v
            to, tou, tov = tt + a2 + w2 * to, tu + a2u + w2 * tou, tv + a2v + w2 * tov
        k, ku, kv, th, thu, thv = o, ou, ov, to, tou, tov
    f1 = lw2 * (ku + thu if ntk else ku)
    f2 = lw2 * (kv + thv if ntk else kv)
    ddiag = lw2 * (qt_f + tht_f if ntk else qt_f)
    return f1.astype(dtype), f2.astype(dtype), ddiag.astype(dtype)


def entry_grad(kind, x1, x2, get="nngp", dtype=np.float64, **hyp):
    """dK[r, j]/dx1[r, :] as [n1, n2, d]."""
    f1, f2, _ = factors(kind, x1, x2, get, dtype=dtype, **hyp)
    x1, x2 = np.asarray(x1, dtype=dtype), np.asarray(x2, dtype=dtype)
    dt = np.dtype(dtype).type
    return (f1[:, :, None] * x2[None, :, :] + dt(2) * f2[:, :, None] * x1[:, None, :]) / dt(x1.shape[1])


def input_grad(kind, x1, x2, seed, get="nngp", dtype=np.float64, **hyp):
    """gx [n1, d] = sum_j seed[r, j] dK_rj/dx1_r = ((seed o F_1) X2 + 2 rowsum(seed o F_2) o x1) / d."""
    f1, f2, _ = factors(kind, x1, x2, get, dtype=dtype, **hyp)
    x1, x2, g = np.asarray(x1, dtype=dtype), np.asarray(x2, dtype=dtype), np.asarray(seed, dtype=dtype)
    dt = np.dtype(dtype).type
    return (((g * f1) @ x2 + dt(2) * (g * f2).sum(axis=1)[:, None] * x1) / dt(x1.shape[1])).astype(dtype)


def predict_grad(kind, x, y, xt, get="nngp", diag_reg=0.0, absolute=False, dtype=np.float64, **hyp):
    """(dmean [T, C, d], dvar [T, d]) of oracle.predict's mean and diagonal covariance with respect to the test inputs, the
    covariance function being K (get="nngp") or Theta (get="ntk"), through oracle.predict's algebra: K~ = K_dd + diag_reg
    tr(K_dd)/N I (or diag_reg I when absolute), alpha = K~^-1 y, U = K_td K~^-1."""
    dt = np.dtype(dtype).type
    x, xt = np.asarray(x, dtype=dtype), np.asarray(xt, dtype=dtype)
    n, d = x.shape
    y2 = np.asarray(y, dtype=dtype).reshape(n, -1)
    kfn = KERNELS[kind]
    k_dd = np.asarray(kfn(x, None, get=get, dtype=dtype, **hyp), dtype=dtype)
    k_td = np.asarray(kfn(xt, x, get=get, dtype=dtype, **hyp), dtype=dtype)
    scale = dt(1) if absolute else np.trace(k_dd) / dt(n)
    cf = sla.cho_factor(k_dd + dt(diag_reg) * scale * np.eye(n, dtype=dtype), lower=True)
    alpha = sla.cho_solve(cf, y2)
    u = sla.cho_solve(cf, k_td.T).T
    f1, f2, ddiag = factors(kind, xt, x, get, dtype=dtype, **hyp)
    dmean = (np.einsum("rj,jk,je->rke", f1, alpha, x) + dt(2) * (f2 @ alpha)[:, :, None] * xt[:, None, :]) / dt(d)
    gx_u = ((u * f1) @ x + dt(2) * (u * f2).sum(axis=1)[:, None] * xt) / dt(d)
    dvar = dt(2) * xt / dt(d) * ddiag[:, None] - dt(2) * gx_u
    return dmean.astype(dtype), dvar.astype(dtype)


def predict_mean_var(kind, x, y, xt, get="nngp", diag_reg=0.0, absolute=False, dtype=np.float64, **hyp):
    """oracle.predict's (mean [T, C], diagonal of cov [T]) with K or Theta as the covariance function."""
    kfn = KERNELS[kind]
    x, xt = np.asarray(x, dtype=dtype), np.asarray(xt, dtype=dtype)
    args = dict(get=get, dtype=dtype, **hyp)
    mean, cov = O.predict(kfn(x, None, **args), kfn(xt, x, **args), kfn(xt, None, **args), np.asarray(y, dtype=dtype).reshape(len(x), -1),
                          diag_reg=diag_reg, diag_reg_absolute_scale=absolute)
    return mean, np.diag(cov).copy()
