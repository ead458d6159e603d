"""Generates tests/golden/nngp_mp_golden.npz: high-precision (mpmath, 40 digits) references for the NNGP / NTK element maps,
the composite MLP / dense-ResNet / conv kernels and the inference heads.

This script is independent of the CPU oracle and of the package on purpose (tests/test_mp_golden.py checks its imports):
it restates the published formulas (experiments/nt_kernels.py:21-45,83-103, spax/utils.py:160-183,
spax/likelihoods.py, spax/kernels.py of the reference) directly in mpmath, so a common-mode error of the oracle and the
kernels cannot hide behind it.  Every input is stored exactly as the device receives it (f32 cases hold f32-representable
values) and every reference is computed from those exact values.  Two runs give identical bytes.

    python tests/golden/make_mp_golden.py

Contents
--------
a. map_*      element-map sweep through smn_recursion (MLP, num_hiddens = 1, w = 1, b = 0, last_w = 1, non-symmetric).
              q is chosen so the per-row tables are exact powers of two (ReLU q = 4^m: r = 2^-m; erf q = (4^m - 1)/2:
              r = 1/sqrt(1 + 2q) = 2^-m; the f32 NNGP-only erf path folds r' = sqrt(2) r, so there q = 4^m - 1/2) and
              K0 = c * 2^(m_i + m_j) (erf: / 2), so the device forms the correlation c exactly and only the map (plus the
              rounding of the s-table / sigma products) is left.  c runs over a uniform grid of [-1, 1], +-(1 - 2^-k) down to the
              dtype's epsilon, +-1 (ReLU), 0 and +-2^-k, and 0.5 with its neighbours (the branch point of asin_abs).
b. cmp_*      composite kernels: MLP and dense ResNet, relu / erf, L in {1, 3, 6}, NNGP and NTK, symmetric (x2 = None) and
              cross (x2 holds rows of x1), on edge input sets (d = 1 rows, exact duplicates, power-of-two scaled rows,
              antiparallel rows, near-duplicates x + delta z, all-zero rows with b = 0, row norms over 1e-3 .. 1e3) and a
              Gaussian control set; plus one small conv case (get_cnn_kernel, 4x4x1 images with a duplicate and a negated one).
c. head_*     Gaussian / Student-t log-marginal likelihood (smn_lml), posterior mean / covariance with the relative ridge
              (smn_predict) from f64-rounded kernel matrices, and one Student-t SPR.test_nll from the raw inputs.

Error budgets (stored per entry, per dtype; computed in mp, not fitted to any device result)
------------------------------------------------------------------------------------------
Kernels: the recursion is re-run with the correlation rho = K / sqrt(q_i q_j) of EVERY activation pushed by k * u_T toward
+-1 and, separately, away from it (clamped to [-1, 1]; for erf the push acts on rho, so the erf argument stays physical),
with k = d + 2 L + 4 (the Gram's gamma_d plus two roundings per layer plus the table / read-out products), u_T = 2^-53 (f64)
or 2^-24 (f32).  The budget of an entry is the larger of the two deviations plus (2 L + 4) u_T (|K_ij| + sqrt(K_ii K_jj))
for the final roundings and the absolute evaluation error of the maps (which is relative to the row / column scale, not to
K_ij: J(c) -> 0 at c -> -1).  This carries the sqrt-type sensitivity of Kdot at c -> 1 as well as ordinary conditioning, and
of the closed-form diagonal asin(2q / (1 + 2q)) of erf at large q.  The same rule covers diagonal entries.

Heads: Cholesky of K~ (n x n) is backward stable, (K~ + E) = L L^T with |E| <= gamma |K~|, gamma = 4 (n + 1) u_T (forming
K + eps I included).  First-order perturbation then bounds
    logdet:   n kappa gamma                quad = y^T K~^-1 y:   kappa gamma quad
    Gaussian LML: gamma kappa (n + quad) / 2
    Student-t LML: gamma kappa (n + 2 t quad / (df s + quad)) / 2 <= gamma kappa (n + df + n) / 2,   t = (df + n) / 2
    mean = K_td K~^-1 y:   gamma (kappa ||K_td||_2 ||alpha||_2 + max |K_td| |alpha|)
    cov  = K_tt - K_td K~^-1 K_dt:   gamma (kappa ||K~||_2 ||A||_2^2 + max |K_tt| + max |K_td| |A|),   A = K~^-1 K_dt
with kappa = kappa_2(K~) stored with each case.  test_nll (kernels built on the device as well): gamma grows by the kernel's
k u_T and the budget is 2 gamma (kappa(K~) + kappa(K^)) (1 + |nll|), K^ = (b/a) K + 1e-6 I the matrix of the quadratic form.
"""
import io
import os
import zipfile

import mpmath as mp
import numpy as np

mp.mp.dps = 40
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nngp_mp_golden.npz")
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
NPT = {"f64": np.float64, "f32": np.float32}
PI = mp.pi


# ----------------------------------------------------------------------------------------------------------- the maps
def relu_J(c):
    """J(c) = sqrt(1 - c^2) + (pi - acos c) c  (Cho & Saul)."""
    return mp.sqrt(1 - c * c) + (PI - mp.acos(c)) * c


def act_map(act, k, qi, qj, push=0):
    """One activation on a pre-activation entry k with pre-activation variances qi, qj.  push = s * k * u: the correlation
    rho = k / sqrt(qi qj) is moved by push toward +-1 (push > 0) or away (push < 0), clamped to [-1, 1].
    Returns (k', kdot, qi', qj')."""
    sp = mp.sqrt(qi * qj)
    if sp == 0:
        rho = mp.mpf(0)
    else:
        rho = k / sp
        if push:
            rho = rho + (push if rho >= 0 else -push)
        rho = min(max(rho, mp.mpf(-1)), mp.mpf(1))
        k = rho * sp
    if act == "relu":
        kn = sp * relu_J(rho) / (2 * PI)
        kd = (PI - mp.acos(rho)) / (2 * PI)
        return kn, kd, qi / 2, qj / 2
    pij = (1 + 2 * qi) * (1 + 2 * qj)
    c = 2 * k / mp.sqrt(pij)
    kn = 2 / PI * mp.asin(c)
    kd = 4 / (PI * mp.sqrt(pij - 4 * k * k))
    return kn, kd, 2 / PI * mp.asin(2 * qi / (1 + 2 * qi)), 2 / PI * mp.asin(2 * qj / (1 + 2 * qj))


def mlp_entry(k, qi, qj, L, act, w, b, lw, push=0):
    """experiments/nt_kernels.py:21-31: L x [Dense(w, b); act]; Dense(lw, 0).  NTK parameterisation."""
    w2, b2, lw2 = mp.mpf(w) ** 2, mp.mpf(b) ** 2, mp.mpf(lw) ** 2
    th = mp.mpf(0)
    for _ in range(L):
        k, qi, qj = w2 * k + b2, w2 * qi + b2, w2 * qj + b2
        th = k + w2 * th
        k, kd, qi, qj = act_map(act, k, qi, qj, push)
        th = th * kd
    k = lw2 * k
    return k, k + lw2 * th


def resnet_entry(k, qi, qj, L, act, w, b, lw, push=0):
    """experiments/nt_kernels.py:83-103: Dense; L x {(act; Dense) + Identity}; act; Dense(lw, 0)."""
    w2, b2, lw2 = mp.mpf(w) ** 2, mp.mpf(b) ** 2, mp.mpf(lw) ** 2
    k, qi, qj = w2 * k + b2, w2 * qi + b2, w2 * qj + b2
    th = k
    for _ in range(L):
        kb, kd, qib, qjb = act_map(act, k, qi, qj, push)
        tb = th * kd
        kb, qib, qjb = w2 * kb + b2, w2 * qib + b2, w2 * qjb + b2
        tb = kb + w2 * tb
        k, qi, qj, th = k + kb, qi + qib, qj + qjb, th + tb
    k, kd, qi, qj = act_map(act, k, qi, qj, push)
    th = th * kd
    k = lw2 * k
    return k, k + lw2 * th


ENTRY = {"mlp": mlp_entry, "resnet": resnet_entry}


def mpf_rows(x):
    return [[mp.mpf(float(v)) for v in row] for row in np.asarray(x, dtype=np.float64)]


def gram(xa, xb, d):
    """K0 = x1 x2^T / d, q = ||x||^2 / d, exact inputs."""
    k0 = [[mp.fsum(p * q for p, q in zip(ra, rb)) / d for rb in xb] for ra in xa]
    qa = [mp.fsum(p * p for p in r) / d for r in xa]
    qb = [mp.fsum(p * p for p in r) / d for r in xb]
    return k0, qa, qb


def kernel_with_budget(net, act, L, w, b, lw, x1, x2, dtypes):
    """Reference NNGP / NTK of one (net, act, L) on exact inputs plus the per-entry budgets of the module docstring."""
    d = x1.shape[1]
    sym = x2 is None
    xa = mpf_rows(x1)
    xb = xa if sym else mpf_rows(x2)
    k0, qa, qb = gram(xa, xb, d)
    n1, n2 = len(xa), len(xb)
    f = ENTRY[net]
    ref = np.zeros((2, n1, n2))
    bud = {t: np.zeros((2, n1, n2)) for t in dtypes}
    dia1 = [f(q, q, q, L, act, w, b, lw) for q in qa]   # K(x, x) of every row: the scale of an entry's row and column
    dia2 = dia1 if sym else [f(q, q, q, L, act, w, b, lw) for q in qb]
    for i in range(n1):
        for j in range(n2):
            if sym and j < i:
                ref[:, i, j] = ref[:, j, i]
                for t in dtypes:
                    bud[t][:, i, j] = bud[t][:, j, i]
                continue
            kt = f(k0[i][j], qa[i], qb[j], L, act, w, b, lw)
            ref[:, i, j] = [float(v) for v in kt]
            scale = [mp.sqrt(abs(dia1[i][m] * dia2[j][m])) for m in (0, 1)]
            for t in dtypes:
                push = (d + 2 * L + 4) * U[t]
                dev = [mp.mpf(0), mp.mpf(0)]
                for s in (1, -1):
                    pt = f(k0[i][j], qa[i], qb[j], L, act, w, b, lw, s * push)
                    dev = [max(dev[m], abs(pt[m] - kt[m])) for m in (0, 1)]
                for m in (0, 1):
                    bud[t][m, i, j] = float(dev[m] + (2 * L + 4) * U[t] * (abs(kt[m]) + scale[m]))
    return ref, bud


# ----------------------------------------------------------------------------------------------------------- a. maps
def c_grid(t, act):
    nt = NPT[t]
    eps_bits = 53 if t == "f64" else 24
    c = [float(nt(v)) for v in np.linspace(-1.0, 1.0, 2001)]
    for k in range(1, eps_bits + 1):
        c += [1.0 - 2.0 ** -k, -(1.0 - 2.0 ** -k)]
    c += [0.0, -0.0]
    for k in range(1, 41 if t == "f64" else 31):
        c += [2.0 ** -k, -(2.0 ** -k)]
    h = nt(0.5)
    lo = hi = h
    for _ in range(3):
        lo, hi = np.nextafter(lo, nt(0)), np.nextafter(hi, nt(1))
        c += [float(lo), float(hi), -float(lo), -float(hi)]
    c += [0.5, -0.5]
    if act == "relu":
        c += [1.0, -1.0]
    else:   # erf: Kdot is singular at |c| = 1 (the NTK request); keep the interior
        c = [v for v in c if abs(v) < 1.0]
    while len(c) % 4:
        c.append(0.0)
    arr = np.array(c, dtype=np.float64)
    assert np.array_equal(arr.astype(nt).astype(np.float64), arr)
    return arr


MAP_M = {"f64": [1, 26], "f32": [1, 12]}   # row table exponents; the column exponent is 1


def map_case(t, act, fast_erf=False):
    """One map sweep: rows i carry q = Q(m_i), columns q = Q(1); K0[i, j] = c_j * scale_i."""
    ms = MAP_M[t] if not fast_erf else [1, 11]
    if act == "relu":
        qf = lambda m: mp.mpf(4) ** m
        kscale = lambda mi, mj: mp.mpf(2) ** (mi + mj)
    elif fast_erf:
        qf = lambda m: mp.mpf(4) ** m - mp.mpf(1) / 2
        kscale = lambda mi, mj: mp.mpf(2) ** (mi + mj)
    else:
        qf = lambda m: (mp.mpf(4) ** m - 1) / 2
        kscale = lambda mi, mj: mp.mpf(2) ** (mi + mj) / 2
    c = c_grid(t, act)
    q1 = np.array([float(qf(m)) for m in ms])
    q2 = np.full(len(c), float(qf(1)))
    k0 = np.array([[float(mp.mpf(cj) * kscale(m, 1)) for cj in c] for m in ms])
    nt = NPT[t]
    for a in (q1, q2, k0):
        assert np.array_equal(a.astype(nt).astype(np.float64), a)
    nngp = np.zeros(k0.shape)
    ntk = np.zeros(k0.shape)
    for i, m in enumerate(ms):
        qi, qj = qf(m), qf(1)
        for j, cj in enumerate(c):
            kk = mp.mpf(float(k0[i, j]))
            if act == "relu":   # c = K0 / sqrt(qi qj) exactly
                cc = mp.mpf(cj)
                kn = mp.sqrt(qi * qj) * relu_J(cc) / (2 * PI)
                kd = (PI - mp.acos(cc)) / (2 * PI)
            else:
                pij = (1 + 2 * qi) * (1 + 2 * qj)
                cc = 2 * kk / mp.sqrt(pij)
                kn = 2 / PI * mp.asin(cc)
                kd = 4 / (PI * mp.sqrt(pij - 4 * kk * kk))
            nngp[i, j] = float(kn)
            ntk[i, j] = float(kn + kk * kd)   # Dense(1, 0) -> act -> Dense(1, 0): Theta = K' + K0 Kdot
    return dict(c=c, q1=q1.astype(nt), q2=q2.astype(nt), k0=k0.astype(nt), nngp=nngp, ntk=ntk)


# ----------------------------------------------------------------------------------------------------------- b. sets
def f32r(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def input_sets():
    """name -> (x1, x2, (w, b, lw), dtypes).  f32-representable unless the set is f64 only."""
    rng = np.random.default_rng(20261016)
    sets = {}
    h0 = (1.3, 0.0, 1.0)
    h1 = (1.3, 0.2, 0.9)
    x = f32r(rng.standard_normal((8, 1)))
    x[3] = -x[2]
    sets["d1"] = (x, f32r(np.concatenate([x[[0, 2, 5]], rng.standard_normal((3, 1))])), h0, ("f64", "f32"))
    base = f32r(rng.standard_normal((4, 5)))
    x = base[[0, 0, 1, 1, 2, 2, 3, 3]]
    sets["dup"] = (x, f32r(np.concatenate([base[[0, 3]], rng.standard_normal((4, 5))])), h0, ("f64", "f32"))
    base = f32r(rng.standard_normal((3, 5)))
    x = np.stack([base[0], 2 * base[0], 0.25 * base[0], base[1], 8 * base[1], 0.5 * base[1], base[2], 4 * base[2]])
    sets["scaled"] = (x, np.stack([0.125 * base[0], 2 * base[2], base[1], *f32r(rng.standard_normal((3, 5)))]), h0,
                      ("f64", "f32"))
    base = f32r(rng.standard_normal((4, 5)))
    x = np.stack([base[0], -base[0], base[1], -2 * base[1], base[2], -0.5 * base[2], base[3], -base[3]])
    sets["anti"] = (x, np.stack([-base[0], base[1], -base[3], *f32r(rng.standard_normal((3, 5)))]), h0, ("f64", "f32"))
    base = rng.standard_normal((2, 50))
    z = rng.standard_normal((6, 50))
    x = np.stack([base[0], base[0] + 1e-3 * z[0], base[0] + 1e-6 * z[1], base[0] + 1e-9 * z[2],
                  base[1], base[1] + 1e-3 * z[3], base[1] + 1e-6 * z[4], base[1] + 1e-9 * z[5]])
    sets["neardup"] = (x, np.stack([base[0], base[1] + 1e-9 * z[0], *rng.standard_normal((4, 50))]), h1, ("f64",))
    x = f32r(rng.standard_normal((8, 5)))
    x[2] = 0.0
    x[7] = 0.0
    x2 = f32r(rng.standard_normal((6, 5)))
    x2[1] = 0.0
    sets["zero"] = (x, x2, h0, ("f64", "f32"))
    x = rng.standard_normal((8, 5))
    x = f32r(x / np.linalg.norm(x, axis=1, keepdims=True) * np.logspace(-3, 3, 8)[:, None])
    sets["norms"] = (x, f32r(np.concatenate([x[[1, 6]], rng.standard_normal((4, 5)) * 30.0])), h1, ("f64", "f32"))
    x = f32r(rng.standard_normal((16, 50)))
    sets["control"] = (x, f32r(np.concatenate([x[[0, 5, 9]], rng.standard_normal((5, 50))])), h1, ("f64", "f32"))
    return sets


LAYERS = (1, 3, 6)


def composite_case(name, net, act, L):
    x1, x2, (w, b, lw), dts = input_sets()[name]
    out = {}
    for tag, xb in (("sym", None), ("cross", x2)):
        ref, bud = kernel_with_budget(net, act, L, w, b, lw, x1, xb, dts)
        out[tag] = (ref, bud)
    return out


# ----------------------------------------------------------------------------------------------------------- conv
def box3(m):
    h, w = len(m), len(m[0])
    return [[mp.fsum(m[a][b] for a in range(max(0, i - 1), min(h, i + 2)) for b in range(max(0, j - 1), min(w, j + 2)))
             for j in range(w)] for i in range(h)]


def cnn_entry(xa, xb, L, act, w, b, lw, push=0):
    """experiments/nt_kernels.py:34-45: L x [Conv(3x3, SAME, w, b); act]; Flatten; Dense(lw).  One channel: K0 per pixel."""
    w2, b2, lw2 = mp.mpf(w) ** 2, mp.mpf(b) ** 2, mp.mpf(lw) ** 2
    k = [[p * q for p, q in zip(ra, rb)] for ra, rb in zip(xa, xb)]
    qa = [[p * p for p in ra] for ra in xa]
    qb = [[p * p for p in rb] for rb in xb]
    for _ in range(L):
        k, qa, qb = ([[w2 * v / 9 + b2 for v in row] for row in box3(m)] for m in (k, qa, qb))
        res = [[act_map(act, k[i][j], qa[i][j], qb[i][j], push) for j in range(len(k[0]))] for i in range(len(k))]
        k = [[r[0] for r in row] for row in res]
        qa = [[r[2] for r in row] for row in res]
        qb = [[r[3] for r in row] for row in res]
    return lw2 * mp.fsum(v for row in k for v in row) / (len(k) * len(k[0]))


def conv_case():
    rng = np.random.default_rng(4411)
    x = f32r(rng.standard_normal((6, 4, 4, 1)))
    x[1] = x[0]
    x[2] = -x[0]
    L, act, w, b, lw = 2, "relu", 1.3, 0.1, 0.9
    imgs = [[[mp.mpf(float(v)) for v in row] for row in im[:, :, 0]] for im in x]
    n = len(imgs)
    ref = np.zeros((n, n))
    bud = {t: np.zeros((n, n)) for t in ("f64", "f32")}
    for i in range(n):
        for j in range(i, n):
            kk = cnn_entry(imgs[i], imgs[j], L, act, w, b, lw)
            ref[i, j] = ref[j, i] = float(kk)
            for t in bud:
                push = (9 + 2 * L + 4) * U[t]
                dev = max(abs(cnn_entry(imgs[i], imgs[j], L, act, w, b, lw, s * push) - kk) for s in (1, -1))
                bud[t][i, j] = bud[t][j, i] = float(dev + (2 * L + 4) * U[t] * abs(kk))
    return dict(x=x.astype(np.float32), ref=ref, bud64=bud["f64"], bud32=bud["f32"].astype(np.float32),
                params=np.array([L, w, b, lw]))


# ----------------------------------------------------------------------------------------------------------- c. heads
def mpmat(a):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(a, dtype=np.float64)])


def spd_facts(a):
    """Cholesky factor, logdet and kappa_2 of an mp SPD matrix."""
    lc = mp.cholesky(a)
    logdet = 2 * mp.fsum(mp.log(lc[i, i]) for i in range(a.rows))
    ev = mp.eigsy(a, eigvals_only=True)
    ev = [ev[i] for i in range(a.rows)]
    return lc, logdet, max(ev) / min(ev), max(ev)


def chol_solve(lc, bm):
    """(L L^T)^-1 bm by two triangular solves."""
    n = lc.rows
    out = mp.matrix(n, bm.cols)
    for c in range(bm.cols):
        y = [mp.mpf(0)] * n
        for i in range(n):
            y[i] = (bm[i, c] - mp.fsum(lc[i, k] * y[k] for k in range(i))) / lc[i, i]
        xv = [mp.mpf(0)] * n
        for i in reversed(range(n)):
            xv[i] = (y[i] - mp.fsum(lc[k, i] * xv[k] for k in range(i + 1, n))) / lc[i, i]
        for i in range(n):
            out[i, c] = xv[i]
    return out


def lml_ref(k, y, eps, df, scale, t):
    """smn_lml: Gaussian (df <= 0) or Student-t with shape = scale (K + eps I) (spax/likelihoods.py:25-28,45-50,
    spax/utils.py:178-183).  k, y exact values."""
    n = k.shape[0]
    km = mpmat(k) + mp.mpf(float(eps)) * mp.eye(n)
    lc, logdet, kappa, _ = spd_facts(km)
    ym = mpmat(np.asarray(y, dtype=np.float64)[:, None])
    quad = mp.fsum(ym[i, 0] * v for i, v in enumerate(chol_solve(lc, ym)))
    gam = 4 * (n + 1) * U[t]
    if df <= 0:
        lp = -quad / 2 - n / mp.mpf(2) * mp.log(2 * PI) - logdet / 2
        bound = gam * kappa * (n + quad) / 2
    else:
        df, scale = mp.mpf(df), mp.mpf(scale)
        tt = (df + n) / 2
        lp = (-tt * mp.log(1 + quad / (scale * df)) - n / mp.mpf(2) * mp.log(df * PI) + mp.loggamma(tt)
              - mp.loggamma(df / 2) - (logdet + n * mp.log(scale)) / 2)
        bound = gam * kappa * (n + df + n) / 2
    return float(lp), float(quad), float(logdet), float(kappa), float(bound)


def predict_ref(kj, n, y, eps, t):
    """smn_predict: K~ = K_dd + eps tr(K_dd)/n I, mean = K_td K~^-1 y, cov = K_tt - K_td K~^-1 K_dt (spax/kernels.py:29-32)."""
    m = mpmat(kj)
    tn = kj.shape[0] - n
    kdd = m[0:n, 0:n]
    tr = mp.fsum(kdd[i, i] for i in range(n))
    kt = kdd + mp.mpf(float(eps)) * tr / n * mp.eye(n)
    ktd = m[n:n + tn, 0:n]
    ktt = m[n:n + tn, n:n + tn]
    lc, _, kappa, lmax = spd_facts(kt)
    ym = mpmat(y)
    alpha = chol_solve(lc, ym)
    a = chol_solve(lc, ktd.T)
    mean = ktd * alpha
    cov = ktt - ktd * a
    gam = 4 * (n + 1) * U[t]
    nrm2 = lambda x: mp.sqrt(max(mp.eigsy(x.T * x, eigvals_only=True)))
    absmul = lambda p, q: max(mp.fsum(abs(p[i, k]) * abs(q[k, j]) for k in range(p.cols))
                              for i in range(p.rows) for j in range(q.cols))
    bm = gam * (kappa * nrm2(ktd) * nrm2(alpha) + absmul(ktd, alpha))
    bc = gam * (kappa * lmax * nrm2(a) ** 2 + max(abs(v) for v in ktt) + absmul(ktd, a))
    tonp = lambda x: np.array([[float(x[i, j]) for j in range(x.cols)] for i in range(x.rows)])
    return tonp(mean), tonp(cov), float(kappa), float(bm), float(bc)


HEAD_NET = ("mlp", "relu", 3, 1.3, 0.2, 0.9)   # kernel of the head cases: net, act, L, w, b, lw
HEAD_N, HEAD_T = 40, 8


def head_inputs():
    rng = np.random.default_rng(7)
    x = f32r(rng.standard_normal((HEAD_N + HEAD_T, 5)))
    y = f32r(rng.standard_normal((HEAD_N + HEAD_T, 2)))
    return x, y


def head_kernel():
    """The joint kernel of the head inputs in mp (nominal values only)."""
    x, _ = head_inputs()
    net, act, L, w, b, lw = HEAD_NET
    xa = mpf_rows(x)
    k0, qa, _ = gram(xa, xa, x.shape[1])
    n = len(xa)
    km = mp.matrix(n, n)
    for i in range(n):
        for j in range(i + 1):
            km[i, j] = km[j, i] = ENTRY[net](k0[i][j], qa[i], qa[j], L, act, w, b, lw)[0]
    return km


def test_nll_ref(km, y, yt, eps, alpha, beta):
    """SPR.test_nll, Student-t head (spax/models.py:100-120, likelihoods.py:52-65): posterior with the relative ridge,
    then the data term of the quadratic form from K WITHOUT eps plus 1e-6 (likelihoods.py:60), y_mean = 0, y_std = 1."""
    n = HEAD_N
    kdd = km[0:n, 0:n]
    ktd = km[n:, 0:n]
    ktt = km[n:, n:]
    tr = mp.fsum(kdd[i, i] for i in range(n))
    kt = kdd + mp.mpf(eps) * tr / n * mp.eye(n)
    lc, _, kap1, _ = spd_facts(kt)
    ym = mpmat(y[:, None])
    mean = ktd * chol_solve(lc, ym)
    cov = ktt - ktd * chol_solve(lc, ktd.T)
    df = 2 * mp.mpf(alpha)
    s = mp.mpf(beta) / mp.mpf(alpha)
    kh = s * kdd + mp.mpf("1e-6") * mp.eye(n)
    lh, _, kap2, _ = spd_facts(kh)
    d = df + mp.fsum(ym[i, 0] * v for i, v in enumerate(chol_solve(lh, ym)))
    nu = df + n
    lps = []
    for i in range(ktt.rows):
        sig = mp.sqrt(d / nu * s * cov[i, i])
        z = (mp.mpf(float(yt[i])) - mean[i, 0]) / sig
        lps.append(mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2) - mp.log(nu * PI) / 2 - mp.log(sig)
                   - (nu + 1) / 2 * mp.log(1 + z * z / nu))
    nll = -mp.fsum(lps) / len(lps)
    return float(nll), float(kap1), float(kap2)


# ----------------------------------------------------------------------------------------------------------- output
def build_all():
    data = {}
    for t in ("f64", "f32"):
        for act in ("relu", "erf"):
            for key, v in map_case(t, act).items():
                data["map_%s_%s_%s" % (act, t, key)] = v
        fe = map_case(t, "erf", fast_erf=True) if t == "f32" else None
        if fe is not None:   # the f32 NNGP-only erf path (FAST tables): same c grid, same reference, its own q / K0
            assert np.array_equal(fe["c"], data["map_erf_f32_c"]) and np.array_equal(fe["nngp"], data["map_erf_f32_nngp"])
            data["map_erf_f32_q1fast"] = fe["q1"]
            data["map_erf_f32_q2fast"] = fe["q2"]
            data["map_erf_f32_k0fast"] = fe["k0"]
    sets = input_sets()
    names = sorted(sets)
    data["cmp_sets"] = np.array(names)
    for name in names:
        x1, x2, hyp, dts = sets[name]
        data["cmp_%s_x1" % name] = x1
        data["cmp_%s_x2" % name] = x2
        data["cmp_%s_hyp" % name] = np.array(hyp)
        data["cmp_%s_dtypes" % name] = np.array(dts)
        for net in ("mlp", "resnet"):
            for act in ("relu", "erf"):
                for L in LAYERS:
                    res = composite_case(name, net, act, L)
                    for tag, (ref, bud) in res.items():
                        key = "cmp_%s_%s_%s_L%d_%s" % (name, net, act, L, tag)
                        data[key + "_ref"] = ref
                        data[key + "_bud64"] = bud["f64"]
                        if "f32" in bud:
                            data[key + "_bud32"] = bud["f32"].astype(np.float32)
    for k, v in conv_case().items():
        data["conv_" + k] = v
    # heads: kernels rounded to f64 (and to f32 at eps >= 1e-2), references from those exact values
    km = head_kernel()
    kfull = np.array([[float(km[i, j]) for j in range(km.cols)] for i in range(km.rows)])
    x, y = head_inputs()
    data["head_x"] = x
    data["head_y"] = y
    data["head_net"] = np.array([str(v) for v in HEAD_NET])
    data["head_k64"] = kfull
    dup = data["cmp_dup_mlp_relu_L3_sym_ref"][0]   # a singular kernel (duplicate rows): kappa ~ 1 / eps
    data["head_kdup"] = dup
    cases = []
    for src, kk in (("k64", kfull[:HEAD_N, :HEAD_N]), ("kdup", dup)):
        for t, eps in (("f64", 1e-6), ("f64", 1e-2), ("f32", 1e-2)):
            kin = kk.astype(NPT[t]).astype(np.float64)
            for df, sc in ((0.0, 1.0), (4.0, 1.5)):
                lp, quad, logdet, kappa, bound = lml_ref(kin, y[:kk.shape[0], 0], eps, df, sc, t)
                cases.append([len(cases), {"k64": 0, "kdup": 1}[src], {"f64": 64, "f32": 32}[t], eps, df, sc, lp, quad,
                              logdet, kappa, bound])
    data["head_lml"] = np.array(cases)
    data["head_lml_cols"] = np.array(["id", "src", "dtype", "eps", "df", "scale", "logpdf", "quad", "logdet", "kappa",
                                      "bound"])
    for t, eps in (("f64", 1e-6), ("f64", 1e-2), ("f32", 1e-2)):
        kin = kfull.astype(NPT[t]).astype(np.float64)
        mean, cov, kappa, bm, bc = predict_ref(kin, HEAD_N, y[:HEAD_N], eps, t)
        key = "head_pred_%s_eps%g" % (t, eps)
        data[key + "_mean"] = mean
        data[key + "_cov"] = cov
        data[key + "_info"] = np.array([eps, kappa, bm, bc])
    yt = y[HEAD_N:, 0]
    for eps in (1e-6, 1e-2):
        nll, k1, k2 = test_nll_ref(km, y[:HEAD_N, 0], yt, eps, 2.0, 2.0)
        gam = (4 * (HEAD_N + 1) + x.shape[1] + 2 * HEAD_NET[2] + 4) * U["f64"]
        data["head_testnll_eps%g" % eps] = np.array([eps, 2.0, 2.0, nll, k1, k2, 2 * gam * (k1 + k2) * (1 + abs(nll))])
    return data


def write_npz(data, path):
    """np.savez with a fixed member order and timestamp, so the file is a pure function of the arrays."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(data):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.asarray(data[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, a.getvalue())
    with open(path, "wb") as f:
        f.write(buf.getvalue())


if __name__ == "__main__":
    write_npz(build_all(), OUT)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
