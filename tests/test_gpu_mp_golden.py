"""The HIP path against the independent mpmath fixture (tests/golden/nngp_mp_golden.npz; generator: make_mp_golden.py).

Unlike test_gpu_parity.py this needs no oracle: numpy and the fixture only.  Three families:
  * element maps through smn_recursion, each held to the accuracy nngp_math.hpp claims for it plus the table rounding;
  * composite MLP / dense-ResNet / conv kernels through the public kernel_fn surface, held to the fixture's per-entry budgets;
  * the heads (smn_lml, smn_predict, SPR.test_nll) on exact kernel matrices, held to the fixture's kappa-based bounds.
Each test prints the largest observed error against its bound (run with -s to see them)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from _kernel_budget import fast_erf_allowance  # noqa: E402
from _tol import relerr  # noqa: E402

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nngp_mp_golden.npz"))
SETS = [str(s) for s in Z["cmp_sets"]]
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
NPT = {"f64": np.float64, "f32": np.float32}


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def _report(tag, err, bound):
    r = float(np.max(err / bound))
    print("\n[mp] %-44s max err %.3e  max err/bound %.3f" % (tag, float(np.max(err)), r))
    return r


# ----------------------------------------------------------------------------- element maps
def _recursion(L, ctx, t, act, k0, q1, q2, mask):
    """smn_recursion, MLP, one hidden layer, w = 1, b = 0, last_w = 1, non-symmetric.  The fixture's row length is a
    multiple of 4, so ld keeps the 16-byte alignment rule (ld % (16 / sizeof(T)) == 0) and device buffers are aligned."""
    dt = NPT[t]
    n1, n2 = k0.shape
    assert n2 % 4 == 0
    kd, qd1, qd2 = ctx.to_device(k0.astype(dt)), ctx.to_device(q1.astype(dt)), ctx.to_device(q2.astype(dt))
    ok = ctx.empty((n1, n2), dt)
    ot = ctx.empty((n1, n2), dt) if mask & L.GET_NTK else None
    ctx.call("smn_recursion", L.dtype_code(dt), L.NET_MLP, L.ACT[act], 1, 1.0, 0.0, 1.0, kd.ptr, n1, n2, n2, qd1.ptr,
             qd2.ptr, 0, mask, ok.ptr, None if ot is None else ot.ptr, n2)
    return ok.numpy().astype(np.float64), None if ot is None else ot.numpy().astype(np.float64)


def _map_inputs(act, t, fast=False):
    sfx = "fast" if fast else ""
    g = lambda k: Z["map_%s_%s_%s" % (act, t, k)]
    return (g("k0" + sfx).astype(np.float64), g("q1" + sfx).astype(np.float64), g("q2" + sfx).astype(np.float64),
            g("nngp"), g("ntk"), g("c"))


def test_map_relu_f64_nngp_only(L, ctx):
    """relu_j_f64 (nngp_math.hpp: |J error| <= 4.4e-16 absolute, <= 3.9e-16 relative also as J -> 0)."""
    k0, q1, q2, ref, _, c = _map_inputs("relu", "f64")
    got, _ = _recursion(L, ctx, "f64", "relu", k0, q1, q2, L.GET_NNGP)
    S = np.sqrt(np.outer(q1, q2)) / (2 * np.pi)     # K' = S J(c)
    u = U["f64"]
    # claim 4.4e-16 on J, plus the s-table products s_i s_j and the final product: 3 roundings of the output
    bound = S * 4.4e-16 + 3 * u * np.abs(ref)
    err = np.abs(got - ref)
    _report("relu f64 NNGP-only (relu_j_f64) abs", err, bound)
    assert (err <= bound).all()
    nz = ref != 0
    # relative: claim 3.9e-16 + the same 3 roundings (3.3e-16) -> 7.2e-16, asserted at 1e-15 including c -> -1
    rel = err[nz] / np.abs(ref[nz])
    _report("relu f64 NNGP-only (relu_j_f64) rel", rel, 1e-15)
    assert rel.max() <= 1e-15
    assert (got[:, c == -1.0] == 0).all()                # J(-1) = 0 exactly (d = 0)


def test_map_relu_f64_ntk(L, ctx):
    """asin_abs<double> (<= 2.3e-16 absolute), fast_sqrt(double), the asin form of J and Kdot = 1/4 + asin(c) / (2 pi)."""
    k0, q1, q2, ref, rt, c = _map_inputs("relu", "f64")
    gk, gt = _recursion(L, ctx, "f64", "relu", k0, q1, q2, L.GET_NNGP | L.GET_NTK)
    S = np.sqrt(np.outer(q1, q2)) / (2 * np.pi)
    u = U["f64"]
    # J = pi/2 c + (|c| asin|c| + sqrt(1 - c^2)): the asin claim 2.3e-16, the square root (fma-exact argument, <= 2 u),
    # four roundings of terms <= pi  ->  2.3e-16 + 10 u absolute on J; the s-table products add 3 u relative
    ek = S * (2.3e-16 + 10 * u) + 3 * u * np.abs(ref)
    err = np.abs(gk - ref)
    _report("relu f64 NTK-mode NNGP (asin form) abs", err, ek)
    assert (err <= ek).all()
    nz = (ref != 0) & (np.abs(c)[None, :] < 1)
    rel = err[nz] / np.abs(ref[nz])
    print("\n[mp] relu f64 NTK-mode NNGP relative error (no claim; the asin form cancels as c -> -1): max %.3e" % rel.max())
    # Theta = K' + K0 Kdot; Kdot error <= 2.3e-16 / (2 pi) + 2 u Kdot (one fma, one constant)
    kdot = (rt - ref) / np.where(k0 != 0, k0, 1.0)
    et = ek + np.abs(k0) * (2.3e-16 / (2 * np.pi) + 3 * u * np.abs(kdot)) + u * np.abs(rt)
    err = np.abs(gt - rt)
    _report("relu f64 NTK", err, et)
    assert (err <= et).all()


@pytest.mark.parametrize("mask_name", ["nngp", "both"])
def test_map_erf_f64(L, ctx, mask_name):
    """asin_abs<double> (<= 2.3e-16) for K' = (2/pi) asin c, and Kdot = 4/pi r_i r_j fast_rsqrt(1 - c^2) (fast_rsqrt has no
    stated claim: a correctly rounded rsqrt is 0.5 ulp, the bound below grants it 2 u)."""
    k0, q1, q2, ref, rt, c = _map_inputs("erf", "f64")
    mask = L.GET_NNGP | (L.GET_NTK if mask_name == "both" else 0)
    gk, gt = _recursion(L, ctx, "f64", "erf", k0, q1, q2, mask)
    u = U["f64"]
    ek = (2 / np.pi) * 2.3e-16 + 2 * u * np.abs(ref)      # claim + the 2/pi constant and product
    err = np.abs(gk - ref)
    _report("erf f64 NNGP (asin_abs<double>) [%s]" % mask_name, err, ek)
    assert (err <= ek).all()
    if gt is not None:
        kt = rt - ref                                     # K0 Kdot, same sign as K'
        # Kdot: 1 - c^2 by one fma (u), its rsqrt (u/2 + 2 u), r_i r_j, 4/pi and two products (4 u); then the sum (u)
        et = ek + 7 * u * np.abs(kt) + u * np.abs(rt)
        err = np.abs(gt - rt)
        _report("erf f64 NTK (fast_rsqrt(double))", err, et)
        assert (err <= et).all()


def test_map_relu_f32_fast(L, ctx):
    """relu_j_fast (nngp_math.hpp: |J - exact| <= 3.2e-7 over [-1, 1] in f32 arithmetic) on the FAST tables (u = 2^-m exact,
    sigma = sqrt(q / 2) rounded to f32)."""
    k0, q1, q2, ref, _, _ = _map_inputs("relu", "f32")
    got, _ = _recursion(L, ctx, "f32", "relu", k0, q1, q2, L.GET_NNGP)
    S = np.sqrt(np.outer(q1, q2)) / (2 * np.pi)
    u = U["f32"]
    # the map returns J / pi (claim 3.2e-7 / pi), sigma_i sigma_j = S pi: two table roundings + two products
    bound = S * 3.2e-7 + 4 * u * np.abs(ref)
    err = np.abs(got - ref)
    _report("relu f32 FAST (relu_j_fast)", err, bound)
    assert (err <= bound).all()


def test_map_erf_f32_fast(L, ctx):
    """asin_fast (nngp_math.hpp: <= 2.6e-7 absolute over [-1, 1]) on the FAST erf tables (r' = sqrt(2) r = 2^-m exact,
    sigma = sqrt(2 / pi) rounded to f32)."""
    k0, q1, q2, ref, _, _ = _map_inputs("erf", "f32", fast=True)
    got, _ = _recursion(L, ctx, "f32", "erf", k0, q1, q2, L.GET_NNGP)
    u = U["f32"]
    bound = (2 / np.pi) * 2.6e-7 + 4 * u * np.abs(ref)
    err = np.abs(got - ref)
    _report("erf f32 FAST (asin_fast)", err, bound)
    assert (err <= bound).all()


@pytest.mark.parametrize("act", ["relu", "erf"])
def test_map_f32_ntk(L, ctx, act):
    """asin_abs<float> (nngp_math.hpp: ~1.2 ulp of asin) and the f32 square roots on the generic f32 path (NTK requested)."""
    k0, q1, q2, ref, rt, c = _map_inputs(act, "f32")
    gk, gt = _recursion(L, ctx, "f32", act, k0, q1, q2, L.GET_NNGP | L.GET_NTK)
    u = U["f32"]
    if act == "relu":
        S = np.sqrt(np.outer(q1, q2)) / (2 * np.pi)
        # J: asin 1.2 ulp of <= pi/2, sqrt 1 ulp, four roundings of terms <= pi -> 10 u pi absolute; 3 table roundings
        ek = S * 10 * u * np.pi + 3 * u * np.abs(ref)
        kdot_err = 2 * u                                  # 1/4 + asin / (2 pi): asin error / (2 pi) + 2 roundings
    else:
        ek = (2 / np.pi) * 1.2 * u * (np.pi / 2) + 2 * u * np.abs(ref)
        kdot_err = None
    err = np.abs(gk - ref)
    _report("%s f32 NTK-mode NNGP (asin_abs<float>)" % act, err, ek)
    assert (err <= ek).all()
    kt = rt - ref
    et = ek + (np.abs(k0) * kdot_err if kdot_err else 8 * u * np.abs(kt)) + u * np.abs(rt) + 2 * u * np.abs(kt)
    err = np.abs(gt - rt)
    _report("%s f32 NTK" % act, err, et)
    assert (err <= et).all()


# ----------------------------------------------------------------------------- composite kernels
def _cmp_cases():
    out = []
    for name in SETS:
        for t in [str(v) for v in Z["cmp_%s_dtypes" % name]]:
            for net in ("mlp", "resnet"):
                for act in ("relu", "erf"):
                    out.append((name, t, net, act))
    return out


def _dup_columns(x1, x2):
    """(column of x2, row of x1) for the rows of x2 that are rows of x1."""
    out = []
    for j, r in enumerate(x2):
        hit = np.nonzero((x1 == r).all(axis=1))[0]
        if len(hit):
            out.append((j, int(hit[0])))
    return out


@pytest.mark.parametrize("name,t,net,act", _cmp_cases())
def test_composite_kernels_against_mp(name, t, net, act):
    from smnngp import nt_kernels
    fac = nt_kernels.get_mlp_kernel if net == "mlp" else nt_kernels.get_dense_resnet_kernel
    dt = NPT[t]
    x1, x2 = Z["cmp_%s_x1" % name], Z["cmp_%s_x2" % name]
    w, b, lw = (float(v) for v in Z["cmp_%s_hyp" % name])
    worst = 0.0
    for Ln in (1, 3, 6):
        kfn = fac(Ln, act=act, w_std=w, b_std=b, last_w_std=lw)
        got = {}
        for tag, xb in (("sym", None), ("cross", x2)):
            allows = {}
            key = "cmp_%s_%s_%s_L%d_%s" % (name, net, act, Ln, tag)
            ref, bud = Z[key + "_ref"], Z[key + ("_bud64" if t == "f64" else "_bud32")].astype(np.float64)
            xbd = None if xb is None else xb.astype(dt)
            both = kfn(x1.astype(dt), xbd, get=("nngp", "ntk"))
            k = np.asarray(both.nngp, np.float64)
            th = np.asarray(both.ntk, np.float64)
            k1 = np.asarray(kfn(x1.astype(dt), xbd, get="nngp"), np.float64)   # NNGP-only maps (relu_j_f64 / FAST f32)
            for lbl, g, m in (("nngp", k, 0), ("ntk", th, 1), ("nngp-only", k1, 0)):
                assert np.isfinite(g).all(), (key, lbl)
                err = np.abs(g - ref[m])
                allow = bud[m]
                if lbl == "nngp-only" and t == "f32" and net == "mlp" and act == "erf":
                    # FAST erf (asin_fast): its error is ABSOLUTE, <= 2.6e-7 on asin over [-1, 1] (nngp_math.hpp), not relative
                    # to the entry's scale -- at small row norms it dominates the budget (d1 / norms sets: 0.2 % relative on an
                    # entry of 2e-5).  The allowance (injected per layer, amplified by the layers behind it) is shared with
                    # test_gpu_kernel_budget.py: _kernel_budget.fast_erf_allowance.
                    allow = allow + fast_erf_allowance(Ln, w, lw)
                allows[lbl] = allow
                r = float(np.max(err / allow))
                worst = max(worst, r)
                # the fixture's per-entry budget (mp perturbation of every layer's correlation by (d + 2L + 4) u)
                assert (err <= allow).all(), (key, lbl, r)
            if name == "control" and t == "f64":
                # generic inputs: 1e-12 relative (the first 3 rows of x2 are rows of x1, i.e. edge entries)
                gen = slice(None) if xb is None else slice(3, None)
                for g, m in ((k, 0), (th, 1), (k1, 0)):
                    assert relerr(g[:, gen], ref[m][:, gen]) < 1e-12, (key, relerr(g[:, gen], ref[m][:, gen]))
            got[tag] = (k, th, k1, allows)
        # symmetric and cross at the same pair (x2 rows that are rows of x1; the cross entry has c = 1 without the exact
        # diagonal write): within the two budgets
        ks, ts, k1s, bs = got["sym"]
        kc, tc, k1c, bc = got["cross"]
        for j, i in _dup_columns(x1, x2):
            for lbl, gs, gc in (("nngp", ks, kc), ("ntk", ts, tc), ("nngp-only", k1s, k1c)):
                assert (np.abs(gs[:, i] - gc[:, j]) <= bs[lbl][:, i] + bc[lbl][:, j]).all(), (name, Ln, i, j, lbl)
    print("\n[mp] composite %-8s %s %-6s %-4s max err/budget %.3f" % (name, t, net, act, worst))


@pytest.mark.parametrize("t", ["f64", "f32"])
def test_conv_kernel_against_mp(t):
    from smnngp import nt_kernels
    Ln, w, b, lw = Z["conv_params"]
    x = Z["conv_x"].astype(NPT[t])
    k = np.asarray(nt_kernels.get_cnn_kernel(int(Ln), act="relu", w_std=w, b_std=b, last_w_std=lw)(x, None), np.float64)
    bud = Z["conv_bud64" if t == "f64" else "conv_bud32"].astype(np.float64)
    err = np.abs(k - Z["conv_ref"])
    _report("conv relu L=2 %s" % t, err, bud)
    assert (err <= bud).all()


# ----------------------------------------------------------------------------- heads
def test_lml_against_mp(L, ctx):
    y = Z["head_y"]
    worst = 0.0
    for row in Z["head_lml"]:
        _, src, dtb, eps, df, sc, lp, quad, logdet, kappa, bound = row
        dt = np.float32 if dtb == 32 else np.float64
        k = (Z["head_k64"][:40, :40] if src == 0 else Z["head_kdup"]).astype(dt)
        n = k.shape[0]
        kd, yd = ctx.to_device(np.ascontiguousarray(k)), ctx.to_device(y[:n, 0].astype(dt))
        out, info = C.c_double(), C.c_int()
        ctx.call("smn_lml", L.dtype_code(dt), kd.ptr, n, n, yd.ptr, eps, df, sc, C.byref(out), None, None, C.byref(info))
        assert info.value == 0
        # Cholesky backward error gamma = 4 (n + 1) u, first order in kappa(K~) (generator docstring)
        worst = max(worst, abs(out.value - lp) / bound)
        assert abs(out.value - lp) <= bound, (row, out.value)
    print("\n[mp] smn_lml max err/bound %.3e" % worst)


@pytest.mark.parametrize("t,eps", [("f64", 1e-6), ("f64", 1e-2), ("f32", 1e-2)])
def test_predict_against_mp(L, ctx, t, eps):
    dt = NPT[t]
    kj = np.ascontiguousarray(Z["head_k64"].astype(dt))
    y = np.ascontiguousarray(Z["head_y"][:40].astype(dt))
    n, tt, c = 40, kj.shape[0] - 40, y.shape[1]
    key = "head_pred_%s_eps%g" % (t, eps)
    _, kappa, bm, bc = Z[key + "_info"]
    kd, yd = ctx.to_device(kj), ctx.to_device(y)
    mean, cov = ctx.empty((tt, c), dt), ctx.empty((tt, tt), dt)
    quad = (C.c_double * c)()
    logdet, info = C.c_double(), C.c_int()
    ctx.call("smn_predict", L.dtype_code(dt), kd.ptr, n, tt, n + tt, yd.ptr, c, eps, 0.0, mean.ptr, cov.ptr, tt, quad,
             C.byref(logdet), C.byref(info))
    assert info.value == 0
    em = np.abs(mean.numpy().astype(np.float64) - Z[key + "_mean"]).max()
    ec = np.abs(cov.numpy().astype(np.float64) - Z[key + "_cov"]).max()
    print("\n[mp] smn_predict %s eps=%g kappa %.2e: mean %.2e / %.2e, cov %.2e / %.2e" % (t, eps, kappa, em, bm, ec, bc))
    assert em <= bm and ec <= bc      # kappa-based first-order bounds (generator docstring)


@pytest.mark.parametrize("eps", [1e-6, 1e-2])
def test_student_t_test_nll_against_mp(eps):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import StudentTLikelihood
    from smnngp.spax.models import SPR
    x, y = Z["head_x"], Z["head_y"]
    net, act, Ln, w, b, lw = (str(v) for v in Z["head_net"])
    assert net == "mlp"
    _, alpha, beta, nll, _, _, bound = Z["head_testnll_eps%g" % eps]
    kernel = NNGPKernel(lambda ws, bs, ls: nt_kernels.get_mlp_kernel(int(Ln), act=act, w_std=ws, b_std=bs, last_w_std=ls),
                        float(w), float(b), float(lw))
    model = SPR(kernel, StudentTLikelihood(alpha, beta), x[:40], y[:40, 0], 0.0, 1.0, eps=eps)
    got = model.test_nll(x[40:], y[40:, 0])
    print("\n[mp] SPR.test_nll eps=%g: err %.2e bound %.2e" % (eps, abs(got - nll), bound))
    assert abs(got - nll) <= bound
