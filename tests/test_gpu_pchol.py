"""Greedy pivoted Cholesky on the device (csrc/pchol.hip, smnngp/lowrank.py) against the fp64 reference kernels.

Every check is made against the reference's K, never against the device's own output:
  1. factor identity   K[:, P] = L L[P, :]^T for the device's own pivots P; L[P[t], s] = 0 exactly for s > t; L[P[t], t] > 0;
                       resid = diag(K) - sum_t L_it^2; the trace history.
  2. greedy by value   at every step the fp64 residual of the device's pivot, recomputed from K conditional on the device's
                       previous pivots, lies within delta of the largest one (no gap assumption, ties allowed); in f64, on data
                       whose gaps the rules find far above delta, the pivot list equals the rules' list outright.
Tolerances (none taken from the code under test):
  f64   1e-10 of the largest diagonal entry; delta = 1e-10 of the mean diagonal.
  f32   16 x the error of the float32 run of the NumPy rules against their fp64 run on the same pivots (the project's margin
        for a same-precision yardstick: another summation order, not another algorithm), quantity by quantity: for the
        identity its error in L L[P]^T, for the residuals and for delta its largest residual error over all its steps.
  trace a sum of N residuals: N x the residual tolerance.
Each test prints "pchol-multiple" lines: the measured error as a multiple of the yardstick (f32) or of the bound (f64)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _cnn_pool_rules as PR  # noqa: E402
import _pchol_rules as R  # noqa: E402
import _windows as W  # noqa: E402
from oracle import nngp_oracle as O  # noqa: E402

HP = dict(w_std=1.3, b_std=0.2, last_w_std=0.9)
DTYPES = [np.float64, np.float32]
_PI64, _PD = C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) * np.exp(0.5 * rng.standard_normal((n, 1)))


def images(n, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 4, 4, 1)) * np.exp(0.5 * rng.standard_normal((n, 1, 1, 1)))


_ORACLE = {}


def oracle_k(kind, act, x, hp, get="nngp"):
    """The fp64 reference matrix, computed once per (kind, act, data, hyper-parameters) and shared (never modified)."""
    key = (kind, act, x.shape, float(np.sum(x * np.arange(1, x.size + 1).reshape(x.shape))), tuple(sorted(hp.items())), get)
    if key not in _ORACLE:
        if kind == "mlp":
            k = O.mlp_kernel(x, None, num_hiddens=2, act=act, get=get, **hp)
        elif kind == "resnet":
            k = O.dense_resnet_kernel(x, None, num_hiddens=2, act=act, get=get, **hp)
        elif kind == "cnn":
            k = O.cnn_kernel(x, None, num_hiddens=2, act=act, **hp)
        else:
            k = PR.pool_kernel(x, None, num_hiddens=2, act=act, **hp)
        k = np.asarray(k, dtype=np.float64)
        k.setflags(write=False)
        _ORACLE[key] = k
    return _ORACLE[key]


def kernel_fn(kind, act, hp):
    from smnngp import nt_kernels as nt
    make = {"mlp": nt.get_mlp_kernel, "resnet": nt.get_dense_resnet_kernel, "cnn": nt.get_cnn_kernel, "pool": nt.get_cnn_pool_kernel}
    return make[kind](2, act=act, **hp)


def bounds(K, P, dtype):
    """(tolerance of the identity check, of the residual check, delta, yardsticks or None) for the pivots P."""
    dmax, dmean = float(np.diag(K).max()), float(np.diag(K).mean())
    if np.dtype(dtype) == np.float64:
        return 1e-10 * dmax, 1e-10 * dmax, 1e-10 * dmean, None
    m = max(1, len(P))
    r64 = R.pivoted_cholesky(K, m, pivots=P, keep_resid=True)
    r32 = R.pivoted_cholesky(K, m, dtype=np.float32, pivots=P, keep_resid=True)
    assert r32.rank == r64.rank == len(P), "the rules cannot follow the device's pivots: a pivot with a non-positive residual"
    h32, h64 = np.asarray(r32.resid_hist[:len(P)] + [r32.resid]), np.asarray(r64.resid_hist[:len(P)] + [r64.resid])
    e_res = float(np.abs(h32 - h64).max())                  # the largest residual error of the float32 run, over all its steps
    e_id = float(np.abs(r32.L @ r32.L[P].T - r64.L @ r64.L[P].T).max()) if len(P) else 0.0
    return 16.0 * e_id, 16.0 * e_res, 16.0 * e_res, (e_id, e_res)


def check_factor(K, res, dtype, what, max_rank, tol=0.0, rules_pivots=False):
    """Checks 1 and 2 on a result (pivots, factor as a host array, resid, trace, rank)."""
    n = K.shape[0]
    P, Lh, resid, trace, rank = res
    P = np.asarray(P, dtype=np.int64)
    Lh = np.asarray(Lh, dtype=np.float64).reshape(n, rank)
    assert P.shape == (rank,) and trace.shape == (rank + 1,) and resid.shape == (n,) and resid.dtype == np.float64
    assert rank <= max_rank and len(set(P.tolist())) == rank and (rank == 0 or (P.min() >= 0 and P.max() < n))
    assert np.all(np.isfinite(Lh)) and np.all(np.isfinite(resid)) and np.all(np.isfinite(trace))
    tol_id, tol_res, delta, yard = bounds(K, P, dtype)
    unit_id, unit_res = (tol_id, tol_res) if yard is None else yard
    diag = np.diag(K)
    # 1. factor identity
    if rank:
        LP = Lh[P]
        assert np.all(np.triu(LP, 1) == 0.0), "%s: a pivot row is not exactly zero behind its own column" % what
        assert np.all(np.diag(LP) > 0.0), what
        e = float(np.abs(K[:, P] - Lh @ LP.T).max())
        print("pchol-multiple %s identity %.3g" % (what, e / unit_id))
        assert e <= tol_id, (what, e, tol_id)
    sq = np.cumsum(Lh * Lh, axis=1) if rank else np.zeros((n, 0))
    left = [diag] + [diag - sq[:, j] for j in range(rank)]
    e = float(np.abs(resid - left[-1]).max())
    print("pchol-multiple %s resid %.3g" % (what, e / unit_res))
    assert e <= tol_res, (what, e, tol_res)
    tr = np.asarray([np.maximum(v, 0.0).sum() for v in left])
    e = float(np.abs(trace - tr).max())
    print("pchol-multiple %s trace %.3g" % (what, e / (n * unit_res)))
    assert e <= n * tol_res, (what, e, n * tol_res)
    assert np.all(resid[P] == 0.0), what
    # 2. greedy by value
    H = R.conditional_residuals(K, P)
    assert H.shape[0] == rank + 1, what
    worst = max([float(H[j].max() - H[j][P[j]]) for j in range(rank)] + [0.0])
    print("pchol-multiple %s greedy %.3g" % (what, worst / (delta / 16.0 if yard is not None else delta)))
    assert worst <= delta, (what, worst, delta)
    # the stop: an early one needs a reason the reference can see
    floor = R.noise_floor(rank, dtype, diag.max())
    if rank < max_rank:
        by_rank = H[rank].max() <= floor + delta
        by_tol = tol > 0.0 and tr[rank] <= tol * tr[0] + n * delta
        assert by_rank or by_tol, (what, rank, max_rank, float(H[rank].max()), floor, float(tr[rank]), tol * float(tr[0]))
    if rules_pivots:
        rr = R.pivoted_cholesky(K, max_rank, tol=tol)
        assert rr.gaps.min() > 1e3 * delta, "test data: the rules' pivots are not well separated"
        assert P.tolist() == rr.pivots.tolist(), what
    return delta


def run(fn, x, max_rank, dtype, route="auto", tol=0.0):
    from smnngp import lowrank
    r = lowrank.pivoted_cholesky(fn, np.asarray(x, dtype=dtype), max_rank, tol=tol, route=route)
    assert tuple(r.factor.shape) == (x.shape[0], r.rank) and r.factor.dtype == np.dtype(dtype)
    assert r.pivots.dtype == np.int64 and r.trace.dtype == np.float64
    return r.pivots, r.factor.raw_numpy(), r.resid, r.trace, r.rank


# (N, d, max_rank): wave and workgroup edges, more than one argmax partial, more than one thread of the reducing workgroup
# (N = 1000 is 63 partials; the LDS tile is 2048 elements, below every d and rank here except in test_long_rows)
FUSED_SHAPES = [(1, 3, 1), (63, 3, 63), (64, 130, 64), (65, 1, 65), (65, 5, 24), (65, 130, 1), (257, 130, 64), (257, 3, 1),
                (1000, 3, 24), (1000, 130, 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=lambda s: "n%d-d%d-m%d" % s)
def test_fused_mlp(ctx, shape, act, dtype):
    n, d, m = shape
    x = data(n, d).astype(dtype).astype(np.float64)      # the reference sees the values the device holds
    K = oracle_k("mlp", act, x, HP)
    res = run(kernel_fn("mlp", act, HP), x, m, dtype, route="fused")
    check_factor(K, res, dtype, "mlp-%s-%s-n%d-d%d-m%d" % (act, np.dtype(dtype).name, n, d, m), m,
                 rules_pivots=(dtype == np.float64 and shape == (65, 5, 24)))
    if d >= 5 and m < n:
        assert res[4] == m      # these kernels are far from running out of rank


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_fused_dense_resnet(ctx, act, dtype):
    n, d, m = 65, 5, 24
    x = data(n, d).astype(dtype).astype(np.float64)
    K = oracle_k("resnet", act, x, HP)
    res = run(kernel_fn("resnet", act, HP), x, m, dtype)          # "auto" picks the fused route
    check_factor(K, res, dtype, "resnet-%s-%s" % (act, np.dtype(dtype).name), m)
    assert res[4] == m


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_many_rows_are_not_cut_short(ctx, dtype):
    """The rank floor grows with the columns made, not with N: on 3000 points of the plane the largest residual is under
    N eps32 max K_ii from step 24 on, and the f32 factor still runs to its 48 columns (188 partials: the reducing workgroup's
    strided pass)."""
    n, d, m = 3000, 2, 48
    x = data(n, d, seed=7).astype(dtype).astype(np.float64)
    K = oracle_k("mlp", "relu", x, HP)
    H = R.conditional_residuals(K, R.pivoted_cholesky(K, m).pivots)
    assert H[m - 1].max() < n * float(np.finfo(np.float32).eps) * np.diag(K).max()      # what a floor of N eps would have cut
    res = run(kernel_fn("mlp", "relu", HP), x, m, dtype)
    check_factor(K, res, dtype, "many-rows-%s" % np.dtype(dtype).name, m)
    assert res[4] == m


def test_long_rows_cross_the_lds_tile(ctx):
    """d above one LDS tile (2048 elements) and not a multiple of it, and the same through input scales."""
    n, d, m = 33, 2048 + 517, 8
    x = data(n, d, seed=5)
    fn = kernel_fn("mlp", "relu", HP)
    check_factor(oracle_k("mlp", "relu", x, HP), run(fn, x, m, np.float64), np.float64, "long-rows", m)
    s = np.linspace(0.5, 1.5, d)
    check_factor(oracle_k("mlp", "relu", x * s, HP), run(fn.with_input_scales(s), x, m, np.float64), np.float64, "long-rows-scaled", m)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["cnn", "pool", "ntk"])
def test_matrix_route(ctx, kind, dtype):
    m = 12
    if kind == "ntk":
        x = data(65, 5).astype(dtype).astype(np.float64)
        K = oracle_k("mlp", "relu", x, HP, get="ntk")
        fn = kernel_fn("mlp", "relu", HP).with_cov("ntk")
    else:
        x = images(33).astype(dtype).astype(np.float64)
        K = oracle_k(kind, "relu", x, HP)
        fn = kernel_fn(kind, "relu", HP)
    res = run(fn, x, m, dtype)
    check_factor(K, res, dtype, "matrix-%s-%s" % (kind, np.dtype(dtype).name), m)
    assert res[4] == m


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_routes_agree_with_the_reference(ctx, act, dtype):
    """4. the same MLP kernel through both routes: each passes checks 1 and 2 (their bits may differ: one Gram row comes from
    a GEMV, the other from the tile engine)."""
    n, d, m = 65, 5, 24
    x = data(n, d).astype(dtype).astype(np.float64)
    K = oracle_k("mlp", act, x, HP)
    fn = kernel_fn("mlp", act, HP)
    for route in ("fused", "matrix"):
        res = run(fn, x, m, dtype, route=route)
        check_factor(K, res, dtype, "routes-%s-%s-%s" % (route, act, np.dtype(dtype).name), m, rules_pivots=dtype == np.float64)


def test_foreign_callable_with_a_diagonal(ctx):
    K = np.array(oracle_k("mlp", "relu", data(65, 5), HP))
    x = np.arange(65, dtype=np.float64)[:, None]          # the "inputs" are row numbers

    class Stored:
        def __call__(self, a, b):
            return K[np.asarray(a).astype(int).ravel()][:, np.asarray(b).astype(int).ravel()]

        def diag(self, a):
            return np.diag(K)[np.asarray(a).astype(int).ravel()]
    res = run(Stored(), x, 24, np.float64, route="auto")
    check_factor(K, res, np.float64, "foreign", 24, rules_pivots=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_prefix_property_and_repeatability(ctx, dtype):
    """3. the first r columns and pivots of a rank-m call are the bits of a rank-r call; two identical calls give identical bits."""
    x = data(257, 130)
    fn = kernel_fn("mlp", "erf", HP)
    a, b, c = run(fn, x, 40, dtype), run(fn, x, 40, dtype), run(fn, x, 7, dtype)
    assert a[4] == 40 and c[4] == 7
    for u, v in zip(a[:4], b[:4]):
        assert np.array_equal(u, v)
    assert np.array_equal(a[0][:7], c[0]) and np.array_equal(a[3][:8], c[3])
    assert np.array_equal(a[1].reshape(257, 40)[:, :7], c[1].reshape(257, 7))


def call_mlp(ctx, L, dtype, act, hp, xbuf, n, ldx, d, max_rank, tol, lbuf, ldl, net=0):
    resid = ctx.empty((n,), np.float64)
    piv = np.full(max_rank, -1, dtype=np.int64)
    tr = np.full(max_rank + 1, np.nan)
    rank = C.c_int64(-1)
    ctx.call("smn_pchol_mlp", L.dtype_code(dtype), net, L.ACT[act], 2, hp["w_std"], hp["b_std"], hp["last_w_std"], xbuf, n, ldx, d,
             max_rank, tol, lbuf, ldl, resid.ptr, piv.ctypes.data_as(_PI64), tr.ctypes.data_as(_PD), C.byref(rank))
    return piv, resid.raw_numpy(), tr, int(rank.value)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_duplicates_zero_rows_and_rank(ctx, L, act, dtype):
    """5. exact duplicates (a pair and a triple) and an all-zero row under b_std = 0: the lowest index of equals is the pivot, its
    duplicates and the zero row never are, no NaN, the call stops at rank < N with zero columns behind it."""
    n, d = 65, 5
    hp = dict(HP, b_std=0.0)
    x = data(n, d).astype(dtype)
    x[9] = x[5]
    x[20] = x[12]; x[30] = x[12]
    x[7] = 0.0
    K = oracle_k("mlp", act, x.astype(np.float64), hp)
    assert K[7, 7] == 0.0
    xd = ctx.to_device(x)
    lw = W.out_window(ctx, n, n, dtype, "aligned")
    piv, resid, tr, rank = call_mlp(ctx, L, dtype, act, hp, xd.ptr, n, d, d, n, 0.0, lw.ptr, lw.ld)
    Lfull = lw.result("L")
    assert 0 < rank <= n - 4 and np.all(piv[rank:] == -1) and np.all(np.isnan(tr[rank + 1:]))
    assert np.all(Lfull[:, rank:] == 0.0) and np.all(np.isfinite(Lfull))
    P = piv[:rank].tolist()
    assert 5 in P and 12 in P and not {7, 9, 20, 30} & set(P)
    assert np.all(Lfull[7] == 0.0) and resid[7] == 0.0
    check_factor(K, (piv[:rank], Lfull[:, :rank], resid, tr[:rank + 1], rank), dtype,
                 "duplicates-%s-%s" % (act, np.dtype(dtype).name), n)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_tolerance_stops_where_the_rules_stop(ctx, dtype):
    n, d, tol = 65, 5, 0.05
    x = data(n, d).astype(dtype).astype(np.float64)
    K = oracle_k("mlp", "relu", x, HP)
    res = run(kernel_fn("mlp", "relu", HP), x, n, dtype, tol=tol)
    delta = check_factor(K, res, dtype, "tol-%s" % np.dtype(dtype).name, n, tol=tol)
    rr = R.pivoted_cholesky(K, n, tol=tol)
    full = R.pivoted_cholesky(K, n)
    assert 0 < rr.rank < n
    if res[4] != rr.rank:      # one step either side, and only where the rules' trace is within delta N of the threshold
        assert abs(res[4] - rr.rank) == 1
        j = min(res[4], rr.rank)
        assert abs(full.trace[j] - tol * full.trace[0]) <= delta * n
    res_m = run(kernel_fn("mlp", "relu", HP), x, n, dtype, tol=tol, route="matrix")
    delta_m = check_factor(K, res_m, dtype, "tol-matrix-%s" % np.dtype(dtype).name, n, tol=tol)
    if res_m[4] != rr.rank:
        assert abs(res_m[4] - rr.rank) == 1
        j = min(res_m[4], rr.rank)
        assert abs(full.trace[j] - tol * full.trace[0]) <= delta_m * n


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("layout", ["aligned", "unaligned"])
def test_fused_windows(ctx, L, layout, dtype):
    """6. ldx > d with d no multiple of the 16-byte vector, ldl > max_rank: the bits of the contiguous call, NaN around x never
    read, nothing written outside the L window."""
    n, d, m = 65, 7, 24
    x = data(n, d).astype(dtype)
    xd = ctx.to_device(x)
    lc = ctx.empty((n, m), dtype)
    want = call_mlp(ctx, L, dtype, "relu", HP, xd.ptr, n, d, d, m, 0.0, lc.ptr, m)
    xw = W.in_window(ctx, x, layout)
    lw = W.out_window(ctx, n, m, dtype, layout)
    assert xw.ld > d and lw.ld > m
    got = call_mlp(ctx, L, dtype, "relu", HP, xw.ptr, n, xw.ld, d, m, 0.0, lw.ptr, lw.ld)
    assert want[3] == got[3] == m
    for u, v in zip(want[:3], got[:3]):
        assert np.array_equal(u, v, equal_nan=True)
    assert np.array_equal(lw.result("L"), lc.raw_numpy())
    check_factor(oracle_k("mlp", "relu", x.astype(np.float64), HP), (got[0], lw.result("L"), got[1], got[2], m), dtype,
                 "windows-%s-%s" % (layout, np.dtype(dtype).name), m)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("layout", ["aligned", "unaligned"])
def test_matrix_form_entries_on_a_stored_matrix(ctx, L, layout, dtype):
    """smn_pchol_begin / smn_pchol_step on rows of the reference matrix, L in a window: in f64 the rules' pivots and values."""
    n, m = 257, 20
    K = oracle_k("mlp", "erf", data(n, 5), HP)
    Kd = K.astype(dtype)
    K_seen = Kd.astype(np.float64)
    code = L.dtype_code(dtype)
    diag = ctx.to_device(np.ascontiguousarray(np.diag(Kd)))
    resid = ctx.empty((n,), np.float64)
    lw = W.out_window(ctx, n, m, dtype, layout)
    piv, rmax, tr = C.c_int64(-1), C.c_double(), C.c_double()
    ctx.call("smn_pchol_begin", code, n, diag.ptr, resid.ptr, C.byref(piv), C.byref(rmax), C.byref(tr))
    assert piv.value == int(np.argmax(np.diag(K_seen))) and rmax.value == np.diag(K_seen).max()
    P, trace = [], [tr.value]
    for j in range(m):
        p = piv.value
        row = ctx.to_device(np.ascontiguousarray(Kd[p]))
        ctx.call("smn_pchol_step", code, n, j, p, row.ptr, lw.ptr, lw.ld, resid.ptr, C.byref(piv), C.byref(rmax), C.byref(tr))
        P.append(p); trace.append(tr.value)
    Lh = lw.result("L")
    res = (np.asarray(P), Lh, resid.raw_numpy(), np.asarray(trace), m)
    check_factor(K_seen, res, dtype, "entries-%s-%s" % (layout, np.dtype(dtype).name), m)
    rr = R.pivoted_cholesky(K_seen, m, dtype=dtype)
    assert P == rr.pivots.tolist()
    assert np.abs(Lh - rr.L).max() <= 64 * np.finfo(dtype).eps * np.abs(rr.L).max()      # the same steps in the same precision
    # a pivot whose residual is not > 0 is refused and nothing moves
    before = (lw.download(), resid.raw_numpy())
    with pytest.raises(L.SmnError) as e:
        ctx.call("smn_pchol_step", code, n, m - 1, P[0], row.ptr, lw.ptr, lw.ld, resid.ptr, C.byref(piv), C.byref(rmax), C.byref(tr))
    assert e.value.code == L.EINVAL
    assert np.array_equal(lw.download(), before[0]) and np.array_equal(resid.raw_numpy(), before[1])


def test_entries_refuse_bad_arguments(ctx, L):
    n, d, m = 20, 3, 5
    xd = ctx.to_device(data(n, d))
    lc = ctx.empty((n, m), np.float64)
    bad = [dict(max_rank=n + 1, ldl=n + 1), dict(max_rank=0), dict(tol=-1e-3), dict(ldl=m - 1), dict(ldx=d - 1), dict(x=None),
           dict(l=None)]
    for kw in bad:
        with pytest.raises(L.SmnError) as e:
            call_mlp(ctx, L, np.float64, "relu", HP, kw.get("x", xd.ptr), n, kw.get("ldx", d), d, kw.get("max_rank", m),
                     kw.get("tol", 0.0), kw.get("l", lc.ptr), kw.get("ldl", m))
        assert e.value.code == L.EINVAL, kw
    with pytest.raises(L.SmnError) as e:
        call_mlp(ctx, L, np.float64, "relu", HP, xd.ptr, n, d, d, m, 0.0, lc.ptr, m, net=L.NET_NTK)
    assert e.value.code == L.ENOTSUP
    resid = ctx.empty((n,), np.float64)
    piv, rmax, tr = C.c_int64(), C.c_double(), C.c_double()
    with pytest.raises(L.SmnError) as e:      # j >= ldl
        ctx.call("smn_pchol_step", L.F64, n, m, 0, xd.ptr, lc.ptr, m, resid.ptr, C.byref(piv), C.byref(rmax), C.byref(tr))
    assert e.value.code == L.EINVAL
    with pytest.raises(L.SmnError) as e:
        ctx.call("smn_pchol_begin", L.F64, n, None, resid.ptr, C.byref(piv), C.byref(rmax), C.byref(tr))
    assert e.value.code == L.EINVAL


def test_svsp_from_greedy(ctx):
    """7. the inducing images are x_pool[pivots] of greedy_variance_points; the model's moments and loss run on them."""
    from smnngp import lowrank, nt_kernels as nt
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import SVSP
    from smnngp.spax.priors import GaussianPrior
    pool = images(33)
    kernel = NNGPKernel(lambda w, b, l: nt.get_cnn_kernel(2, 3, "relu", w_std=w, b_std=b, last_w_std=l), 1.3, 0.2, 0.9)
    model = SVSP.from_greedy(GaussianPrior(), kernel, pool, 10, num_latent_gps=3, eps=1e-3)
    piv = lowrank.greedy_variance_points(kernel.get_kernel_fn(), pool, 10)
    assert piv.shape == (10,) and len(set(piv.tolist())) == 10
    assert model.num_inducing == 10 and np.array_equal(model.inducing_variable.value, pool[piv])
    K = oracle_k("cnn", "relu", pool, HP)
    assert piv.tolist() == R.pivoted_cholesky(K, 10).pivots.tolist()
    rng = np.random.default_rng(2)
    xb, yb = images(16, seed=9), rng.integers(0, 3, 16)
    mean, var, info, nonpos = model.posterior_moments(xb)
    assert info == 0 and nonpos == 0 and np.all(np.isfinite(mean.raw_numpy())) and np.all(np.isfinite(var.raw_numpy()))
    value, grads = model.loss_and_grad(3, xb, yb, 1000, 8, kernel_grads=False)
    assert np.isfinite(value) and all(np.all(np.isfinite(g)) for g in grads.values())
    with pytest.raises(ValueError, match="numerical rank"):
        SVSP.from_greedy(GaussianPrior(), kernel, np.repeat(pool[:3], 4, axis=0), 6, num_latent_gps=3)
