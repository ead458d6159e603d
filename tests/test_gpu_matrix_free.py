"""Matrix-free exact GP on the device: smn_kernel_mlp_matmul (K V without K) and smn_pcg_solve (block PCG on K + lam I).

K-apply
  unit-vector probes   V = columns of the identity: out must equal the matching columns of smn_kernel_mlp (same arguments, full
                       fill) bit for bit, as fp64 of the stored value -- one exact product plus zeros is exact.  Shapes: n = 130
                       symmetric (two row tiles, a ragged edge, a duplicate row, a scaled row, a zero row with b_std = 0), cross
                       130 x 70 with d = 33 (two K-steps in f64, a ragged K-step), and n2 = SMN_MATMUL_SPLIT + 5 (columns in both
                       splits).  More probes than one column pass holds.
  dense V              |out - K_ref V|_ik <= sum_j E_ij |V_jk| + (SMN_MATMUL_SPLIT + 2) u sum_j |K_ij V_jk| with E the entry budget
                       of tests/_kernel_budget.py as test_gpu_kernel_budget.py holds the build to it (f64: twice the budget, the
                       FAST erf allowance), K_ref in fp64 on the stored inputs; a shift adds one fp64 rounding.
  same bits            two calls; odd ldx / ldv / ldo with every base misaligned by one element; column 0 alone against the same
                       column inside t = pass width + 1.
  validation           every SMN_EINVAL / SMN_ENOTSUP case by name.
PCG (n = 300 and 130, d = 7, eps = 1e-2, three right-hand sides): see the tests.
Each dense case prints its largest err / bound (run with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _kernel_budget as KB
import _pcg_rules as CG
import _windows as W
from oracle import nngp_oracle as O

pytestmark = pytest.mark.gpu

NETS = (("mlp", "relu", 0), ("mlp", "relu", 3), ("mlp", "erf", 2), ("resnet", "relu", 1), ("resnet", "erf", 3))
NET_IDS = ["%s-%s%d" % n for n in NETS]
WS, BS, LW = 1.4, 0.3, 0.8
HP = dict(w_std=1.3, b_std=0.2, last_w_std=0.9)


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def _kfn(net, act, layers, cov="nngp", b_std=BS):
    from smnngp import nt_kernels
    fac = nt_kernels.get_mlp_kernel if net == "mlp" else nt_kernels.get_dense_resnet_kernel
    return fac(layers, act=act, w_std=WS, b_std=b_std, last_w_std=LW).with_cov(cov)


def _probe(kfn, x1, x2, cols):
    """(out, want): the product with unit vectors at `cols`, and those columns of the stored kernel as fp64."""
    from smnngp import lowrank
    n2 = x1.shape[0] if x2 is None else x2.shape[0]
    v = np.zeros((n2, len(cols)), dtype=x1.dtype)
    v[cols, np.arange(len(cols))] = 1.0
    out = lowrank.kernel_matmul(kfn, x1, x2, v).numpy()
    k = kfn(x1, x2, get=kfn.cov).numpy()
    assert k.dtype == x1.dtype and out.dtype == np.float64
    return out, k[:, cols].astype(np.float64)


def _special_rows(n, d, t):
    x = KB.gauss(n, d, t, seed=3).copy()
    x[77] = x[5]            # an exact duplicate, in another MFMA block of the same tile
    x[129] = 3.0 * x[40]    # a scaled row, in the ragged second tile
    x[64] = 0.0             # a zero row
    return x


@pytest.mark.parametrize("cov", ["nngp", "ntk"])
@pytest.mark.parametrize("net,act,layers", NETS, ids=NET_IDS)
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_unit_vector_probes_symmetric(t, net, act, layers, cov):
    n, d = 130, 7
    cols = [0, 1, 5, 15, 16, 40, 63, 64, 65, 77, 100, 127, 128, 129, 3, 31, 32, 111, 126]      # 19 > one pass of 16
    for b_std in (BS, 0.0):
        x = _special_rows(n, d, t)
        out, want = _probe(_kfn(net, act, layers, cov, b_std), x, None, cols)
        assert np.isfinite(out).all(), (b_std,)
        assert np.array_equal(out, want), (b_std, np.argwhere(out != want)[:4])


@pytest.mark.parametrize("cov", ["nngp", "ntk"])
@pytest.mark.parametrize("net,act,layers", NETS[1:], ids=NET_IDS[1:])
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_unit_vector_probes_cross(t, net, act, layers, cov):
    xa = KB.gauss(200, 33, t, seed=4)
    x1, x2 = xa[:130], xa[130:]
    cols = [0, 1, 15, 16, 17, 63, 64, 69, 33, 2, 50, 68, 31, 32, 48, 5, 7]                   # 17 probes of the 70 columns
    out, want = _probe(_kfn(net, act, layers, cov), x1, x2, cols)
    assert np.array_equal(out, want), np.argwhere(out != want)[:4]


@pytest.mark.parametrize("t,net,act,layers,cov", [("f32", "mlp", "relu", 3, "nngp"), ("f32", "resnet", "erf", 3, "ntk"),
                                                  ("f64", "mlp", "erf", 2, "nngp"), ("f64", "resnet", "relu", 1, "ntk")])
def test_unit_vector_probes_across_the_split(L, t, net, act, layers, cov):
    n2 = L.MATMUL_SPLIT + 5
    xa = KB.gauss(130 + n2, 7, t, seed=5)
    x1, x2 = xa[:130], xa[130:]
    cols = [0, 127, 128, 2047, L.MATMUL_SPLIT - 1, L.MATMUL_SPLIT, L.MATMUL_SPLIT + 1, n2 - 1]
    out, want = _probe(_kfn(net, act, layers, cov), x1, x2, cols)
    assert np.array_equal(out, want), np.argwhere(out != want)[:4]
    # one vector with ones on both sides of the split: the two partials meet in the fp64 reduction
    from smnngp import lowrank
    v = np.zeros((n2, 1), dtype=x1.dtype)
    v[[5, L.MATMUL_SPLIT + 2], 0] = 1.0
    k = _kfn(net, act, layers, cov)(x1, x2, get=cov).numpy().astype(np.float64)
    got = lowrank.kernel_matmul(_kfn(net, act, layers, cov), x1, x2, v).numpy()[:, 0]
    assert np.array_equal(got, k[:, 5] + k[:, L.MATMUL_SPLIT + 2])


# ---------------------------------------------------------------------------------------------------------------- dense V
@functools.lru_cache(maxsize=None)
def _dense_reference(t, n1, n2, d, net, act, layers):
    """Inputs and, once per case, the fp64 reference entries and budgets of the whole rectangle (both kernels)."""
    xa = KB.gauss(n1 + (n2 or 0), d, t, seed=6)
    x1, x2 = xa[:n1], (None if n2 is None else xa[n1:])
    m2 = n1 if n2 is None else n2
    i, j = np.divmod(np.arange(n1 * m2), m2)
    ref, bud = KB.reference(net, act, layers, WS, BS, LW, x1, x2, i, j, d, KB.U[t])
    for a in list(ref) + list(bud):
        a.setflags(write=False)
    return x1, x2, [r.reshape(n1, m2) for r in ref], [b.reshape(n1, m2) for b in bud]


def _entry_allow(t, bud, net, act, layers, cov):
    """The allowance test_gpu_kernel_budget.py gives a stored entry: f64 twice the budget; f32 the budget plus asin_fast's."""
    if t == "f64":
        return 2.0 * bud
    fast = layers if (net == "mlp" and act == "erf" and cov == "nngp") else 0
    return bud + (KB.fast_erf_allowance(fast, WS, LW) if fast else 0.0)


DENSE = [("sym130-d7", 130, None, 7), ("cross130x70-d33", 130, 70, 33), ("cross130xsplit+5-d7", 130, 4096 + 5, 7)]


@pytest.mark.parametrize("cov", ["nngp", "ntk"])
@pytest.mark.parametrize("net,act,layers", NETS[1:], ids=NET_IDS[1:])
@pytest.mark.parametrize("case", DENSE, ids=[c[0] for c in DENSE])
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_dense_product_within_the_entry_budget(L, t, case, net, act, layers, cov):
    from smnngp import lowrank
    name, n1, n2, d = case
    assert n2 is None or n2 < 4096 or n2 == L.MATMUL_SPLIT + 5
    x1, x2, ref, bud = _dense_reference(t, n1, n2, d, net, act, layers)
    m = 0 if cov == "nngp" else 1
    kref, allow = ref[m], _entry_allow(t, bud[m], net, act, layers, cov)
    m2 = kref.shape[1]
    v = np.random.default_rng([n1, m2, 9]).standard_normal((m2, 5)).astype(KB.NPT[t])
    v64 = v.astype(np.float64)
    u = KB.U[t]
    bound = allow @ np.abs(v64) + (L.MATMUL_SPLIT + 2) * u * (np.abs(kref) @ np.abs(v64))
    kfn = _kfn(net, act, layers, cov)
    out = lowrank.kernel_matmul(kfn, x1, x2, v).numpy()
    err = np.abs(out - kref @ v64)
    print("\n[matmul] %-28s %s %s-%s%d %s  max err/bound %.3f" % (name, t, net, act, layers, cov, float((err / bound).max())))
    assert (err <= bound).all(), float((err / bound).max())
    if n2 is None:
        shift = 0.37
        outs = lowrank.kernel_matmul(kfn, x1, None, v, shift=shift).numpy()
        want = kref @ v64 + shift * v64
        errs = np.abs(outs - want)
        assert (errs <= bound + 2.0 ** -52 * (np.abs(want) + np.abs(shift * v64))).all()
        # the shift is one fp64 operation (a fused multiply-add, or a product and a sum) behind the reduction
        assert (np.abs(outs - (out + shift * v64)) <= 2.0 ** -52 * (np.abs(out) + np.abs(shift * v64))).all()


# --------------------------------------------------------------------------------------------------------------- same bits
def _raw_matmul(ctx, L, kfn, x1, x2, v, layout, shift=0.0):
    """The C entry on windows: inputs inside NaN guards, the output inside a pattern guard that must come back untouched."""
    wx1 = W.in_window(ctx, x1, layout)
    wx2 = None if x2 is None else W.in_window(ctx, x2, layout)
    wv = W.in_window(ctx, v, layout)
    wo = W.out_window(ctx, x1.shape[0], v.shape[1], np.float64, layout)
    ctx.call("smn_kernel_mlp_matmul", L.dtype_code(x1.dtype), kfn.params[0], kfn.act, kfn.num_hiddens, kfn.w_std, kfn.b_std,
             kfn.last_w_std, wx1.ptr, x1.shape[0], wx1.ld, None if wx2 is None else wx2.ptr, 0 if x2 is None else x2.shape[0],
             0 if wx2 is None else wx2.ld, x1.shape[1], shift, wv.ptr, v.shape[1], wv.ld, wo.ptr, wo.ld)
    return wo.result("smn_kernel_mlp_matmul out")


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "cross"])
def test_same_bits_across_calls_layouts_and_column_counts(ctx, L, t, sym):
    from smnngp import lowrank
    xa = KB.gauss(200, 33, t, seed=8)
    x1, x2 = xa[:130], (None if sym else xa[130:])
    m2 = 130 if sym else 70
    tw = L.MATMUL_PASS + 1
    v = np.random.default_rng(12).standard_normal((m2, tw)).astype(KB.NPT[t])
    for net, act, layers, cov in (("mlp", "relu", 3, "nngp"), ("resnet", "erf", 3, "ntk")):
        kfn = _kfn(net, act, layers, cov)
        a = lowrank.kernel_matmul(kfn, x1, x2, v).numpy()
        assert np.array_equal(a, lowrank.kernel_matmul(kfn, x1, x2, v).numpy())
        assert np.array_equal(a, _raw_matmul(ctx, L, kfn, x1, x2, v, "aligned"))
        assert np.array_equal(a, _raw_matmul(ctx, L, kfn, x1, x2, v, "unaligned"))
        alone = lowrank.kernel_matmul(kfn, x1, x2, np.ascontiguousarray(v[:, :1])).numpy()
        assert np.array_equal(alone[:, 0], a[:, 0])
        last = lowrank.kernel_matmul(kfn, x1, x2, np.ascontiguousarray(v[:, tw - 1:])).numpy()
        assert np.array_equal(last[:, 0], a[:, tw - 1])          # the column of the second pass, alone in a first pass


# -------------------------------------------------------------------------------------------------------------- validation
def test_matmul_validation_by_name(ctx, L):
    x = ctx.to_device(np.ones((10, 3), np.float32))
    v = ctx.to_device(np.ones((10, 2), np.float32))
    out = ctx.empty((10, 2), np.float64)
    good = dict(dtype=L.F32, net=L.NET_MLP, act=0, nh=2, x1=x.ptr, n1=10, ldx1=3, x2=None, n2=0, ldx2=0, d=3, shift=0.0, v=v.ptr, t=2,
                ldv=2, out=out.ptr, ldo=2)

    def call(**kw):
        a = dict(good, **kw)
        ctx.call("smn_kernel_mlp_matmul", a["dtype"], a["net"], a["act"], a["nh"], 1.0, 0.5, 1.0, a["x1"], a["n1"], a["ldx1"], a["x2"],
                 a["n2"], a["ldx2"], a["d"], a["shift"], a["v"], a["t"], a["ldv"], a["out"], a["ldo"])

    call()
    cross = dict(x2=x.ptr, n2=10, ldx2=3)
    call(**cross)
    for kw, word in ((dict(x1=None), "NULL"), (dict(v=None), "NULL"), (dict(out=None), "NULL"), (dict(n1=0), "empty"),
                     (dict(d=0), "empty"), (dict(t=0), "t ="), (dict(cross, n2=0), "empty"), (dict(ldx1=2), "ldx1"),
                     (dict(cross, ldx2=2), "ldx2"), (dict(ldv=1), "ldv"), (dict(ldo=1), "ldo"), (dict(dtype=7), "dtype"),
                     (dict(act=5), "act"), (dict(net=3), "net"), (dict(nh=-1), "num_hiddens"), (dict(shift=float("nan")), "shift"),
                     (dict(shift=float("inf")), "shift"), (dict(cross, shift=0.5), "shift")):
        with pytest.raises(L.SmnError) as e:
            call(**kw)
        assert e.value.code == L.EINVAL and word in str(e.value), (kw, str(e.value))
    for kw in (dict(nh=17), dict(net=L.NET_DENSE_RESNET, nh=16)):
        with pytest.raises(L.SmnError) as e:
            call(**kw)
        assert e.value.code == L.ENOTSUP and "16" in str(e.value), (kw, str(e.value))
    call(nh=16)
    call(net=L.NET_DENSE_RESNET | L.NET_NTK, nh=15)


# --------------------------------------------------------------------------------------------------------------------- PCG
def _mlp2(cov="nngp"):
    from smnngp import nt_kernels
    return nt_kernels.get_mlp_kernel(2, act="relu", **HP).with_cov(cov)


@functools.lru_cache(maxsize=None)
def _pcg_problem(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 7)) * np.exp(0.5 * rng.standard_normal((n, 1)))
    K = np.asarray(O.mlp_kernel(x, None, num_hiddens=2, act="relu", **HP), dtype=np.float64)
    lam = 1e-2 * np.trace(K) / n
    b = np.stack([np.sin(x[:, 0]), rng.standard_normal(n), rng.standard_normal(n)], axis=1)
    import scipy.linalg
    xd = scipy.linalg.solve(K + lam * np.eye(n), b, assume_a="pos")
    for a in (x, K, b, xd):
        a.setflags(write=False)
    return x, K, lam, b, xd


@pytest.mark.parametrize("n", [300, 130])
def test_pcg_f64_against_the_dense_solve_and_the_restatement(n):
    from smnngp import lowrank
    x, K, lam, b, xd = _pcg_problem(n)
    tol = 1e-8
    kfn = _mlp2()
    res32 = lowrank.pivoted_cholesky(kfn, x, 32)
    Lh = np.asarray(res32.factor.raw_numpy(), np.float64)
    iters = {}
    for tag, pre, Lr in (("none", None, None), ("rank32", res32, Lh)):
        r = lowrank.pcg_solve(kfn, x, b, lam, precond=pre, tol=tol, max_iter=2000)
        assert r.info == 0 and r.converged and (r.resid <= 2 * tol).all(), (tag, r.info, r.resid)
        xs = r.x.numpy()
        for k in range(3):
            bound = np.linalg.norm(b[:, k] - (K @ xs[:, k] + lam * xs[:, k])) / lam + 1e-12 * np.linalg.norm(xd[:, k])
            assert np.linalg.norm(xs[:, k] - xd[:, k]) <= bound, (tag, k)
        lo = CG.pcg(K, b, lam, Lr, tol=4 * tol, max_iter=2000)
        hi = CG.pcg(K, b, lam, Lr, tol=tol / 4, max_iter=2000)
        print("\n[pcg] n=%d %s: device col_iters %s, restatement %s .. %s" % (n, tag, r.col_iters, lo.col_iters, hi.col_iters))
        assert (lo.col_iters <= r.col_iters).all() and (r.col_iters <= hi.col_iters).all(), (tag, lo.col_iters, r.col_iters, hi.col_iters)
        assert r.iters == r.col_iters.max() and r.history.shape == (r.iters + 1, 3)
        again = lowrank.pcg_solve(kfn, x, b, lam, precond=pre, tol=tol, max_iter=2000)
        assert np.array_equal(again.x.numpy(), xs) and np.array_equal(again.history, r.history)          # two calls, same bits
        assert np.array_equal(again.resid, r.resid) and np.array_equal(again.col_iters, r.col_iters)
        warm = lowrank.pcg_solve(kfn, x, b, lam, precond=pre, tol=2 * tol, x0=xs)
        assert warm.iters == 0 and warm.info == 0 and np.array_equal(warm.x.numpy(), xs)
        iters[tag] = r.iters
    assert 2 * iters["rank32"] <= iters["none"], iters
    full = lowrank.pcg_solve(kfn, x, b, lam, precond=lowrank.pivoted_cholesky(kfn, x, n), tol=tol)
    assert full.info == 0 and full.iters <= 2, full.iters


@pytest.mark.parametrize("n", [300, 130])
def test_pcg_f32_against_the_same_precision_yardstick(n):
    from smnngp import lowrank
    x, K, lam, b, _ = _pcg_problem(n)
    tol = 1e-4
    x32 = x.astype(np.float32)
    K32 = np.asarray(O.mlp_kernel(x32.astype(np.float64), None, num_hiddens=2, act="relu", **HP), dtype=np.float64)
    kfn = _mlp2()
    for pre in (None, lowrank.pivoted_cholesky(kfn, x32, 32)):
        Lr = None if pre is None else np.asarray(pre.factor.raw_numpy(), np.float64)
        r = lowrank.pcg_solve(kfn, x32, b, lam, precond=pre, tol=tol, max_iter=2000)
        ref = CG.pcg(K32, b, lam, Lr, tol=tol, max_iter=2000, round_to=np.float32)
        ratio = r.resid / np.maximum(tol, ref.resid)
        print("\n[pcg f32] n=%d precond=%s resid %s yardstick %s worst ratio %.3f" % (n, pre is not None, r.resid, ref.resid, ratio.max()))
        assert r.info == 0 and ref.info == 0
        assert (ratio <= 16.0).all(), ratio


def test_pcg_other_cases(ctx, L):
    from smnngp import lowrank
    x, K, lam, b, xd = _pcg_problem(130)
    kfn = _mlp2()
    short = lowrank.pcg_solve(kfn, x, b, lam, tol=1e-8, max_iter=2)
    assert short.info == 1 and not short.converged and short.iters == 2 and np.isfinite(short.x.numpy()).all()
    assert np.isfinite(short.resid).all() and (short.resid > 1e-8).any()
    bz = b.copy()
    bz[:, 1] = 0.0
    z = lowrank.pcg_solve(kfn, x, bz, lam, tol=1e-8)
    assert z.info == 0 and (z.x.numpy()[:, 1] == 0.0).all() and z.col_iters[1] == 0 and z.resid[1] == 0.0
    one = lowrank.pcg_solve(kfn, x, b[:, 0], lam, tol=1e-8)
    assert one.info == 0 and one.x.shape == (130, 1)
    assert np.linalg.norm(one.x.numpy()[:, 0] - xd[:, 0]) <= 1e-6 * np.linalg.norm(xd[:, 0])
    wide = np.random.default_rng(48).standard_normal((130, 48))
    r48 = lowrank.pcg_solve(kfn, x, wide, lam, tol=1e-8)
    assert r48.info == 0 and (r48.resid <= 2e-8).all()
    ntk = lowrank.pcg_solve(_mlp2("ntk"), x, b, lam, tol=1e-8, max_iter=2000)
    assert ntk.info == 0 and (ntk.resid <= 2e-8).all()
    xdev = ctx.to_device(x)
    bdev = ctx.to_device(np.zeros((130, 49)))
    sol = ctx.empty((130, 49), np.float64)
    it, info = C.c_int(0), C.c_int(0)
    resid = np.zeros(49)

    def call(**kw):
        a = dict(dtype=L.F64, net=L.NET_MLP, act=0, x=xdev.ptr, n=130, ldx=7, d=7, lam=lam, Lp=None, m=0, ldl=1, b=bdev.ptr, c=3, ldb=49,
                 tol=1e-6, max_iter=5, sol=sol.ptr, lds=49, resid=resid.ctypes.data_as(C.POINTER(C.c_double)))
        a.update(kw)
        ctx.call("smn_pcg_solve", a["dtype"], a["net"], a["act"], 2, 1.3, 0.2, 0.9, a["x"], a["n"], a["ldx"], a["d"], a["lam"], a["Lp"],
                 a["m"], a["ldl"], a["b"], a["c"], a["ldb"], a["tol"], a["max_iter"], 0, a["sol"], a["lds"], C.byref(it), None, a["resid"],
                 None, C.byref(info))

    call()
    with pytest.raises(L.SmnError) as e:
        call(c=49)
    assert e.value.code == L.ENOTSUP and "48" in str(e.value)
    for kw, word in ((dict(lam=0.0), "lambda"), (dict(lam=float("inf")), "lambda"), (dict(tol=0.0), "tol"), (dict(tol=1.0), "tol"),
                     (dict(max_iter=0), "max_iter"), (dict(m=-1), "m ="), (dict(Lp=xdev.ptr, m=131), "m ="),
                     (dict(Lp=xdev.ptr, m=4, ldl=3), "ldl"), (dict(c=0), "c ="), (dict(b=None), "NULL"), (dict(sol=None), "NULL"),
                     (dict(x=None), "NULL"), (dict(ldb=2), "ldb"), (dict(lds=2), "lds"), (dict(ldx=6), "ldx"), (dict(act=9), "act"),
                     (dict(dtype=5), "dtype"), (dict(resid=None), "NULL")):
        with pytest.raises(L.SmnError) as e:
            call(**kw)
        assert e.value.code == L.EINVAL and word in str(e.value), (kw, str(e.value))


# ------------------------------------------------------------------------------------------------------------------- model
def _models(cov, lik):
    """(IterativeSPR, SPR) on one data set in fp64, tol = 1e-10, and the fp64 host pieces the bounds need."""
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel, NTKKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR, IterativeSPR
    rng = np.random.default_rng(300)
    n, t, d = 300, 53, 7
    xa = rng.standard_normal((n + t, d)) * np.exp(0.5 * rng.standard_normal((n + t, 1)))
    y = np.sin(xa[:n, 0]) + 0.1 * rng.standard_normal(n)
    yt = np.sin(xa[n:, 0])
    cls = NNGPKernel if cov == "nngp" else NTKKernel
    kernel = cls(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.3, 0.2, 0.9)
    like = GaussianLikelihood() if lik == "gauss" else StudentTLikelihood(2.0, 2.0)
    exact = SPR(kernel, like, xa[:n], y, 0.1, 1.7, eps=1e-2)
    it = IterativeSPR.from_model(exact, rank=32, tol=1e-10, max_iter=3000)
    return it, exact, xa[:n], y, xa[n:], yt


@pytest.mark.parametrize("cov", ["nngp", "ntk"])
def test_model_predictions_against_spr(cov):
    it, exact, x, y, xt, yt = _models(cov, "gauss")
    assert it.eps.safe_value == exact.eps.safe_value and it.kernel is exact.kernel
    mean, var = it.predict(xt, var=True, var_block=20)
    sol = it.solve_info
    assert sol.info == 0 and sol.resid[0] <= 2e-10
    m_ref, c_ref = exact.predict(xt)
    m_ref, c_ref = np.asarray(m_ref.numpy(), np.float64), np.asarray(c_ref.numpy(), np.float64)
    kfn = exact.kernel.get_kernel_fn()
    kst = np.asarray(kfn(xt, x, get=kfn.cov).numpy(), np.float64)                 # k*_i: row i
    lam = it._fit_cache[2]
    knorm = np.linalg.norm(kst, axis=1)
    r_abs = sol.resid[0] * np.linalg.norm(y)
    bound = knorm * r_abs / lam + 1e-10 * np.abs(m_ref).max()
    assert (np.abs(mean[:, 0] - m_ref[:, 0]) <= bound).all(), float((np.abs(mean[:, 0] - m_ref[:, 0]) / bound).max())
    v_ref = np.diag(c_ref)
    for bi, blk in enumerate(it.var_info):
        sl = slice(20 * bi, 20 * bi + blk.x.shape[1])
        assert blk.info == 0
        r_cols = blk.resid * knorm[sl]                                             # |b_j| = |k*_j|: the absolute residual of column j
        vb = knorm[sl] * r_cols / lam + 1e-10 * np.abs(v_ref).max()
        assert (np.abs(var[sl] - v_ref[sl]) <= vb).all(), (bi, float((np.abs(var[sl] - v_ref[sl]) / vb).max()))
    nll, nll_ref = it.test_nll(xt, yt), exact.test_nll(xt, yt)
    assert abs(nll - nll_ref) <= 1e-6 * abs(nll_ref), (nll, nll_ref)


def test_model_student_t_head_and_carry_over():
    from smnngp.spax.models import IterativeSPR, LowRankSPR
    it, exact, x, y, xt, yt = _models("nngp", "student")
    nll = it.test_nll(xt, yt)
    mean, var = it.predict(xt, var=True)
    kfn = exact.kernel.get_kernel_fn()
    K = np.asarray(O.mlp_kernel(x, None, num_hiddens=2, act="relu", **HP), dtype=np.float64)
    lam = 1e-2 * np.trace(K) / 300
    quad = float(y @ np.linalg.solve(K + lam * np.eye(300), y))
    df, scale = exact.likelihood.lml_params()
    ys, mu, v = yt * 1.7 + 0.1, mean[:, 0] * 1.7 + 0.1, var * 1.7 ** 2
    sigma = np.sqrt((df + quad / scale) / (df + 300) * scale * v)
    want = -np.mean(O.student_t_logpdf(ys, df + 300, mu, sigma))
    assert abs(nll - want) <= 1e-6 * abs(want), (nll, want)          # the Gaussian head's figure: the same marginals, quad to 1e-10 / lam
    low = LowRankSPR(exact.kernel, exact.likelihood, x, y, 0.1, 1.7, rank=16, eps=3e-3)
    again = IterativeSPR.from_model(low, rank=0, tol=1e-6)
    assert again.eps.safe_value == low.eps.safe_value and again.kernel is low.kernel and again.rank == 0
    assert np.array_equal(again.y_host, low.y_host) and again.y_std == 1.7 and again.y_mean == 0.1
    assert again.fit().info == 0
    for call in (it.loss, it.loss_and_grad, it.loo_loss, it.posterior):
        with pytest.raises(NotImplementedError):
            call()
    short = IterativeSPR.from_model(exact, rank=0, tol=1e-10, max_iter=2)
    with pytest.warns(RuntimeWarning, match="info = 1"):
        m2, _ = short.predict(xt)
    assert np.isfinite(m2).all()
