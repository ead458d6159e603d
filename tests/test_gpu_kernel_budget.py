"""The fused Gram + layer-recursion build beyond one tile, held to rounding-level per-entry budgets.

test_gpu_mp_golden.py holds the build to mpmath budgets on 8- and 16-row inputs (one partial tile, the plain K loop); every
multi-tile test elsewhere asserts relerr < 2e-3 (f32) / 1e-8 (f64) or bit-identity of one form against another.  Here every
dispatch form of launch_build_n / run_build_t (csrc/kernel_build.hip) and of mainloop (csrc/gemm_nt.hpp) is compared entry
by entry with the fixture's budget rule, evaluated by its NumPy port (tests/_kernel_budget.py, checked against the fixture and
against mpmath in test_kernel_budget_host.py):

    BM = 128 / plain K loop        fewer than 64 tiles, fewer than 8 K-steps (f32: d <= 224)
    BM = 128 / pipelined K loop    f32 from 8 K-steps on: d = 225 (the threshold), 257 (9 steps, odd), 3072
    BM = 64 half tiles             f32 launches of 64..600 tiles, grid padded to a multiple of 8 tiles
    the XCD tile map               from 512 tiles on: with BM = 64 (528 tiles) and with BM = 128 (630 tiles)
    FAST correlation-space maps    f32 MLP NNGP-only calls (every f32 `get="nngp"` MLP case below)
    f64                            the 128 x 128 tile on the plain loop, NTK at one workgroup per CU

Inputs are either Gaussian with d <= 64 (budget term d u) or small integers (tests/_kernel_budget.exact: the Gram sum is
exact in any order, so d = 3072 is as tight as d = 5); no two rows are closer than 1 - |c0| = 1e-3.  f32 results must lie
within the budget (plus the absolute allowance of asin_fast on the FAST erf path), f64 results within twice the u = 2^-53
budget: the fp64 port is itself rounded at that level (the host test bounds its error by 0.07 of that budget on a 40-digit
sample of the n = 1300, d = 257 inputs, for all four nets, so no f64 case is left out).
Each case prints its largest err / budget (run with -s); profiles/r19_kernel_budget.txt is that table."""
import functools

import numpy as np
import pytest

import _kernel_budget as KB

pytestmark = pytest.mark.gpu

NETS = (("mlp", "relu", 3), ("mlp", "erf", 6), ("resnet", "relu", 2), ("resnet", "erf", 1))
W, B, LW = 1.4, 0.3, 0.8
NET_IDS = ["%s-%s%d" % n for n in NETS]

# (id, dtype, input kind, n1, n2 or None for the symmetric build, d)
FORMS = [
    ("f32-bm128-plainloop-sym300-d40-gauss", "f32", "gauss", 300, None, 40),              # 6 tiles, 2 K-steps
    ("f32-bm128-plainloop-sym300-d40-exact", "f32", "exact", 300, None, 40),
    ("f32-bm128-plainloop-cross260x132-d33-exact", "f32", "exact", 260, 132, 33),         # 3 x 2 tiles
    ("f32-bm128-pipelined8-sym300-d225-exact", "f32", "exact", 300, None, 225),           # 8 K-steps: the threshold
    ("f32-bm128-pipelined9-sym300-d257-exact", "f32", "exact", 300, None, 257),           # 9: odd
    ("f32-bm128-pipelined96-sym300-d3072-exact", "f32", "exact", 300, None, 3072),
    ("f32-bm64-pad72-plainloop-sym1300-d40-gauss", "f32", "gauss", 1300, None, 40),       # 66 tiles -> 72
    ("f32-bm64-pad72-pipelined9-sym1300-d257-exact", "f32", "exact", 1300, None, 257),    # the headline configuration's forms
    ("f32-bm64-pipelined9-cross1025x900-d257-exact", "f32", "exact", 1025, 900, 257),     # 9 x 8 = 72 tiles
    ("f32-bm64-tilemap-sym4000-d64-exact", "f32", "exact", 4000, None, 64),               # 528 tiles, sampled
    ("f32-bm128-tilemap-sym4400-d64-exact", "f32", "exact", 4400, None, 64),              # 630 tiles > 600, sampled
    ("f64-plainloop-sym300-d257-exact", "f64", "exact", 300, None, 257),
    ("f64-plainloop-sym1300-d40-exact", "f64", "exact", 1300, None, 40),
    ("f64-tilemap-sym4000-d64-exact", "f64", "exact", 4000, None, 64),                    # sampled
]
# NNGP + NTK in one call (the generic maps; f64 NTK runs at one workgroup per CU): inputs shared with FORMS
JOINT = [
    ("f32-joint-bm128-sym300-d40-exact", "f32", "exact", 300, None, 40),
    ("f32-joint-bm64-sym1300-d257-exact", "f32", "exact", 1300, None, 257),
    ("f64-joint-sym300-d257-exact", "f64", "exact", 300, None, 257),
    ("f64-joint-sym1300-d40-exact", "f64", "exact", 1300, None, 40),
]


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def _kfn(net, act, layers):
    from smnngp import nt_kernels
    fac = nt_kernels.get_mlp_kernel if net == "mlp" else nt_kernels.get_dense_resnet_kernel
    return fac(layers, act=act, w_std=W, b_std=B, last_w_std=LW)


@functools.lru_cache(maxsize=None)
def _inputs(kind, t, n1, n2, d):
    """(x1, x2, d_terms): a cross case takes its two operands from ONE generated set, so the separation holds across them."""
    x = (KB.gauss if kind == "gauss" else KB.exact)(n1 + (n2 or 0), d, t)
    return x[:n1], (None if n2 is None else x[n1:]), (d if kind == "gauss" else 2)


@functools.lru_cache(maxsize=None)
def _entries(n1, n2, sym):
    i, j = KB.select_entries(n1, n2, sym)
    assert KB.tiles_covered(i, j, n1, n2, sym)
    return i, j


def _host_uncached(kind, t, n1, n2, d, net, act, layers):
    x1, x2, d_terms = _inputs(kind, t, n1, n2, d)
    i, j = _entries(n1, n2 or n1, n2 is None)
    ref, bud = KB.reference(net, act, layers, W, B, LW, x1, x2, i, j, d_terms, KB.U[t])
    return i, j, ref, bud


_host_cached = functools.lru_cache(maxsize=None)(_host_uncached)


def _host(kind, t, n1, n2, d, net, act, layers):
    """Entries, references and budgets of one case, computed once.  Kept only where a second test comes back for them (the
    inputs of JOINT): a full n = 1300 case holds 27 MB."""
    shared = (t, kind, n1, n2, d) in {c[1:] for c in JOINT}
    return (_host_cached if shared else _host_uncached)(kind, t, n1, n2, d, net, act, layers)


def _allow(t, bud_m, fast_erf_layers=0):
    """f32: the budget (plus asin_fast's absolute error over the layers of a FAST erf call); f64: twice the u = 2^-53 budget."""
    if t == "f64":
        return 2.0 * bud_m
    return bud_m + (KB.fast_erf_allowance(fast_erf_layers, W, LW) if fast_erf_layers else 0.0)


def _hold(tag, got, i, j, ref_m, allow, sym):
    g = np.asarray(got, np.float64)
    v = g[i, j]
    assert np.isfinite(v).all(), tag
    err = np.abs(v - ref_m)
    r = float(np.max(err / allow))
    at = int(np.argmax(err / allow))
    print("\n[budget] %-72s max err/budget %.3f  at (%d, %d)" % (tag, r, i[at], j[at]))
    assert (err <= allow).all(), (tag, r, int(i[at]), int(j[at]))
    if sym:
        assert np.isfinite(g).all(), tag
        assert np.array_equal(g, g.T), tag + ": not symmetric to the bit"
    return r


def _fast_erf_layers(t, net, act, layers):
    """The depth of a call that takes the FAST erf maps when it asks for the NNGP alone (f32, MLP), else 0."""
    return layers if t == "f32" and net == "mlp" and act == "erf" else 0


@pytest.mark.parametrize("net,act,layers", NETS, ids=NET_IDS)
@pytest.mark.parametrize("case", FORMS, ids=[c[0] for c in FORMS])
def test_nngp_build_within_budget(case, net, act, layers):
    """get="nngp": in f32 the FAST maps for the MLP, relu_j_fast / asin_abs for the ResNet; in f64 relu_j_f64 / asin_abs."""
    name, t, kind, n1, n2, d = case
    x1, x2, _ = _inputs(kind, t, n1, n2, d)
    i, j, ref, bud = _host(kind, t, n1, n2, d, net, act, layers)
    k = _kfn(net, act, layers)(x1, x2, get="nngp").numpy()
    assert k.dtype == KB.NPT[t] and k.shape == (n1, n2 or n1)
    _hold("%s %s-%s%d nngp-only" % (name, net, act, layers), k, i, j, ref[0],
          _allow(t, bud[0], _fast_erf_layers(t, net, act, layers)), n2 is None)


@pytest.mark.parametrize("net,act,layers", NETS, ids=NET_IDS)
@pytest.mark.parametrize("case", JOINT, ids=[c[0] for c in JOINT])
def test_joint_build_within_budget(case, net, act, layers):
    """get=("nngp", "ntk"): the generic maps (asin_abs, Kdot) in both dtypes."""
    name, t, kind, n1, n2, d = case
    x1, x2, _ = _inputs(kind, t, n1, n2, d)
    i, j, ref, bud = _host(kind, t, n1, n2, d, net, act, layers)
    both = _kfn(net, act, layers)(x1, x2, get=("nngp", "ntk"))
    for lbl, g, m in (("nngp", both.nngp, 0), ("ntk", both.ntk, 1)):
        _hold("%s %s-%s%d %s" % (name, net, act, layers, lbl), g.numpy(), i, j, ref[m], _allow(t, bud[m]), n2 is None)


# ----------------------------------------------------------------------------- row shards of the symmetric kernel
N_ROWS, D_ROWS = 1300, 257


def _rows_host(rb, re, cols, lower, net, act, layers):
    x, _, d_terms = _inputs("exact", "f32", N_ROWS, None, D_ROWS)
    i, j = np.divmod(np.arange((re - rb) * cols), cols)
    if lower:                     # the lower trapezoid: what the entry promises (tiles wholly above the diagonal are not written)
        keep = j <= rb + i
        i, j = i[keep], j[keep]
    ref, bud = KB.reference(net, act, layers, W, B, LW, x[rb:re], x[:cols], i, j, d_terms, KB.U["f32"], diag=(rb + i == j))
    return i, j, ref, bud


@pytest.mark.parametrize("net,act,layers", NETS, ids=NET_IDS)
@pytest.mark.parametrize("entry,rb,re", [("smn_kernel_mlp_rows", 301, 1001),          # off a tile boundary: the re-pad route;
                                         ("smn_kernel_mlp_lower_rows", 384, 1200)],   # 6 x 11 = 66 and 7 x 10 = 70 tiles: BM = 64
                         ids=["f32-bm64-rows301-1001-repad", "f32-bm64-lower-rows384-1200"])
def test_row_shards_within_budget(L, ctx, entry, rb, re, net, act, layers):
    """Only the entries the call writes, to the budgets of the full build (its diagonal entries are the closed-form ones)."""
    lower = entry.endswith("lower_rows")
    cols = re if lower else N_ROWS
    x, _, _ = _inputs("exact", "f32", N_ROWS, None, D_ROWS)
    i, j, ref, bud = _rows_host(rb, re, cols, lower, net, act, layers)
    xd = ctx.to_device(x)
    netc = L.NET_MLP if net == "mlp" else L.NET_DENSE_RESNET
    for mask, lbls in ((L.GET_NNGP, ("nngp-only",)), (L.GET_NNGP | L.GET_NTK, ("nngp", "ntk"))):
        ok = ctx.to_device(np.full((re - rb, cols), np.nan, np.float32))
        ot = ctx.to_device(np.full((re - rb, cols), np.nan, np.float32)) if mask & L.GET_NTK else None
        ctx.call(entry, L.F32, netc, L.ACT[act], layers, W, B, LW, xd.ptr, N_ROWS, D_ROWS, D_ROWS, rb, re, mask, ok.ptr,
                 None if ot is None else ot.ptr, cols)
        for lbl, o, m in zip(lbls, (ok, ot), (0, 1)):
            fast_erf = _fast_erf_layers("f32", net, act, layers) if lbl == "nngp-only" else 0
            _hold("%s[%d:%d] %s-%s%d %s" % (entry, rb, re, net, act, layers, lbl), o.numpy(), i, j, ref[m],
                  _allow("f32", bud[m], fast_erf), False)


# ----------------------------------------------------------------------------- the stand-alone recursion over a stored K0
N_REC, N_REC2, D_REC = 516, 388, 24    # 64 x 64 tiles: 9 tile rows (the last 4 rows wide), 7 tile columns in the cross form


def _rec_host(t, sym, net, act, layers):
    """K0 and q computed in fp64 and rounded ONCE to the dtype: the values the device receives are the reference's inputs,
    d_terms = 1 (the fixture's d = 1 rule)."""
    dt = KB.NPT[t]
    x = KB.gauss(N_REC + N_REC2, D_REC, "f64")
    x1, x2 = x[:N_REC], (x[:N_REC] if sym else x[N_REC:])
    k0 = (x1 @ x2.T / D_REC).astype(dt)
    q1, q2 = ((x1 * x1).sum(1) / D_REC).astype(dt), ((x2 * x2).sum(1) / D_REC).astype(dt)
    n2 = k0.shape[1]
    i, j = np.divmod(np.arange(N_REC * n2), n2)
    q1d, q2d = q1.astype(np.float64), q2.astype(np.float64)
    ref, bud = KB.entry_budget(net, act, layers, W, B, LW, k0.astype(np.float64)[i, j], q1d[i], q2d[j], 1, KB.U[t],
                               diag=(i == j) if sym else None)
    return k0, q1, q2, i, j, ref, bud


@pytest.mark.parametrize("net,act,layers", NETS, ids=NET_IDS)
@pytest.mark.parametrize("sym", [1, 0], ids=["sym516-lower-tiles-mirror", "cross516x388"])
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_recursion_within_budget(L, ctx, t, sym, net, act, layers):
    k0, q1, q2, i, j, ref, bud = _rec_host(t, bool(sym), net, act, layers)
    dt = KB.NPT[t]
    n2 = k0.shape[1]
    assert n2 % 4 == 0                      # (16-byte rows: the entry's contract)
    kd, qd1 = ctx.to_device(k0), ctx.to_device(q1)
    qd2 = qd1 if sym else ctx.to_device(q2)
    netc = L.NET_MLP if net == "mlp" else L.NET_DENSE_RESNET
    for mask, lbls in ((L.GET_NNGP, ("nngp-only",)), (L.GET_NNGP | L.GET_NTK, ("nngp", "ntk"))):
        ok = ctx.empty((N_REC, n2), dt)
        ot = ctx.empty((N_REC, n2), dt) if mask & L.GET_NTK else None
        ctx.call("smn_recursion", L.dtype_code(dt), netc, L.ACT[act], layers, W, B, LW, kd.ptr, N_REC, n2, n2, qd1.ptr, qd2.ptr,
                 sym, mask, ok.ptr, None if ot is None else ot.ptr, n2)
        for lbl, o, m in zip(lbls, (ok, ot), (0, 1)):
            fast_erf = _fast_erf_layers(t, net, act, layers) if lbl == "nngp-only" else 0
            _hold("smn_recursion %s %s %s-%s%d %s" % (t, "sym516" if sym else "cross516x388", net, act, layers, lbl), o.numpy(),
                  i, j, ref[m], _allow(t, bud[m], fast_erf), bool(sym))
