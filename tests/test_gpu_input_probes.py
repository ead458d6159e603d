"""The input-gradient kernels held PAIR BY PAIR to a long-double reference: ig_tile_kernel, ig_seed_kernel, ig_rowsum_kernel and
ig_contract_kernel (csrc/input_grad.hip) through smn_kernel_mlp_input_grad, igs_pass_kernel and igs_rowsum_kernel
(csrc/input_grad_sym.hip) through smn_kernel_mlp_input_grad_sym, the chain of csrc/input_tangent.hpp in both, in f32 and f64, MLP
and dense ResNet, ReLU and erf, NNGP and NTK.

How a call reads single pairs, the exact inputs, the seeds, the reference, the yardstick Y and the acceptance rule
    |device - ref| <= 16 max(Y, 4 u_T) s_e  per component of every probed row,  rows without a seed entry exactly 0,
    16 max(Y, 4 u_T) <= the kernel tolerance of the dtype
are in tests/_input_probe_rules.py, checked on the host by test_input_probe_host.py (which also holds the Y cap of every case
below).  coef = 0, alpha = 0, c = 1 for the symmetric entry, the strict upper triangle of its seed NaN; operands in the guarded
windows of tests/_windows.py, device buffers reused across the calls of a case.

  A  smn_kernel_mlp_input_grad, every pair: n1 = n2 = 130 (one full and one 2-wide ragged 128-tile on both sides: every (wave,
     m, i, n) slot of the tile kernel, the 16-lane row sums), 130 shifted one-per-row seeds, the 16 forms, two hidden layers.  The
     f64 NTK forms take the unfused route (plain form + ig_seed_kernel).  n1 in {1, 5} x n2 = 257 (three tile columns) on a
     selection of shifts.
  B  smn_kernel_mlp_input_grad_sym, every pair: n = 130 (three 64-row tile rows, the last 2 wide: diagonal tiles with the
     tile + mirror store, off-diagonal tiles with both stores, row-side slots 0..t and column-side slots t+1..T), 129 matching
     rounds and the diagonal seed, the 16 forms; feat_h against the device's own gx; n = 1, 64, 65.
  C  singular and near-singular pairs on both entries: on-grid near-duplicates x_j = x_r + 2^-k e_0 at the smallest gaps whose
     yardstick stays within the kernel tolerance (same 64-tile, another tile, the ragged tile), anti-parallel rows, exactly
     duplicate rows off the diagonal, an all-zero row, rows scaled by 2^-6 .. 2^6; b_std = 0 and b_std > 0; each its own case
     and Y.  The NTK forms are held to the guarded rules; pairs ON a ReLU guard (duplicates; anti-parallel rows under b_std = 0)
     get _input_probe_rules.singular_allowance on top, which is derived, not measured.
  D  one dense random seed per entry at n2 = 257 / n = 257: every component within 16 max(Y, 4u) sum_j |G_rj| s_e(r, j); two calls
     give the same bits.
  E  depths 0, 1, 3 (the ResNet takes zero, one and several residual steps) on a selection of seeds.
  F  d = 7, where 1 / d rounds (the yardstick includes that rounding of u).
Every case prints its Y / u, its largest error / (max(Y, 4u) s) and the use of a derived allowance (run with -s); the table of
the run on an MI355X is profiles/r33_input_probes.txt."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _input_probe_rules as P
from _windows import in_window, out_window

pytestmark = pytest.mark.gpu

LD = np.longdouble
DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
FORM_IDS = ["%s-%s-%s" % f for f in P.FORMS]
NETS = {"mlp": 0, "resnet": 1}


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


# ---------------------------------------------------------------------------------------------------------- the cases
class Spec:
    """One case: the form, the inputs, the seeds of its calls."""

    def __init__(self, tag, sym, kind, act, get, layers, b_std, x1, x2, seeds, T):
        self.tag, self.sym, self.form, self.layers, self.b_std = tag, sym, (kind, act, get), layers, b_std
        self.x1, self.x2, self.seeds, self.T = x1, x2, seeds, T

    @functools.lru_cache(maxsize=None)
    def reference(self):
        return P.reference(*self.form, self.layers, self.b_std, self.x1, self.x2, self.seeds, self.T, self.sym)


def _tn(T):
    return np.dtype(T).name


SHIFTS_257 = (0, 1, 126, 127, 128, 129, 255, 256)


def cases_a(form, T):
    x1, x2 = P.stored_rows("a1"), P.stored_rows("a2")
    out = [Spec("A asym130 %s-%s-%s %s" % (form + (_tn(T),)), False, *form, 2, P.B, x1, x2[:130], P.shift_seeds(130, 130), T)]
    for n1 in (1, 5):
        out.append(Spec("A asym%dx257 %s-%s-%s %s" % ((n1,) + form + (_tn(T),)), False, *form, 2, P.B, x1[:n1], x2,
                        P.shift_seeds(n1, 257, SHIFTS_257), T))
    return out


def cases_b(form, T):
    x = P.stored_rows("s")[:130]
    return [Spec("B sym130 %s-%s-%s %s" % (form + (_tn(T),)), True, *form, 2, P.B, x, x, P.matching_seeds(130), T)]


SMALL_B = [(1, ("mlp", "relu", "ntk")), (64, ("resnet", "erf", "ntk")), (65, ("mlp", "relu", "ntk")), (65, ("resnet", "erf", "nngp"))]


def cases_b_small(n, form, T):
    x = P.stored_rows("s")[:n]
    return [Spec("B sym%d %s-%s-%s %s" % ((n,) + form + (_tn(T),)), True, *form, 2, P.B, x, x, P.matching_seeds(n), T)]


def cases_c(sym, form, b_std, T):
    x, cases = P.hard_inputs(T)
    out = []
    for name, pairs in cases.items():
        both = pairs if sym else pairs + [(j, r) for r, j in pairs]
        out.append(Spec("C %s %s %s-%s-%s b%g %s" % (("sym" if sym else "asym", name) + form + (b_std, _tn(T))), sym, *form, 2, b_std,
                        x, x, P.pack_pairs(both, sym), T))
    return out


DENSE_FORMS = [("mlp", "relu", "ntk"), ("resnet", "erf", "nngp"), ("resnet", "relu", "ntk"), ("mlp", "erf", "ntk")]
DEPTHS = [("mlp", "relu", "ntk", 0), ("mlp", "erf", "nngp", 1), ("mlp", "relu", "ntk", 3), ("resnet", "erf", "ntk", 0),
          ("resnet", "relu", "ntk", 1), ("resnet", "relu", "nngp", 3), ("resnet", "erf", "ntk", 3)]
DEPTH_SHIFTS = (0, 5, 64, 129)
DEPTH_ROUNDS = (0, 1, 64, 128, 129)                                   # 129: the diagonal seed


def cases_e(sym, kind, act, get, layers, T):
    tag = "E %s %s-%s-%s L%d %s" % ("sym" if sym else "asym", kind, act, get, layers, _tn(T))
    if sym:
        x = P.stored_rows("s")[:130]
        seeds = P.matching_seeds(130)
        return [Spec(tag, True, kind, act, get, layers, P.B, x, x, [seeds[t] for t in DEPTH_ROUNDS], T)]
    return [Spec(tag, False, kind, act, get, layers, P.B, P.stored_rows("a1"), P.stored_rows("a2")[:130],
                 P.shift_seeds(130, 130, DEPTH_SHIFTS), T)]


D7_FORMS = [("resnet", "relu", "ntk"), ("mlp", "erf", "nngp")]


def cases_f(sym, form, T):
    tag = "F %s d7 %s-%s-%s %s" % (("sym" if sym else "asym",) + form + (_tn(T),))
    if sym:
        x = P.stored_rows("fs")
        return [Spec(tag, True, *form, 2, P.B, x, x, P.matching_seeds(len(x)), T)]
    x1, x2 = P.stored_rows("f1"), P.stored_rows("f2")
    return [Spec(tag, False, *form, 2, P.B, x1, x2, P.shift_seeds(len(x1), len(x2)), T)]


@functools.lru_cache(maxsize=None)
def dense_case(sym, form, T):
    """(x1, x2, seed, ref [n1, d], bound scale [n1, d], Y)."""
    x1, x2 = (P.stored_rows("s"),) * 2 if sym else (P.stored_rows("a1"), P.stored_rows("a2"))
    g = P.dense_seed(len(x1), len(x2), T, sym)
    return (x1, x2, g) + P.dense_reference(*form, 2, P.B, x1, x2, g, T, sym)


def all_cases(T):
    """(tag, build) of every case of this file for the dtype: build() gives the reference (an object with .y, or for the dense
    seeds a tuple ending in Y).  What test_input_probe_host.py holds the Y caps of."""
    specs = []
    for form in P.FORMS:
        specs += cases_a(form, T) + cases_b(form, T)
        for sym in (False, True):
            for b in (0.0, P.B):
                specs += cases_c(sym, form, b, T)
    for n, form in SMALL_B:
        specs += cases_b_small(n, form, T)
    for sym in (False, True):
        for dep in DEPTHS:
            specs += cases_e(sym, *dep, T)
        for form in D7_FORMS:
            specs += cases_f(sym, form, T)
    for s in specs:
        yield s.tag, s.reference
    for sym in (False, True):
        for form in DENSE_FORMS:
            yield "D %s %s-%s-%s" % (("sym" if sym else "asym",) + form), functools.partial(lambda a, b, c: dense_case(a, b, c)[3:], sym, form, T)


# ------------------------------------------------------------------------------------------------------- device calls
def _rewrite(ctx, w, data=None):
    """The window's allocation uploaded again (with new contents inside): the buffer itself is reused."""
    if data is not None:
        w.inside(w.host0)[...] = data
    ctx.call("smn_memcpy_h2d", w.dev.ptr, w.host0.ctypes.data_as(C.c_void_p), w.host0.nbytes)


class Entry:
    """The device buffers of one (entry, inputs, dtype): inputs uploaded once, the seed and the output window rewritten per call."""

    def __init__(self, L, ctx, sym, x1, x2, T, layout):
        self.L, self.ctx, self.sym, self.T = L, ctx, sym, T
        self.n1, self.d = x1.shape
        self.n2 = x2.shape[0]
        self.w1 = in_window(ctx, np.asarray(x1, T), layout)
        self.w2 = self.w1 if sym else in_window(ctx, np.asarray(x2, T), layout)
        self.wg = in_window(ctx, np.zeros((self.n1, self.n2), T), layout)
        self.wa = in_window(ctx, np.zeros((self.n1, 1), T), "block") if sym else None
        self.out = out_window(ctx, self.n1, self.d, T, layout)

    def call(self, form, layers, b_std, g, want_feat=False):
        """(gx [n1, d], feat [d] or None) under the seed matrix g (sym: its strict upper triangle NaN)."""
        L, ctx = self.L, self.ctx
        kind, act, get = form
        net = NETS[kind] | (L.NET_NTK if get == "ntk" else 0)
        _rewrite(ctx, self.wg, g)
        _rewrite(ctx, self.out)
        feat = np.full(self.d, 7.25)
        if self.sym:
            ctx.call("smn_kernel_mlp_input_grad_sym", L.dtype_code(self.T), net, L.ACT[act], layers, P.W, b_std, P.LW, self.w1.ptr,
                     self.n1, self.w1.ld, self.d, self.wg.ptr, self.wg.ld, self.wa.ptr, 1, 0.0, self.out.ptr, self.out.ld,
                     feat.ctypes.data_as(C.POINTER(C.c_double)) if want_feat else None)
        else:
            ctx.call("smn_kernel_mlp_input_grad", L.dtype_code(self.T), net, L.ACT[act], layers, P.W, b_std, P.LW, self.w1.ptr, self.n1,
                     self.w1.ld, self.w2.ptr, self.n2, self.w2.ld, self.d, self.wg.ptr, self.wg.ld, self.out.ptr, self.out.ld)
        return self.out.result("gx_d"), (feat if want_feat else None)


_ENTRIES = {}


def _entry(L, ctx, sym, key, x1, x2, T, layout="aligned"):
    k = (sym, key, T, layout)
    if k not in _ENTRIES:
        _ENTRIES[k] = Entry(L, ctx, sym, x1, x2, T, layout)
    return _ENTRIES[k]


def _run(L, ctx, spec, key, layout="aligned", feat=False):
    """gx [nseeds, n1, d] of the case's calls (and feat [nseeds, d])."""
    e = _entry(L, ctx, spec.sym, key, spec.x1, spec.x2, spec.T, layout)
    gx, ft = [], []
    for s in spec.seeds:
        a, b = e.call(spec.form, spec.layers, spec.b_std, P.dense_matrix(s, e.n1, e.n2, spec.T, spec.sym), feat)
        gx.append(a)
        ft.append(b)
    return np.stack(gx), (np.stack(ft) if feat else None)


def _hold(spec, gx):
    case = spec.reference()
    ratio, used = P.hold(case, gx, spec.tag)
    extra = "" if not case.extra.any() else "  allowance/s up to %.3g, used %.3g of it" % (
        float(np.where(case.s > 0, case.extra / np.where(case.s > 0, case.s, 1), 0).max()), used)
    print("\n[input-probe] %-52s calls %3d readings %5d  Y/u %8.1f  max err/(max(Y,4u) s) %6.3f%s" % (
        spec.tag, len(spec.seeds), len(case.rd.seed), case.y / P.U[spec.T], ratio, extra))
    return case


def _hold_feat(spec, gx, feat):
    """feat_h is the fp64 sum of the device's own gx o x over the rows: within n u_64 sum |terms|."""
    x = np.asarray(spec.x1, LD)
    terms = gx.astype(LD) * x[None, :, :]
    err = np.abs(feat.astype(LD) - terms.sum(1))
    assert (err <= len(x) * P.U[np.float64] * np.abs(terms).sum(1)).all(), spec.tag + ": feat_h"


# ------------------------------------------------------------------------------------------------------ A. asymmetric
def test_the_f64_ntk_forms_take_the_unfused_route():
    """input_grad_seeded_fused's rule, read from the source: the seeded f64 NTK forms are not built, so section A's f64 NTK cases
    run the plain form of ig_tile_kernel and ig_seed_kernel; every other form runs the seeded tile kernel and ig_rowsum_kernel."""
    from smnngp import _lib
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "input_grad.hip")).read()
    assert "bool input_grad_seeded_fused(int dtype, bool ntk) { return !(dtype == SMN_F64 && ntk); }" in src
    assert "if (fused) {\n    SMN_TRY(input_grad_factors(ctx, o, w, gbar_d, ldg));" in src
    assert "SMN_TRY(input_grad_seed(ctx, o, w, gp, o.rows2));" in src


@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
def test_a_every_pair_of_the_asymmetric_entry(L, ctx, form, T):
    layout = "unaligned" if form[0] == "resnet" else "aligned"
    for spec in cases_a(form, T):
        gx, _ = _run(L, ctx, spec, "a%d" % len(spec.x1) + "x%d" % len(spec.x2), layout)
        case = _hold(spec, gx)
        if len(spec.x1) == 130:                                       # the reading trick: between a P row and a Q row, to the bit
            rd = case.rd
            f1 = case.fac.f1[rd.fr, rd.fc]
            assert np.array_equal(case.ref[:, 6], rd.g * f1 / 8) and len(rd.seed) == 130 * 130


# ------------------------------------------------------------------------------------------------------- B. symmetric
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
def test_b_every_pair_of_the_symmetric_entry(L, ctx, form, T):
    layout = "unaligned" if form[0] == "resnet" else "aligned"
    (spec,) = cases_b(form, T)
    gx, feat = _run(L, ctx, spec, "s130", layout, feat=True)
    case = _hold(spec, gx)
    assert len(case.rd.seed) == 130 * 129 + 130
    _hold_feat(spec, gx, feat)


@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n,form", SMALL_B, ids=["n%d-%s-%s-%s" % ((n,) + f) for n, f in SMALL_B])
def test_b_small_sizes(L, ctx, n, form, T):
    (spec,) = cases_b_small(n, form, T)
    gx, feat = _run(L, ctx, spec, "s%d" % n, feat=True)
    _hold(spec, gx)
    _hold_feat(spec, gx, feat)


# ------------------------------------------------------------------------------------------ C. singular, near-singular
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("b_std", [0.0, P.B], ids=["b0", "b"])
@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
def test_c_singular_and_near_singular_pairs(L, ctx, sym, form, b_std, T):
    """The guard hits, counted from the reference, are exactly the constructed ones: ReLU duplicates at every activation,
    anti-parallel rows under b_std = 0 at the first; the zero row has zero variance under b_std = 0 alone."""
    for spec in cases_c(sym, form, b_std, T):
        gx, feat = _run(L, ctx, spec, "hard", feat=sym)
        case = _hold(spec, gx)
        name = spec.tag.split()[2]
        rd = case.rd
        off = rd.side != 2
        hits = (case.fac.hits != 0)[:, rd.fr[off], rd.fc[off]]
        relu = form[1] == "relu"
        if relu and name == "dup":
            assert hits.all() and case.extra.any()
        elif relu and name == "anti" and b_std == 0.0:
            assert hits[0].all() and not hits[1:].any()
        else:
            assert not hits.any() and not case.extra.any()
        zero = case.fac.zero1[rd.fr[off]] | case.fac.zero2[rd.fc[off]]
        assert zero.all() if (name == "zero" and b_std == 0.0) else not zero.any()
        if sym:
            _hold_feat(spec, gx, feat)


# -------------------------------------------------------------------------------------------------------- D. dense seeds
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", DENSE_FORMS, ids=["%s-%s-%s" % f for f in DENSE_FORMS])
@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
def test_d_dense_seeds(L, ctx, sym, form, T):
    x1, x2, g, ref, bound, y = dense_case(sym, form, T)
    e = _entry(L, ctx, sym, "dense", x1, x2, T)
    seed = np.array(g)
    if sym:
        seed[np.triu_indices(len(x1), 1)] = np.nan
    gx, feat = e.call(form, 2, P.B, seed, sym)
    yy = max(y, 4 * P.U[T])
    assert P.FACTOR * yy <= P.TOL[T]
    err = np.abs(gx.astype(LD) - ref)
    ratio = float((err / (LD(yy) * bound)).max())
    print("\n[input-probe] %-52s Y/u %8.1f  max err/(max(Y,4u) sum|G|s) %6.3f" % (
        "D %s dense257 %s-%s-%s %s" % (("sym" if sym else "asym",) + form + (_tn(T),)), y / P.U[T], ratio))
    assert (err <= P.FACTOR * LD(yy) * bound).all()
    gx2, feat2 = e.call(form, 2, P.B, seed, sym)
    assert np.array_equal(gx.view(np.uint8), gx2.view(np.uint8)), "two calls differ in bits"
    if sym:
        assert np.array_equal(feat, feat2)
        terms = gx.astype(LD) * np.asarray(x1, LD)
        assert (np.abs(feat.astype(LD) - terms.sum(0)) <= len(x1) * P.U[np.float64] * np.abs(terms).sum(0)).all()


# ------------------------------------------------------------------------------------------------- E. depths, F. d = 7
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind,act,get,layers", DEPTHS, ids=["%s-%s-%s-L%d" % d for d in DEPTHS])
@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
def test_e_depths(L, ctx, sym, kind, act, get, layers, T):
    (spec,) = cases_e(sym, kind, act, get, layers, T)
    gx, _ = _run(L, ctx, spec, "s130" if sym else "a130x130")
    _hold(spec, gx)


@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", D7_FORMS, ids=["%s-%s-%s" % f for f in D7_FORMS])
@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
def test_f_seven_features(L, ctx, sym, form, T):
    (spec,) = cases_f(sym, form, T)
    gx, feat = _run(L, ctx, spec, "d7", "unaligned", feat=sym)
    _hold(spec, gx)
    if sym:
        _hold_feat(spec, gx, feat)
