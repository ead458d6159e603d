"""The CPU oracle against the independent mpmath fixture (tests/golden/nngp_mp_golden.npz, tests/golden/make_mp_golden.py).

Every other numerical test compares the HIP path with oracle/nngp_oracle.py; this file checks the oracle itself against
references restated from the formulas at 40 digits, at the inputs where kernels and oracles go wrong (d = 1 rows,
duplicates, scaled and antiparallel rows, near-duplicates, zero rows, spread norms) and on a generic control set.
The per-entry budgets are the fixture's (computed in mp, see the generator's docstring)."""
import ast
import importlib.util
import os
import sys

import numpy as np
import pytest

from _tol import relerr
from oracle import nngp_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GEN = os.path.join(HERE, "golden", "make_mp_golden.py")
NPZ = os.path.join(HERE, "golden", "nngp_mp_golden.npz")
Z = np.load(NPZ)
SETS = [str(s) for s in Z["cmp_sets"]]
OFN = {"mlp": O.mlp_kernel, "resnet": O.dense_resnet_kernel}


def _gen():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_mp_golden", GEN)
    mod = importlib.util.module_from_spec(spec)
    keep, sys.dont_write_bytecode = sys.dont_write_bytecode, True   # no __pycache__ next to the fixture
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.dont_write_bytecode = keep
    return mod


def test_generator_imports_neither_the_oracle_nor_the_package():
    tree = ast.parse(open(GEN).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0, "relative import in the generator"
            names.add(node.module.split(".")[0])
        elif isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", "")) in (
                "__import__", "import_module", "spec_from_file_location"):
            raise AssertionError("dynamic import in the generator")
    assert names <= {"io", "os", "zipfile", "mpmath", "numpy"}, names
    src = open(GEN).read()
    assert "sys.path" not in src


def test_fixture_stays_small():
    assert os.path.getsize(NPZ) < 1024 * 1024


def test_regenerated_cases_are_bit_identical():
    g = _gen()
    m = g.map_case("f64", "relu")
    for k, v in m.items():
        assert np.array_equal(v, Z["map_relu_f64_" + k]) and v.dtype == Z["map_relu_f64_" + k].dtype, k
    fe = g.map_case("f32", "erf", fast_erf=True)
    assert np.array_equal(fe["k0"], Z["map_erf_f32_k0fast"]) and np.array_equal(fe["nngp"], Z["map_erf_f32_nngp"])
    res = g.composite_case("d1", "resnet", "erf", 3)
    for tag, (ref, bud) in res.items():
        key = "cmp_d1_resnet_erf_L3_%s" % tag
        assert np.array_equal(ref, Z[key + "_ref"])
        assert np.array_equal(bud["f64"], Z[key + "_bud64"])
        assert np.array_equal(bud["f32"].astype(np.float32), Z[key + "_bud32"])
    c = g.conv_case()
    assert np.array_equal(c["ref"], Z["conv_ref"]) and np.array_equal(c["x"], Z["conv_x"])


def test_fixture_inputs_are_what_the_device_receives():
    """f32 cases hold f32-representable values; the map tables are exact powers of two."""
    for name in SETS:
        dts = [str(t) for t in Z["cmp_%s_dtypes" % name]]
        for side in ("x1", "x2"):
            x = Z["cmp_%s_%s" % (name, side)]
            if "f32" in dts:
                assert np.array_equal(x.astype(np.float32).astype(np.float64), x), (name, side)
    for act in ("relu", "erf"):
        q1 = Z["map_%s_f64_q1" % act].astype(np.float64)
        r = 1.0 / np.sqrt(q1) if act == "relu" else 1.0 / np.sqrt(1.0 + 2.0 * q1)
        assert np.array_equal(np.log2(r), np.round(np.log2(r)))


# ----------------------------------------------------------------------------- the element maps (oracle's relu_map / erf_map)
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("t", ["f64", "f32"])
def test_oracle_element_maps(act, t):
    k0 = Z["map_%s_%s_k0" % (act, t)].astype(np.float64)
    q1 = Z["map_%s_%s_q1" % (act, t)].astype(np.float64)
    q2 = Z["map_%s_%s_q2" % (act, t)].astype(np.float64)
    kn, _, _, th = O.get_act(act)(k0, q1, q2, k0.copy())
    ref_k, ref_t = Z["map_%s_%s_nngp" % (act, t)], Z["map_%s_%s_ntk" % (act, t)]
    # NumPy's sqrt / arccos / arcsin in fp64 on an exact correlation: a few ulp of the row's scale
    scale = np.abs(ref_k).max(axis=1, keepdims=True)
    assert (np.abs(kn - ref_k) <= 8 * 2.0 ** -53 * (scale + np.abs(ref_k))).all()
    tscale = np.abs(ref_t).max(axis=1, keepdims=True)
    assert (np.abs(kn + th - ref_t) <= 8 * 2.0 ** -53 * (tscale + np.abs(ref_t))).all()


# ----------------------------------------------------------------------------- composite kernels
def _cases():
    out = []
    for name in SETS:
        for net in ("mlp", "resnet"):
            for act in ("relu", "erf"):
                for L in (1, 3, 6):
                    out.append((name, net, act, L))
    return out


@pytest.mark.parametrize("name,net,act,L", _cases())
def test_oracle_composite_kernels_against_mp(name, net, act, L):
    x1, x2 = Z["cmp_%s_x1" % name], Z["cmp_%s_x2" % name]
    w, b, lw = (float(v) for v in Z["cmp_%s_hyp" % name])
    for tag, xb in (("sym", None), ("cross", x2)):
        key = "cmp_%s_%s_%s_L%d_%s" % (name, net, act, L, tag)
        ref, bud = Z[key + "_ref"], Z[key + "_bud64"]
        with np.errstate(all="ignore"):
            k, t = OFN[net](x1, xb, L, act, w, b, lw, ("nngp", "ntk"))
        got = np.stack([k, t])
        assert np.isfinite(got).all()
        if name == "control":   # generic inputs: the oracle is fp64-accurate (the first 3 rows of x2 are rows of x1: edges)
            gen = slice(None) if xb is None else slice(3, None)
            assert relerr(got[0][:, gen], ref[0][:, gen]) < 1e-13, key
            assert relerr(got[1][:, gen], ref[1][:, gen]) < 1e-13, key
        err = np.abs(got - ref)
        assert (err <= bud).all(), (key, float((err / np.maximum(bud, 1e-300)).max()))


def test_oracle_conv_kernel_against_mp():
    L, w, b, lw = Z["conv_params"]
    x = Z["conv_x"].astype(np.float64)
    k = O.cnn_kernel(x, None, int(L), "relu", w, b, lw)
    assert (np.abs(k - Z["conv_ref"]) <= Z["conv_bud64"]).all()


# ----------------------------------------------------------------------------- heads (fp64 oracle on the fixture's exact matrices)
def test_oracle_lml_against_mp():
    y = Z["head_y"]
    for row in Z["head_lml"]:
        _, src, dt, eps, df, sc, lp, quad, logdet, kappa, bound = row
        k = (Z["head_k64"][:40, :40] if src == 0 else Z["head_kdup"])
        k = k.astype(np.float32 if dt == 32 else np.float64).astype(np.float64)
        n = k.shape[0]
        cov = k + eps * np.eye(n)
        got = O.mvn_logpdf(y[:n, 0], cov) if df <= 0 else O.mvt_logpdf(y[:n, 0], sc * cov, df)
        # the fp64 oracle is held to the f64 form of the bound (gamma = 4 (n + 1) 2^-53), whatever the input dtype
        b64 = bound if dt == 64 else bound * 2.0 ** -53 / 2.0 ** -24
        assert abs(got - lp) <= b64, (row, got)


def test_oracle_predict_and_test_nll_against_mp():
    k, y = Z["head_k64"], Z["head_y"]
    for eps in (1e-6, 1e-2):
        key = "head_pred_f64_eps%g" % eps
        _, kappa, bm, bc = Z[key + "_info"]
        mean, cov = O.predict(k[:40, :40], k[40:, :40], k[40:, 40:], y[:40], diag_reg=eps)
        assert np.abs(mean - Z[key + "_mean"]).max() <= bm
        assert np.abs(cov - Z[key + "_cov"]).max() <= bc
    x = Z["head_x"]
    net, act, L, w, b, lw = (str(v) for v in Z["head_net"])
    for eps in (1e-6, 1e-2):
        _, alpha, beta, nll, _, _, bound = Z["head_testnll_eps%g" % eps]
        got = O.spr_test_nll(x[:40], y[:40, 0], x[40:], y[40:, 0], kernel=net, num_hiddens=int(L), act=act,
                             w_std=float(w), b_std=float(b), last_w_std=float(lw), eps=eps, method="tp", alpha=alpha,
                             beta=beta)
        assert abs(got - nll) <= bound, (eps, got, nll, bound)
