"""CPU-side checks of the exact C-output model (MultiSPR): the NumPy rules of tests/_multi_rules.py pin themselves against
SciPy's multivariate densities and against their own central differences, the C ABI declares and binds the six *_multi
entries, the classification targets are what the issue states, and every case the GPU tests use factors in fp64."""
import os
import re

import numpy as np
import pytest
from scipy import stats

import _multi_rules as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI_SYMBOLS = ("smn_lml_multi", "smn_spr_loss_multi", "smn_lml_grad_terms_multi", "smn_kernel_cnn_grad_terms_multi",
                 "smn_spr_loss_grad_multi", "smn_spr_cnn_loss_grad_multi")
HYP = dict(M.HYP, eps=5e-2)


def small(family, seed=3, n=12, c=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 5)) if family in ("mlp", "resnet") else rng.standard_normal((n, 4, 5, 2))
    return x, rng.standard_normal((n, c))


# ------------------------------------------------------------------------------------------- the rules pin themselves
@pytest.mark.parametrize("family", ["mlp", "cnn"])
def test_closed_forms_equal_scipy_on_the_kronecker_covariance(family):
    """N = 12, C = 3: the Gaussian / Student-t closed forms equal multivariate_normal / multivariate_t.logpdf of vec(Y)
    under I_C x K~ to 1e-12."""
    x, y = small(family)
    n, c = y.shape
    kt = M.kernel(family, x, None, 2, "relu", 1.3, 0.4, 0.9) + 5e-2 * np.eye(n)
    big = np.kron(np.eye(c), kt)
    vec = y.T.reshape(-1)                                   # column after column: the blocks of I_C x K~
    lp = M.head(kt, y, "gp", 0, 0)[0]
    ref = stats.multivariate_normal(np.zeros(n * c), big).logpdf(vec)
    ref_sum = sum(stats.multivariate_normal(np.zeros(n), kt).logpdf(y[:, k]) for k in range(c))
    assert abs(lp - ref) < 1e-12 * max(1.0, abs(ref)) and abs(lp - ref_sum) < 1e-12 * max(1.0, abs(ref))
    a, b = 1.7, 2.4
    lp = M.head(kt, y, "tp", a, b)[0]
    ref = stats.multivariate_t(np.zeros(n * c), (b / a) * big, df=2 * a).logpdf(vec)
    assert abs(lp - ref) < 1e-12 * max(1.0, abs(ref))
    # and the joint Student-t is NOT the sum of C independent ones
    ind = sum(stats.multivariate_t(np.zeros(n), (b / a) * kt, df=2 * a).logpdf(y[:, k]) for k in range(c))
    assert abs(lp - ind) > 1e-3


@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("family,act", [("mlp", "relu"), ("mlp", "erf"), ("resnet", "relu"), ("resnet", "erf"),
                                        ("cnn", "relu"), ("cnn", "erf")])
def test_analytic_gradient_equals_central_differences_of_the_rules(family, act, method):
    """N = 12, C = 3: 1/2 sum G dK~/d theta with G = coef A A^T - C K~^-1 and the closed-form (a, b) part against central
    differences of the rules' own loss (2e-6 of the largest gradient: the project's gradient tolerance in fp64)."""
    x, y = small(family, seed=5)
    keys = M.KEYS if method == "tp" else M.KEYS[:4]
    val, grad = M.loss_grad(family, x, y, 2, act, method, **HYP)
    assert abs(val - M.loss(family, x, y, 2, act, method, **HYP)) < 1e-12 * max(1.0, abs(val))
    fd = M.loss_fd(family, x, y, 2, act, method, keys, **HYP)
    scale = max(abs(v) for v in fd.values())
    assert set(grad) == set(keys)
    for k in keys:
        assert abs(grad[k] - fd[k]) < 2e-6 * max(scale, abs(fd[k])), (k, grad[k], fd[k])


def test_tangent_kernels_equal_the_oracle_kernels():
    for family, act in (("mlp", "relu"), ("mlp", "erf"), ("resnet", "relu"), ("resnet", "erf")):
        x, _ = small(family, seed=7)
        k = M.dense_tangents(family, x, 2, act, 1.3, 0.4, 0.9)[0]
        ref = M.kernel(family, x, None, 2, act, 1.3, 0.4, 0.9)
        assert np.max(np.abs(k - ref)) < 1e-13 * np.max(np.abs(ref))


def test_one_column_is_the_single_output_loss():
    from oracle import nngp_oracle as O
    x, y = small("mlp", c=1)
    kw = dict(num_hiddens=2, act="erf", w_std=1.3, b_std=0.4, last_w_std=0.9, eps=5e-2, alpha=1.7, beta=2.4)
    for method in ("gp", "tp"):
        ref = O.spr_loss(x, y[:, 0], method=method, **kw)
        assert abs(M.loss("mlp", x, y, 2, "erf", method, **HYP) - ref) < 1e-12 * max(1.0, abs(ref))


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_the_binding_binds_the_multi_entries():
    import ctypes

    import __graft_entry__ as g
    g.build()
    from smnngp import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smnngp.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in MULTI_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, "include/smnngp.h does not declare %s" % name
        assert name in _lib.PROTOTYPES, "_lib does not bind %s" % name
        assert len(m.group(1).split(",")) == len(_lib.PROTOTYPES[name]), name
        assert hasattr(raw, name), "libsmnngp.so does not export %s" % name
    from smnngp.spax import models
    assert hasattr(models, "MultiSPR") and models.multi_grad_route is not None


def test_from_labels_targets():
    """onehot(labels) - 1/C: row sums are zero and the arg-max returns the labels."""
    import __graft_entry__ as g
    g.build()
    from smnngp.spax.models import MultiSPR
    rng = np.random.default_rng(0)
    for c in (2, 3, 10, 48):
        labels = rng.integers(0, c, size=57)
        y = MultiSPR.label_targets(labels, c)
        assert y.shape == (57, c) and np.max(np.abs(y.sum(axis=1))) < 1e-15
        assert np.array_equal(np.argmax(y, axis=1), labels)
        assert np.array_equal(y, M.label_targets(labels, c))
    with pytest.raises(ValueError):
        MultiSPR.label_targets([0, 3], 3)


# ---------------------------------------------------------------------------------- the GPU tests' cases, on the CPU
def gpu_cases():
    for n, c in M.DENSE_NC:
        for family, act in M.DENSE_NETS:
            yield family, ("dense", n, c), M.DENSE_LAYERS, act
    for h, w, ch in M.CONV_IMAGES:
        for n, c in M.CONV_NC:
            for act in ("relu", "erf"):
                yield "cnn", ("conv", n, c, h, w, ch), M.CONV_LAYERS, act
    yield "conv_resnet", ("conv", 12, 3, 8, 8, 1), 1, "relu"


def test_the_fp64_rules_factor_every_gpu_case():
    """Both the fp64 data and the fp32-rounded data (eps = 1e-3) of every shape the GPU tests use give a finite loss under
    both heads (head() factors K~ with numpy's Cholesky, which raises when it is not positive definite)."""
    for family, key, layers, act in gpu_cases():
        for f32 in (False, True):
            for method in ("gp", "tp"):
                assert np.isfinite(M.ref_loss(family, key + (f32,), layers, act, method)), (family, key, act, f32, method)


def test_classification_cases_have_a_margin_fp32_cannot_flip():
    """The issue asks for a top-two margin above 1e-6; the fp32 posterior mean is held to 1e-2 of max |mean| norm-wise, so the
    arg-max is safe only above twice that: the cases are chosen to have it."""
    for family, act, layers, key in M.PRED_CASES:
        for f32 in (False, True):
            ref = M.ref_prediction(family, act, layers, key, f32)
            assert ref["margin"] * float(np.max(np.abs(ref["mean"]))) > 1e-6
            assert ref["margin"] > 2e-2, (family, key, f32, ref["margin"])
            assert np.isfinite(ref["nll_gp"]) and np.isfinite(ref["nll_tp"]) and np.all(ref["var"] > 0)
