"""CPU-side tests of per-feature input scales (ARD): the rules of tests/_ard_rules.py against central differences of the
oracle's log-pdf, the variable registration, the refusals (raised before a context exists), the array-valued training helpers and
the checkpoint round trip.  No device call anywhere in this file."""
import itertools
import os
import re

import numpy as np
import pytest

import _ard_rules as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 24, 7


def _mlp(w, b, l):
    from smnngp import nt_kernels
    return nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l)


def _cnn(w, b, l):
    from smnngp import nt_kernels
    return nt_kernels.get_cnn_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l)


# ----------------------------------------------------------------------------- the rules against the oracle
@pytest.mark.parametrize("kind,get,act,method", list(itertools.product(("mlp", "resnet"), ("nngp", "ntk"), ("relu", "erf"), ("gp", "tp"))))
def test_rules_match_central_differences_of_the_oracle_logpdf(kind, get, act, method):
    """feat / s against central differences in every scale (step 1e-6 s_j) and one row of gx against central differences in that
    row of x~: <= 1e-6 relative to the largest component (measured: up to 1.4e-8)."""
    rng = np.random.default_rng(5)
    x, s = rng.standard_normal((N, D)), np.exp(0.5 * rng.standard_normal(D))
    y = rng.standard_normal((N, 3 if method == "tp" else 1))
    kw = dict(eps=1e-3, method=method, a=1.7, b=2.4, num_hiddens=2, act=act, w_std=1.3, b_std=0.4, last_w_std=0.9)
    gx, feat = A.lml_input_grad(kind, x * s, y, get, **kw)
    fd = A.loss_scale_grad_fd(kind, x, s, y, get, **kw)
    got = -(feat / s) / N
    err = np.abs(got - fd).max() / np.abs(fd).max()
    xs, row = x * s, 3
    fdx = np.empty(D)
    for j in range(D):
        up, dn = xs.copy(), xs.copy()
        up[row, j] += 1e-6
        dn[row, j] -= 1e-6
        fdx[j] = (A.logpdf(kind, up, y, get, **kw) - A.logpdf(kind, dn, y, get, **kw)) / 2e-6
    errx = np.abs(gx[row] - fdx).max() / np.abs(fdx).max()
    print("%s %s %s %s: feat/s %.3g, gx row %.3g" % (kind, get, act, method, err, errx))
    assert err <= 1e-6 and errx <= 1e-6


def test_float32_rules_stay_in_float32():
    rng = np.random.default_rng(6)
    x, y = rng.standard_normal((9, 4)), rng.standard_normal(9)
    gx, feat = A.lml_input_grad("mlp", x, y, "ntk", eps=1e-2, method="tp", a=1.7, b=2.4, dtype=np.float32, num_hiddens=1, act="erf",
                                w_std=1.3, b_std=0.4, last_w_std=0.9)
    assert gx.dtype == np.float32 and feat.dtype == np.float32 and gx.shape == (9, 4) and feat.shape == (4,)


# ----------------------------------------------------------------------------- variable registration
@pytest.mark.parametrize("cls", ["NNGPKernel", "NTKKernel"])
def test_input_scales_register_exactly_one_more_variable(cls):
    from smnngp.spax import kernels
    from smnngp.spax.base import ConstraintTrainVar
    K = getattr(kernels, cls)
    plain, scaled = K(_mlp, 1.3, 0.4, 0.9), K(_mlp, 1.3, 0.4, 0.9, input_scales=[0.5, 1.0, 2.0])
    names = ["(%s).%s" % (cls, k) for k in ("w_std", "b_std", "last_w_std")]
    assert list(plain.vars()) == names and plain.get_input_scales() is None
    assert not hasattr(plain, "input_scales") and plain.get_kernel_fn().input_scales is None
    assert set(scaled.vars()) - set(plain.vars()) == {"(%s).input_scales" % cls} and len(scaled.vars()) == 4
    var = scaled.input_scales
    assert isinstance(var, ConstraintTrainVar) and var.value.shape == (3,)
    assert np.allclose(scaled.get_input_scales(), [0.5, 1.0, 2.0], rtol=1e-12)
    fn = scaled.get_kernel_fn()
    assert np.allclose(fn.input_scales, [0.5, 1.0, 2.0], rtol=1e-12) and fn.cov == ("ntk" if cls == "NTKKernel" else "nngp")
    assert np.array_equal(fn.with_cov("ntk").input_scales, fn.input_scales)          # with_cov preserves the scales
    assert fn.params == plain.get_kernel_fn().params                                 # params is unchanged
    assert fn.with_input_scales(None).input_scales is None
    var.assign(var.constraint.inverse(np.array([3.0, 4.0, 5.0])))                    # the current values ride on the kernel function
    assert np.allclose(scaled.get_kernel_fn().input_scales, [3.0, 4.0, 5.0], rtol=1e-12)


# ----------------------------------------------------------------------------- refusals, before a context exists
class _NoDevice:
    """A context that fails the test on any device call."""

    handle = None

    def __getattr__(self, name):
        raise AssertionError("device call %r before the refusal" % name)


class _FakeX:
    shape, dtype, ctx = (6, 3), np.dtype(np.float64), _NoDevice()


def _bare(cls, kernel):
    from smnngp.spax.likelihoods import GaussianLikelihood
    model = object.__new__(cls)
    model.kernel, model.likelihood, model.x_data, model.num_data = kernel, GaussianLikelihood(), _FakeX(), 6
    return model


def test_refusals_come_before_any_device_call():
    from smnngp import nt_kernels, sweeps, train
    from smnngp.spax.kernels import NNGPKernel, NTKKernel
    from smnngp.spax.likelihoods import GaussianLikelihood
    from smnngp.spax.models import SPR, SVSP, MultiSPR
    for bad in ([], [1.0, -1.0], [1.0, np.nan], [0.0]):
        with pytest.raises(ValueError, match="input_scales"):
            NNGPKernel(_mlp, input_scales=bad)
    with pytest.raises(ValueError, match="input_scales"):
        nt_kernels.get_mlp_kernel(1).with_input_scales([1.0, 0.0])
    for K in (NNGPKernel, NTKKernel):                      # a conv kernel or a foreign callable under scales
        with pytest.raises(NotImplementedError):
            K(_cnn, input_scales=[1.0, 1.0]).get_kernel_fn()
        with pytest.raises(NotImplementedError, match="input_scales"):
            K(lambda w, b, l: (lambda x1, x2=None, get="nngp": None), input_scales=[1.0, 1.0]).get_kernel_fn()
    for cls in (SPR, MultiSPR):                            # a length other than d, when the model is built
        with pytest.raises(ValueError, match="input_scales has 2 entries"):
            cls(NNGPKernel(_mlp, input_scales=[1.0, 1.0]), GaussianLikelihood(), np.zeros((6, 3)), np.zeros(6), 0.0, 1.0)
        with pytest.raises(NotImplementedError, match="input scales"):
            _bare(cls, NNGPKernel(_mlp, input_scales=[1.0, 1.0, 1.0])).loo_loss_and_grad()
    with pytest.raises(NotImplementedError, match="input scales"):
        train.build_multistart_step(_bare(SPR, NNGPKernel(_mlp, input_scales=[1.0, 1.0, 1.0])), {})
    x = _FakeX()
    common = dict(w_std=1.0, b_std=0.1, input_scales=[1.0, 1.0, 1.0])
    with pytest.raises(NotImplementedError, match="input scales"):
        sweeps.loss_batch(_NoDevice(), x, x, eps=1e-3, **common)
    with pytest.raises(NotImplementedError, match="input scales"):
        sweeps.loss_and_grad_batch(_NoDevice(), x, x, eps=1e-3, **common)
    with pytest.raises(NotImplementedError, match="input scales"):
        sweeps.predict_batch(_NoDevice(), x, x, x, diag_reg=1e-3, **common)
    with pytest.raises(NotImplementedError, match="input scales"):
        sweeps.find_grid(None, None, None, None, input_scales=[1.0])
    svsp = SVSP(None, NNGPKernel(_cnn, input_scales=[1.0, 1.0]), np.zeros((2, 4, 4, 1)))
    with pytest.raises(NotImplementedError):
        svsp.loss_and_grad(0, np.zeros((2, 4, 4, 1)), np.zeros(2), 10, 4)
    with pytest.raises(NotImplementedError):
        svsp.inducing_state(ctx=_NoDevice())
    fn = nt_kernels.get_mlp_kernel(1).with_input_scales([1.0, 2.0])
    with pytest.raises(NotImplementedError, match="needs x2"):                  # KernelFn.input_grad keeps its refusal
        fn.input_grad(np.zeros((2, 2)), None, np.zeros((2, 2)))


def test_the_new_entries_are_bound_with_the_header_arity():
    from smnngp import _lib
    text = open(os.path.join(ROOT, "include", "smnngp.h")).read()
    for name, arity in (("smn_scale_columns", 9), ("smn_kernel_mlp_input_grad_sym", 20), ("smn_spr_loss_grad_inputs", 25)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
        assert m, "%s is not declared in include/smnngp.h" % name
        assert len(m.group(1).split(",")) == arity == len(_lib.PROTOTYPES[name]), name


# ----------------------------------------------------------------------------- training helpers
def test_adam_moves_a_scalar_beside_a_vector_exactly_as_alone():
    from smnngp.spax.base import TrainVar
    from smnngp.train import Adam
    rng = np.random.default_rng(2)
    a1, a2, v = TrainVar(0.3), TrainVar(0.3), TrainVar(np.array([0.1, -0.2, 0.4]))
    alone, mixed = Adam({"a": a1}), Adam({"a": a2, "v": v})
    for it in range(25):
        g = float(np.sin(0.7 * it) + 0.3)
        gv = rng.standard_normal(3)
        if it == 7:
            gv[1] = np.nan                                   # a component without a finite gradient is left alone
        before = np.array(v.value)
        alone(0.05, {"a": g})
        mixed(0.05, {"a": g, "v": gv})
        assert float(a1.value) == float(a2.value)            # bit-identical trajectory
        assert np.all((v.value != before) == np.isfinite(gv))
    # one vector component against Adam's scalar arithmetic on the same gradients
    s, w = TrainVar(0.5), TrainVar(np.array([0.5, 9.0]))
    one, vec = Adam({"s": s}), Adam({"w": w})
    for it in range(10):
        g = float(np.cos(it))
        one(0.1, {"s": g})
        vec(0.1, {"w": np.array([g, -g])})
        assert float(s.value) == float(w.value[0])


def test_value_and_grad_fd_differentiates_a_vector_variable_component_by_component():
    from smnngp.spax.base import TrainVar
    from smnngp.train import value_and_grad_fd
    q = np.array([[2.0, 0.5, 0.0], [0.5, 1.0, -0.3], [0.0, -0.3, 3.0]])
    v, a = TrainVar(np.array([0.4, -1.2, 2.5])), TrainVar(0.7)
    calls = []

    def loss():
        calls.append(1)
        x = np.asarray(v.value)
        return 0.5 * x @ q @ x + float(a.value) ** 2
    value, grads = value_and_grad_fd(loss, {"v": v, "a": a})
    x0 = np.array([0.4, -1.2, 2.5])
    assert abs(value - (0.5 * x0 @ q @ x0 + 0.49)) < 1e-14 and len(calls) == 1 + 2 * 3 + 2
    assert np.allclose(grads["v"], q @ x0, rtol=1e-9, atol=1e-9)                   # exact for a quadratic, up to rounding
    assert abs(grads["a"] - 1.4) < 1e-9 and isinstance(grads["a"], float)
    assert np.array_equal(v.value, x0) and float(a.value) == 0.7                   # the variables are put back


# ----------------------------------------------------------------------------- checkpoint
def test_checkpoint_round_trips_the_vector_variable(tmp_path):
    from smnngp import checkpoint
    from smnngp.spax.kernels import NNGPKernel
    kernel = NNGPKernel(_mlp, 1.3, 0.4, 0.9, input_scales=[0.5, 1.5, 2.5, 0.25])
    path = str(tmp_path / "vars.npz")
    checkpoint.save_var_collection(path, kernel.vars())
    saved = checkpoint.load_var_collection(path)
    got = checkpoint.get_from_vars(saved, "input_scales")
    assert got.shape == (4,) and np.array_equal(got, kernel.input_scales.value)
    assert np.array_equal(checkpoint.get_from_vars(saved, "w_std"), kernel.w_std.value)
    other = NNGPKernel(_mlp, input_scales=np.ones(4))
    other.input_scales.assign(got)
    assert np.array_equal(other.get_input_scales(), kernel.get_input_scales())
    plain = NNGPKernel(_mlp, 1.3, 0.4, 0.9)                                        # without scales: the file is what it was
    checkpoint.save_var_collection(path, plain.vars())
    saved = checkpoint.load_var_collection(path)
    assert checkpoint.get_from_vars(saved, "input_scales") is None and len(saved["names"]) == 3
