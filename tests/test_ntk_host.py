"""CPU-side checks of the tangent-kernel GP (spax.kernels.NTKKernel, SMN_NET_NTK): the six-state forward-mode rules of
tests/_ntk_rules.py (what csrc/grad.hip's NTK form computes) against central differences of the oracle's Theta and of the
oracle-built log-marginal likelihood, the host logic of NTKKernel / KernelFn's covariance mode, and the flag's value in the
header and in _lib."""
import os
import re

import numpy as np
import pytest

import _ntk_rules as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, B, LW = 1.3, 0.4, 0.9


@pytest.mark.parametrize("family,act,layers", [("mlp", "relu", 2), ("mlp", "erf", 3), ("resnet", "relu", 2), ("resnet", "erf", 3),
                                               ("mlp", "relu", 1), ("resnet", "erf", 1), ("mlp", "erf", 0)])
def test_tangents_equal_central_differences_of_the_oracle_theta(family, act, layers):
    """n = 40, d = 6: Theta itself to 1e-12 of its largest entry, dTheta/d(w_std, b_std, last_w_std) against central
    differences (h = 1e-6) to 1e-7 of the largest entry of each.  The differences' own rounding error is u |Theta| / h =
    2e-10 of the largest entry, times the slope of acos towards c = 1, 1 / sqrt(1 - c^2), a few tens for random rows; the
    truncation error h^2 f''' / 6 is below that.  Measured: at most 4.3e-9."""
    rng = np.random.default_rng(17)
    x = rng.standard_normal((40, 6))
    th, dw, db, dl = N.tangents(family, x, layers, act, W, B, LW)
    ref = N.theta(family, x, None, layers, act, W, B, LW)
    assert np.max(np.abs(th - ref)) <= 1e-12 * np.max(np.abs(ref))
    h = 1e-6
    for got, (dw_, db_, dl_) in ((dw, (h, 0, 0)), (db, (0, h, 0)), (dl, (0, 0, h))):
        fd = (N.theta(family, x, None, layers, act, W + dw_, B + db_, LW + dl_)
              - N.theta(family, x, None, layers, act, W - dw_, B - db_, LW - dl_)) / (2 * h)
        err = np.max(np.abs(got - fd)) / max(np.max(np.abs(fd)), 1e-300)
        print(family, act, layers, "max |tangent - fd| / max |fd| = %.3g" % err)
        assert err <= 1e-7


@pytest.mark.parametrize("family,act,layers,method", [("mlp", "relu", 2, "tp"), ("resnet", "erf", 3, "gp"), ("mlp", "erf", 6, "tp"),
                                                      ("resnet", "relu", 1, "tp")])
def test_analytic_lml_gradient_equals_central_differences(family, act, layers, method):
    """The data of the GPU gradient test (n = 150, d = 6): the restated gradient against central differences (h = 1e-5) of the
    oracle-built loss, at the project's fp64 gradient tolerance, 2e-6 of max(scale, |ref|) -- the room the device result is
    given too.  Measured: within 1.5e-9."""
    x, y = N.reg_data(150)
    ref_loss, fd = N.ref_loss_and_fd(family, act, layers, method, 150)
    val, grads = N.loss_grad(family, x, y, layers, act, method, **N.HYP)
    assert abs(val - ref_loss) <= 1e-12 * max(1.0, abs(ref_loss))
    scale = max(abs(v) for v in fd.values())
    assert set(grads) == set(fd)
    for k, v in fd.items():
        print(family, act, layers, method, k, grads[k], v, abs(grads[k] - v) / max(scale, abs(v)))
        assert abs(grads[k] - v) <= 2e-6 * max(scale, abs(v)), (k, grads[k], v)


def test_duplicate_rows_keep_the_relu_tangent_finite():
    """x[7] = x[3] exactly, ReLU, mlp depth 2: c = 1 off the diagonal.  Every tangent is finite and the gradient stays within
    1e-3 of the scale of the central differences (the quotient of acos at c = 1 is the noisy side; measured 3.1e-5)."""
    x, y = N.reg_data(150, dup=True)
    for m in N.tangents("mlp", x, 2, "relu", W, B, LW):
        assert np.isfinite(m).all()
    _, fd = N.ref_loss_and_fd("mlp", "relu", 2, "tp", 150, True)
    val, grads = N.loss_grad("mlp", x, y, 2, "relu", "tp", **N.HYP)
    scale = max(abs(v) for v in fd.values())
    assert np.isfinite(val)
    for k, v in fd.items():
        assert np.isfinite(grads[k]) and abs(grads[k] - v) <= 1e-3 * scale, (k, grads[k], v)


def test_loo_gradient_rules_equal_central_differences():
    x, y = N.reg_data(60)
    hyp = dict(N.HYP)
    val, grads = N.loo_loss_grad("mlp", x, y, 2, "erf", "tp", **hyp)
    fd = N.loo_loss_fd("mlp", x, y, 2, "erf", "tp", N.KEYS, **hyp)
    assert abs(val - N.loo_loss("mlp", x, y, 2, "erf", "tp", **hyp)) <= 1e-12 * max(1.0, abs(val))
    scale = max(abs(v) for v in fd.values())
    for k, v in fd.items():
        assert abs(grads[k] - v) <= 2e-6 * max(scale, abs(v)), (k, grads[k], v)


# --------------------------------------------------------------------------------------------------------- host logic
def test_header_and_lib_agree_on_the_flag():
    from smnngp import _lib
    text = open(os.path.join(ROOT, "include", "smnngp.h")).read()
    m = re.search(r"SMN_NET_NTK\s*=\s*(0x[0-9a-fA-F]+|\d+)", text)
    assert m, "SMN_NET_NTK is not in include/smnngp.h"
    flag = int(m.group(1), 0)
    assert flag == _lib.NET_NTK
    assert flag & (_lib.NET_MLP | _lib.NET_DENSE_RESNET | 2) == 0          # clear of both nets and of the internal NET_NONE = 2
    assert bin(flag).count("1") == 1
    for entry in ("smn_spr_loss", "smn_spr_loss_multi", "smn_spr_predict", "smn_spr_loss_grad", "smn_spr_loss_grad_multi",
                  "smn_lml_grad_terms", "smn_lml_grad_terms_multi", "smn_spr_loo_grad"):
        block = text[text.index("SMN_NET_NTK, OR-ed"):text.index("enum { SMN_NET_NTK")]
        assert entry in block, entry


@pytest.mark.parametrize("factory,net", [("get_mlp_kernel", "NET_MLP"), ("get_dense_resnet_kernel", "NET_DENSE_RESNET")])
def test_ntk_kernel_carries_the_flag_in_params(factory, net):
    from smnngp import _lib, nt_kernels
    from smnngp.spax.kernels import NNGPKernel, NTKKernel
    make = lambda w, b, l: getattr(nt_kernels, factory)(3, 1, act="erf", w_std=w, b_std=b, last_w_std=l)   # noqa: E731
    ntk, nngp = NTKKernel(make, 1.3, 0.4, 0.9), NNGPKernel(make, 1.3, 0.4, 0.9)
    assert isinstance(ntk, NNGPKernel)
    assert set(k.replace("NTKKernel", "NNGPKernel") for k in ntk.vars()) == set(nngp.vars())
    assert ntk.get_params() == nngp.get_params()
    f_ntk, f_nngp = ntk.get_kernel_fn(), nngp.get_kernel_fn()
    assert f_ntk.cov == "ntk" and f_nngp.cov == "nngp"
    assert f_ntk.params[0] == getattr(_lib, net) | _lib.NET_NTK and f_nngp.params[0] == getattr(_lib, net)
    assert f_ntk.params[1:] == f_nngp.params[1:]
    assert f_ntk.net == getattr(_lib, net)                                  # what smn_kernel_mlp is handed stays the architecture
    assert f_ntk.with_cov("nngp").params == f_nngp.params
    with pytest.raises(ValueError):
        f_ntk.with_cov("both")


@pytest.mark.parametrize("factory", ["get_cnn_kernel", "get_conv_resnet_kernel"])
def test_conv_factories_raise_before_any_device_call(factory):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NTKKernel
    kernel = NTKKernel(lambda w, b, l: getattr(nt_kernels, factory)(1, 1, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 0.5, 1.0)
    with pytest.raises(NotImplementedError):
        kernel.get_kernel_fn()
    conv_fn = getattr(nt_kernels, factory)(1, 1)
    with pytest.raises(NotImplementedError):
        kernel.K(conv_fn, np.zeros((2, 8, 8, 1)))
    with pytest.raises(NotImplementedError):
        kernel.predict(conv_fn, np.zeros((2, 8, 8, 1)), np.zeros(2), np.zeros((1, 8, 8, 1)))


def test_any_other_callable_is_asked_for_the_ntk():
    from smnngp.spax.kernels import NNGPKernel, NTKKernel
    asked = []

    def kernel_fn(x1, x2=None, get="nngp"):
        asked.append(get)
        return np.eye(len(x1))

    x = np.zeros((3, 2))
    assert NTKKernel(lambda w, b, l: kernel_fn).get_kernel_fn() is kernel_fn
    NTKKernel(lambda w, b, l: kernel_fn).K(kernel_fn, x)
    NNGPKernel(lambda w, b, l: kernel_fn).K(kernel_fn, x)
    assert asked == ["ntk", "nngp"]


def test_sweeps_know_the_covariance_argument():
    from smnngp import _lib, sweeps
    assert sweeps._net_code("resnet", "ntk") == _lib.NET_DENSE_RESNET | _lib.NET_NTK
    assert sweeps._net_code("mlp", "nngp") == _lib.NET_MLP
    with pytest.raises(ValueError):
        sweeps._net_code("mlp", "both")
