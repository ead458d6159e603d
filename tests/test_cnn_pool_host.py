"""Host tests of the pooled conv-NNGP kernel (nt_kernels.get_cnn_pool_kernel / smn_kernel_cnn_pool): the rules of
tests/_cnn_pool_rules.py against themselves (brute-force 6-D state against the per-offset slices), against the oracle's Flatten
kernel where the two coincide, against the closed form at depth 0 and against a finite-width Monte-Carlo network; and the
public surface (factory, header, library symbols).  No GPU: nothing here launches a kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _cnn_pool_rules as P
from oracle import nngp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYP = dict(w_std=1.3, b_std=0.4, last_w_std=0.9)


def images(n, h, w, c, seed):
    return np.random.default_rng(seed).standard_normal((n, h, w, c))


# ------------------------------------------------------------------------------------------------------------- rules
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("h,w,layers", [(3, 4, 3), (5, 1, 2), (6, 5, 2)])
def test_slices_equal_the_6d_state(h, w, layers, act):
    x1, x2 = images(3, h, w, 2, 10 * h + w), images(2, h, w, 2, 10 * h + w + 1)
    for b in (None, x2):
        full = P.pool_kernel(x1, b, layers, act, form="6d", **HYP)
        fast = P.pool_kernel(x1, b, layers, act, form="slices", **HYP)
        assert np.abs(full - fast).max() <= 1e-13 * np.abs(full).max()
    sym = P.pool_kernel(x1, None, layers, act, **HYP)
    assert np.abs(sym - sym.T).max() <= 1e-14 * np.abs(sym).max()


@pytest.mark.parametrize("act", ["relu", "erf"])
def test_same_pixel_entries_are_the_flatten_kernel(act):
    h, w = 4, 3
    x1, x2 = images(3, h, w, 2, 1), images(2, h, w, 2, 2)
    for b in (None, x2):
        k = P.state_6d(x1, b, 2, act, HYP["w_std"], HYP["b_std"])
        same = np.einsum("nmhwhw->nmhw", k)
        flat = HYP["last_w_std"] ** 2 * same.mean(axis=(2, 3))
        ref = O.cnn_kernel(x1, b, 2, act, **HYP)
        assert np.abs(flat - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("act", ["relu", "erf"])
def test_one_pixel_images_have_nothing_to_pool(act):
    x1, x2 = images(4, 1, 1, 3, 3), images(3, 1, 1, 3, 4)
    for b in (None, x2):
        got, ref = P.pool_kernel(x1, b, 3, act, **HYP), O.cnn_kernel(x1, b, 3, act, **HYP)
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_depth_zero_is_the_product_of_the_pixel_means():
    x1, x2 = images(4, 3, 5, 2, 5), images(3, 3, 5, 2, 6)
    m1, m2 = x1.mean(axis=(1, 2)), x2.mean(axis=(1, 2))
    for b, mb in ((None, m1), (x2, m2)):
        for form in ("slices", "6d"):
            got = P.pool_kernel(x1, b, 0, "relu", form=form, **HYP)
            ref = HYP["last_w_std"] ** 2 * (m1 @ mb.T) / x1.shape[-1]
            assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_finite_width_network_average():
    """relu, 4x4x2, two layers of 256 channels, weights N(0, w^2 / (9 c_in)), biases N(0, b^2), mean over pixels, Dense:
    the empirical covariance of 400 networks x 8 outputs against the kernel.  The standard error of an entry is about
    sqrt(2 / 3200) = 2.5 %; the tolerance is 6 % of the largest entry."""
    rng = np.random.default_rng(2024)
    n, h, w, c, width, nets, outs = 4, 4, 4, 2, 256, 400, 8
    ws, bs, lws = 1.2, 0.3, 1.0
    x = rng.standard_normal((n, h, w, c))

    def conv(a, wt, bias):                          # a [n,h,w,ci], wt [3,3,ci,co]: SAME, stride 1
        p = np.pad(a, [(0, 0), (1, 1), (1, 1), (0, 0)])
        out = np.zeros(a.shape[:3] + (wt.shape[-1],))
        for dh in range(3):
            for dw in range(3):
                out += p[:, dh:dh + h, dw:dw + w, :] @ wt[dh, dw]
        return out + bias

    acc = np.zeros((n, n))
    for _ in range(nets):
        a, ci = x, c
        for _layer in range(2):
            wt = rng.standard_normal((3, 3, ci, width)) * (ws / np.sqrt(9.0 * ci))
            a = np.maximum(conv(a, wt, bs * rng.standard_normal(width)), 0.0)
            ci = width
        f = a.mean(axis=(1, 2)) @ (rng.standard_normal((width, outs)) * (lws / np.sqrt(width)))
        acc += f @ f.T
    emp = acc / (nets * outs)
    ref = P.pool_kernel(x, None, 2, "relu", ws, bs, lws)
    err = np.abs(emp - ref).max() / np.abs(ref).max()
    print("Monte-Carlo network against the rules: %.3g of the largest entry" % err)
    assert err < 0.06


# ----------------------------------------------------------------------------------------------------------- surface
def test_header_declares_both_entries():
    text = open(os.path.join(ROOT, "include", "smnngp.h")).read()
    assert re.search(r"#define\s+SMN_CNN_POOL_MAX_PIXELS\s+1024\b", text)
    assert re.search(r"\bint\s+smn_kernel_cnn_pool\s*\(", text) and re.search(r"\bint\s+smn_kernel_cnn_pool_diag\s*\(", text)


@pytest.fixture(scope="module")
def L():
    """The binding, as tests/test_abi.py gets it: a library that does not build, or a package that does not import, fails the
    tests that need it."""
    import __graft_entry__ as g
    g.build()
    from smnngp import _lib
    return _lib


def test_library_exports_both_entries_with_the_bound_signatures(L):
    i, i64, d, vp = C.c_int, C.c_int64, C.c_double, C.c_void_p
    assert L.PROTOTYPES["smn_kernel_cnn_pool"] == [vp, i, i, i, d, d, d, vp, i64, vp, i64, i64, i64, i64, i, vp, i64]
    assert L.PROTOTYPES["smn_kernel_cnn_pool"] == L.PROTOTYPES["smn_kernel_cnn"]
    assert L.PROTOTYPES["smn_kernel_cnn_pool_diag"] == [vp, i, i, i, d, d, d, vp, i64, i64, i64, i64, vp]
    lib = C.CDLL(L.LIB_PATH)
    for name in ("smn_kernel_cnn_pool", "smn_kernel_cnn_pool_diag"):
        assert hasattr(lib, name)


def test_factory_surface(L):
    from smnngp import nt_kernels
    assert "get_cnn_pool_kernel" in nt_kernels.__all__
    fn = nt_kernels.get_cnn_pool_kernel(3, 10, act="erf", w_std=1.1, b_std=0.2, last_w_std=0.7)
    assert isinstance(fn, nt_kernels.CnnKernelFn) and fn.entry == "smn_kernel_cnn_pool"
    assert fn.params == (nt_kernels.get_act_class("erf"), 3, 1.1, 0.2, 0.7)
    assert nt_kernels.get_cnn_kernel(3).entry == "smn_kernel_cnn"           # the siblings are what they were
    assert nt_kernels.get_conv_resnet_kernel(1, 1).entry == "smn_kernel_conv_resnet"
    with pytest.raises(KeyError):
        nt_kernels.get_cnn_pool_kernel(1, act="tanh")
    with pytest.raises(NotImplementedError):
        fn(np.zeros((2, 3, 3, 1)), None, get="ntk")
    for bad in (np.zeros((2, 9)), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError, match=r"\[N,H,W,C\]"):
            fn(bad)
        with pytest.raises(ValueError, match=r"\[N,H,W,C\]"):
            fn.diag(bad)


def test_analytic_gradients_are_refused_before_any_device_call(L):
    from smnngp import nt_kernels
    from smnngp.spax.likelihoods import GaussianLikelihood
    from smnngp.spax.models import grad_route
    with pytest.raises(NotImplementedError):
        grad_route(nt_kernels.get_cnn_pool_kernel(2), GaussianLikelihood())
    assert grad_route(nt_kernels.get_cnn_kernel(2), GaussianLikelihood()) == "smn_spr_cnn_loss_grad"
