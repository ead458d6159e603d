"""CPU-side checks of the conv-NNGP analytic gradient (csrc/cnn_grad.hip, SPR.loss_and_grad): the two C-ABI entries
exist and reject a NULL context, the host function shared by both gradient routes turns (terms, quad, logdet) into the
right derivatives, and the dispatch accepts get_cnn_kernel but still refuses the conv ResNet.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from oracle import nngp_oracle as O  # noqa: E402  (test infrastructure only)

import _cnn_grad_rules as R  # noqa: E402

HYP = dict(w_std=1.3, b_std=0.4, last_w_std=0.9, eps=5e-2, alpha=1.7, beta=2.4)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from smnngp import _lib
    return _lib


def test_library_exports_the_conv_gradient_entries_and_they_reject_a_null_context(lib):
    raw = C.CDLL(lib.LIB_PATH)
    for name in ("smn_kernel_cnn_grad_terms", "smn_spr_cnn_loss_grad"):
        assert hasattr(raw, name), "libsmnngp.so does not export %s" % name
        assert name in lib.PROTOTYPES
    terms = (C.c_double * 4)()
    rc = lib._lib.smn_kernel_cnn_grad_terms(None, lib.F64, 0, 1, 1.0, 0.1, 1.0, None, 4, 4, 4, 1, None, 4, None, 1.0, terms)
    assert rc == lib.EINVAL
    q, ld, info = C.c_double(), C.c_double(), C.c_int()
    rc = lib._lib.smn_spr_cnn_loss_grad(None, lib.F64, 0, 1, 1.0, 0.1, 1.0, None, 4, 4, 4, 1, None, 1e-2, 0.0, 1.0,
                                        C.byref(q), C.byref(ld), C.byref(info), terms)
    assert rc == lib.EINVAL


@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("n,h,w,c,layers", [(24, 6, 6, 2, 3), (20, 5, 7, 3, 2), (12, 8, 8, 1, 4)])
def test_host_function_reproduces_finite_differences_of_the_reference_loss(lib, n, h, w, c, layers, act, method):
    """spax.models.lml_value_and_grads, fed terms / quad / logdet computed in NumPy by the forward-mode rules the device
    code implements, against central differences (relative step 1e-5) of the fp64 reference loss, all six trainables.
    Bound 2e-6 of max(largest reference gradient, |reference|): the project's fp64 bound for the MLP gradient; the rules
    themselves reach ~2e-9 and the step noise of the reference is ~8e-8."""
    from smnngp.spax.models import lml_value_and_grads
    rng = np.random.default_rng(100 * n + layers)
    x = rng.standard_normal((n, h, w, c))
    y = np.sin(x[:, 0, 0, 0]) + 0.3 * rng.standard_normal(n)
    k = O.cnn_kernel(x, None, layers, act, HYP["w_std"], HYP["b_std"], HYP["last_w_std"])
    g, _, _, _, quad, logdet, df, scale = R.g_matrix(k, y, HYP["eps"], method, HYP["alpha"], HYP["beta"])
    terms, _ = R.contract(g, x, layers, act, HYP["w_std"], HYP["b_std"], HYP["last_w_std"])
    lp, dlp = lml_value_and_grads(list(terms), quad, logdet, n, df, scale,
                                  HYP["alpha"] if method == "tp" else None, HYP["beta"] if method == "tp" else None)
    rl = R.ref_loss(x, y, layers, act, method, **HYP)
    assert abs(-lp / n - rl) < 1e-10 * max(1.0, abs(rl))
    keys = ("w_std", "b_std", "last_w_std", "eps") + (("alpha", "beta") if method == "tp" else ())
    ref = R.ref_grad_fd(x, y, layers, act, method, keys, **HYP)
    assert set(dlp) == {"w_std", "b_std", "last_w_std", "eps"} | ({"a", "b"} if method == "tp" else set())
    scale_g = max(abs(v) for v in ref.values())
    for key in keys:
        got = -dlp[{"alpha": "a", "beta": "b"}.get(key, key)] / n
        err = abs(got - ref[key]) / max(scale_g, abs(ref[key]))
        print("%s %s %s: %s got %.12g ref %.12g err %.3g" % ((n, h, w, c, layers), act, method, key, got, ref[key], err))
        assert err < 2e-6, (key, got, ref[key])


def test_cnn_kernel_fn_has_params_and_the_conv_resnet_is_still_refused(lib):
    from smnngp import nt_kernels
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import grad_route
    kfn = nt_kernels.get_cnn_kernel(3, 1, act="erf", w_std=1.3, b_std=0.4, last_w_std=0.9)
    assert kfn.params == (lib.ACT["erf"], 3, 1.3, 0.4, 0.9)
    assert grad_route(kfn, GaussianLikelihood()) == "smn_spr_cnn_loss_grad"
    assert grad_route(kfn, StudentTLikelihood(1.7, 2.4)) == "smn_spr_cnn_loss_grad"
    assert grad_route(nt_kernels.get_mlp_kernel(2), GaussianLikelihood()) == "smn_spr_loss_grad"
    res = nt_kernels.get_conv_resnet_kernel(1, 10, act="relu", w_std=1.2, b_std=0.3, last_w_std=0.9)
    assert res.params == (lib.ACT["relu"], 1, 1.2, 0.3, 0.9)
    with pytest.raises(NotImplementedError):
        grad_route(res, GaussianLikelihood())
    with pytest.raises(NotImplementedError):
        grad_route(kfn, object())
