"""GPU tests of the joint posterior draws: smn_mvn_draws against the fp64 rules of tests/_draws_rules.py on given variates
(every tile edge), the fused generator against the same call on its own downloaded variates (equal bits), how a draw is
keyed, smn_rng_chi2 against its NumPy restatement and its law, the argument errors, and SPR / MultiSPR.predictive_params and
sample_posterior against the oracle and against the composition predict + smn_cholesky + smn_rng_variates + smn_rng_chi2.

The error bound of every product comparison is D.error_bound: (T + 8) u (|mean| + r sum |L| |Z|), the inner-product bound
gamma_{T+8} in any summation order, with the reference computed in fp64 from the dtype-rounded operands."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _draws_rules as D  # noqa: E402

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def mvn_draws(ctx, dtype, mean, lo, T, Cn, S, df=0.0, shape=1.0, seed=0, point0=0, noise=None, mix=None, ldl=None):
    """mean [T,C], lo [T,ldl] host or device arrays -> out [S,T,C] device array."""
    mean_d = mean if hasattr(mean, "ptr") else ctx.to_device(np.ascontiguousarray(mean, dtype=dtype))
    lo_d = lo if hasattr(lo, "ptr") else ctx.to_device(np.ascontiguousarray(lo, dtype=dtype))
    out = ctx.empty((S, T, Cn), dtype)
    ctx.call("smn_mvn_draws", out.dcode, mean_d.ptr, lo_d.ptr, T if ldl is None else ldl, T, Cn, S, df, shape, seed, point0,
             noise.ptr if noise is not None else None, mix.ptr if mix is not None else None, out.ptr)
    return out


def variates(ctx, dtype, seed, point0, T, Cn, S):
    out = ctx.empty((T, Cn, S), dtype)
    ctx.call("smn_rng_variates", out.dcode, seed, 0.0, point0, T, Cn, S, out.ptr)
    return out


def chi2(ctx, seed, df, S):
    out = ctx.empty((S,), np.float64)
    ctx.call("smn_rng_chi2", seed, df, S, out.ptr)
    return out


def lower_with_nan(rng, T, ldl, dtype):
    """Random lower factor in a [T,ldl] window: NaN in the strict upper triangle and in the ld - T padding columns."""
    lo = np.full((T, ldl), np.nan, dtype=dtype)
    lo[:, :T] = np.where(np.tri(T, dtype=bool), rng.standard_normal((T, T)), np.nan)
    return lo


def check(out, mean, lo, z, r, dtype, what):
    out = np.asarray(out, dtype=np.float64)
    ref = D.draws(mean, lo, z, r)
    bound = D.error_bound(mean, lo, z, r, dtype)
    assert out.shape == ref.shape, what
    assert np.all(np.isfinite(out)), what
    ratio = float(np.max(np.abs(out - ref) / bound))
    assert ratio <= 1.0, (what, ratio)
    return ratio


# ----------------------------------------------------------------------------- 1. the product against the rules
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 15, 16, 17, 33, 130])
def test_product_on_given_variates_matches_the_rules(ctx, dtype, T):
    rng = np.random.default_rng(1000 + T)
    worst = 0.0
    for ldl in (T, T + 5):
        lo = lower_with_nan(rng, T, ldl, dtype)
        lo_d = ctx.to_device(lo)
        for Cn in (1, 3, 4, 5, 10):
            mean = rng.standard_normal((T, Cn)).astype(dtype)
            mean_d = ctx.to_device(mean)
            for S in (1, 5, 64, 130):
                z = rng.standard_normal((T, Cn, S)).astype(dtype)
                z_d = ctx.to_device(z)
                g = rng.chisquare(7.5, S)
                g_d = ctx.to_device(g)
                for df in (0.0, 7.5):
                    out = mvn_draws(ctx, dtype, mean_d, lo_d, T, Cn, S, df=df, shape=0.8, noise=z_d, mix=g_d, ldl=ldl).numpy()
                    r = D.scale_r(df, 0.8, g, dtype)
                    worst = max(worst, check(out, mean, lo[:, :T], z, r, dtype, (T, ldl, Cn, S, df)))
    print("product %s T %d: worst error / bound = %.3g" % (np.dtype(dtype).name, T, worst))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("window", ["ldl=T", "ldl=T+5", "odd base"])
def test_product_with_interior_column_tiles_matches_the_rules(ctx, dtype, window):
    """T = 300: three column tiles, the last one partial.  The K-steps of the middle tile that lie wholly left of its first
    row are staged with unmasked 16-byte loads when l_d and ldl allow them (ldl = T: 1200 / 2400 bytes per row) and element by
    element when they do not: ldl = T + 5, or an aligned ldl = T + 4 behind a base one element off.  NaN in the strict upper
    triangle, in the padding columns and around the window, so any read outside the triangle shows."""
    T = 300
    rng = np.random.default_rng(300)
    isz = np.dtype(dtype).itemsize
    ldl, off = {"ldl=T": (T, 0), "ldl=T+5": (T + 5, 0), "odd base": (T + 4, 1)}[window]
    lo = lower_with_nan(rng, T, ldl, dtype)
    flat = np.full(T * ldl + 2, np.nan, dtype=dtype)
    flat[off:off + T * ldl] = lo.ravel()
    flat_d = ctx.to_device(flat)
    lo_p = C.c_void_p(flat_d.ptr.value + off * isz)
    assert (lo_p.value % 16 == 0 and (ldl * isz) % 16 == 0) == (window == "ldl=T")      # the case takes the path it is named for
    worst = 0.0
    for Cn, S in ((5, 70), (3, 130)):
        mean = rng.standard_normal((T, Cn)).astype(dtype)
        z = rng.standard_normal((T, Cn, S)).astype(dtype)
        g = rng.chisquare(7.5, S)
        mean_d, z_d, g_d = ctx.to_device(mean), ctx.to_device(z), ctx.to_device(g)
        for df in (0.0, 7.5):
            out = ctx.empty((S, T, Cn), dtype)
            ctx.call("smn_mvn_draws", out.dcode, mean_d.ptr, lo_p, ldl, T, Cn, S, df, 0.8, 0, 0, z_d.ptr, g_d.ptr, out.ptr)
            worst = max(worst, check(out.numpy(), mean, lo[:, :T], z, D.scale_r(df, 0.8, g, dtype), dtype, (window, Cn, S, df)))
    print("product %s T %d %s: worst error / bound = %.3g" % (np.dtype(dtype).name, T, window, worst))


# ----------------------------------------------------------------------------- 2. fused equals given
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("df", [0.0, 7.5])
@pytest.mark.parametrize("T,Cn,S", [(33, 1, 64), (64, 10, 130), (130, 5, 17), (300, 3, 40)])
def test_fused_call_equals_the_call_on_its_own_variates(ctx, dtype, df, T, Cn, S):
    seed, point0 = 991, 1000
    rng = np.random.default_rng(T + Cn)
    lo_d = ctx.to_device(lower_with_nan(rng, T, T, dtype))
    mean_d = ctx.to_device(rng.standard_normal((T, Cn)).astype(dtype))
    z_d = variates(ctx, dtype, seed, point0, T, Cn, S)
    g_d = chi2(ctx, seed, df, S) if df > 0 else None
    given = mvn_draws(ctx, dtype, mean_d, lo_d, T, Cn, S, df=df, shape=1.3, seed=seed, point0=point0, noise=z_d, mix=g_d).numpy()
    fused = mvn_draws(ctx, dtype, mean_d, lo_d, T, Cn, S, df=df, shape=1.3, seed=seed, point0=point0).numpy()
    assert np.all(np.isfinite(fused))
    assert np.array_equal(fused, given)                                                 # the same bits


# ----------------------------------------------------------------------------- 3. keying
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("df", [0.0, 7.5])
def test_draws_are_keyed_by_seed_point_class_and_draw(ctx, dtype, df):
    T, seed, point0 = 40, 77, 300
    rng = np.random.default_rng(9)
    lo = lower_with_nan(rng, T, T, dtype)
    lo_d = ctx.to_device(lo)
    mean = rng.standard_normal((T, 10)).astype(dtype)
    mean_d = ctx.to_device(mean)
    mean3_d = ctx.to_device(np.ascontiguousarray(mean[:, :3]))

    def run(S=130, Cn=10, seed=seed, point0=point0):
        return mvn_draws(ctx, dtype, mean_d if Cn == 10 else mean3_d, lo_d, T, Cn, S, df=df, shape=0.7, seed=seed,
                         point0=point0).numpy()

    whole = run()
    assert np.array_equal(run(), whole)                                                 # a second call: equal bits
    assert np.array_equal(run(S=17), whole[:17])                                        # not by the number of draws
    assert np.array_equal(run(Cn=3), whole[:, :, :3])                                   # nor by the number of outputs
    assert not np.array_equal(run(seed=78), whole)
    assert not np.array_equal(run(seed=(1 << 40) + 77), whole)                          # the high seed word is part of the key
    assert not np.array_equal(run(point0=301), whole)


@pytest.mark.parametrize("dtype", DTYPES)
def test_point0_selects_the_variates_of_those_points(ctx, dtype):
    """point0 = 100, T = 8: the variates of points 100 .. 107, through the rules on smn_rng_variates(point0 = 100)."""
    T, Cn, S, seed = 8, 5, 33, 4242
    rng = np.random.default_rng(2)
    lo = lower_with_nan(rng, T, T, dtype)
    mean = rng.standard_normal((T, Cn)).astype(dtype)
    z = variates(ctx, dtype, seed, 100, T, Cn, S).numpy()
    out = mvn_draws(ctx, dtype, mean, lo, T, Cn, S, seed=seed, point0=100).numpy()
    check(out, mean, lo, z, np.ones(S), dtype, "point0")
    other = variates(ctx, dtype, seed, 0, T, Cn, S).numpy()
    assert np.max(np.abs(out - D.draws(mean, lo, other, np.ones(S)))) > 1e-2            # and not those of points 0 .. 7


# ----------------------------------------------------------------------------- 4. the mixing variates
@pytest.mark.parametrize("df", D.STAT_DFS)
def test_chi2_on_the_device_equals_the_restatement_and_follows_its_law(ctx, df):
    s = D.STAT_DRAWS
    g = chi2(ctx, D.STAT_SEED, df, s).numpy()
    assert g.shape == (s,) and np.all(np.isfinite(g)) and np.all(g > 0)
    d, lag1 = D.chi2_statistics(g, df)
    ref = D.chi2(D.STAT_SEED, df, s)
    rel = np.abs(g - ref) / ref
    off = int(np.sum(rel > 1e-9))
    inside = rel[rel <= 1e-9]
    print("chi2 df %g: KS D sqrt(S) = %.3f, lag-1 sqrt(S) = %.3f, max relative difference %.3g (%d of %d outside 1e-9)"
          % (df, d * np.sqrt(s), lag1 * np.sqrt(s), float(inside.max()) if inside.size else float("nan"), off, s))
    assert d < 1.95 / np.sqrt(s)
    assert lag1 < 5 / np.sqrt(s)
    assert off <= 2            # an acceptance decision on a rounding edge may flip; a wrong generator flips thousands


# ----------------------------------------------------------------------------- 5. argument errors
def test_bad_arguments_are_refused(ctx, L):
    T, Cn, S = 8, 3, 4
    mean, lo, out = ctx.to_device(np.zeros((T, Cn))), ctx.to_device(np.eye(T)), ctx.empty((S, T, Cn), np.float64)

    def call(dtype=L.F64, mean_p=mean.ptr, lo_p=lo.ptr, ldl=T, T=T, Cn=Cn, S=S, df=0.0, shape=1.0, point0=0, out_p=out.ptr):
        ctx.call("smn_mvn_draws", dtype, mean_p, lo_p, ldl, T, Cn, S, df, shape, 1, point0, None, None, out_p)

    call()
    bad = [dict(mean_p=None), dict(lo_p=None), dict(out_p=None), dict(dtype=7), dict(T=0), dict(Cn=0), dict(S=0),
           dict(df=3.0, shape=0.0), dict(df=3.0, shape=-1.0), dict(df=3.0, shape=float("nan")), dict(point0=-1),
           dict(point0=(1 << 32) - T + 1), dict(S=(1 << 32) + 1)]
    for kw in bad:
        with pytest.raises(L.SmnError) as e:
            call(**kw)
        assert e.value.code == L.EINVAL, kw
    with pytest.raises(L.SmnError) as e:
        call(Cn=129)
    assert e.value.code == L.ENOTSUP
    with pytest.raises(L.SmnError) as e:
        call(ldl=T - 1)
    assert e.value.code == L.EINVAL and "ldl" in str(e.value) and "smn_mvn_draws" in str(e.value)
    g = ctx.empty((S,), np.float64)
    for kw in (dict(df=0.0), dict(df=-1.0), dict(df=float("nan")), dict(S=0), dict(S=(1 << 32) + 1), dict(out=None)):
        a = dict(dict(df=3.0, S=S, out=g.ptr), **kw)
        with pytest.raises(L.SmnError) as e:
            ctx.call("smn_rng_chi2", 1, a["df"], a["S"], a["out"])
        assert e.value.code == L.EINVAL, kw


# ----------------------------------------------------------------------------- 6 / 7. the models
def make_model(name, method, dtype, hyp=D.HYP):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    x, y, xt = D.case_data(name, np.dtype(dtype) == np.float32)
    get = nt_kernels.get_mlp_kernel if D.CASES[name]["family"] == "mlp" else nt_kernels.get_cnn_kernel
    kernel = NNGPKernel(lambda w, b, l: get(D.LAYERS, act=D.ACT, w_std=w, b_std=b, last_w_std=l),
                        hyp["w_std"], hyp["b_std"], hyp["last_w_std"])
    lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(hyp["alpha"], hyp["beta"])
    if name == "spr":
        model = SPR(kernel, lik, x.astype(dtype), y[:, 0].astype(dtype), 0.0, 1.0, eps=hyp["eps"])
    else:
        model = MultiSPR(kernel, lik, x.astype(dtype), y.astype(dtype), eps=hyp["eps"])
    return model, xt.astype(dtype)


def composition(ctx, model, xt, seed, point0, S, jitter):
    """What sample_posterior is made of, piece by piece: predict's mean, the factor of a copy of its covariance from a
    second smn_cholesky call with the documented arguments, the downloaded variates and mixing variates.
    -> (mean, L, Z, r, info, df_post, shape) as host arrays."""
    mean, cov = model.predict(xt)
    t, c = mean.shape
    info = C.c_int()
    ctx.call("smn_cholesky", cov.dcode, cov.ptr, t, t, t, t, 0.0, jitter, C.byref(info), None)
    df_post, shape = model.predictive_params()
    z = variates(ctx, mean.dtype, seed, point0, t, c, S).numpy()
    if df_post is None:
        r = np.ones(S)
    else:
        r = D.scale_r(df_post, shape, chi2(ctx, seed, df_post, S).numpy(), mean.dtype)
    return mean.raw_numpy(), cov.raw_numpy(), z, r, info.value, df_post, shape


def as_stc(f, model):
    f = f.numpy() if hasattr(f, "numpy") else np.asarray(f)
    return f if hasattr(model, "num_outputs") else f[:, :, None]


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_predictive_params_match_the_oracle(name):
    """6a: (None, 1) for the Gaussian model; df_post = 2a + N C exactly and shape within 1e-7 of the oracle's (the fp64
    tolerance tests/test_gpu_multi.py holds test_nll to)."""
    model, _ = make_model(name, "gp", np.float64)
    assert model.predictive_params() == (None, 1.0)
    model, _ = make_model(name, "tp", np.float64)
    df_post, shape = model.predictive_params()
    ref_df, ref_shape = D.oracle_predictive_params(name)
    print("%s: df_post %g, shape %.15g (oracle %.15g)" % (name, df_post, shape, ref_shape))
    assert abs(df_post - ref_df) < 1e-7 * ref_df
    assert abs(shape - ref_shape) < 1e-7 * max(1.0, abs(ref_shape))


def test_spr_on_a_conv_kernel_takes_the_matrix_route_of_test_nll(ctx):
    """SPR has no fused quadratic form for a conv kernel: predictive_params factors (b/a) K + 1e-6 I as a matrix, as
    SPR.test_nll does there.  The conv case's images with its first target column: shape within 1e-7 of the oracle's, and
    sample_posterior equals the composition."""
    import scipy.linalg as sla
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import StudentTLikelihood
    from smnngp.spax.models import SPR
    hyp = D.HYP
    x, y, xt = D.case_data("multi")
    y = y[:, 0]
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_kernel(D.LAYERS, act=D.ACT, w_std=w, b_std=b, last_w_std=l),
                        hyp["w_std"], hyp["b_std"], hyp["last_w_std"])
    model = SPR(kernel, StudentTLikelihood(hyp["alpha"], hyp["beta"]), x, y, 0.0, 1.0, eps=hyp["eps"])
    df, scale = 2.0 * hyp["alpha"], hyp["beta"] / hyp["alpha"]
    khat = scale * D.oracle_kernel("multi", x) + 1e-6 * np.eye(len(y))
    quad = float(y @ sla.cho_solve(sla.cho_factor(khat, lower=True), y))
    ref_df, ref_shape = df + len(y), (df + quad) / (df + len(y)) * scale
    df_post, shape = model.predictive_params()
    print("spr on cnn: df_post %g, shape %.15g (oracle %.15g)" % (df_post, shape, ref_shape))
    assert abs(df_post - ref_df) < 1e-7 * ref_df
    assert abs(shape - ref_shape) < 1e-7 * max(1.0, abs(ref_shape))
    f = model.sample_posterior((5, 200), xt, 64, jitter=1e-8)
    mean, lo, z, r, info, _, _ = composition(ctx, model, xt, 5, 200, 64, 1e-8)
    assert info == 0 and f.shape == (64, xt.shape[0])
    check(as_stc(f, model), mean, lo, z, r, np.float64, "spr on cnn")


@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("name", sorted(D.CASES))
def test_sample_posterior_equals_the_composition(ctx, name, method):
    """6b, fp64."""
    model, xt = make_model(name, method, np.float64)
    f = model.sample_posterior((5, 200), xt, 64, jitter=1e-8)
    mean, lo, z, r, info, _, _ = composition(ctx, model, xt, 5, 200, 64, 1e-8)
    assert info == 0 and f.dtype == np.float64
    assert f.shape == ((64,) + mean.shape if name == "multi" else (64, mean.shape[0]))
    ratio = check(as_stc(f, model), mean, lo, z, r, np.float64, (name, method))
    print("%s %s: worst error / bound = %.3g" % (name, method, ratio))


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_gaussian_draws_have_the_posterior_moments(ctx, name):
    """6c: sample mean and per-output sample covariance of 4096 draws within 5 sd / sqrt(S) per entry of predict's mean and
    of cov + jitter tr/T I; at most 5 % of the entries may miss (tests/test_draws_host.py: the reference alone misses none)."""
    model, xt = make_model(name, "gp", np.float64)
    mean, cov = model.predict(xt)
    f = as_stc(model.sample_posterior(D.MOMENT_SEED, xt, D.MOMENT_DRAWS, jitter=D.MOMENT_JITTER), model)
    total, miss = D.moment_misses(f, mean.numpy().astype(np.float64), D.ridged(cov.numpy(), D.MOMENT_JITTER))
    print("%s: %d of %d entries outside 5 sd / sqrt(S)" % (name, miss, total))
    assert np.all(np.isfinite(f)) and miss <= 0.05 * total


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_student_draws_have_t_marginals_and_one_scale_per_draw(ctx, name):
    """6d: the marginal at a point is t(df_post) in units of sqrt(shape (L L^T)_tt), and the scale r_s recovered from two
    different (point, output) pairs of one draw is the same number, the one smn_rng_chi2 gives."""
    from scipy import stats
    S, seed = 4096, 31
    model, xt = make_model(name, "tp", np.float64)
    f = as_stc(model.sample_posterior(seed, xt, S, jitter=1e-8), model)
    mean, lo, z, r, info, df_post, shape = composition(ctx, model, xt, seed, 0, S, 1e-8)
    assert info == 0 and np.all(np.isfinite(f))
    t, c = mean.shape
    lo = np.tril(lo)
    var = np.einsum("tk,tk->t", lo, lo)
    for pt, out in ((0, 0), (t // 2, c - 1), (t - 1, c // 2)):
        u = (f[:, pt, out] - mean[pt, out]) / np.sqrt(shape * var[pt])
        d = stats.kstest(u, stats.t(df_post).cdf).statistic
        print("%s point %d output %d: KS D sqrt(S) = %.3f" % (name, pt, out, d * np.sqrt(S)))
        assert d < 1.95 / np.sqrt(S)
    lz = np.einsum("tk,kcs->stc", lo, z)
    bound = D.error_bound(mean, lo, z, r, np.float64)
    (t1, c1), (t2, c2) = (0, 0), (t - 1, c - 1)
    r1 = (f[:, t1, c1] - mean[t1, c1]) / lz[:, t1, c1]
    r2 = (f[:, t2, c2] - mean[t2, c2]) / lz[:, t2, c2]
    slack = bound[:, t1, c1] / np.abs(lz[:, t1, c1]) + bound[:, t2, c2] / np.abs(lz[:, t2, c2])
    assert np.all(np.abs(r1 - r2) <= slack)
    assert np.all(np.abs(r1 - r) <= slack)
    assert np.std(r) > 1e-3                                          # and it does vary from draw to draw


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_covariance_that_does_not_factor_gives_nan(ctx, name):
    """6e: test points = training points, eps tiny, no ridge (tests/test_draws_host.py: NumPy's Cholesky fails too)."""
    model, _ = make_model(name, "gp", np.float64, hyp=dict(D.HYP, eps=D.TINY_EPS))
    x = D.case_data(name)[0]
    f = model.sample_posterior(3, x, 7, jitter=0.0)
    assert f.shape == ((7, x.shape[0], 3) if name == "multi" else (7, x.shape[0]))
    assert np.all(np.isnan(f.numpy()))


@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("name", sorted(D.CASES))
def test_sample_posterior_fp32(ctx, name, method):
    """7: jitter 1e-3, test points apart from the training points (tests/test_draws_host.py: the ridged covariance is far
    from marginal in fp32): the factorisation succeeds, the draws are finite and equal the composition within the bound."""
    model, xt = make_model(name, method, np.float32)
    f = model.sample_posterior((5, 200), xt, 64, jitter=D.F32_JITTER)
    mean, lo, z, r, info, _, _ = composition(ctx, model, xt, 5, 200, 64, D.F32_JITTER)
    assert info == 0 and f.dtype == np.float32
    ratio = check(as_stc(f, model), mean, lo, z, r, np.float32, (name, method))
    print("%s %s fp32: worst error / bound = %.3g" % (name, method, ratio))
