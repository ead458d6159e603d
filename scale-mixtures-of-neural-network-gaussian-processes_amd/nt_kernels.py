"""Kernel factories — same names, arguments and defaults as experiments/nt_kernels.py:21-103.

Each factory returns ``kernel_fn(x1, x2=None, get="nngp")`` like neural_tangents' stax.serial does;
here it is a small object that launches the fused HIP build (smn_kernel_mlp) and returns device
arrays.  ``get`` accepts "nngp", "ntk" or a tuple of both (a namedtuple-like Kernels result).
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DeviceArray, as_device, default_context

__all__ = ["get_mlp_kernel", "get_cnn_kernel", "get_cnn_pool_kernel", "get_conv_resnet_kernel", "get_dense_resnet_kernel"]

Kernels = collections.namedtuple("Kernels", ["nngp", "ntk"])


def get_act_class(act):
    """experiments/nt_kernels.py:12-18 — KeyError for anything but relu / erf."""
    if act == "relu":
        return _lib.ACT["relu"]
    elif act == "erf":
        return _lib.ACT["erf"]
    else:
        raise KeyError("Unsupported act '{}'".format(act))


def _parse_get(get):
    if isinstance(get, str):
        names = (get,)
    else:
        names = tuple(get)
    mask = 0
    for g in names:
        if g == "nngp":
            mask |= _lib.GET_NNGP
        elif g == "ntk":
            mask |= _lib.GET_NTK
        else:
            raise ValueError("get must be 'nngp', 'ntk' or a tuple of them, got %r" % (g,))
    return names, mask


def _check_scales(s):
    """input_scales as a positive float64 vector (None stays None)."""
    if s is None:
        return None
    s = np.array(s, dtype=np.float64).reshape(-1)
    if s.size == 0 or not np.all(np.isfinite(s)) or not np.all(s > 0.0):
        raise ValueError("input_scales must be a non-empty vector of positive finite numbers")
    return s


def _scale_columns(ctx, a, s, out=None):
    """a [n, d] with column j multiplied by s[j], in a's dtype (smn_scale_columns); `out` may be a itself."""
    n, d = a.shape
    if s.shape[0] != d:
        raise ValueError("input_scales has %d entries for inputs with %d features" % (s.shape[0], d))
    out = ctx.empty((n, d), a.dtype) if out is None else out
    s = np.ascontiguousarray(s, dtype=np.float64)
    ctx.call("smn_scale_columns", a.dcode, a.ptr, n, d, d, s.ctypes.data_as(C.POINTER(C.c_double)), out.ptr, d)
    return out


class KernelFn:
    """kernel_fn of an MLP-family architecture (net = MLP or dense ResNet)."""

    def __init__(self, net, num_hiddens, act, w_std, b_std, last_w_std, ctx=None, cov="nngp", input_scales=None):
        self.net, self.num_hiddens = int(net), int(num_hiddens)
        self.act_name, self.act = act, get_act_class(act)
        self.w_std, self.b_std, self.last_w_std = float(w_std), float(b_std), float(last_w_std)
        self.ctx = ctx
        if cov not in ("nngp", "ntk"):
            raise ValueError("cov must be 'nngp' or 'ntk', got %r" % (cov,))
        self.cov = cov
        self.input_scales = _check_scales(input_scales)

    @property
    def params(self):
        """What the model entries of the C ABI take in front of the data: (net, act, num_hiddens, w_std, b_std,
        last_w_std).  In covariance mode "ntk" net carries SMN_NET_NTK, and those entries work on Theta instead of K."""
        net = self.net | _lib.NET_NTK if self.cov == "ntk" else self.net
        return (net, self.act, self.num_hiddens, self.w_std, self.b_std, self.last_w_std)

    def with_cov(self, cov):
        """The same kernel function in covariance mode `cov` ("nngp" or "ntk"): which of its two kernels a model built on
        it (spax.kernels.NNGPKernel / NTKKernel) takes as the covariance function of its GP.  `__call__` is unaffected."""
        return KernelFn(self.net, self.num_hiddens, self.act_name, self.w_std, self.b_std, self.last_w_std, self.ctx, cov,
                        self.input_scales)

    def with_input_scales(self, s):
        """The same kernel function on scaled inputs, k(x, x') = K(s o x, s o x'): s is a positive vector with one entry per
        input feature (automatic relevance determination; None takes the scales off).  The scaling multiplies in the storage
        dtype with s rounded to it first, so the results are the bits of this kernel function without scales on
        x * s.astype(dtype).  `params` is unchanged: the model entries are handed `scaled(x)`."""
        return KernelFn(self.net, self.num_hiddens, self.act_name, self.w_std, self.b_std, self.last_w_std, self.ctx, self.cov, s)

    def scaled(self, x, ctx=None, dtype=None):
        """x as the kernel sees it: the device array x * input_scales (smn_scale_columns), or x itself without scales."""
        ctx = ctx or self.ctx or (x.ctx if isinstance(x, DeviceArray) else default_context())
        a = as_device(x, ctx, dtype=dtype)
        if len(a.shape) != 2:
            a = ctx.to_device(a.numpy().reshape(a.shape[0], -1))
        if self.input_scales is None:
            return a
        return _scale_columns(ctx, a, self.input_scales)

    def cov_matrix(self, x1, x2=None, fill="full"):
        """The matrix of the covariance mode: K or Theta of x1 against x2."""
        return self(x1, x2, get=self.cov, fill=fill)

    def __call__(self, x1, x2=None, get="nngp", fill="full"):
        ctx = self.ctx or (x1.ctx if isinstance(x1, DeviceArray) else default_context())
        names, mask = _parse_get(get)
        a = as_device(x1, ctx)
        if len(a.shape) != 2:
            a_host = a.numpy().reshape(a.shape[0], -1)
            a = ctx.to_device(a_host)
        b = None
        if x2 is not None and x2 is not x1:
            b = as_device(x2, ctx, dtype=a.dtype)
            if len(b.shape) != 2:
                b = ctx.to_device(b.numpy().reshape(b.shape[0], -1))
            if b.shape[1] != a.shape[1]:
                raise ValueError("x1 and x2 feature dimensions differ: %s vs %s" % (a.shape, b.shape))
            if b.dtype != a.dtype:
                raise TypeError("x1 and x2 dtypes differ")
        if self.input_scales is not None:
            a = _scale_columns(ctx, a, self.input_scales)
            b = None if b is None else _scale_columns(ctx, b, self.input_scales)
        n1, d = a.shape
        n2 = n1 if b is None else b.shape[0]
        k = ctx.empty((n1, n2), a.dtype) if mask & _lib.GET_NNGP else None
        t = ctx.empty((n1, n2), a.dtype) if mask & _lib.GET_NTK else None
        ctx.call("smn_kernel_mlp", a.dcode, self.net, self.act, self.num_hiddens, self.w_std, self.b_std,
                 self.last_w_std, a.ptr, n1, d, None if b is None else b.ptr, n2, d, d, mask,
                 _lib.FILL_FULL if fill == "full" else _lib.FILL_LOWER,
                 None if k is None else k.ptr, None if t is None else t.ptr, n2)
        out = {"nngp": k, "ntk": t}
        if isinstance(get, str):
            return out[get]
        if len(names) == 2:
            return Kernels(**{n: out[n] for n in names}) if set(names) == {"nngp", "ntk"} else tuple(out[n] for n in names)
        return tuple(out[n] for n in names)

    def input_grad(self, x1, x2, gbar, get=None):
        """gx [n1, d] = sum_j gbar[r, j] dK(x1_r, x2_j)/dx1_r as a device array (smn_kernel_mlp_input_grad): the kernel
        differentiated in its first argument, contracted with the seed gbar [n1, n2].  `get` ("nngp" or "ntk") picks K or
        Theta and defaults to the covariance mode.  x2 must be given: the form in which both arguments move is the seeded
        one of the exact models (SPR.loss_input_grad).  Under input scales both arguments are scaled first and the result is
        multiplied by s: the derivative in x1 as handed in."""
        get = self.cov if get is None else get
        if get not in ("nngp", "ntk"):
            raise ValueError("get must be 'nngp' or 'ntk', got %r" % (get,))
        if x2 is None:
            raise NotImplementedError("input_grad needs x2: the symmetric form, in which both arguments move, is not implemented")
        ctx = self.ctx or (x1.ctx if isinstance(x1, DeviceArray) else default_context())
        a = as_device(x1, ctx)
        if len(a.shape) != 2:                      # [N, ...] is flattened, as __call__ does (gx comes back [n1, d])
            a = ctx.to_device(a.numpy().reshape(a.shape[0], -1))
        b = as_device(x2, ctx, dtype=a.dtype)
        if len(b.shape) != 2:
            b = ctx.to_device(b.numpy().reshape(b.shape[0], -1))
        g = as_device(gbar, ctx, dtype=a.dtype)
        if a.shape[1] != b.shape[1]:
            raise ValueError("x1 and x2 feature dimensions differ: %s vs %s" % (a.shape, b.shape))
        if tuple(g.shape) != (a.shape[0], b.shape[0]):
            raise ValueError("gbar must be [n1, n2] = %s, got %s" % ((a.shape[0], b.shape[0]), g.shape))
        n1, d = a.shape
        if self.input_scales is not None:
            a, b = _scale_columns(ctx, a, self.input_scales), _scale_columns(ctx, b, self.input_scales)
        out = ctx.empty((n1, d), a.dtype)
        net = self.net | _lib.NET_NTK if get == "ntk" else self.net
        ctx.call("smn_kernel_mlp_input_grad", a.dcode, net, self.act, self.num_hiddens, self.w_std, self.b_std, self.last_w_std,
                 a.ptr, n1, d, b.ptr, b.shape[0], d, d, g.ptr, b.shape[0], out.ptr, d)
        if self.input_scales is not None:
            _scale_columns(ctx, out, self.input_scales, out=out)
        return out


def get_mlp_kernel(num_hiddens, num_class=1, act="relu", w_std=1., b_std=0., last_w_std=1.):
    """experiments/nt_kernels.py:21-31.  `num_class` and the hidden width (512) do not enter the kernel."""
    return KernelFn(_lib.NET_MLP, num_hiddens, act, w_std, b_std, last_w_std)


def get_dense_resnet_kernel(num_hiddens, num_class=1, act="relu", w_std=1., b_std=0., last_w_std=1.):
    """experiments/nt_kernels.py:83-103."""
    return KernelFn(_lib.NET_DENSE_RESNET, num_hiddens, act, w_std, b_std, last_w_std)


class CnnKernelFn:
    """kernel_fn of get_cnn_kernel (experiments/nt_kernels.py:34-45) or, with entry="smn_kernel_conv_resnet", of
    get_conv_resnet_kernel (:48-80, num_hiddens = block size), or, with entry="smn_kernel_cnn_pool", of get_cnn_pool_kernel
    (GlobalAvgPool in place of Flatten); x is [N,H,W,C]; NNGP only."""

    def __init__(self, num_hiddens, act, w_std, b_std, last_w_std, ctx=None, entry="smn_kernel_cnn"):
        self.num_hiddens, self.act_name, self.act = int(num_hiddens), act, get_act_class(act)
        self.w_std, self.b_std, self.last_w_std = float(w_std), float(b_std), float(last_w_std)
        self.ctx = ctx
        self.entry = entry

    @property
    def params(self):
        return (self.act, self.num_hiddens, self.w_std, self.b_std, self.last_w_std)

    def __call__(self, x1, x2=None, get="nngp", fill="full"):
        if get != "nngp":
            raise NotImplementedError("conv kernel: only get='nngp' is on the hot path")
        if not isinstance(x1, DeviceArray) and np.ndim(x1) != 4:   # a host array: refused before a context is made
            raise ValueError("conv kernel expects x of shape [N,H,W,C]")
        ctx = self.ctx or (x1.ctx if isinstance(x1, DeviceArray) else default_context())
        a = as_device(x1, ctx)
        if len(a.shape) != 4:
            raise ValueError("conv kernel expects x of shape [N,H,W,C]")
        b = None
        if x2 is not None and x2 is not x1:
            b = as_device(x2, ctx, dtype=a.dtype)
            if b.shape[1:] != a.shape[1:]:
                raise ValueError("x1 and x2 image shapes differ")
        n1, h, w, c = a.shape
        n2 = n1 if b is None else b.shape[0]
        k = ctx.empty((n1, n2), a.dtype)
        ctx.call(self.entry, a.dcode, self.act, self.num_hiddens, self.w_std, self.b_std, self.last_w_std,
                 a.ptr, n1, None if b is None else b.ptr, n2, h, w, c,
                 _lib.FILL_FULL if fill == "full" else _lib.FILL_LOWER, k.ptr, n2)
        return k

    def diag(self, x):
        """K(x_i, x_i) [N] as a device array without the other pairs: the bits of the diagonal of kernel_fn(x, None).  The
        Flatten kernels run their per-image pass (smn_kernel_conv_diag, kind 0 / 1); the pooled kernel has no per-image closed
        form -- every pixel of an image meets every other -- and runs its N diagonal pairs (smn_kernel_cnn_pool_diag)."""
        if not isinstance(x, DeviceArray) and np.ndim(x) != 4:
            raise ValueError("conv kernel expects x of shape [N,H,W,C]")
        ctx = self.ctx or (x.ctx if isinstance(x, DeviceArray) else default_context())   # __call__'s precedence
        a = as_device(x, ctx)
        if len(a.shape) != 4:
            raise ValueError("conv kernel expects x of shape [N,H,W,C]")
        n, h, w, c = a.shape
        out = ctx.empty((n,), a.dtype)
        if self.entry == "smn_kernel_cnn_pool":
            ctx.call("smn_kernel_cnn_pool_diag", a.dcode, self.act, self.num_hiddens, self.w_std, self.b_std, self.last_w_std,
                     a.ptr, n, h, w, c, out.ptr)
        else:
            ctx.call("smn_kernel_conv_diag", a.dcode, 0 if self.entry == "smn_kernel_cnn" else 1, self.act, self.num_hiddens,
                     self.w_std, self.b_std, self.last_w_std, a.ptr, n, h, w, c, out.ptr)
        return out

    def _check_input_grad(self, h, w):
        """What the reverse pass of the conv kernel covers: get_cnn_kernel and images of at most 1024 pixels."""
        if self.entry != "smn_kernel_cnn":
            raise NotImplementedError("input_grad exists for get_cnn_kernel only: the pooled kernel and the conv ResNet have no "
                                      "input derivative here")
        if int(h) * int(w) > 1024:
            raise NotImplementedError("input_grad needs images of at most 1024 pixels, got %d x %d" % (h, w))

    def input_grad(self, x1, x2, gbar):
        """gx [n1,H,W,C] = sum_j gbar[r, j] dK(x1_r, x2_j)/dx1_r as a device array (smn_kernel_cnn_input_grad_cross with the
        seed as its variance seed and no diagonal term): the kernel differentiated in its first argument, contracted with
        the seed gbar [n1, n2]; mirrors KernelFn.input_grad.  x2 must be given: the form in which both arguments move is
        the seeded one of SVSP (smn_kernel_cnn_input_grad).  get_cnn_kernel only, images of at most 1024 pixels."""
        if x2 is None:
            raise NotImplementedError("input_grad needs x2: the symmetric form, in which both arguments move, is not implemented")
        shape = tuple(x1.shape) if isinstance(x1, DeviceArray) else np.shape(x1)
        if len(shape) != 4:
            raise ValueError("conv kernel expects x of shape [N,H,W,C]")
        self._check_input_grad(shape[1], shape[2])           # refused before a context is made
        ctx = self.ctx or (x1.ctx if isinstance(x1, DeviceArray) else default_context())
        a = as_device(x1, ctx)
        b = as_device(x2, ctx, dtype=a.dtype)
        if b.shape[1:] != a.shape[1:]:
            raise ValueError("x1 and x2 image shapes differ")
        g = as_device(gbar, ctx, dtype=a.dtype)
        n1, h, w, c = a.shape
        n2 = b.shape[0]
        if tuple(g.shape) != (n1, n2):
            raise ValueError("gbar must be [n1, n2] = %s, got %s" % ((n1, n2), g.shape))
        out = ctx.empty((n1, h, w, c), a.dtype)
        ctx.call("smn_kernel_cnn_input_grad_cross", a.dcode, self.act, self.num_hiddens, self.w_std, self.b_std, self.last_w_std,
                 a.ptr, n1, b.ptr, n2, h, w, c, None, 0, g.ptr, n2, None, None, out.ptr)
        return out


def get_cnn_pool_kernel(num_hiddens, num_class=1, act="relu", w_std=1., b_std=0., last_w_std=1.):
    """get_cnn_kernel with stax.GlobalAvgPool() in place of stax.Flatten() (the pooling experiments/nt_kernels.py:75 leaves
    commented out): num_hiddens x [Conv(3x3, SAME); act]; GlobalAvgPool; Dense.  Translation-aware: the read-out averages the
    covariance of every pixel of one image with every pixel of the other, (H W)^2 entries per pair and layer
    (csrc/cnn_pool.hip); H W <= 1024.  `num_class` does not enter the kernel.  NNGP only, no analytic gradients."""
    return CnnKernelFn(num_hiddens, act, w_std, b_std, last_w_std, entry="smn_kernel_cnn_pool")


def get_cnn_kernel(num_hiddens, num_class=1, act="relu", w_std=1., b_std=0., last_w_std=1.):
    """experiments/nt_kernels.py:34-45."""
    return CnnKernelFn(num_hiddens, act, w_std, b_std, last_w_std)


def get_conv_resnet_kernel(num_hiddens, num_class, act="relu", w_std=1., b_std=0., last_w_std=1.):
    """experiments/nt_kernels.py:48-80 — WideResnet(block_size=num_hiddens, k=1) without pooling; x [N,H,W,C] with H, W
    multiples of 8 (three stride-2 stages); NNGP only.  `num_class` does not enter the kernel."""
    return CnnKernelFn(num_hiddens, act, w_std, b_std, last_w_std, entry="smn_kernel_conv_resnet")
