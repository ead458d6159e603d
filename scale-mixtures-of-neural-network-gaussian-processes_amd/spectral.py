"""Spectrum of a symmetric positive definite matrix on the device (smn_eigh_pd) and what neural_tangents derives from it.

    w, v = eigh_pd(a)                      a = v @ diag(w) @ v.T, w ascending          (jnp.linalg.eigh)
    lr   = max_learning_rate(g_dd, y_size) neural_tangents.predict.max_learning_rate
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import as_device, default_context

__all__ = ["eigh_pd", "max_learning_rate"]


class EighResult(tuple):
    """(w, v) plus `info` (0 converged, k > 0 not positive definite at pivot k, -1 not converged) and `sweeps`."""
    info = 0
    sweeps = 0


def eigh_pd(a, ctx=None, max_sweeps=0):
    """Eigenvalues (ascending) and eigenvectors (columns of v) of the symmetric positive definite matrix `a` (its lower
    triangle is read).  NumPy arrays out; a matrix that is not positive definite gives NaN and info > 0, as a failed
    factorisation does everywhere in this package."""
    ad = as_device(a, ctx or (getattr(a, "ctx", None) or default_context()))
    ctx = ad.ctx
    if len(ad.shape) != 2 or ad.shape[0] != ad.shape[1] or ad.shape[0] == 0:
        raise ValueError("eigh_pd expects a non-empty square matrix, got shape %s" % (ad.shape,))
    n = ad.shape[0]
    w, v = ctx.empty((n,), ad.dtype), ctx.empty((n, n), ad.dtype)
    info, sweeps = C.c_int(), C.c_int()
    ctx.call("smn_eigh_pd", ad.dcode, ad.ptr, n, n, w.ptr, v.ptr, n, int(max_sweeps), C.byref(info), C.byref(sweeps))
    res = EighResult((w.numpy(), v.numpy()))
    res.info, res.sweeps = info.value, sweeps.value
    return res


def max_learning_rate(g_dd, y_size, momentum=0.0, eps=1e-12, ctx=None):
    """2 (1 + momentum) y_size / (lambda_max + eps): the largest stable step of (momentum) gradient descent on the MSE loss
    of the linearised network whose train-train kernel is g_dd.  A 1-D argument is taken as the eigenvalues themselves
    (PredictResult.evals); a matrix goes through eigh_pd."""
    g = g_dd if hasattr(g_dd, "shape") else np.asarray(g_dd)
    lam = np.asarray(g, dtype=np.float64) if len(g.shape) == 1 else np.asarray(eigh_pd(g_dd, ctx)[0], dtype=np.float64)
    return 2.0 * (1.0 + float(momentum)) * float(y_size) / (float(lam.max()) + float(eps))
