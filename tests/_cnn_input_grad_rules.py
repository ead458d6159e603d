"""NumPy fp64 restatement of the reverse-mode rules of csrc/cnn_input_grad.hip (shared by test_cnn_input_grad_host.py and
test_gpu_cnn_input_grad.py; not a test module): gx_i = sum_ab g_ab dK_ab/dx_i of the conv-NNGP kernel for a symmetric g.

Notation of _cnn_grad_rules.py (box = 3x3 zero-padded box sum, self-adjoint).  Forward, per layer l = 1..L:
    pair (n, m):  kt_l = w^2 box(k_{l-1})/9 + b^2,  k_l = phi(kt_l, qt_l^n, qt_l^m);     k_0 = x_n.x_m / C
    image:        qt_l = w^2 box(q_{l-1})/9 + b^2,  q_l = phi_diag(qt_l);                q_0 = |x|^2 / C
    K_nm = lw^2 mean k_L,  K_nn = lw^2 mean q_L (the exact diagonal).
Pair pass, n != m:   kbar_L = 2 g_nm lw^2 / HW;  for l = L..1: qtbar_n^l += phi_qi(l) kbar_l, kbar_{l-1} = w^2 box(phi_A(l) kbar_l)/9;
                     gx_n += kbar_0 x_m / C.     (the partner's variance-side term belongs to the visit from its side)
Per-image pass:      r = g_nn lw^2 / HW;  for l = L..1: r = w^2 box(dq_l r + qtbar^l)/9;  gx += 2 x r / C.
"""
import numpy as np

from _cnn_grad_rules import act_d, box3


def _diag_chain(x, layers, act, w2, b2):
    """Per image and layer: the pre-activation variance qt_l and dq_l = d phi_diag / d qt_l, each [L][n,H,W]."""
    q = np.einsum("nhwc,nhwc->nhw", x, x) / x.shape[-1]
    qts, dqs = [], []
    for _ in range(layers):
        qt = w2 * box3(q) / 9.0 + b2
        if act == "relu":
            dq, q = np.full_like(qt, 0.5), qt / 2.0
        else:
            dq = (4 / np.pi) / ((1.0 + 2.0 * qt) * np.sqrt(1.0 + 4.0 * qt))
            q = (2 / np.pi) * np.arcsin(2.0 * qt / (1.0 + 2.0 * qt))
        qts.append(qt)
        dqs.append(dq)
    return qts, dqs


def input_grad(g, x, layers, act, w_std, b_std, last_w_std, n_grad=None):
    """(gx, S), each [n_grad,H,W,C]: gx_i = sum_ab g_ab dK_ab/dx_i for the first n_grad images (default: all), g taken as
    symmetric from its lower triangle; S is the same sum over the absolute values of every term (|g|, |phi| factors, |x|): the
    scale a rounding-error bound has to be relative to, since the terms of the sum may cancel."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    g = np.tril(g) + np.tril(g, -1).T
    n, h, w, c = x.shape
    ng = n if n_grad is None else int(n_grad)
    w2, b2, lw2 = w_std ** 2, b_std ** 2, last_w_std ** 2
    qts, dqs = _diag_chain(x, layers, act, w2, b2)
    k = np.einsum("nhwc,mhwc->nmhw", x[:ng], x) / c
    das, d1s = [], []
    for l in range(layers):
        kt = w2 * box3(k) / 9.0 + b2
        k, da, d1, _ = act_d(kt, qts[l][:ng][:, None], qts[l][None, :], act)
        das.append(da)
        d1s.append(d1)
    off = (np.arange(ng)[:, None] != np.arange(n)[None, :]).astype(np.float64)[:, :, None, None]
    kb = 2.0 * g[:ng, :, None, None] * lw2 / (h * w) * off * np.ones((1, 1, h, w))
    ka = np.abs(kb)
    qbar, qabs = [None] * layers, [None] * layers
    for l in range(layers - 1, -1, -1):
        qbar[l] = np.sum(d1s[l] * kb, axis=1)
        qabs[l] = np.sum(np.abs(d1s[l]) * ka, axis=1)
        kb = w2 * box3(das[l] * kb) / 9.0
        ka = w2 * box3(np.abs(das[l]) * ka) / 9.0
    gx = np.einsum("nmhw,mhwc->nhwc", kb, x) / c
    s = np.einsum("nmhw,mhwc->nhwc", ka, np.abs(x)) / c
    gd = np.diag(g)[:ng]
    r = gd[:, None, None] * lw2 / (h * w) * np.ones((1, h, w))
    ra = np.abs(r)
    for l in range(layers - 1, -1, -1):
        r = w2 * box3(dqs[l][:ng] * r + qbar[l]) / 9.0
        ra = w2 * box3(np.abs(dqs[l][:ng]) * ra + qabs[l]) / 9.0
    gx += 2.0 * x[:ng] * r[..., None] / c
    s += 2.0 * np.abs(x[:ng]) * ra[..., None] / c
    return gx, s
