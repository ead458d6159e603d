"""fp64 NumPy rules of the pooled conv-NNGP kernel (nt_kernels.get_cnn_pool_kernel / smn_kernel_cnn_pool):

    L x [Conv(3x3, SAME, stride 1, W_std=w, b_std=b); act];  GlobalAvgPool;  Dense(last_w, b=0)

The reference has no pooled kernel (experiments/nt_kernels.py:75 leaves its AvgPool commented out), so the yardstick is this
restatement of the formulas, written from them and not from the device code.  For an image pair (n, m), p a pixel of image n
and q a pixel of image m:

    K0[p,q]  = sum_c x1[n,p,c] x2[m,q,c] / C
    K~[p,q]  = w^2/9 sum_{d in 3x3} K[p+d, q+d] + b^2          (a term is 0 when p+d or q+d is outside the image)
    K[p,q]   = act(K~[p,q]; q~_n[p], q~_m[q])                  (q~_n[p] = K~_nn[p,p]: the same-pixel recursion of cnn_kernel)
    out[n,m] = last_w^2 sum_{p,q} K_L[p,q] / (H W)^2

Two forms.  `state_6d` carries the whole [n, m, h, w, h', w'] state and applies oracle.nngp_oracle's maps to each pair's
[P, P] matrix.  `pool_kernel(form="slices")` uses that the shift d moves p and q together: for every offset D = q - p the
slice S_D[h,w] = K[(h,w), (h,w)+D] is an independent 2-D map over the rectangle where both pixels are inside, stepped by the
ordinary zero-padded 3x3 box sum (oracle._box3) of that rectangle; the activation there is written out elementwise.  In the
symmetric build (x2 None) the same-pixel entries K_nn[p,p] of a diagonal pair are the per-image variances themselves (the
oracle's _fix_diag: the generic map at c = 1 loses half the digits).
"""
import numpy as np

from oracle import nngp_oracle as O


def _q_maps(x, num_hiddens, act, w_std, b_std):
    """Per image: pre-activation variances q~_l [L, N, H, W] and the variance after the last activation [N, H, W]."""
    q = np.einsum("nhwc,nhwc->nhw", x, x) / x.shape[-1]
    pre = []
    for _ in range(num_hiddens):
        qt = w_std ** 2 * O._box3(q) / 9.0 + b_std ** 2
        pre.append(qt)
        q = qt / 2.0 if act == "relu" else (2.0 / np.pi) * np.arcsin(2.0 * qt / (1.0 + 2.0 * qt))
    return pre, q


def _box3_pairs(k):
    """sum_d K[p+d, q+d] over the 3x3 shifts, zero outside either image; k [..., H, W, H, W]."""
    h, w = k.shape[-2:]
    p = np.pad(k, [(0, 0)] * (k.ndim - 4) + [(1, 1)] * 4)
    out = np.zeros_like(k)
    for dh in range(3):
        for dw in range(3):
            out += p[..., dh:dh + h, dw:dw + w, dh:dh + h, dw:dw + w]
    return out


def state_6d(x1, x2=None, num_hiddens=1, act="relu", w_std=1.0, b_std=0.0):
    """K_L [n, m, H, W, H, W] by brute force, the activation through the oracle's own maps on each pair's [P, P] matrix."""
    x1 = np.asarray(x1, dtype=np.float64)
    sym = x2 is None
    x2 = x1 if sym else np.asarray(x2, dtype=np.float64)
    amap = O.get_act(act)
    n1, h, w, c = x1.shape
    n2, pix = x2.shape[0], h * w
    k = np.einsum("nhwc,mijc->nmhwij", x1, x2) / c
    pre1, _ = _q_maps(x1, num_hiddens, act, w_std, b_std)
    pre2, _ = _q_maps(x2, num_hiddens, act, w_std, b_std)
    for l in range(num_hiddens):
        k = w_std ** 2 * _box3_pairs(k) / 9.0 + b_std ** 2
        new = np.empty_like(k)
        for n in range(n1):
            for m in range(n2):
                q1, q2 = pre1[l][n].reshape(pix), pre2[l][m].reshape(pix)
                kp = k[n, m].reshape(pix, pix).copy()
                if sym and n == m:
                    np.fill_diagonal(kp, q1)
                kn, q1n, _, _ = amap(kp, q1, q2)
                if sym and n == m:
                    np.fill_diagonal(kn, q1n)
                new[n, m] = kn.reshape(h, w, h, w)
        k = new
    return k


def _act_el(act, kt, qa, qb):
    """The activation elementwise: kt, qa, qb broadcast against each other."""
    if act == "relu":
        sp = np.sqrt(qa * qb)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(sp > 0, kt / sp, 0.0)
        c = np.clip(c, -1.0, 1.0)
        return sp * (np.sqrt(np.maximum((1.0 - c) * (1.0 + c), 0.0)) + (np.pi - np.arccos(c)) * c) / (2.0 * np.pi)
    if act == "erf":
        c = np.clip(2.0 * kt / np.sqrt((1.0 + 2.0 * qa) * (1.0 + 2.0 * qb)), -1.0, 1.0)
        return (2.0 / np.pi) * np.arcsin(c)
    raise KeyError("Unsupported act '{}'".format(act))


def _pool_slices(x1, x2, sym, num_hiddens, act, w_std, b_std):
    n1, h, w, c = x1.shape
    n2 = x2.shape[0]
    pre1, post1 = _q_maps(x1, num_hiddens, act, w_std, b_std)
    pre2, _ = _q_maps(x2, num_hiddens, act, w_std, b_std)
    idx = np.arange(n1)
    total = np.zeros((n1, n2))
    for dh in range(-h + 1, h):
        for dw in range(-w + 1, w):
            h0, h1, w0, w1 = max(0, -dh), min(h, h - dh), max(0, -dw), min(w, w - dw)   # the rectangle of p; q = p + (dh, dw)
            a = x1[:, h0:h1, w0:w1]
            b = x2[:, h0 + dh:h1 + dh, w0 + dw:w1 + dw]
            s = np.einsum("nhwc,mhwc->nmhw", a, b) / c
            for l in range(num_hiddens):
                s = w_std ** 2 * O._box3(s) / 9.0 + b_std ** 2
                qa = pre1[l][:, None, h0:h1, w0:w1]
                qb = pre2[l][None, :, h0 + dh:h1 + dh, w0 + dw:w1 + dw]
                s = _act_el(act, s, qa, qb)
                if sym and dh == 0 and dw == 0:   # K_nn[p,p] is the per-image variance
                    q = pre1[l] / 2.0 if act == "relu" else (2.0 / np.pi) * np.arcsin(2.0 * pre1[l] / (1.0 + 2.0 * pre1[l]))
                    s[idx, idx] = q
            total += s.sum(axis=(2, 3))
    return total


def pool_kernel(x1, x2=None, num_hiddens=1, act="relu", w_std=1.0, b_std=0.0, last_w_std=1.0, form="slices"):
    """out [n1, n2] in fp64; form "slices" (every offset's 2-D map) or "6d" (brute force, tiny shapes only)."""
    x1 = np.asarray(x1, dtype=np.float64)
    if x1.ndim != 4:
        raise ValueError("pool_kernel expects x of shape [N,H,W,C]")
    sym = x2 is None
    x2 = x1 if sym else np.asarray(x2, dtype=np.float64)
    pix = x1.shape[1] * x1.shape[2]
    if form == "6d":
        total = state_6d(x1, None if sym else x2, num_hiddens, act, w_std, b_std).sum(axis=(2, 3, 4, 5))
    elif form == "slices":
        total = _pool_slices(x1, x2, sym, num_hiddens, act, w_std, b_std)
    else:
        raise ValueError("form must be 'slices' or '6d'")
    return last_w_std ** 2 * total / float(pix) ** 2
