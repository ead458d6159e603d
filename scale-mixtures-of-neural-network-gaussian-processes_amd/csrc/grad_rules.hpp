// grad_rules.hpp — the forward-mode rules in (w^2, b^2) that the hyper-parameter gradients share (grad.hip: the symmetric
// contraction over X X^T / d; lowrank_grad.hip: the rectangular one over X Z^T / d): the activation maps with their first
// derivatives, in fp64 with libm (the diagonal's own chain) and per element in the arithmetic of the storage type, and the per-row
// tables the per-element form reads.
//
// Forward-mode rules (SURVEY.md Appendix A.1/A.2 differentiated; q_i, q_j = variances entering the map):
//   Dense:  A = w2 K + b2           dA/dw2 = K + w2 dK/dw2          dA/db2 = 1 + w2 dK/db2
//   ReLU:   phi   = sqrt(q_i q_j)/(2 pi) * (sqrt(1-c^2) + (pi - acos c) c),   c = A / sqrt(q_i q_j)
//           phi_A = (pi - acos c)/(2 pi)        phi_qi = sqrt(1-c^2) sqrt(q_i q_j) / (4 pi q_i)
//   Erf:    phi   = (2/pi) asin s,   s = 2A / sqrt(P),  P = (1+2q_i)(1+2q_j)
//           phi_A = 4 / (pi sqrt(P) sqrt(1-s^2))     phi_qi = -(2/pi) s / (sqrt(1-s^2) (1+2q_i))
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "act_tangent.hpp"
#include "layer_prog.hpp"
#include "nngp_math.hpp"

namespace grad_rules {

struct ActD {
  double o, dA, d1, d2;
};

template <int ACT>
__device__ __forceinline__ ActD act_d(double a, double qi, double qj) {
  ActD r;
  if (ACT == ACT_RELU) {
    const double sp = sqrt(qi * qj);
    double c = a / sp;
    c = fmin(fmax(c, -1.0), 1.0);
    const double s1 = sqrt(fmax(1.0 - c * c, 0.0));
    const double pm = kPiD - acos(c);
    r.o = sp * (s1 + pm * c) * (1.0 / (2.0 * kPiD));
    r.dA = pm * (1.0 / (2.0 * kPiD));
    r.d1 = s1 * sp / (4.0 * kPiD * qi);
    r.d2 = s1 * sp / (4.0 * kPiD * qj);
  } else {
    const double ti = 1.0 + 2.0 * qi, tj = 1.0 + 2.0 * qj;
    const double sP = sqrt(ti * tj);
    double s = 2.0 * a / sP;
    s = fmin(fmax(s, -1.0), 1.0);
    const double den = sqrt(fmax(1.0 - s * s, 1e-300));
    r.o = (2.0 / kPiD) * asin(s);
    r.dA = 4.0 / (kPiD * sP * den);
    r.d1 = -(2.0 / kPiD) * s / (den * ti);
    r.d2 = -(2.0 / kPiD) * s / (den * tj);
  }
  return r;
}

// The same maps per ELEMENT, in the arithmetic R of the storage type (float for f32 matrices: the Gram entries and
// -K~^-1 carry f32 rounding already, fp64 arithmetic on them recovers nothing; double for f64), division-free from per-row
// tables and with the branch-free asin of the forward kernels (nngp_math.hpp) instead of libm's acos:
//   ReLU: ra = 1/sqrt(q), rb = sqrt(q):   c = A ra_i ra_j,  pi - acos c = pi/2 + asin c,  sp = rb_i rb_j,
//         phi_qi = sqrt(1-c^2) sp / (4 pi q_i) = sqrt(1-c^2)/(4 pi) * rb_j ra_i
//   Erf:  ra = 1/sqrt(1+2q), rb = ra^2:   s = 2 A ra_i ra_j,  phi_A = (4/pi) ra_i ra_j / sqrt(1-s^2),
//         phi_qi = -(2/pi) s rb_i / sqrt(1-s^2)
template <typename R>
struct ActR {
  R o, dA, d1, d2;
};

template <int ACT, typename R>
__device__ __forceinline__ ActR<R> act_r(R a, R rai, R rbi, R raj, R rbj) {
  ActR<R> r;
  if (ACT == ACT_RELU) {
    const R c = nngp::clamp1(a * (rai * raj));
    const R as = nngp::asin_abs(fabs(c), c * c);
    const R s1 = nngp::fast_sqrt(fmax(fma(-c, c, R(1)), R(0)));
    const R pm = R(kPiD / 2) + copysign(as, c);
    const R sp = rbi * rbj;
    r.o = sp * fma(pm, c, s1) * R(1.0 / (2.0 * kPiD));
    r.dA = pm * R(1.0 / (2.0 * kPiD));
    const R t = s1 * R(1.0 / (4.0 * kPiD));
    r.d1 = t * (rbj * rai);
    r.d2 = t * (rbi * raj);
  } else {
    const R uu = rai * raj;
    const R sv = nngp::clamp1(R(2) * a * uu);
    const R as = nngp::asin_abs(fabs(sv), sv * sv);
    const R rden = nngp::fast_rsqrt(fmax(fma(-sv, sv, R(1)), sizeof(R) == 8 ? R(1e-300) : R(1e-30)));
    r.o = R(2.0 / kPiD) * copysign(as, sv);
    r.dA = R(4.0 / kPiD) * uu * rden;
    const R t = R(-2.0 / kPiD) * sv * rden;
    r.d1 = t * rbi;
    r.d2 = t * rbj;
  }
  return r;
}

constexpr int kGradTabFields = 5;   // per activation layer and row: q, dq/dw2, dq/db2, ra, rb

// (K_ii, dK_ii/dw2, dK_ii/db2) behind the last activation layer, in front of last_w_std^2: what grad_tables_row's chain ends on
struct DiagEnd {
  double k, dw, db;
};

// Diagonal of the same recursion (fp64 arithmetic): variance entering each activation, its derivatives and the two
// per-row factors of act_r.  tab[(s*5 + f)*n + i], f = 0: q, 1: dq/dw2, 2: dq/db2, 3: ra, 4: rb.
template <int NET, int ACT, typename R>
__device__ __forceinline__ DiagEnd grad_tables_row(const double* __restrict__ q0, int64_t n, int nsets, double w2, double b2,
                                                   R* __restrict__ tab, int64_t i) {
  double q = q0[i], dw = 0.0, db = 0.0;
  if (NET == NET_RESNET) {
    dw = q;
    db = 1.0;
    q = w2 * q + b2;
  }
  for (int s = 0; s < nsets; ++s) {
    if (NET == NET_MLP) {   // Dense in front of every activation
      const double qa = w2 * q + b2;
      dw = q + w2 * dw;
      db = 1.0 + w2 * db;
      q = qa;
    }
    R* t = tab + (int64_t)s * kGradTabFields * n + i;
    t[0] = (R)q;
    t[n] = (R)dw;
    t[2 * n] = (R)db;
    // a row of zero variance (an all-zero input row under b_std == 0) under ReLU: the map is not differentiable there.  ra = 0
    // beside rb = 0 gives the tile code c = 0, sp = 0 and zero variance-side factors without a branch in its loop (1 / sqrt(0)
    // would give it 0 * inf), and the row's own chain stays at phi(q, q, q) = q / 2 = 0 with slope 1/2 instead of act_d's 0 / 0
    const bool dead = ACT == ACT_RELU && q == 0.0;
    if (ACT == ACT_RELU) {
      t[3 * n] = dead ? R(0) : (R)(1.0 / sqrt(q));
      t[4 * n] = (R)sqrt(q);
    } else {
      t[3 * n] = (R)(1.0 / sqrt(1.0 + 2.0 * q));
      t[4 * n] = (R)(1.0 / (1.0 + 2.0 * q));
    }
    ActD r{0.0, 0.5, 0.0, 0.0};
    if (!dead) r = act_d<ACT>(q, q, q);           // on the diagonal A = q_i = q_j
    const double dq = r.dA + r.d1 + r.d2;
    double o = r.o, ow = dq * dw, ob = dq * db;
    if (NET == NET_RESNET && s != nsets - 1) {    // K <- [Dense o act](K) + K
      const double ka = w2 * o + b2;
      const double kw = o + w2 * ow, kb = 1.0 + w2 * ob;
      o = q + ka;
      ow = dw + kw;
      ob = db + kb;
    }
    q = o; dw = ow; db = ob;
  }
  return DiagEnd{q, dw, db};
}

}  // namespace grad_rules
