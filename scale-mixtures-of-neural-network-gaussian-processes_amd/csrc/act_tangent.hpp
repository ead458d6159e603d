// act_tangent.hpp — the activation maps with their first and second derivatives, per element and division-free from per-row
// tables: what a forward-mode chain through the layer stack needs (grad.hip: tangents in (w^2, b^2); input_grad.hip: tangents
// in the first argument's (k0, q0)).
#pragma once
#include <hip/hip_runtime.h>

#include "layer_prog.hpp"
#include "nngp_math.hpp"

constexpr double kPiD = 3.14159265358979323846;

// NTK form: the same maps with the second derivatives of the activation map that the tangent of Theta needs.  D = phi_A is the
// factor Theta takes per layer (Theta <- T D, T = A + w2 Theta), so  dD = D_A dA + D_1 dq_i + D_2 dq_j:
//   ReLU: D_A = 1 / (2 pi sqrt(1-c^2) sqrt(q_i q_j)) = ra_i ra_j / (2 pi sqrt(1-c^2)),   D_i = -c / (4 pi q_i sqrt(1-c^2))
//         = -c ra_i^2 / (4 pi sqrt(1-c^2)).  Where (1-c)(1+c) <= 0 after clamping -- and on the exact diagonal -- D is 1/2
//         whatever the hyper-parameters (c = 1 identically: the diagonal, exactly duplicate rows): D_A = D_i = 0.
//   Erf:  R = (1+2q_i)(1+2q_j) - 4A^2 = (1-s^2) / (ra_i ra_j)^2 >= 1 + 4q:   D_A = 16 A / (pi R^(3/2)) = (16/pi) A (uu rden)^3,
//         D_i = -4 (1+2q_j) / (pi R^(3/2)) = -(4/pi) uu rb_i rden^3,   uu = ra_i ra_j, rden = 1/sqrt(1-s^2).
// Division-free from the same per-row fields as act_r.
template <typename R>
struct ActR2 {
  R o, dA, d1, d2, hA, h1, h2;
};

template <int ACT, typename R>
__device__ __forceinline__ ActR2<R> act_r2(R a, R rai, R rbi, R raj, R rbj, bool diag) {
  ActR2<R> r;
  if (ACT == ACT_RELU) {
    const R uu = rai * raj;
    // the diagonal: c = 1 exactly (q ra^2 is 1 only to rounding, and asin has no slope to spare there: 1e-16 in c is 1e-8 in D)
    const R c = diag ? R(1) : nngp::clamp1(a * uu);
    const R as = nngp::asin_abs(fabs(c), c * c);
    const R om = (R(1) - c) * (R(1) + c);
    const bool flat = diag || !(om > R(0));
    const R s1 = nngp::fast_sqrt(fmax(om, R(0)));
    const R rs1 = flat ? R(0) : nngp::fast_rsqrt(flat ? R(1) : om);
    const R pm = R(kPiD / 2) + copysign(as, c);
    const R sp = rbi * rbj;
    r.o = sp * fma(pm, c, s1) * R(1.0 / (2.0 * kPiD));
    r.dA = pm * R(1.0 / (2.0 * kPiD));
    const R t = s1 * R(1.0 / (4.0 * kPiD));
    r.d1 = t * (rbj * rai);
    r.d2 = t * (rbi * raj);
    r.hA = R(1.0 / (2.0 * kPiD)) * rs1 * uu;
    const R u = R(-1.0 / (4.0 * kPiD)) * c * rs1;
    r.h1 = u * (rai * rai);
    r.h2 = u * (raj * raj);
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
    const R ur = uu * rden, r2 = rden * rden;
    r.hA = R(16.0 / kPiD) * a * (ur * ur * ur);
    const R v = R(-4.0 / kPiD) * ur * r2;
    r.h1 = v * rbi;
    r.h2 = v * rbj;
  }
  return r;
}
