// input_tangent.hpp — the forward-mode chain through the layer stack that differentiates an MLP / dense-ResNet kernel entry in
// its INPUTS: the arithmetic of one entry, shared by input_grad.hip (the first argument moves) and input_grad_sym.hip (both do).
//
// K(x_r, x_j) = F(u, v_r, v_j) with u = k0_rj = x_r . x_j / d and v_r = q0_r = |x_r|^2 / d.  The chain carries F_1 = dF/du and,
// per variance side, F_2 = dF/dv:  NV = 1 is the row side alone (x_j a constant: dK_rj / dx_r = (F_1 x_j + 2 F_2 x_r) / d); NV = 2
// adds the column side, for a caller whose entry (r, j) of the lower triangle serves (j, r) at once.  It is the chain grad.hip
// carries for (w^2, b^2) with other seeds: k_u = 1, k_v = 0, dq_r/dv_r = p_r (a per-row table), the column side likewise with
// p_j.  With act_r2's quantities (act_tangent.hpp: phi, D = phi_A, phi_1, phi_2, D_A, D_1, D_2; 1 = row = first argument) and t in
// {u, v, v'}:
//     Dense:       A = w2 k + b2,  A_t = w2 k_t;   NTK: T = A + w2 Theta,  T_t = A_t + w2 Theta_t
//     activation:  k <- phi(A),  k_u <- D A_u,  k_v <- D A_v + phi_1 p_r   (v': phi_2 p_j)
//                  NTK: Theta <- T D,  Theta_u <- T_u D + T D_A A_u,  Theta_v <- T_v D + T (D_A A_v + D_1 p_r)   (v': D_2 p_j)
//     last Dense:  K = lw2 k,  Theta_out = lw2 (k + Theta)
// The dense ResNet applies the same rules in the order Dense; L x {S <- Dense(act(S)) + S}; act; Dense, the Theta slots holding T
// between blocks (as in grad.hip).  Singular points follow act_r2: ReLU with (1 - c)(1 + c) <= 0 after clamping (x_r equal to
// x_j) has D_A = D_1 = D_2 = 0; a zero-variance row (ReLU, q = 0) gets ra = rb = 0 from the table kernel (ig_tables_kernel), i.e.
// c = 0, the value the stax.Relu transform takes where sqrt(q_i q_j) = 0, and no variance-side term.  Every output stays finite
// there.
#pragma once
#include "act_tangent.hpp"

// one entry's live state: (k, k_u, k_v) and, NTK, (theta, theta_u, theta_v); side 0 = row, side 1 = column
template <typename T, int NV>
struct TangentState {
  T k, ku, kv[NV], th, thu, thv[NV];
};

template <typename T, int NET, int ACT, bool NTK, int NV>
struct InputTangent {
  static_assert(NV == 1 || NV == 2, "variance-side tangents: row, or row and column");
  using State = TangentState<T, NV>;
  T w2, b2, lw2;

  // k0 = x_r . x_j / d
  __device__ __forceinline__ void init(State& s, T k0) const {
    s.k = k0;
    s.ku = T(1);
    s.th = s.thu = T(0);
#pragma unroll
    for (int v = 0; v < NV; ++v) s.kv[v] = s.thv[v] = T(0);
    if (NET == NET_RESNET) {   // the Dense in front of the first block: A, and T = A (Theta = 0)
      s.k = fma(w2, s.k, b2);
      s.ku = w2;
      s.th = s.k;
      s.thu = w2;
    }
  }

  // one activation layer with the Dense around it.  (rra, rrb) / (cra, crb): the row's / the column's table entries of the
  // layer; p[side] = dq/dq0 of that side's row; last: the stack's last activation (a ResNet leaves (k, Theta) there, too)
  __device__ __forceinline__ void step(State& s, bool last, T rra, T rrb, T cra, T crb, const T (&p)[NV]) const {
    T aa = s.k, au = s.ku, tt = s.th, tu = s.thu, av[NV], tv[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      av[v] = s.kv[v];
      tv[v] = s.thv[v];
    }
    if (NET == NET_MLP) {
      au = w2 * au;
#pragma unroll
      for (int v = 0; v < NV; ++v) av[v] = w2 * av[v];
      aa = fma(w2, aa, b2);
      if (NTK) {
        tt = fma(w2, tt, aa);
        tu = fma(w2, tu, au);
#pragma unroll
        for (int v = 0; v < NV; ++v) tv[v] = fma(w2, tv[v], av[v]);
      }
    }
    const ActR2<T> q = act_r2<ACT, T>(aa, rra, rrb, cra, crb, false);
    T o = q.o, ou = q.dA * au, ov[NV];
    T to = T(0), tou = T(0), tov[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      ov[v] = fma(q.dA, av[v], (v == 0 ? q.d1 : q.d2) * p[v]);
      tov[v] = T(0);
    }
    if (NTK) {
      const T du = q.hA * au;
      to = tt * q.dA;
      tou = fma(tu, q.dA, tt * du);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const T dv = fma(q.hA, av[v], (v == 0 ? q.h1 : q.h2) * p[v]);
        tov[v] = fma(tv[v], q.dA, tt * dv);
      }
    }
    if (NET == NET_RESNET && !last) {   // S <- Dense(act(S)) + S
      const T a2 = fma(w2, o, b2), a2u = w2 * ou;
      T a2v[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) a2v[v] = w2 * ov[v];
      o = aa + a2;
      ou = au + a2u;
#pragma unroll
      for (int v = 0; v < NV; ++v) ov[v] = av[v] + a2v[v];
      if (NTK) {
        to = tt + fma(w2, to, a2);
        tou = tu + fma(w2, tou, a2u);
#pragma unroll
        for (int v = 0; v < NV; ++v) tov[v] = tv[v] + fma(w2, tov[v], a2v[v]);
      }
    }
    s.k = o;
    s.ku = ou;
    s.th = to;
    s.thu = tou;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      s.kv[v] = ov[v];
      s.thv[v] = tov[v];
    }
  }

  // behind the last Dense (K = lw2 k, Theta_out = lw2 (k + Theta)): dF/du, and dF/dv of side v
  __device__ __forceinline__ T f1(const State& s) const { return lw2 * (NTK ? s.ku + s.thu : s.ku); }
  __device__ __forceinline__ T f2(const State& s, int v) const { return lw2 * (NTK ? s.kv[v] + s.thv[v] : s.kv[v]); }
};
