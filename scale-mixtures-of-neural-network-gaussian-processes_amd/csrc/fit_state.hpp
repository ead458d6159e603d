// fit_state.hpp — the fitted posterior's state (smn_fit), shared by fit.hip (create, predict, append) and fit_remove.hip.
#pragma once
#include "internal.hpp"

struct smn_fit {
  smn_ctx* ctx = nullptr;
  int dtype = 0, net = 0, act = 0, num_hiddens = 0;
  bool ntk = false, fused = false;
  double w_std = 0.0, b_std = 0.0, last_w_std = 0.0;
  int64_t n = 0, n_pad = 0, c = 0, capacity = 0, cap_pad = 0, n_total = 0, lda = 0, d = 0, kp = 0;
  void* a = nullptr;    // [n_total, lda]
  void* xs = nullptr;   // fused form: q [n_pad] doubles, then the padded x [n_pad, kp]
  // made by the first smn_fit_predict_grad call: L' = J L^T J with cap_pad appended rows [n_pad + cap_pad, n_pad], alpha^T
  // [c, n_pad] and X^T [round_up(d, 128), n_pad]
  void* lt = nullptr; void* alpha = nullptr; void* xt = nullptr;
  bool grad_ready = false;
  size_t bytes = 0;
  int info = 0;
  // what smn_fit_append carries forward: the absolute ridge lambda the factor was made with (frozen at creation) and the
  // running totals y_k^T K~^-1 y_k, log det K~
  double ridge = 0.0, quad[48] = {}, logdet = 0.0;
  size_t es() const { return dtype_size(dtype); }
  char* at(int64_t r, int64_t col) const { return static_cast<char*>(a) + es() * (size_t)(r * lda + col); }
  double* q() const { return static_cast<double*>(xs); }
  char* xp() const { return reinterpret_cast<char*>(q() + n_pad); }
  char* lt_at(int64_t r) const { return static_cast<char*>(lt) + es() * (size_t)(r * n_pad); }
  int64_t beta_row() const { return n_pad + cap_pad; }
};
