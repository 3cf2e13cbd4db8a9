// The per-voxel gradient of the partial-label soft Dice + per-class BCE on softmax probabilities (reference
// loss_partial.py:59-99, DiceLoss :10-57), shared by loss_bwd_kernel (loss.hip) and the head backward that forms it in
// registers (head_loss_bwd_kernel, head.hip): one definition, so both produce the same bits.
#pragma once
#include "common.h"

// dispatch on the class count: exact instantiations for the model heads, a guarded 32-wide fallback
#define U3D_NC_DISPATCH(C, F)        \
  switch (C) {                       \
    case 2: F(2); break;             \
    case 8: F(8); break;             \
    case 14: F(14); break;           \
    case 16: F(16); break;           \
    default: F(32); break;           \
  }

namespace u3d {

constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

// Softmax path on the hardware transcendentals (v_exp_f32 / v_log_f32 / v_rcp_f32, ~1 ulp): e_c = 2^((x_c-m)
// log2 e), p_c = e_c / s, and the two logs BCE needs are exact identities of the softmax instead of log(p):
//   log p_c = (x_c - m) - ln s,   log(1 - p_c) = ln(s - e_c) - ln s.
// The loss was transcendental-bound with libm expf/logf/log1pf (48 calls per voxel at C = 16).
// Shared by loss.hip and deepsup.hip (the deep-supervision levels take the same softmax).
template <int NC>
__device__ __forceinline__ void softmax_fast(const float* __restrict__ lg, int C, float (&x)[NC], float (&e)[NC],
                                             float& s, float& inv) {
  if constexpr (NC % 4 == 0 && NC <= 16) {
#pragma unroll
    for (int c = 0; c < NC; c += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lg + c);
      x[c] = v[0]; x[c + 1] = v[1]; x[c + 2] = v[2]; x[c + 3] = v[3];
    }
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c) x[c] = c < C ? lg[c] : 0.f;
  }
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < C) m = fmaxf(m, x[c]);
  s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    x[c] -= m;
    e[c] = c < C ? __builtin_amdgcn_exp2f(x[c] * LOG2E) : 0.f;
    s += e[c];
  }
  inv = __builtin_amdgcn_rcpf(s);
}

// per-class coefficients: dL/dp_c = t_c * a + p_c * b (+ the BCE term e * (p_c - t_c) / ((1 - p_c) p_c))
//   d(1 - num/den)/dp = -(2 t den - num * 2 p) / den^2, num = 2 I + 1e-5, den = Z + Y + 1e-5 (per class sums)
__device__ __forceinline__ void dice_bce_coefs(int c, int C, const double* __restrict__ sums,
                                               const float* __restrict__ wt, const float* __restrict__ gout, int uce,
                                               double count, float& a, float& b, float& e) {
  a = b = e = 0.f;
  if (c < C) {
    const double I = sums[c * 4], Z = sums[c * 4 + 1], Y = sums[c * 4 + 2];
    const double num = 2.0 * I + 1e-5, den = Z + Y + 1e-5;
    const double scale = (double)wt[c] / C * gout[0];
    a = (float)(-2.0 / den * scale);
    b = (float)(2.0 * num / (den * den) * scale);
    e = uce == 1 ? (float)((double)wt[c] / count * gout[0]) : uce == 2 ? (float)(1.0 / count * gout[0]) : 0.f;
  }
}

// Per-sample supervision (loss_ps.hip, the _ps kernels of deepsup.hip). w [S][C]: sample s supervises class c when
// w[s][c] != 0; pooled[c] = (I, Z, Y, B, n_c) = the per-sample sums added over the n_c supervising samples.
// ps_class_weight: w^_c = sum_s w[s][c] / n_c in fp64, s ascending (0 when nobody supervises the class): the one
// definition the forward's final kernel and every backward block use, so both see the same bits.
__device__ __forceinline__ double ps_class_weight(int c, int S, int C, const float* __restrict__ w, double n) {
  double sw = 0;
  for (int s = 0; s < S; ++s) sw += (double)w[(long long)s * C + c];
  return n > 0 ? sw / n : 0.0;
}

// dice_bce_coefs for sample s: a, b from the pooled sums with w^_c, e = w^_c / (n_c V) * g (uce 1: the BCE mean runs
// over the supervising samples' voxels only); all three 0 where the sample does not supervise the class. Every load
// is issued before the sample's own weight is looked at (one memory latency per block, not two: a backward block
// covers few voxels, and its prologue is on its critical path).
__device__ __forceinline__ void dice_bce_coefs_ps(int c, int s, int S, int C, const double* __restrict__ pooled,
                                                  const float* __restrict__ w, const float* __restrict__ gout, int uce,
                                                  double V, float& a, float& b, float& e) {
  a = b = e = 0.f;
  if (c < C) {
    const float wsc = w[(long long)s * C + c], g = gout[0];
    const double I = pooled[c * 5], Z = pooled[c * 5 + 1], Y = pooled[c * 5 + 2], n = pooled[c * 5 + 4];
    const double wh = ps_class_weight(c, S, C, w, n);
    const double num = 2.0 * I + 1e-5, den = Z + Y + 1e-5;
    const double scale = wh / C * g;
    const bool sup = wsc != 0.f;  // then n >= 1
    a = sup ? (float)(-2.0 / den * scale) : 0.f;
    b = sup ? (float)(2.0 * num / (den * den) * scale) : 0.f;
    e = sup && uce == 1 ? (float)(wh / (n * V) * g) : 0.f;
  }
}

// dL/dlogits of one voxel, 16 classes, softmax + per-class BCE (uce 1): the logits in x4 (4 x 16 B), its label t,
// the coefficient tables (LDS) -> r[16]. Softmax on the hardware exp2 / rcp (~1 ulp), as the forward. The sums over
// the classes run as two halves (classes 0-7, 8-15) added at the end — the order dice_bce_softmax_grad8 reproduces
// with each half in one lane of a lane pair (fp addition commutes, max is exact).
__device__ __forceinline__ void dice_bce_softmax_grad16(const f32x4 (&x4)[4], float t, const float* kd_a,
                                                        const float* kd_b, const float* kb, float (&r)[16]) {
  constexpr float kLog2e = 1.4426950408889634f;
  float x[16], p[16];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) x[4 * k + j] = x4[k][j];
  float m = x[0];
#pragma unroll
  for (int c = 1; c < 16; ++c) m = fmaxf(m, x[c]);
  float sh[2] = {0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    p[c] = __builtin_amdgcn_exp2f((x[c] - m) * kLog2e);
    sh[c >> 3] += p[c];
  }
  const float inv = __builtin_amdgcn_rcpf(sh[0] + sh[1]);
#pragma unroll
  for (int c = 0; c < 16; ++c) p[c] *= inv;
  float g[16], dh[2] = {0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const float tc = (t == (float)c) ? 1.f : 0.f;
    float gc = fmaf(tc, kd_a[c], p[c] * kd_b[c]);
    gc += kb[c] * (p[c] - tc) * __builtin_amdgcn_rcpf(fmaxf((1.f - p[c]) * p[c], 1e-12f));
    g[c] = gc;
    dh[c >> 3] = fmaf(gc, p[c], dh[c >> 3]);
  }
  const float dot = dh[0] + dh[1];
#pragma unroll
  for (int c = 0; c < 16; ++c) r[c] = p[c] * (g[c] - dot);
}

// The same gradient with the voxel's classes split over a lane pair (lanes i, i ^ 32 of a wave): this lane holds
// classes 8h .. 8h+7 in x4 and gets r for them; the max, the softmax sum and the dot product are exchanged once each.
// Bitwise dice_bce_softmax_grad16's values for those classes.
__device__ __forceinline__ void dice_bce_softmax_grad8(const f32x4 (&x4)[2], float t, int h, const float* kd_a,
                                                       const float* kd_b, const float* kb, float (&r)[8]) {
  constexpr float kLog2e = 1.4426950408889634f;
  float x[8], p[8];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) x[4 * k + j] = x4[k][j];
  float m = x[0];
#pragma unroll
  for (int c = 1; c < 8; ++c) m = fmaxf(m, x[c]);
  m = fmaxf(m, __shfl_xor(m, 32));
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    p[c] = __builtin_amdgcn_exp2f((x[c] - m) * kLog2e);
    s += p[c];
  }
  const float inv = __builtin_amdgcn_rcpf(s + __shfl_xor(s, 32));
#pragma unroll
  for (int c = 0; c < 8; ++c) p[c] *= inv;
  float g[8], d = 0.f;
  const int c0 = 8 * h;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float tc = (t == (float)(c0 + c)) ? 1.f : 0.f;
    float gc = fmaf(tc, kd_a[c0 + c], p[c] * kd_b[c0 + c]);
    gc += kb[c0 + c] * (p[c] - tc) * __builtin_amdgcn_rcpf(fmaxf((1.f - p[c]) * p[c], 1e-12f));
    g[c] = gc;
    d = fmaf(gc, p[c], d);
  }
  const float dot = d + __shfl_xor(d, 32);
#pragma unroll
  for (int c = 0; c < 8; ++c) r[c] = p[c] * (g[c] - dot);
}

}  // namespace u3d
