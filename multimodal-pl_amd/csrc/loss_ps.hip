// Partial-label soft Dice + per-class BCE with one supervision row per sample (DESIGN.md "Per-sample supervision").
// loss.hip weights the whole batch with one row (the reference's mask[0], loss_partial.py:87); here w is [S][C] and
// sample s enters class c's sums only when w[s][c] != 0:
//   n_c = #{s: w_sc != 0},  w^_c = sum_s w_sc / n_c,  X_c = sum_{s: w_sc != 0} X_sc for X in (I, Z, Y, B)
//   loss = sum_c w^_c d_c / C + [uce] sum_{c: n_c > 0} w^_c B_c / (n_c V),  d_c = 1 - (2 I_c + 1e-5) / (Z_c + Y_c + 1e-5)
// With equal rows this is loss.hip's loss with that row. uce 2 (cross entropy, unweighted) has no per-sample form.
//
// Forward: one pass over the logits on a 2-D grid, the sample on blockIdx.y (no block straddles two samples);
// per-(sample, block) fp32 partials to fixed workspace slots, added per sample in fp64 in fixed order (sums_ps), then
// one small kernel pools them over the supervising samples (s ascending) and forms the scalar loss on the device.
// No float atomics, no host read, no state kept between launches. Backward: one elementwise pass on the same grid;
// each block builds its own sample's coefficient table (loss_grad.h) and a block whose sample supervises nothing
// writes zeros without reading the logits.
#include "common.h"
#include "loss_grad.h"

namespace u3d {

constexpr int PT = 256;
constexpr int PS_CMAX = 32;
constexpr int PS_MAXS = 65535;    // gridDim.y
constexpr int PS_FWD_NB = 512;    // forward blocks over all samples at most: two per CU resident (loss.hip's U3D_LOSS_NB)
constexpr int PS_PAIR_NB = 1280;  // the same for the lane-pair forward (loss.hip's LP_NB), 128 voxels per block
// Backward blocks over all samples at most: four 4-wave blocks per CU, all resident, each thread taking several voxels
// through the pipelined loop, so the block prologue (the sample's row, a barrier, the coefficient table) is paid once
// per 6.75 voxels at 2 x 96^3 and not once per voxel as with loss.hip's 8192. 2 x 96^3 x 16, softmax + BCE, one
// MI355X, one session (tools/kbench.py lossbwd96_ps; the batch backward lossb96 took 43.4 us next to each):
// 8192 / 4096 / 2048 / 1024 blocks -> 49.3 / 48.4 / 43.8 / 42.4 us
#ifndef U3D_LOSS_PS_BWD_NB
#define U3D_LOSS_PS_BWD_NB 1024
#endif
constexpr int PS_BWD_NB = U3D_LOSS_PS_BWD_NB;

// softmax == 1: softmax, 0: sigmoid (libm expf), 2: identity; loss.hip's probs for the two modes without a softmax
template <int NC>
__device__ __forceinline__ void ps_probs(const float* __restrict__ lg, int C, int mode, float (&p)[NC]) {
  if constexpr (NC % 4 == 0 && NC <= 16) {
#pragma unroll
    for (int c = 0; c < NC; c += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lg + c);
      p[c] = v[0]; p[c + 1] = v[1]; p[c + 2] = v[2]; p[c + 3] = v[3];
    }
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = c < C ? lg[c] : 0.f;
  }
  if (mode == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < C) p[c] = 1.f / (1.f + expf(-p[c]));
  }
}

// torch BCELoss element: (t - 1) * max(log1p(-p), -100) - t * max(log(p), -100)
__device__ __forceinline__ float ps_bce_elem(float p, float t) {
  return (t - 1.f) * fmaxf(log1pf(-p), -100.f) - t * fmaxf(logf(p), -100.f);
}

// blocks per sample: the budget shared by the samples, at least one each, no more than the sample's voxels need
static int ps_blocks(int S, long long V, int budget, int vox_per_block) {
  return (int)std::max<long long>(1, std::min<long long>(budget / S, (V + vox_per_block - 1) / vox_per_block));
}

// sample blockIdx.y, voxels blockIdx.x * PT + threadIdx.x + k * gridDim.x * PT; ws[(s * gridDim.x + bx)][k * C + c]
template <int NC>
__global__ __launch_bounds__(PT) void loss_ps_partial_kernel(const float* __restrict__ lg,
                                                            const float* __restrict__ lab, long long V, int C,
                                                            int mode, int uce, float* __restrict__ ws) {
  __shared__ float red[PT / 64][4 * NC];
  float acc[4][NC];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[k][c] = 0.f;
  const int smp = blockIdx.y;
  lg += (long long)smp * V * C;
  lab += (long long)smp * V;
  const long long stride = (long long)gridDim.x * PT;
  for (long long v = blockIdx.x * (long long)PT + threadIdx.x; v < V; v += stride) {
    const float t = lab[v];
    if (mode == 1) {
      float x[NC], e[NC], s, inv;
      softmax_fast<NC>(lg + v * C, C, x, e, s, inv);
      const float ls = __builtin_amdgcn_logf(s) * LN2;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < C) {
          const bool hit = t == (float)c;
          const float tc = hit ? 1.f : 0.f, p = e[c] * inv;
          acc[0][c] = fmaf(p, tc, acc[0][c]);
          acc[1][c] = fmaf(p, p, acc[1][c]);
          acc[2][c] += tc;
          if (uce == 1) {
            const float lq = hit ? x[c] - ls : __builtin_amdgcn_logf(s - e[c]) * LN2 - ls;
            acc[3][c] -= fmaxf(lq, -100.f);
          }
        }
    } else {
      float p[NC];
      ps_probs<NC>(lg + v * C, C, mode, p);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < C) {
          const float tc = (t == (float)c) ? 1.f : 0.f;
          acc[0][c] = fmaf(p[c], tc, acc[0][c]);
          acc[1][c] = fmaf(p[c], p[c], acc[1][c]);
          acc[2][c] += tc;
          if (uce == 1) acc[3][c] += ps_bce_elem(p[c], tc);
        }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < C) {
        float s = wave_sum(acc[k][c]);
        if (lane == 0) red[wave][k * NC + c] = s;
      }
  __syncthreads();
  float* out = ws + ((long long)smp * gridDim.x + blockIdx.x) * 4 * C;
  for (int i = threadIdx.x; i < 4 * C; i += PT) {
    const int k = i / C, c = i % C;
    float s = 0.f;
    for (int w = 0; w < PT / 64; ++w) s += red[w][k * NC + c];
    out[i] = s;
  }
}

// The trunk's loss (C = 16, softmax, uce 1): loss.hip's loss_partial16_pair_kernel per sample. Each voxel's classes
// are split over a lane pair (lanes i, i + 32 hold classes 0-7 / 8-15; the max and the softmax sum are exchanged once
// each), the next voxel's logits and label are loaded before this voxel's math. 128 voxels per block and trip.
__global__ __launch_bounds__(PT) void loss_ps_partial16_pair_kernel(const float* __restrict__ lg,
                                                                   const float* __restrict__ lab, long long V,
                                                                   float* __restrict__ ws) {
  __shared__ float red[PT / 64][64];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
  float acc[4][8];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[k][c] = 0.f;
  const int smp = blockIdx.y;
  lg += (long long)smp * V * 16;
  lab += (long long)smp * V;
  const long long stride = (long long)gridDim.x * (PT / 2);
  long long v = (long long)blockIdx.x * (PT / 2) + wave * 32 + r;  // lanes r and r + 32: the same voxel
  auto load = [&](long long vv, f32x4 (&q)[2], float& t) {  // clamped index, no branch around the loads
    vv = vv < V ? vv : V - 1;
#pragma unroll
    for (int k = 0; k < 2; ++k) q[k] = *reinterpret_cast<const f32x4*>(lg + vv * 16 + 8 * h + 4 * k);
    t = lab[vv];
  };
  f32x4 cur[2], nxt[2];
  float tcur = 0.f, tnxt = 0.f;
  load(v, cur, tcur);
  for (; v < V; v += stride) {  // both lanes of a pair take the same trips (the exchanges need both)
    load(v + stride, nxt, tnxt);
    float x[8], e[8];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) x[4 * k + j] = cur[k][j];
    float m = x[0];
#pragma unroll
    for (int c = 1; c < 8; ++c) m = fmaxf(m, x[c]);
    m = fmaxf(m, __shfl_xor(m, 32));
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      x[c] -= m;
      e[c] = __builtin_amdgcn_exp2f(x[c] * LOG2E);
      s += e[c];
    }
    s += __shfl_xor(s, 32);
    const float inv = __builtin_amdgcn_rcpf(s), ls = __builtin_amdgcn_logf(s) * LN2;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const bool hit = tcur == (float)(8 * h + c);
      const float tc = hit ? 1.f : 0.f, p = e[c] * inv;
      acc[0][c] = fmaf(p, tc, acc[0][c]);
      acc[1][c] = fmaf(p, p, acc[1][c]);
      acc[2][c] += tc;
      const float lq = hit ? x[c] - ls : __builtin_amdgcn_logf(s - e[c]) * LN2 - ls;
      acc[3][c] -= fmaxf(lq, -100.f);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) cur[k] = nxt[k];
    tcur = tnxt;
  }
  // per class over the wave's 32 voxels (lanes with equal h), then the block's waves in order
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float t = acc[k][c];
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) t += __shfl_xor(t, o, 32);
      if (r == 0) red[wave][k * 16 + 8 * h + c] = t;
    }
  __syncthreads();
  if (threadIdx.x < 64) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < PT / 64; ++w) t += red[w][threadIdx.x];
    ws[((long long)smp * gridDim.x + blockIdx.x) * 64 + threadIdx.x] = t;
  }
}

// one block per (k, c) and sample: sums_ps[s][c][k] = the sample's per-block partials added in fp64, fixed order
__global__ __launch_bounds__(PT) void loss_ps_combine_kernel(const float* __restrict__ ws, int nblk, int C,
                                                            double* __restrict__ sums_ps) {
  __shared__ double red[PT / 64];
  const int i = blockIdx.x, smp = blockIdx.y;  // i = k * C + c
  const float* src = ws + (long long)smp * nblk * 4 * C;
  double a = 0;
  for (int b = threadIdx.x; b < nblk; b += PT) a += src[(long long)b * 4 * C + i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int k = i / C, c = i % C;
    sums_ps[((long long)smp * C + c) * 4 + k] = red[0] + red[1] + red[2] + red[3];
  }
}

// one workgroup, thread c: pooled[c] = (I, Z, Y, B, n_c) over the supervising samples in ascending s (fp64), then
// the loss as loss_final_kernel forms it (d_c and the BCE mean rounded to fp32) with w^_c and the mean over n_c V
__global__ __launch_bounds__(64) void loss_ps_final_kernel(int S, int C, double V, const float* __restrict__ w, int uce,
                                                          const double* __restrict__ sums_ps,
                                                          double* __restrict__ pooled, float* __restrict__ loss) {
  __shared__ double sd[PS_CMAX], sb[PS_CMAX];
  const int c = threadIdx.x;
  if (c < C) {
    double X[4] = {0, 0, 0, 0}, n = 0;
    for (int s = 0; s < S; ++s)
      if (w[(long long)s * C + c] != 0.f) {
        const double* q = sums_ps + ((long long)s * C + c) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) X[k] += q[k];
        n += 1;
      }
#pragma unroll
    for (int k = 0; k < 4; ++k) pooled[c * 5 + k] = X[k];
    pooled[c * 5 + 4] = n;
    const double wh = ps_class_weight(c, S, C, w, n);
    const float d = 1.f - (float)((2.0 * X[0] + 1e-5) / (X[1] + X[2] + 1e-5));
    sd[c] = (double)d * wh;
    sb[c] = (uce == 1 && n > 0) ? (double)(float)(X[3] / (n * V)) * wh : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double dice = 0, ce = 0;
    for (int k = 0; k < C; ++k) {
      dice += sd[k];
      ce += sb[k];
    }
    double l = dice / C;
    if (uce) l += ce;
    loss[0] = (float)l;
  }
}

template <int NC, typename TO>
__global__ __launch_bounds__(PT) void loss_ps_bwd_kernel(const float* __restrict__ lg, const float* __restrict__ lab,
                                                        long long V, int S, int C, int mode, int uce,
                                                        const float* __restrict__ w, const double* __restrict__ pooled,
                                                        const float* __restrict__ gout, TO* __restrict__ dl) {
  __shared__ float kd_a[NC], kd_b[NC], kb[NC];
  const int smp = blockIdx.y;
  int sup = 0;
  if (threadIdx.x < NC) sup = threadIdx.x < C && w[(long long)smp * C + threadIdx.x] != 0.f;
  const int any = __syncthreads_or(sup);
  lg += (long long)smp * V * C;
  lab += (long long)smp * V;
  dl += (long long)smp * V * C;
  const long long stride = (long long)gridDim.x * PT;
  if (!any) {  // the sample supervises no class: its gradient is 0, written without reading the logits
    for (long long i = blockIdx.x * (long long)PT + threadIdx.x; i < V * C; i += stride) dl[i] = from_f<TO>(0.f);
    return;
  }
  auto build_table = [&]() {
    if (threadIdx.x < NC) {
      const int c = threadIdx.x;
      float a, b, e;
      dice_bce_coefs_ps(c, smp, S, C, pooled, w, gout, uce, (double)V, a, b, e);
      kd_a[c] = a;
      kd_b[c] = b;
      kb[c] = e;
    }
    __syncthreads();
  };
  if constexpr (NC == 16 && sizeof(TO) == 4) {
    if (mode == 1 && uce == 1 && C == NC) {
      // software-pipelined softmax + BCE path (the trunk's loss), as loss_bwd_kernel: the next voxel's logits and
      // label are loaded before this voxel's math; same arithmetic as the generic loop below. The first voxel's loads
      // are issued before the coefficient table is built: they are in flight during the table's loads and divisions
      // (a block covers one or two voxels per thread, so its prologue is on its critical path).
      long long v = blockIdx.x * (long long)PT + threadIdx.x;
      f32x4 cur[4], nxt[4];
      float tcur = 0.f, tnxt = 0.f;
      auto load = [&](long long vv, f32x4 (&q)[4], float& t) {  // clamped index, no branch around the loads
        vv = vv < V ? vv : V - 1;
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = *reinterpret_cast<const f32x4*>(lg + vv * 16 + 4 * k);
        t = lab[vv];
      };
      load(v, cur, tcur);
      build_table();
      for (; v < V; v += stride) {
        load(v + stride, nxt, tnxt);
        float r[16];
        dice_bce_softmax_grad16(cur, tcur, kd_a, kd_b, kb, r);
#pragma unroll
        for (int c = 0; c < 16; c += 4)
          *reinterpret_cast<f32x4*>(dl + v * 16 + c) = f32x4{r[c], r[c + 1], r[c + 2], r[c + 3]};
#pragma unroll
        for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
        tcur = tnxt;
      }
      return;
    }
  }
  build_table();
  for (long long v = blockIdx.x * (long long)PT + threadIdx.x; v < V; v += stride) {
    float p[NC], g[NC];
    if (mode == 1) {
      float x[NC], s, inv;
      softmax_fast<NC>(lg + v * C, C, x, p, s, inv);
#pragma unroll
      for (int c = 0; c < NC; ++c) p[c] *= inv;
    } else {
      ps_probs<NC>(lg + v * C, C, mode, p);
    }
    const float t = lab[v];
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      g[c] = 0.f;
      if (c < C) {
        const float tc = (t == (float)c) ? 1.f : 0.f;
        float gc = fmaf(tc, kd_a[c], p[c] * kd_b[c]);
        if (uce == 1) gc += kb[c] * (p[c] - tc) * __builtin_amdgcn_rcpf(fmaxf((1.f - p[c]) * p[c], 1e-12f));
        g[c] = gc;
        dot = fmaf(gc, p[c], dot);
      }
    }
    float r[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) r[c] = mode == 1 ? p[c] * (g[c] - dot) : mode == 0 ? g[c] * (1.f - p[c]) * p[c] : g[c];
    if constexpr (NC == 16 && sizeof(TO) == 4) {
#pragma unroll
      for (int c = 0; c < 16; c += 4)
        *reinterpret_cast<f32x4*>(dl + v * 16 + c) = f32x4{r[c], r[c + 1], r[c + 2], r[c + 3]};
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < C) dl[v * C + c] = from_f<TO>(r[c]);
    }
  }
}

}  // namespace u3d

using namespace u3d;

extern "C" long long u3d_loss_ps_workspace_bytes(int S, long long V, int C) {
  if (S < 1 || V < 1 || C < 1) return 0;
  const int nb = std::max(ps_blocks(S, V, PS_FWD_NB, PT), C == 16 ? ps_blocks(S, V, PS_PAIR_NB, PT / 2) : 0);
  return (long long)S * nb * 4 * C * 4;
}

extern "C" int u3d_partial_loss_ps_fwd(const float* logits, const float* labels, int S, long long V, int C, int softmax,
                                       const float* weights, int uce, double* sums_ps, double* pooled, float* loss,
                                       float* ws, u3d_stream_t stream) {
  U3D_REQUIRE(logits && labels && weights && sums_ps && pooled && loss && ws, "partial_loss_ps_fwd: null pointer");
  U3D_REQUIRE(C >= 1 && C <= PS_CMAX && S >= 1 && V >= 1, "partial_loss_ps_fwd: C=%d unsupported (max %d)", C, PS_CMAX);
  U3D_REQUIRE(S <= PS_MAXS, "partial_loss_ps_fwd: S=%d samples (the grid takes %d at most)", S, PS_MAXS);
  U3D_REQUIRE(uce == 0 || uce == 1, "partial_loss_ps_fwd: uce=%d (the cross entropy of uce 2 is unweighted: it has no "
              "per-sample form)", uce);
  hipStream_t s = (hipStream_t)stream;
  int nb;
  if (C == 16 && softmax == 1 && uce == 1) {
    nb = ps_blocks(S, V, PS_PAIR_NB, PT / 2);
    hipLaunchKernelGGL(loss_ps_partial16_pair_kernel, dim3(nb, S), dim3(PT), 0, s, logits, labels, V, ws);
  } else {
    nb = ps_blocks(S, V, PS_FWD_NB, PT);
#define LAUNCH(NCV) \
  hipLaunchKernelGGL(loss_ps_partial_kernel<NCV>, dim3(nb, S), dim3(PT), 0, s, logits, labels, V, C, softmax, uce, ws)
    U3D_NC_DISPATCH(C, LAUNCH)
#undef LAUNCH
  }
  hipLaunchKernelGGL(loss_ps_combine_kernel, dim3(4 * C, S), dim3(PT), 0, s, ws, nb, C, sums_ps);
  hipLaunchKernelGGL(loss_ps_final_kernel, dim3(1), dim3(64), 0, s, S, C, (double)V, weights, uce, sums_ps, pooled,
                     loss);
  return check_launch("partial_loss_ps_fwd");
}

extern "C" int u3d_partial_loss_ps_bwd(int dtype_out, const float* logits, const float* labels, int S, long long V,
                                       int C, int softmax, const float* weights, int uce, const double* pooled,
                                       const float* grad_out, void* dlogits, u3d_stream_t stream) {
  U3D_REQUIRE(logits && labels && weights && pooled && grad_out && dlogits, "partial_loss_ps_bwd: null pointer");
  U3D_REQUIRE(C >= 1 && C <= PS_CMAX && S >= 1 && V >= 1, "partial_loss_ps_bwd: C=%d unsupported", C);
  U3D_REQUIRE(S <= PS_MAXS, "partial_loss_ps_bwd: S=%d samples (the grid takes %d at most)", S, PS_MAXS);
  U3D_REQUIRE(uce == 0 || uce == 1, "partial_loss_ps_bwd: bad uce=%d", uce);
  hipStream_t s = (hipStream_t)stream;
  const int nb = ps_blocks(S, V, PS_BWD_NB, PT);
  if (dtype_out == U3D_BF16) {
#define LAUNCH(NCV)                                                                                                  \
  hipLaunchKernelGGL((loss_ps_bwd_kernel<NCV, bf16>), dim3(nb, S), dim3(PT), 0, s, logits, labels, V, S, C, softmax, \
                     uce, weights, pooled, grad_out, (bf16*)dlogits)
    U3D_NC_DISPATCH(C, LAUNCH)
#undef LAUNCH
  } else {
#define LAUNCH(NCV)                                                                                                   \
  hipLaunchKernelGGL((loss_ps_bwd_kernel<NCV, float>), dim3(nb, S), dim3(PT), 0, s, logits, labels, V, S, C, softmax, \
                     uce, weights, pooled, grad_out, (float*)dlogits)
    U3D_NC_DISPATCH(C, LAUNCH)
#undef LAUNCH
  }
  return check_launch("partial_loss_ps_bwd");
}
