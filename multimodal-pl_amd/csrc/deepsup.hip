// Deep-supervision loss of get_loss (reference losses.py:119-129): over up to four decoder levels,
//   sum_l weight_l * EDiceLoss_partial(C)(logits_l, F.interpolate(target, size_l, mode='nearest'), uce=False),
// forward and backward in one launch each over all levels. The resized targets are never built: every voxel of a
// level reads its label from the full-resolution target through torch's nearest index map
//   src = min((int)floorf(i * scale), in - 1),  scale = (float)in / out in fp32
// (an identity level has scale 1 and maps i to i exactly). Per level the loss keeps EDiceLoss_partial's quirks
// (loss.hip): the sums run over the whole batch, the weighted class sum is divided by C.
//
// Level pointers, extents, scales and the block prefix table travel by value in the kernel arguments (no host to
// device copy: the calls can be captured in a graph); a block finds its level by comparing its index against the
// prefix table. Forward: per-block partial sums to fixed workspace slots, then a one-workgroup finalize launch that
// adds them per level in fp64 in fixed order (no float atomics, no inter-workgroup hand-off: deterministic).
// Backward: recomputes the softmax and the nearest label, applies the Dice gradient from the sums (loss_grad.h).
#include "common.h"
#include "loss_grad.h"

namespace u3d {

constexpr int DT = 256;
constexpr int DS_MAXL = 4;
constexpr int DS_CMAX = 32;
constexpr int DS_FWD_NB = 256;   // forward blocks per level at most (each leaves one row of partials)
constexpr int DS_BWD_NB = 2048;  // backward blocks per level at most

struct DsArgs {  // kernel argument, by value
  const float* lg[DS_MAXL];
  float* dl[DS_MAXL];
  int d[DS_MAXL], h[DS_MAXL], w[DS_MAXL];
  float sd[DS_MAXL], sh[DS_MAXL], sw[DS_MAXL];  // (float)in / out per axis
  float lw[DS_MAXL];
  int blk[DS_MAXL + 1];  // blocks [blk[l], blk[l + 1]) work on level l
  int L;
};

struct DsLevel {
  const float* lg;
  float* dl;
  int d, h, w;
  float sd, sh, sw, lw;
  int b0, nb, l;
};

// the level of block b: compile-time indices only, so the argument struct stays in scalar registers
__device__ __forceinline__ DsLevel ds_level(const DsArgs& g, int b) {
  DsLevel r{g.lg[0], g.dl[0], g.d[0], g.h[0], g.w[0], g.sd[0], g.sh[0], g.sw[0], g.lw[0], g.blk[0],
            g.blk[1] - g.blk[0], 0};
#pragma unroll
  for (int k = 1; k < DS_MAXL; ++k)
    if (k < g.L && b >= g.blk[k])
      r = DsLevel{g.lg[k], g.dl[k], g.d[k], g.h[k], g.w[k], g.sd[k], g.sh[k], g.sw[k], g.lw[k], g.blk[k],
                  g.blk[k + 1] - g.blk[k], k};
  return r;
}

__device__ __forceinline__ int ds_nearest(int i, float scale, int in) {
  return min((int)floorf((float)i * scale), in - 1);
}

// label of voxel v (flat over [S][d][h][w] of the level) from the full-resolution target [S][D][H][W]
__device__ __forceinline__ float ds_label(const DsLevel& lv, unsigned v, const float* __restrict__ tgt, int D, int H,
                                          int W) {
  const unsigned e = v % (unsigned)lv.w, q = v / (unsigned)lv.w;
  const unsigned b = q % (unsigned)lv.h, r = q / (unsigned)lv.h;
  const unsigned a = r % (unsigned)lv.d, s = r / (unsigned)lv.d;
  const int ia = ds_nearest((int)a, lv.sd, D), ib = ds_nearest((int)b, lv.sh, H), ie = ds_nearest((int)e, lv.sw, W);
  return tgt[(((long long)s * D + ia) * H + ib) * W + ie];
}

template <int NC>
__global__ __launch_bounds__(DT) void deepsup_fwd_kernel(DsArgs g, const float* __restrict__ tgt, int S, int D, int H,
                                                        int W, int C, float* __restrict__ ws) {
  __shared__ float red[DT / 64][3 * NC];
  const DsLevel lv = ds_level(g, blockIdx.x);
  float acc[3][NC];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[k][c] = 0.f;
  const unsigned nvox = (unsigned)S * lv.d * lv.h * lv.w, stride = (unsigned)lv.nb * DT;  // < 2^31 (host check)
  for (unsigned v = (blockIdx.x - lv.b0) * DT + threadIdx.x; v < nvox; v += stride) {
    const float t = ds_label(lv, v, tgt, D, H, W);
    float x[NC], e[NC], s, inv;
    softmax_fast<NC>(lv.lg + (long long)v * C, C, x, e, s, inv);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < C) {
        const float tc = (t == (float)c) ? 1.f : 0.f, p = e[c] * inv;
        acc[0][c] = fmaf(p, tc, acc[0][c]);
        acc[1][c] = fmaf(p, p, acc[1][c]);
        acc[2][c] += tc;
      }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < C) {
        const float s = wave_sum(acc[k][c]);
        if (lane == 0) red[wave][k * NC + c] = s;
      }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * C; i += DT) {
    const int k = i / C, c = i % C;
    float s = 0.f;
    for (int w = 0; w < DT / 64; ++w) s += red[w][k * NC + c];
    ws[(long long)blockIdx.x * 3 * C + i] = s;
  }
}

// One workgroup: sums[l][c][0..2] = the level's per-block partials added in fp64 (a wave per (level, sum, class),
// lanes over the blocks in order, then the xor tree: fixed order), [3] = 0; level_loss[l] as loss_final_kernel forms
// the Dice term; loss = sum_l weight_l * level_loss_l in fp32 in level order, as the reference's Python sum.
__global__ __launch_bounds__(DT) void deepsup_final_kernel(DsArgs g, int C, const float* __restrict__ wt,
                                                          const float* __restrict__ ws, double* __restrict__ sums,
                                                          float* __restrict__ level_loss, float* __restrict__ loss) {
  __shared__ double sm[DS_MAXL][DS_CMAX][3];
  __shared__ int sblk[DS_MAXL + 1];
  __shared__ float slw[DS_MAXL], sll[DS_MAXL];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < DS_MAXL; ++k) {
      sblk[k] = g.blk[k];
      slw[k] = g.lw[k];
    }
    sblk[DS_MAXL] = g.blk[DS_MAXL];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, L = g.L;
  for (int i = wave; i < L * 3 * C; i += DT / 64) {
    const int l = i / (3 * C), r = i - l * 3 * C;
    double a = 0;
    for (int b = sblk[l] + lane; b < sblk[l + 1]; b += 64) a += ws[(long long)b * 3 * C + r];
    a = wave_sum(a);
    if (lane == 0) sm[l][r % C][r / C] = a;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < L * C; i += DT) {
    const int l = i / C, c = i % C;
    double* o = sums + (long long)i * 4;
    o[0] = sm[l][c][0];
    o[1] = sm[l][c][1];
    o[2] = sm[l][c][2];
    o[3] = 0;
  }
  if (threadIdx.x < L) {
    const int l = threadIdx.x;
    double dice = 0;
    for (int c = 0; c < C; ++c) {
      const double I = sm[l][c][0], Z = sm[l][c][1], Y = sm[l][c][2];
      const float d = 1.f - (float)((2.0 * I + 1e-5) / (Z + Y + 1e-5));
      dice += (double)d * wt[c];
    }
    const float ll = (float)(dice / C);
    level_loss[l] = ll;
    sll[l] = ll;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int l = 0; l < L; ++l) t += sll[l] * slw[l];
    loss[0] = t;
  }
}

template <int NC>
__global__ __launch_bounds__(DT) void deepsup_bwd_kernel(DsArgs g, const float* __restrict__ tgt, int S, int D, int H,
                                                        int W, int C, const float* __restrict__ wt,
                                                        const double* __restrict__ sums,
                                                        const float* __restrict__ gout) {
  __shared__ float kd_a[NC], kd_b[NC];
  const DsLevel lv = ds_level(g, blockIdx.x);
  if (threadIdx.x < NC) {
    const int c = threadIdx.x;
    float a, b, e;
    dice_bce_coefs(c, C, sums + (long long)lv.l * C * 4, wt, gout, 0, 1.0, a, b, e);
    kd_a[c] = a * lv.lw;
    kd_b[c] = b * lv.lw;
  }
  __syncthreads();
  const unsigned nvox = (unsigned)S * lv.d * lv.h * lv.w, stride = (unsigned)lv.nb * DT;
  for (unsigned v = (blockIdx.x - lv.b0) * DT + threadIdx.x; v < nvox; v += stride) {
    const float t = ds_label(lv, v, tgt, D, H, W);
    float x[NC], p[NC], s, inv;
    softmax_fast<NC>(lv.lg + (long long)v * C, C, x, p, s, inv);
    float gr[NC], dot = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      p[c] *= inv;
      gr[c] = 0.f;
      if (c < C) {
        const float tc = (t == (float)c) ? 1.f : 0.f;
        gr[c] = fmaf(tc, kd_a[c], p[c] * kd_b[c]);
        dot = fmaf(gr[c], p[c], dot);
      }
    }
    float* o = lv.dl + (long long)v * C;
    if constexpr (NC % 4 == 0 && NC <= 16) {
#pragma unroll
      for (int c = 0; c < NC; c += 4)
        *reinterpret_cast<f32x4*>(o + c) = f32x4{p[c] * (gr[c] - dot), p[c + 1] * (gr[c + 1] - dot),
                                                 p[c + 2] * (gr[c + 2] - dot), p[c + 3] * (gr[c + 3] - dot)};
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < C) o[c] = p[c] * (gr[c] - dot);
    }
  }
}

// host: validate the levels and fill the by-value argument; maxnb = blocks per level at most
static int ds_fill(DsArgs& a, int L, const float* const* logits, float* const* dlogits, const int* dims,
                   const float* lw, int S, int D, int H, int W, int maxnb) {
  a = DsArgs{};
  a.L = L;
  int b = 0;
  for (int l = 0; l < L; ++l) {
    const int d = dims[3 * l], h = dims[3 * l + 1], w = dims[3 * l + 2];
    if (!logits[l] || (dlogits && !dlogits[l]) || d < 1 || h < 1 || w < 1) return 1;
    const long long nvox = (long long)S * d * h * w;
    if (nvox >= (1ll << 31) / DS_CMAX) return 1;  // 32-bit voxel index, v * C within 2^31 floats per level
    a.lg[l] = logits[l];
    a.dl[l] = dlogits ? dlogits[l] : nullptr;
    a.d[l] = d; a.h[l] = h; a.w[l] = w;
    a.sd[l] = (float)D / d; a.sh[l] = (float)H / h; a.sw[l] = (float)W / w;
    a.lw[l] = lw[l];
    a.blk[l] = b;
    b += (int)std::min<long long>(maxnb, (nvox + DT - 1) / DT);
  }
  for (int l = L; l <= DS_MAXL; ++l) a.blk[l] = b;
  return 0;
}

}  // namespace u3d

using namespace u3d;

extern "C" long long u3d_deepsup_loss_workspace_bytes(int L, int C) {
  return (long long)std::max(L, 1) * DS_FWD_NB * 3 * std::max(C, 1) * 4;
}

extern "C" int u3d_deepsup_loss_fwd(int L, const float* const* logits, const int* dims, const float* level_weights,
                                    const float* target, int S, int D, int H, int W, int C, const float* weights,
                                    double* sums, float* level_loss, float* loss, float* ws, u3d_stream_t stream) {
  U3D_REQUIRE(logits && dims && level_weights && target && weights && sums && level_loss && loss && ws,
              "deepsup_loss_fwd: null pointer");
  U3D_REQUIRE(L >= 1 && L <= DS_MAXL && C >= 1 && C <= DS_CMAX && S >= 1 && D >= 1 && H >= 1 && W >= 1,
              "deepsup_loss_fwd: L=%d (max %d) C=%d (max %d) S=%d target %dx%dx%d unsupported", L, DS_MAXL, C, DS_CMAX,
              S, D, H, W);
  DsArgs a;
  U3D_REQUIRE(ds_fill(a, L, logits, nullptr, dims, level_weights, S, D, H, W, DS_FWD_NB) == 0,
              "deepsup_loss_fwd: a level has a null pointer, an empty extent or 2^26 voxels or more");
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(NCV) \
  hipLaunchKernelGGL(deepsup_fwd_kernel<NCV>, dim3(a.blk[L]), dim3(DT), 0, s, a, target, S, D, H, W, C, ws)
  U3D_NC_DISPATCH(C, LAUNCH)
#undef LAUNCH
  hipLaunchKernelGGL(deepsup_final_kernel, dim3(1), dim3(DT), 0, s, a, C, weights, ws, sums, level_loss, loss);
  return check_launch("deepsup_loss_fwd");
}

extern "C" int u3d_deepsup_loss_bwd(int L, const float* const* logits, const int* dims, const float* level_weights,
                                    const float* target, int S, int D, int H, int W, int C, const float* weights,
                                    const double* sums, const float* grad_out, float* const* dlogits,
                                    u3d_stream_t stream) {
  U3D_REQUIRE(logits && dims && level_weights && target && weights && sums && grad_out && dlogits,
              "deepsup_loss_bwd: null pointer");
  U3D_REQUIRE(L >= 1 && L <= DS_MAXL && C >= 1 && C <= DS_CMAX && S >= 1 && D >= 1 && H >= 1 && W >= 1,
              "deepsup_loss_bwd: L=%d C=%d S=%d target %dx%dx%d unsupported", L, C, S, D, H, W);
  DsArgs a;
  U3D_REQUIRE(ds_fill(a, L, logits, dlogits, dims, level_weights, S, D, H, W, DS_BWD_NB) == 0,
              "deepsup_loss_bwd: a level has a null pointer, an empty extent or 2^26 voxels or more");
#define LAUNCH(NCV)                                                                                             \
  hipLaunchKernelGGL(deepsup_bwd_kernel<NCV>, dim3(a.blk[L]), dim3(DT), 0, (hipStream_t)stream, a, target, S, D, \
                     H, W, C, weights, sums, grad_out)
  U3D_NC_DISPATCH(C, LAUNCH)
#undef LAUNCH
  return check_launch("deepsup_loss_bwd");
}

// ------------------------------------------------------------------------------------ per-sample supervision
// The same loss with one supervision row per sample (weights [S][C], the pooling rule of loss_ps.hip with uce 0, per
// level): sample s enters level l's sums of class c only when w[s][c] != 0. The grid is 2-D, the sample on blockIdx.y;
// the block prefix table counts one sample's blocks (ds_fill with S = 1) and the labels are read through the same
// nearest map from the sample's own target volume. Forward: per-(sample, block) partials to fixed workspace slots, a
// combine launch (fp64, fixed order) to sums_ps [L][S][C][4], a one-workgroup launch that pools them over the
// supervising samples in ascending s (pooled [L][C][5] = I, Z, Y, 0, n_c) and forms the level losses and the loss.
namespace u3d {

constexpr int DS_PS_MAXS = 65535;  // gridDim.y

template <int NC>
__global__ __launch_bounds__(DT) void deepsup_ps_fwd_kernel(DsArgs g, const float* __restrict__ tgt, int D, int H,
                                                           int W, int C, float* __restrict__ ws) {
  __shared__ float red[DT / 64][3 * NC];
  const DsLevel lv = ds_level(g, blockIdx.x);
  const int smp = blockIdx.y;
  float acc[3][NC];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[k][c] = 0.f;
  const unsigned nvox = (unsigned)lv.d * lv.h * lv.w, stride = (unsigned)lv.nb * DT;  // one sample's, < 2^31 / 32
  const float* lg = lv.lg + (long long)smp * nvox * C;
  const float* st = tgt + (long long)smp * D * H * W;
  for (unsigned v = (blockIdx.x - lv.b0) * DT + threadIdx.x; v < nvox; v += stride) {
    const float t = ds_label(lv, v, st, D, H, W);
    float x[NC], e[NC], s, inv;
    softmax_fast<NC>(lg + (long long)v * C, C, x, e, s, inv);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < C) {
        const float tc = (t == (float)c) ? 1.f : 0.f, p = e[c] * inv;
        acc[0][c] = fmaf(p, tc, acc[0][c]);
        acc[1][c] = fmaf(p, p, acc[1][c]);
        acc[2][c] += tc;
      }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < C) {
        const float s = wave_sum(acc[k][c]);
        if (lane == 0) red[wave][k * NC + c] = s;
      }
  __syncthreads();
  float* out = ws + ((long long)smp * gridDim.x + blockIdx.x) * 3 * C;
  for (int i = threadIdx.x; i < 3 * C; i += DT) {
    const int k = i / C, c = i % C;
    float s = 0.f;
    for (int w = 0; w < DT / 64; ++w) s += red[w][k * NC + c];
    out[i] = s;
  }
}

// block (l, s): sums_ps[l][s][c][0..2] = the sample's per-block partials of the level added in fp64 (a wave per
// (sum, class), lanes over the blocks in order, then the xor tree: fixed order), [3] = 0
__global__ __launch_bounds__(DT) void deepsup_ps_combine_kernel(DsArgs g, int C, int S, const float* __restrict__ ws,
                                                               double* __restrict__ sums_ps) {
  const int l = blockIdx.x, smp = blockIdx.y;
  int b0 = g.blk[0], b1 = g.blk[1];
#pragma unroll
  for (int k = 1; k < DS_MAXL; ++k)
    if (k == l) {
      b0 = g.blk[k];
      b1 = g.blk[k + 1];
    }
  const float* src = ws + (long long)smp * g.blk[DS_MAXL] * 3 * C;
  double* out = sums_ps + ((long long)l * S + smp) * C * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < 3 * C; i += DT / 64) {
    double a = 0;
    for (int b = b0 + lane; b < b1; b += 64) a += src[(long long)b * 3 * C + i];
    a = wave_sum(a);
    if (lane == 0) out[(i % C) * 4 + i / C] = a;
  }
  for (int c = threadIdx.x; c < C; c += DT) out[c * 4 + 3] = 0;
}

// One workgroup: pooled[l][c] over the supervising samples (s ascending, fp64), level_loss[l] as deepsup_final_kernel
// forms it with w^_c (loss_grad.h), loss = sum_l weight_l * level_loss_l in fp32 in level order.
__global__ __launch_bounds__(DT) void deepsup_ps_final_kernel(DsArgs g, int C, int S, const float* __restrict__ w,
                                                             const double* __restrict__ sums_ps,
                                                             double* __restrict__ pooled,
                                                             float* __restrict__ level_loss, float* __restrict__ loss) {
  __shared__ double sd[DS_MAXL][DS_CMAX];
  __shared__ float slw[DS_MAXL], sll[DS_MAXL];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < DS_MAXL; ++k) slw[k] = g.lw[k];
  }
  const int L = g.L;
  for (int i = threadIdx.x; i < L * C; i += DT) {
    const int l = i / C, c = i % C;
    double X[3] = {0, 0, 0}, n = 0;
    for (int s = 0; s < S; ++s)
      if (w[(long long)s * C + c] != 0.f) {
        const double* q = sums_ps + (((long long)l * S + s) * C + c) * 4;
        X[0] += q[0];
        X[1] += q[1];
        X[2] += q[2];
        n += 1;
      }
    double* o = pooled + (long long)i * 5;
    o[0] = X[0];
    o[1] = X[1];
    o[2] = X[2];
    o[3] = 0;
    o[4] = n;
    const float d = 1.f - (float)((2.0 * X[0] + 1e-5) / (X[1] + X[2] + 1e-5));
    sd[l][c] = (double)d * ps_class_weight(c, S, C, w, n);
  }
  __syncthreads();
  if (threadIdx.x < L) {
    const int l = threadIdx.x;
    double dice = 0;
    for (int c = 0; c < C; ++c) dice += sd[l][c];
    const float ll = (float)(dice / C);
    level_loss[l] = ll;
    sll[l] = ll;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int l = 0; l < L; ++l) t += sll[l] * slw[l];
    loss[0] = t;
  }
}

template <int NC>
__global__ __launch_bounds__(DT) void deepsup_ps_bwd_kernel(DsArgs g, const float* __restrict__ tgt, int S, int D,
                                                           int H, int W, int C, const float* __restrict__ w,
                                                           const double* __restrict__ pooled,
                                                           const float* __restrict__ gout) {
  __shared__ float kd_a[NC], kd_b[NC];
  const DsLevel lv = ds_level(g, blockIdx.x);
  const int smp = blockIdx.y;
  int sup = 0;
  if (threadIdx.x < NC) {
    const int c = threadIdx.x;
    float a, b, e;
    dice_bce_coefs_ps(c, smp, S, C, pooled + (long long)lv.l * C * 5, w, gout, 0, 1.0, a, b, e);
    kd_a[c] = a * lv.lw;
    kd_b[c] = b * lv.lw;
    sup = c < C && w[(long long)smp * C + c] != 0.f;
  }
  const int any = __syncthreads_or(sup);
  const unsigned nvox = (unsigned)lv.d * lv.h * lv.w, stride = (unsigned)lv.nb * DT;
  const float* lg = lv.lg + (long long)smp * nvox * C;
  float* dl = lv.dl + (long long)smp * nvox * C;
  if (!any) {  // the sample supervises no class: zeros, without reading the logits
    const long long total = (long long)nvox * C;
    for (long long i = (long long)(blockIdx.x - lv.b0) * DT + threadIdx.x; i < total; i += stride) dl[i] = 0.f;
    return;
  }
  const float* st = tgt + (long long)smp * D * H * W;
  for (unsigned v = (blockIdx.x - lv.b0) * DT + threadIdx.x; v < nvox; v += stride) {
    const float t = ds_label(lv, v, st, D, H, W);
    float x[NC], p[NC], s, inv;
    softmax_fast<NC>(lg + (long long)v * C, C, x, p, s, inv);
    float gr[NC], dot = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      p[c] *= inv;
      gr[c] = 0.f;
      if (c < C) {
        const float tc = (t == (float)c) ? 1.f : 0.f;
        gr[c] = fmaf(tc, kd_a[c], p[c] * kd_b[c]);
        dot = fmaf(gr[c], p[c], dot);
      }
    }
    float* o = dl + (long long)v * C;
    if constexpr (NC % 4 == 0 && NC <= 16) {
#pragma unroll
      for (int c = 0; c < NC; c += 4)
        *reinterpret_cast<f32x4*>(o + c) = f32x4{p[c] * (gr[c] - dot), p[c + 1] * (gr[c + 1] - dot),
                                                 p[c + 2] * (gr[c + 2] - dot), p[c + 3] * (gr[c + 3] - dot)};
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < C) o[c] = p[c] * (gr[c] - dot);
    }
  }
}

}  // namespace u3d

extern "C" long long u3d_deepsup_loss_ps_workspace_bytes(int L, int C, int S) {
  return (long long)std::max(S, 1) * std::max(L, 1) * DS_FWD_NB * 3 * std::max(C, 1) * 4;
}

extern "C" int u3d_deepsup_loss_ps_fwd(int L, const float* const* logits, const int* dims, const float* level_weights,
                                       const float* target, int S, int D, int H, int W, int C, const float* weights,
                                       double* sums_ps, double* pooled, float* level_loss, float* loss, float* ws,
                                       u3d_stream_t stream) {
  U3D_REQUIRE(logits && dims && level_weights && target && weights && sums_ps && pooled && level_loss && loss && ws,
              "deepsup_loss_ps_fwd: null pointer");
  U3D_REQUIRE(L >= 1 && L <= DS_MAXL && C >= 1 && C <= DS_CMAX && S >= 1 && D >= 1 && H >= 1 && W >= 1,
              "deepsup_loss_ps_fwd: L=%d (max %d) C=%d (max %d) S=%d target %dx%dx%d unsupported", L, DS_MAXL, C,
              DS_CMAX, S, D, H, W);
  U3D_REQUIRE(S <= DS_PS_MAXS, "deepsup_loss_ps_fwd: S=%d samples (the grid takes %d at most)", S, DS_PS_MAXS);
  DsArgs a;
  U3D_REQUIRE(ds_fill(a, L, logits, nullptr, dims, level_weights, 1, D, H, W, DS_FWD_NB) == 0,
              "deepsup_loss_ps_fwd: a level has a null pointer, an empty extent or 2^26 voxels or more per sample");
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(NCV) \
  hipLaunchKernelGGL(deepsup_ps_fwd_kernel<NCV>, dim3(a.blk[L], S), dim3(DT), 0, s, a, target, D, H, W, C, ws)
  U3D_NC_DISPATCH(C, LAUNCH)
#undef LAUNCH
  hipLaunchKernelGGL(deepsup_ps_combine_kernel, dim3(L, S), dim3(DT), 0, s, a, C, S, ws, sums_ps);
  hipLaunchKernelGGL(deepsup_ps_final_kernel, dim3(1), dim3(DT), 0, s, a, C, S, weights, sums_ps, pooled, level_loss,
                     loss);
  return check_launch("deepsup_loss_ps_fwd");
}

extern "C" int u3d_deepsup_loss_ps_bwd(int L, const float* const* logits, const int* dims, const float* level_weights,
                                       const float* target, int S, int D, int H, int W, int C, const float* weights,
                                       const double* pooled, const float* grad_out, float* const* dlogits,
                                       u3d_stream_t stream) {
  U3D_REQUIRE(logits && dims && level_weights && target && weights && pooled && grad_out && dlogits,
              "deepsup_loss_ps_bwd: null pointer");
  U3D_REQUIRE(L >= 1 && L <= DS_MAXL && C >= 1 && C <= DS_CMAX && S >= 1 && D >= 1 && H >= 1 && W >= 1,
              "deepsup_loss_ps_bwd: L=%d C=%d S=%d target %dx%dx%d unsupported", L, C, S, D, H, W);
  U3D_REQUIRE(S <= DS_PS_MAXS, "deepsup_loss_ps_bwd: S=%d samples (the grid takes %d at most)", S, DS_PS_MAXS);
  DsArgs a;
  U3D_REQUIRE(ds_fill(a, L, logits, dlogits, dims, level_weights, 1, D, H, W, DS_BWD_NB) == 0,
              "deepsup_loss_ps_bwd: a level has a null pointer, an empty extent or 2^26 voxels or more per sample");
#define LAUNCH(NCV)                                                                                               \
  hipLaunchKernelGGL(deepsup_ps_bwd_kernel<NCV>, dim3(a.blk[L], S), dim3(DT), 0, (hipStream_t)stream, a, target, S, \
                     D, H, W, C, weights, pooled, grad_out)
  U3D_NC_DISPATCH(C, LAUNCH)
#undef LAUNCH
  return check_launch("deepsup_loss_ps_bwd");
}
