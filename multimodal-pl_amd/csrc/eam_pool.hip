// EAM class message (reference unet3D.py:142-212, the half unet3D_with_feam3 discards): attention pooling of a decoder
// level against <= 16 class tokens x 4 heads, forward and backward, for unet3D_with_eam / unet3D_with_eam_baseline.
//
// Score and pooling fold onto the normalised feature (include/u3d.h has the full statement): with xhat_n the LayerNorm
// (norm2) normalised voxel, u_n = xhat_n g2 + b2 and A[r] = q[t, head i] Wk[head i, :] for the row r = i nt + t,
//     S[r][n] = A[r] . u_n,   P[r][.] = softmax_n(scale S[r][.]),   Yhat[r] = sum_n P[r][n] xhat_n,
// so no k or v projection is formed per voxel and nothing of size [rows][voxels] leaves the chip.
//
// Both kernels walk tiles of EP_TV = 64 voxels with 256 threads, workgroup b taking tiles b, b + grid, ...:
//   1. four lanes per voxel load it, normalise it and park xhat in LDS (XH);
//   2. thread (voxel, sub) forms the scores of rows sub, sub + 4, ... of its voxel (and, backward, dP = dYhat . xhat);
//   3. forward: wave w owns rows w, w + 4, ...; a row's 64 voxels sit one per lane, the tile's maximum and sum are
//      xor-shuffle reductions, the running (m, l) live in registers; P goes to LDS with the row's rescale factor;
//      backward: P is exact from the saved (m, l), dS = scale P (dP - D) + gatt / h;
//   4. thread (channel, row group) adds sum_n W[r][n] xhat_n[c] into C / 4 register accumulators (W = P, rescaled
//      first, forward; W = dS backward); the backward's step 3b turns (dS, P) into dxhat and the LayerNorm backward.
// A workgroup leaves its rows' (m, l, Yhat partial) -- backward: (sum dS xhat, sum dS) -- in `part`; a combine kernel
// merges the partials in block order. No float atomics anywhere: results are bitwise reproducible.
#include "common.h"

namespace u3d {

constexpr int EP_NT = 16;       // max tokens
constexpr int EP_H = 4;         // heads
constexpr int EP_R = 64;        // max rows = EP_H * EP_NT
constexpr int EP_TV = 64;       // voxels per tile
constexpr int EP_BLOCKS = 256;  // workgroup cap (one per CU)
constexpr int EP_SP = EP_TV + 1;  // row stride of the [row][voxel] LDS arrays
constexpr float EP_LN_EPS = 1e-5f;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Step 1: the tile's voxel of this thread (4 lanes per voxel, C / 4 channels each) -> xs = xhat, XH[vl][.] = xhat.
// A voxel past the end reads as zeros (xhat = 0). Returns rstd.
template <typename T, int C>
__device__ __forceinline__ float ep_load_norm(const T* __restrict__ x, long long i, bool live, int sub, int vl,
                                              float (&xs)[C / 4], float* XH) {
  constexpr int CS = C / 4, VN = Vec16<T>::N, CP = C + 1;
  if (live) {
#pragma unroll
    for (int k = 0; k < CS; k += VN) {
      float f[VN];
      load16(x + i * C + sub * CS + k, f);
#pragma unroll
      for (int j = 0; j < VN; ++j) xs[k + j] = f[j];
    }
  } else {
#pragma unroll
    for (int k = 0; k < CS; ++k) xs[k] = 0.f;
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < CS; ++k) s += xs[k];
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  const float mean = s / C;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < CS; ++k) {
    const float d = xs[k] - mean;
    q = fmaf(d, d, q);
  }
  q += __shfl_xor(q, 1);
  q += __shfl_xor(q, 2);
  const float rstd = rsqrtf(q / C + EP_LN_EPS);
#pragma unroll
  for (int k = 0; k < CS; ++k) {
    xs[k] = (xs[k] - mean) * rstd;
    XH[vl * CP + sub * CS + k] = xs[k];
  }
  return rstd;
}

// Step 2: s[j] = A[sub + 4 j] . u (u = xhat g2 + b2) for voxel vl; with DP also dp[j] = DY[sub + 4 j] . xhat.
// The one statement of the score, so the backward recomputes the forward's bits.
template <int C, bool DP>
__device__ __forceinline__ void ep_scores(const float* XH, const float* As, const float* DY, const float* G2,
                                          const float* B2, int sub, int vl, float (&s)[EP_R / 4],
                                          float (&dp)[EP_R / 4]) {
  constexpr int CP = C + 1;
#pragma unroll
  for (int j = 0; j < EP_R / 4; ++j) {
    s[j] = 0.f;
    dp[j] = 0.f;
  }
  for (int c = 0; c < C; ++c) {
    const float xh = XH[vl * CP + c];
    const float u = fmaf(xh, G2[c], B2[c]);
#pragma unroll
    for (int j = 0; j < EP_R / 4; ++j) {
      s[j] = fmaf(As[(sub + 4 * j) * CP + c], u, s[j]);
      if constexpr (DP) dp[j] = fmaf(DY[(sub + 4 * j) * CP + c], xh, dp[j]);
    }
  }
}

// Step 4: acc[k] += sum_vl W[r][vl] XH[vl][c], r = rg + k NR, for the thread's channel c and row group rg.
template <int C>
__device__ __forceinline__ void ep_pool(const float* W, const float* XH, int R, int c, int rg, float (&acc)[C / 4]) {
  constexpr int CP = C + 1, NR = 256 / C;
  for (int vl = 0; vl < EP_TV; ++vl) {
    const float xh = XH[vl * CP + c];
#pragma unroll
    for (int k = 0; k < C / 4; ++k) {
      const int r = rg + k * NR;
      if (r < R) acc[k] = fmaf(W[r * EP_SP + vl], xh, acc[k]);
    }
  }
}

// ------------------------------------------------------------------------------------------ forward
// part[block] = [m R][l R][Yhat partial R * C]
template <typename T, int C>
__global__ __launch_bounds__(256) void eam_pool_fwd_kernel(const T* __restrict__ x, long long v,
                                                          const float* __restrict__ g2, const float* __restrict__ b2,
                                                          const float* __restrict__ a, int nt, float scale,
                                                          float* __restrict__ att, float* __restrict__ part) {
  constexpr int CP = C + 1, NR = 256 / C;
  __shared__ float XH[EP_TV * CP], As[EP_R * CP], S[EP_R * EP_SP], P[EP_R * EP_SP], G2[C], B2[C], AL[EP_R];
  const int tid = threadIdx.x, sub = tid & 3, vl = tid >> 2, lane = tid & 63, wave = tid >> 6;
  const int R = EP_H * nt;
  for (int e = tid; e < EP_R * C; e += 256) {
    const int r = e / C, c = e - r * C;
    As[r * CP + c] = r < R ? a[e] : 0.f;
  }
  for (int e = tid; e < C; e += 256) {
    G2[e] = g2[e];
    B2[e] = b2[e];
  }
  const int pc = tid % C, prg = tid / C;
  float acc[C / 4], mrun[EP_R / 4], lrun[EP_R / 4];
#pragma unroll
  for (int k = 0; k < C / 4; ++k) acc[k] = 0.f;
#pragma unroll
  for (int j = 0; j < EP_R / 4; ++j) {
    mrun[j] = -INFINITY;
    lrun[j] = 0.f;
  }
  const long long ntile = (v + EP_TV - 1) / EP_TV;
  __syncthreads();
  for (long long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const long long i = tile * EP_TV + vl;
    float xs[C / 4];
    ep_load_norm<T, C>(x, i, i < v, sub, vl, xs, XH);
    __syncthreads();
    {
      float s[EP_R / 4], dp[EP_R / 4];
      ep_scores<C, false>(XH, As, nullptr, G2, B2, sub, vl, s, dp);
#pragma unroll
      for (int j = 0; j < EP_R / 4; ++j) S[(sub + 4 * j) * EP_SP + vl] = s[j];
    }
    __syncthreads();
    if (att) {  // the head mean of the raw scores, NCDHW [nt][v]
      for (int e = tid; e < nt * EP_TV; e += 256) {
        const int t = e >> 6, u = e & 63;
        const long long n = tile * EP_TV + u;
        if (n < v)
          att[t * v + n] = 0.25f * ((S[t * EP_SP + u] + S[(nt + t) * EP_SP + u]) +
                                    (S[(2 * nt + t) * EP_SP + u] + S[(3 * nt + t) * EP_SP + u]));
      }
    }
    const bool lv = tile * EP_TV + lane < v;
#pragma unroll
    for (int j = 0; j < EP_R / 4; ++j) {
      const int r = wave + 4 * j;
      if (r < R) {
        const float sc = lv ? scale * S[r * EP_SP + lane] : -INFINITY;
        const float mnew = fmaxf(mrun[j], wave_max(sc));  // finite: a tile holds at least one voxel
        const float p = expf(sc - mnew);
        const float al = expf(mrun[j] - mnew);            // 0 on the workgroup's first tile (m = -inf)
        P[r * EP_SP + lane] = p;
        lrun[j] = fmaf(lrun[j], al, wave_sum(p));
        mrun[j] = mnew;
        if (lane == 0) AL[r] = al;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < C / 4; ++k) {
      const int r = prg + k * NR;
      if (r < R) acc[k] *= AL[r];
    }
    ep_pool<C>(P, XH, R, pc, prg, acc);
    __syncthreads();
  }
  float* pb = part + (long long)blockIdx.x * R * (C + 2);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < EP_R / 4; ++j) {
      const int r = wave + 4 * j;
      if (r < R) {
        pb[r] = mrun[j];
        pb[R + r] = lrun[j];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < C / 4; ++k) {
    const int r = prg + k * NR;
    if (r < R) pb[2 * R + r * C + pc] = acc[k];
  }
}

// One block of EP_BLOCKS threads per row: thread b fetches workgroup b's (m_b, l_b), M = max_b m_b (a tree: the
// maximum does not depend on the order), w_b = e^(m_b - M) and w_b l_b go to LDS; then in block order
// l = sum_b w_b l_b and, thread per channel, Yhat = sum_b w_b Y_b / l (fp64 sums of fp32 terms; the loads of the
// partials are independent, eight in flight). stat[r] = M, stat[R + r] = l.
__global__ __launch_bounds__(EP_BLOCKS) void eam_pool_fwd_combine_kernel(const float* __restrict__ part, int nblk,
                                                                        int R, int c, float* __restrict__ yhat,
                                                                        float* __restrict__ stat) {
  __shared__ float W[EP_BLOCKS], WL[EP_BLOCKS], red[EP_BLOCKS];
  const int r = blockIdx.x, tid = threadIdx.x;
  const long long stride = (long long)R * (c + 2);
  const float mb = tid < nblk ? part[tid * stride + r] : -INFINITY;
  red[tid] = mb;
  __syncthreads();
  for (int s = EP_BLOCKS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  const float M = red[0];
  if (tid < nblk) {
    const float w = expf(mb - M);
    W[tid] = w;
    WL[tid] = w * part[tid * stride + R + r];
  }
  __syncthreads();
  double l = 0;
  for (int b = 0; b < nblk; ++b) l += (double)WL[b];
  const float lf = (float)l;
  if (tid < c) {
    const float* py = part + 2 * R + r * c + tid;
    double y = 0;
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) y += (double)(W[b] * py[b * stride]);
    yhat[r * c + tid] = (float)y / lf;
  }
  if (tid == 0) {
    stat[r] = M;
    stat[R + r] = lf;
  }
}

// ------------------------------------------------------------------------------------------ backward
// part[block] = [sum_n dS[r][n] xhat_n[c]  R * C][sum_n dS[r][n]  R]
template <typename T, int C>
__global__ __launch_bounds__(256) void eam_pool_bwd_kernel(const T* __restrict__ x, long long v,
                                                          const float* __restrict__ g2, const float* __restrict__ b2,
                                                          const float* __restrict__ a, int nt, float scale,
                                                          const float* __restrict__ stat, const float* __restrict__ dy,
                                                          const float* __restrict__ dd, const float* __restrict__ gatt,
                                                          T* __restrict__ dx, int accumulate,
                                                          float* __restrict__ part) {
  constexpr int CS = C / 4, VN = Vec16<T>::N, CP = C + 1, NR = 256 / C;
  __shared__ float XH[EP_TV * CP], As[EP_R * CP], DY[EP_R * CP], P[EP_R * EP_SP], DS[EP_R * EP_SP], G2[C], B2[C],
      MS[EP_R], IL[EP_R], DD[EP_R];
  const int tid = threadIdx.x, sub = tid & 3, vl = tid >> 2;
  const int R = EP_H * nt;
  for (int e = tid; e < EP_R * C; e += 256) {
    const int r = e / C, c = e - r * C;
    As[r * CP + c] = r < R ? a[e] : 0.f;
    DY[r * CP + c] = r < R && dy ? dy[e] : 0.f;
  }
  for (int e = tid; e < C; e += 256) {
    G2[e] = g2[e];
    B2[e] = b2[e];
  }
  if (tid < EP_R) {
    MS[tid] = tid < R ? stat[tid] : 0.f;
    IL[tid] = tid < R ? 1.f / stat[R + tid] : 0.f;
    DD[tid] = tid < R && dd ? dd[tid] : 0.f;
  }
  const int pc = tid % C, prg = tid / C;
  float acc[C / 4], accG = 0.f;
#pragma unroll
  for (int k = 0; k < C / 4; ++k) acc[k] = 0.f;
  const long long ntile = (v + EP_TV - 1) / EP_TV;
  __syncthreads();
  for (long long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const long long i = tile * EP_TV + vl;
    const bool live = i < v;
    float xs[CS];
    const float rstd = ep_load_norm<T, C>(x, i, live, sub, vl, xs, XH);
    __syncthreads();
    {
      float s[EP_R / 4], dp[EP_R / 4];
      ep_scores<C, true>(XH, As, DY, G2, B2, sub, vl, s, dp);
#pragma unroll
      for (int j = 0; j < EP_R / 4; ++j) {
        const int r = sub + 4 * j;
        float p = 0.f, ds = 0.f;
        if (live && r < R) {
          p = expf(scale * s[j] - MS[r]) * IL[r];
          ds = scale * p * (dp[j] - DD[r]);
          if (gatt) ds = fmaf(gatt[(r % nt) * v + i], 0.25f, ds);
        }
        P[r * EP_SP + vl] = p;
        DS[r * EP_SP + vl] = ds;
      }
    }
    __syncthreads();
    // dxhat = sum_r P dYhat[r] + g2 sum_r dS A[r], then the LayerNorm backward over the voxel's four lanes
    float dxh[CS], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < CS; ++k) dxh[k] = 0.f;
    {
      float dl[CS];
#pragma unroll
      for (int k = 0; k < CS; ++k) dl[k] = 0.f;
      for (int r = 0; r < R; ++r) {
        const float p = P[r * EP_SP + vl], ds = DS[r * EP_SP + vl];
#pragma unroll
        for (int k = 0; k < CS; ++k) {
          dl[k] = fmaf(ds, As[r * CP + sub * CS + k], dl[k]);
          dxh[k] = fmaf(p, DY[r * CP + sub * CS + k], dxh[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < CS; ++k) {
        dxh[k] = fmaf(G2[sub * CS + k], dl[k], dxh[k]);
        s1 += dxh[k];
        s2 = fmaf(dxh[k], xs[k], s2);
      }
    }
    s1 += __shfl_xor(s1, 1);
    s1 += __shfl_xor(s1, 2);
    s2 += __shfl_xor(s2, 1);
    s2 += __shfl_xor(s2, 2);
    if (live) {
      const float m1 = s1 / C, m2 = s2 / C;
#pragma unroll
      for (int k = 0; k < CS; k += VN) {
        float f[VN];
        if (accumulate) load16(dx + i * C + sub * CS + k, f);
#pragma unroll
        for (int j = 0; j < VN; ++j) {
          const float d = rstd * (dxh[k + j] - m1 - xs[k + j] * m2);
          f[j] = accumulate ? f[j] + d : d;
        }
        store16(dx + i * C + sub * CS + k, f);
      }
    }
    ep_pool<C>(DS, XH, R, pc, prg, acc);
    if (tid < R) {
      float g = accG;
      for (int u = 0; u < EP_TV; ++u) g += DS[tid * EP_SP + u];
      accG = g;
    }
    __syncthreads();
  }
  float* pb = part + (long long)blockIdx.x * R * (C + 2);
#pragma unroll
  for (int k = 0; k < C / 4; ++k) {
    const int r = prg + k * NR;
    if (r < R) pb[r * C + pc] = acc[k];
  }
  if (tid < R) pb[R * C + tid] = accG;
}

// Block r, thread c: the block-order fp64 sums Ps = sum_b part.P[r][c], Gs = sum_b part.G[r];
// dA[r][c] = g2[c] Ps + b2[c] Gs (u = xhat g2 + b2); tail[r][c] = A Ps, tail[R C + r c] = A Gs for the second step.
__global__ __launch_bounds__(128) void eam_pool_bwd_combine_kernel(const float* __restrict__ part, int nblk, int R,
                                                                  int c, const float* __restrict__ a,
                                                                  const float* __restrict__ g2,
                                                                  const float* __restrict__ b2, float* __restrict__ da,
                                                                  float* __restrict__ tail) {
  const int r = blockIdx.x, ch = threadIdx.x;
  const long long stride = (long long)R * (c + 2);
  double ps = 0, gs = 0;
#pragma unroll 8
  for (int b = 0; b < nblk; ++b) {
    ps += part[b * stride + r * c + ch];
    gs += part[b * stride + R * c + r];
  }
  const int e = r * c + ch;
  da[e] = (float)(g2[ch] * ps + b2[ch] * gs);
  tail[e] = (float)(a[e] * ps);
  tail[R * c + e] = (float)(a[e] * gs);
}

// dg2[c] = sum_r A[r][c] Ps[r][c] (= sum_n dl_n xhat_n), db2[c] = sum_r A[r][c] Gs[r] (= sum_n dl_n), row order
__global__ __launch_bounds__(128) void eam_pool_bwd_norm_kernel(const float* __restrict__ tail, int R, int c,
                                                               float* __restrict__ dg2, float* __restrict__ db2,
                                                               int acc_params) {
  const int ch = threadIdx.x;
  double sg = 0, sb = 0;
  for (int r = 0; r < R; ++r) {
    sg += tail[r * c + ch];
    sb += tail[R * c + r * c + ch];
  }
  dg2[ch] = (acc_params ? dg2[ch] : 0.f) + (float)sg;
  db2[ch] = (acc_params ? db2[ch] : 0.f) + (float)sb;
}

}  // namespace u3d

using namespace u3d;

extern "C" int u3d_eam_pool_blocks(long long v) {
  return (int)std::max<long long>(1, std::min<long long>(EP_BLOCKS, (v + EP_TV - 1) / EP_TV));
}

extern "C" long long u3d_eam_pool_part_floats(long long v, int c, int nt) {
  const long long R = (long long)EP_H * nt;
  return u3d_eam_pool_blocks(v) * R * (c + 2) + 2 * R * c;
}

static int eam_pool_check(const char* who, int dtype, int n, long long v, int c, int nt, int heads) {
  if (dtype != U3D_F32 && dtype != U3D_BF16) return fail(U3D_EINVAL, "%s: bad dtype", who);
  if (n != 1)
    return fail(U3D_EUNSUPPORTED, "%s: n = %d (the class tokens have batch 1; the reference raises for B > 1)", who, n);
  if (heads != EP_H) return fail(U3D_EUNSUPPORTED, "%s: heads = %d (%d supported)", who, heads, EP_H);
  if (nt <= 0 || nt > EP_NT) return fail(U3D_EINVAL, "%s: nt %d (1..%d)", who, nt, EP_NT);
  if (c != 32 && c != 64 && c != 128) return fail(U3D_EUNSUPPORTED, "%s: c = %d (32, 64, 128 supported)", who, c);
  if (v <= 0) return fail(U3D_EINVAL, "%s: v = %lld", who, v);
  return U3D_OK;
}

template <typename T, int C>
static void launch_pool_fwd(int nb, hipStream_t s, const void* x, long long v, const float* g2, const float* b2,
                            const float* a, int nt, float scale, float* att, float* part) {
  hipLaunchKernelGGL((eam_pool_fwd_kernel<T, C>), dim3(nb), dim3(256), 0, s, (const T*)x, v, g2, b2, a, nt, scale, att,
                     part);
}

extern "C" int u3d_eam_pool_fwd(int dtype, const void* x, int n, long long v, int c, const float* g2, const float* b2,
                                const float* a, int nt, int heads, float scale, float* att, float* yhat, float* stat,
                                float* part, u3d_stream_t stream) {
  if (int rc = eam_pool_check("eam_pool_fwd", dtype, n, v, c, nt, heads)) return rc;
  U3D_REQUIRE(x && g2 && b2 && a && yhat && stat && part, "eam_pool_fwd: null pointer");
  const int nb = u3d_eam_pool_blocks(v);
  hipStream_t s = (hipStream_t)stream;
  const bool b16 = dtype == U3D_BF16;
  switch (c) {
    case 32: b16 ? launch_pool_fwd<bf16, 32>(nb, s, x, v, g2, b2, a, nt, scale, att, part)
                 : launch_pool_fwd<float, 32>(nb, s, x, v, g2, b2, a, nt, scale, att, part); break;
    case 64: b16 ? launch_pool_fwd<bf16, 64>(nb, s, x, v, g2, b2, a, nt, scale, att, part)
                 : launch_pool_fwd<float, 64>(nb, s, x, v, g2, b2, a, nt, scale, att, part); break;
    default: b16 ? launch_pool_fwd<bf16, 128>(nb, s, x, v, g2, b2, a, nt, scale, att, part)
                 : launch_pool_fwd<float, 128>(nb, s, x, v, g2, b2, a, nt, scale, att, part); break;
  }
  hipLaunchKernelGGL(eam_pool_fwd_combine_kernel, dim3(EP_H * nt), dim3(EP_BLOCKS), 0, s, part, nb, EP_H * nt, c, yhat,
                     stat);
  return check_launch("eam_pool_fwd");
}

template <typename T, int C>
static void launch_pool_bwd(int nb, hipStream_t s, const void* x, long long v, const float* g2, const float* b2,
                            const float* a, int nt, float scale, const float* stat, const float* dy, const float* dd,
                            const float* gatt, void* dx, int acc, float* part) {
  hipLaunchKernelGGL((eam_pool_bwd_kernel<T, C>), dim3(nb), dim3(256), 0, s, (const T*)x, v, g2, b2, a, nt, scale, stat,
                     dy, dd, gatt, (T*)dx, acc, part);
}

extern "C" int u3d_eam_pool_bwd(int dtype, const void* x, int n, long long v, int c, const float* g2, const float* b2,
                                const float* a, int nt, int heads, float scale, const float* stat, const float* dyhat,
                                const float* dd, const float* gatt, void* dx, int accumulate, float* part, float* da,
                                float* dg2, float* db2, int acc_params, u3d_stream_t stream) {
  if (int rc = eam_pool_check("eam_pool_bwd", dtype, n, v, c, nt, heads)) return rc;
  U3D_REQUIRE(x && g2 && b2 && a && stat && dx && part && da && dg2 && db2, "eam_pool_bwd: null pointer");
  U3D_REQUIRE((dyhat != nullptr) == (dd != nullptr), "eam_pool_bwd: dyhat and d come together");
  const int nb = u3d_eam_pool_blocks(v), R = EP_H * nt;
  hipStream_t s = (hipStream_t)stream;
  const bool b16 = dtype == U3D_BF16;
  switch (c) {
    case 32: b16 ? launch_pool_bwd<bf16, 32>(nb, s, x, v, g2, b2, a, nt, scale, stat, dyhat, dd, gatt, dx, accumulate, part)
                 : launch_pool_bwd<float, 32>(nb, s, x, v, g2, b2, a, nt, scale, stat, dyhat, dd, gatt, dx, accumulate, part); break;
    case 64: b16 ? launch_pool_bwd<bf16, 64>(nb, s, x, v, g2, b2, a, nt, scale, stat, dyhat, dd, gatt, dx, accumulate, part)
                 : launch_pool_bwd<float, 64>(nb, s, x, v, g2, b2, a, nt, scale, stat, dyhat, dd, gatt, dx, accumulate, part); break;
    default: b16 ? launch_pool_bwd<bf16, 128>(nb, s, x, v, g2, b2, a, nt, scale, stat, dyhat, dd, gatt, dx, accumulate, part)
                 : launch_pool_bwd<float, 128>(nb, s, x, v, g2, b2, a, nt, scale, stat, dyhat, dd, gatt, dx, accumulate, part); break;
  }
  float* tail = part + (long long)nb * R * (c + 2);
  hipLaunchKernelGGL(eam_pool_bwd_combine_kernel, dim3(R), dim3(c), 0, s, part, nb, R, c, a, g2, b2, da, tail);
  hipLaunchKernelGGL(eam_pool_bwd_norm_kernel, dim3(1), dim3(c), 0, s, tail, R, c, dg2, db2, acc_params);
  return check_launch("eam_pool_bwd");
}
