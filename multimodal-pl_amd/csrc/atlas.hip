// The probabilistic atlas prior (catlas) on the device: the three places where the reference's step handles it.
//  * atlas_crop_kernel: AMOSDataSet_newatlas.__getitem__ resizes the whole atlas to the image's shape (nearest,
//    MOTSDataset.py:357), pads it (pad_image2, :372), keeps one crop (:383) and transposes it (:392); here the resize is
//    taken inside the crop: only the crop is ever formed.
//  * select_probs_fwd/bwd_kernel: the refiner / discriminator inputs of train_amos_atlas_final.py:277-365,
//    cat([softmax(preds, 1)[0, 1:].unsqueeze(1), catlas.unsqueeze(1)], 1)[index].float() and softmax(attn, 1)[0][index]
//    .unsqueeze(1), with the gradient of the softmax channel (:337, :345 carry one back to the segmentation model).
//  * dice_atlas_count_kernel: the atlas-gated prediction of get_dice / get_dice2 (evaluate_amos.py:144-151, :172-179),
//    (softmax(preds)[l + 1] + 0.15) > (1 - atlas[l]), as integer counts for dice_final_kernel (loss.hip).
// All three are one pass over memory; tensors are fp32.
#include "common.h"
#include "loss_grad.h"

namespace u3d {

constexpr int AT = 256;
constexpr int AT_CMAX = 32;       // classes
constexpr int AT_KMAX = 64;       // selected organs
constexpr int AT_DICE_NB = 1024;  // blocks per sample of dice_atlas_count_kernel at most

// nearest source index of F.interpolate on a float64 tensor (what the reference feeds: the atlas file is float64):
// floor(i * in / out) in exact integer arithmetic. (The float32 form floorf(i * (float)in / out) that a float32 or
// device interpolate takes differs from it, e.g. in = 2, out = 82, i = 41: 0 instead of 1.)
__device__ __forceinline__ int nearest_src(int i, int in, int out) {
  const long long s = ((long long)i * in) / out;
  return (int)(s < in - 1 ? s : in - 1);
}

// out[c][dd][hh][ww] = inside ? atlas[c][(y Ah) / Ih][(x Aw) / Iw][(z Ad) / Id] : 0 with y = b0 + hh, x = c0 + ww,
// z = a0 + dd and inside = y < Ih && x < Iw && z < Id (outside = the zero padding of pad_image2). One block per output
// row (dd, hh): the row's two source indices are uniform, each thread forms its column's once and walks the channels.
__global__ __launch_bounds__(AT) void atlas_crop_kernel(const float* __restrict__ atlas, int C, int Ah, int Aw, int Ad,
                                                       int Ih, int Iw, int Id, int b0, int c0, int a0, int ch, int cw,
                                                       int cd, float* __restrict__ out) {
  const int hh = blockIdx.x % ch, dd = blockIdx.x / ch;
  const int y = b0 + hh, z = a0 + dd;
  const bool row_in = y < Ih && z < Id;
  const int sy = row_in ? nearest_src(y, Ah, Ih) : 0, sz = row_in ? nearest_src(z, Ad, Id) : 0;
  const long long plane = (long long)cd * ch * cw, splane = (long long)Ah * Aw * Ad;
  float* orow = out + ((long long)dd * ch + hh) * cw;
  for (int ww = threadIdx.x; ww < cw; ww += AT) {
    const int x = c0 + ww;
    const bool in = row_in && x < Iw;
    const long long src = in ? ((long long)sy * Aw + nearest_src(x, Aw, Iw)) * Ad + sz : 0;
    for (int c = 0; c < C; ++c) orow[c * plane + ww] = in ? atlas[c * splane + src] : 0.f;
  }
}

// softmax over the C classes of one voxel, logits by element strides (class sc): p_c = expf(x_c - max) / sum, the
// arithmetic of loss.hip's probs<NC>. The three kernels below share it, so the backward recomputes the forward's bits.
template <int NC>
__device__ __forceinline__ void softmax_strided(const float* __restrict__ lg, long long sc, int C, float (&p)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) p[c] = c < C ? lg[c * sc] : 0.f;
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < C) m = fmaxf(m, p[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < C) {
      p[c] = expf(p[c] - m);
      s += p[c];
    }
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < C) p[c] = p[c] / s;
}

// The selection by class: rows[start[c] .. start[c + 1]) = the output rows k (ascending) with first + index[k] == c.
// Walking the classes with compile-time register indices and the rows of each class through this table keeps the
// probabilities in registers (p[first + index[k]] would index them dynamically).
struct SelectTable {
  int start[AT_CMAX + 1];
  int rows[AT_KMAX];
  int atlas_ch[AT_KMAX];  // index[k]: the atlas channel of output row k
};

// out[k][0][v] = softmax_c(logits[.][v])[first + index[k]], out[k][1][v] = atlas[index[k]][v] (nch == 2 only)
template <int NC>
__global__ __launch_bounds__(AT) void select_probs_fwd_kernel(const float* __restrict__ lg, long long lsc,
                                                             long long lsv, int C, long long V, SelectTable tab, int K,
                                                             const float* __restrict__ atlas, int nch,
                                                             float* __restrict__ out) {
  const long long v = blockIdx.x * (long long)AT + threadIdx.x;
  if (v >= V) return;
  float p[NC];
  softmax_strided<NC>(lg + v * lsv, lsc, C, p);
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < C)
      for (int j = tab.start[c]; j < tab.start[c + 1]; ++j) out[(long long)tab.rows[j] * nch * V + v] = p[c];
  if (nch == 2)
    for (int k = 0; k < K; ++k) out[((long long)k * 2 + 1) * V + v] = atlas[(long long)tab.atlas_ch[k] * V + v];
}

// dlogits_c = p_c (G_c - sum_j p_j G_j), G_c = sum of g[k][0][v] over the rows k of class c (ascending k), written
// with the logits' own strides; p recomputed as the forward formed it.
template <int NC>
__global__ __launch_bounds__(AT) void select_probs_bwd_kernel(const float* __restrict__ lg, long long lsc,
                                                             long long lsv, int C, long long V, SelectTable tab,
                                                             const float* __restrict__ g, int nch,
                                                             float* __restrict__ dl) {
  const long long v = blockIdx.x * (long long)AT + threadIdx.x;
  if (v >= V) return;
  float p[NC], G[NC];
  softmax_strided<NC>(lg + v * lsv, lsc, C, p);
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    G[c] = 0.f;
    if (c < C) {
      for (int j = tab.start[c]; j < tab.start[c + 1]; ++j) G[c] += g[(long long)tab.rows[j] * nch * V + v];
      dot = fmaf(G[c], p[c], dot);
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < C) dl[v * lsv + c * lsc] = p[c] * (G[c] - dot);
}

// Per sample (grid.y) and organ l < ncls: cpred = (softmax(logits)[l + 1] + 0.15f) > (1 - atlas[s][l]) and
// t = (label == l + 1); cnt[s][l] = (sum cpred & t, sum cpred, sum t) as dice_count_kernel leaves them, amap = the plain
// argmax. logits NDHWC [S][V][C], atlas [S][A][V] (asn = A V), labels [S][V]. Counts go through wave ballots (every
// organ may be positive in a voxel), one LDS add per wave and organ, one global add per block: integers, any order.
template <int NC>
__global__ __launch_bounds__(AT) void dice_atlas_count_kernel(const float* __restrict__ lg,
                                                             const float* __restrict__ lab,
                                                             const float* __restrict__ atlas, long long asn,
                                                             long long V, int C, int ncls,
                                                             unsigned long long* __restrict__ cnt,
                                                             long long* __restrict__ amap) {
  __shared__ unsigned int h[3 * AT_CMAX];
  for (int i = threadIdx.x; i < 3 * AT_CMAX; i += AT) h[i] = 0;
  __syncthreads();
  const int s = blockIdx.y, lane = threadIdx.x & 63;
  const float* base = lg + (long long)s * V * C;
  const float* ab = atlas + (long long)s * asn;
  // every lane of a wave takes the same trips (the ballots need them all); a lane past V counts nothing
  const long long trips = (V + (long long)gridDim.x * AT - 1) / ((long long)gridDim.x * AT);
  for (long long it = 0; it < trips; ++it) {
    const long long v = (it * gridDim.x + blockIdx.x) * AT + threadIdx.x;
    const bool live = v < V;
    const long long vv = live ? v : V - 1;
    float p[NC];
    softmax_strided<NC>(base + vv * C, 1, C, p);
    if (amap && live) {
      int am = 0;
      float best = p[0];
#pragma unroll
      for (int c = 1; c < NC; ++c)
        if (c < C && p[c] > best) {
          best = p[c];
          am = c;
        }
      amap[(long long)s * V + v] = am;
    }
    const float t = lab[(long long)s * V + vv];
#pragma unroll
    for (int l = 0; l + 1 < NC; ++l)
      if (l < ncls && l + 1 < C) {
        const bool cp = live && (p[l + 1] + 0.15f) > (1.f - ab[(long long)l * V + vv]);
        const bool tt = live && t == (float)(l + 1);
        const unsigned a = __popcll(__ballot(cp && tt)), b = __popcll(__ballot(cp)), c = __popcll(__ballot(tt));
        if (lane == 0) {
          if (a) atomicAdd(&h[l * 3 + 0], a);
          if (b) atomicAdd(&h[l * 3 + 1], b);
          if (c) atomicAdd(&h[l * 3 + 2], c);
        }
      }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * ncls; i += AT)
    if (h[i]) atomicAdd(&cnt[(long long)s * 3 * ncls + i], (unsigned long long)h[i]);
}

// index[0..K) (host) -> the by-class table; 0 or an error code
static int select_table(SelectTable& tab, const int* index, int K, int first, int C, int natlas) {
  U3D_REQUIRE(C >= 1 && C <= AT_CMAX && K >= 1 && K <= AT_KMAX && (first == 0 || first == 1) && index,
              "select_probs: C=%d (max %d), K=%d (1..%d), first=%d (0 or 1)", C, AT_CMAX, K, AT_KMAX, first);
  for (int k = 0; k < K; ++k) {
    U3D_REQUIRE(index[k] >= 0 && first + index[k] < C, "select_probs: index[%d]=%d outside the %d classes after %d", k,
                index[k], C - first, first);
    U3D_REQUIRE(natlas < 0 || index[k] < natlas, "select_probs: index[%d]=%d outside the %d atlas channels", k,
                index[k], natlas);
    tab.atlas_ch[k] = index[k];
  }
  int n = 0;
  for (int c = 0; c <= AT_CMAX; ++c) {
    tab.start[c] = n;
    for (int k = 0; k < K && c < AT_CMAX; ++k)
      if (first + index[k] == c) tab.rows[n++] = k;
  }
  return 0;
}

}  // namespace u3d

using namespace u3d;

extern "C" int u3d_atlas_crop(const float* atlas, int C, int Ah, int Aw, int Ad, int Ih, int Iw, int Id, int b0, int c0,
                              int a0, int ch, int cw, int cd, float* out, u3d_stream_t stream) {
  U3D_REQUIRE(atlas && out && C >= 1 && Ah >= 1 && Aw >= 1 && Ad >= 1 && Ih >= 1 && Iw >= 1 && Id >= 1,
              "atlas_crop: bad atlas / image shape");
  U3D_REQUIRE(ch >= 1 && cw >= 1 && cd >= 1 && b0 >= 0 && c0 >= 0 && a0 >= 0, "atlas_crop: bad crop");
  U3D_REQUIRE((long long)ch * cd < (1LL << 31) && (long long)b0 + ch < (1LL << 31) && (long long)c0 + cw < (1LL << 31) &&
                  (long long)a0 + cd < (1LL << 31), "atlas_crop: crop too large");
  hipLaunchKernelGGL(atlas_crop_kernel, dim3(ch * cd), dim3(AT), 0, (hipStream_t)stream, atlas, C, Ah, Aw, Ad, Ih, Iw,
                     Id, b0, c0, a0, ch, cw, cd, out);
  return check_launch("atlas_crop_kernel");
}

extern "C" int u3d_select_probs_fwd(const float* logits, long long lsc, long long lsv, int C, long long V, int first,
                                    const int* index, int K, const float* atlas, int natlas, float* out,
                                    u3d_stream_t stream) {
  U3D_REQUIRE(logits && out && V >= 1 && (!atlas || natlas >= 1), "select_probs_fwd: bad args");
  SelectTable tab;
  int rc = select_table(tab, index, K, first, C, atlas ? natlas : -1);
  if (rc) return rc;
  const long long nb = (V + AT - 1) / AT;
  U3D_REQUIRE(nb < (1LL << 31), "select_probs_fwd: V too large");
  const int nch = atlas ? 2 : 1;
#define LAUNCH(NCV)                                                                                               \
  hipLaunchKernelGGL(select_probs_fwd_kernel<NCV>, dim3((unsigned)nb), dim3(AT), 0, (hipStream_t)stream, logits, \
                     lsc, lsv, C, V, tab, K, atlas, nch, out)
  U3D_NC_DISPATCH(C, LAUNCH)
#undef LAUNCH
  return check_launch("select_probs_fwd");
}

extern "C" int u3d_select_probs_bwd(const float* logits, long long lsc, long long lsv, int C, long long V, int first,
                                    const int* index, int K, const float* grad_out, int nch, float* dlogits,
                                    u3d_stream_t stream) {
  U3D_REQUIRE(logits && grad_out && dlogits && V >= 1 && (nch == 1 || nch == 2), "select_probs_bwd: bad args");
  SelectTable tab;
  int rc = select_table(tab, index, K, first, C, -1);
  if (rc) return rc;
  const long long nb = (V + AT - 1) / AT;
  U3D_REQUIRE(nb < (1LL << 31), "select_probs_bwd: V too large");
#define LAUNCH(NCV)                                                                                               \
  hipLaunchKernelGGL(select_probs_bwd_kernel<NCV>, dim3((unsigned)nb), dim3(AT), 0, (hipStream_t)stream, logits, \
                     lsc, lsv, C, V, tab, grad_out, nch, dlogits)
  U3D_NC_DISPATCH(C, LAUNCH)
#undef LAUNCH
  return check_launch("select_probs_bwd");
}

extern "C" int u3d_dice_metric_atlas(const float* logits, const float* labels, const float* atlas, int natlas, int S,
                                     long long V, int C, int num_class, long long* counts, float* metrics,
                                     long long* argmax, u3d_stream_t stream) {
  U3D_REQUIRE(logits && labels && atlas && counts && metrics, "dice_metric_atlas: null pointer");
  U3D_REQUIRE(C >= 2 && C <= AT_CMAX && num_class >= 1 && num_class <= C - 1 && natlas >= num_class && S >= 1 && V >= 1,
              "dice_metric_atlas: C=%d, num_class=%d (at most C - 1), atlas channels %d", C, num_class, natlas);
  hipStream_t s = (hipStream_t)stream;
  U3D_HIP(hipMemsetAsync(counts, 0, (size_t)S * num_class * 3 * 8, s));
  const int nb = (int)std::min<long long>(AT_DICE_NB, (V + AT - 1) / AT);
#define LAUNCH(NCV)                                                                                           \
  hipLaunchKernelGGL(dice_atlas_count_kernel<NCV>, dim3(nb, S), dim3(AT), 0, s, logits, labels, atlas,       \
                     (long long)natlas * V, V, C, num_class, (unsigned long long*)counts, argmax)
  U3D_NC_DISPATCH(C, LAUNCH)
#undef LAUNCH
  int rc = launch_dice_final((const unsigned long long*)counts, S, num_class, metrics, s);
  if (rc) return rc;
  return check_launch("dice_metric_atlas");
}
