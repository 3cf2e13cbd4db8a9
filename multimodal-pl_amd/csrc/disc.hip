// Style discriminators: the 4^3 / stride 2 / pad 1 conv + bias + LeakyReLU(0.2) family, no normalisation.
// Reference: unet3D.py:1832-1849 (get_style_discriminator_output), :1852-1905 (deep_style_discriminator_output),
// :1907-1947 (norm_style_discriminator_output); driven by train_amos_atlas_final.py:320-379.
//
// Activations are NDHWC, read and written through (pointer, pitch) views so a block conv and its side conv fill the two
// channel halves of one buffer (the reference's torch.cat is never materialised) and a data gradient splits back the
// same way. T = bf16 (autocast; fp32 accumulation) or float (parity mode; v_mfma_f32_32x32x2_f32, exact fp32 FMAs).
//
// The inner layers are implicit GEMMs on v_mfma_f32_32x32x16_bf16, one 32 x 32 tile per wave, both operands read
// straight from global memory as 8-element fragments (no LDS: correctness-first kernels):
//   forward   M = output voxels, N = cout, K = 64 taps x cin; K-split over taps with a fixed-order combine;
//   dgrad     8 parity classes in one launch (grid.z); for input x = 2q + p one dimension takes kernel taps
//             p = 0: k = 1 (o = q), k = 3 (o = q - 1);  p = 1: k = 2 (o = q), k = 0 (o = q + 1); K = 8 taps x cout;
//   wgrad     rows = cout, columns = cin, k = voxel; fp32 slabs [split][64][cout][cin], summed in fixed order.
// dy * lrelu'(y) is formed on the fly from the stored post-activation y (slope > 0, so sign(y) = sign(pre-activation)).
// The k order inside an MFMA step is free as long as both operands agree: the float path feeds element j of the same
// 8-element fragments to the j-th 32x32x2 MFMA, so both precisions share the addressing.
// No float atomics: every parameter gradient is a fixed-order sum of per-block partials.
#include "common.h"

namespace u3d {

typedef __attribute__((ext_vector_type(8))) __bf16 dc_bf16x8;
constexpr float DC_SLOPE = 0.2f;

template <typename T> struct alignas(16) Frag { T e[8]; };

template <typename T> __device__ __forceinline__ Frag<T> frag_zero() {
  Frag<T> f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f.e[j] = (T)0;
  return f;
}
template <typename T> __device__ __forceinline__ Frag<T> frag_load(const T* p) {
  return *reinterpret_cast<const Frag<T>*>(p);
}
__device__ __forceinline__ void mma(f32x16& acc, const Frag<bf16>& a, const Frag<bf16>& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(dc_bf16x8, a), __builtin_bit_cast(dc_bf16x8, b), acc,
                                                0, 0, 0);
}
__device__ __forceinline__ void mma(f32x16& acc, const Frag<float>& a, const Frag<float>& b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.e[j], b.e[j], acc, 0, 0, 0);
}
__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : DC_SLOPE * v; }
// dy * lrelu'(y) from the stored output (y == 0 takes the slope, as torch's leaky_relu backward does)
template <typename T> __device__ __forceinline__ float gval(T dy, T y) {
  return to_f(dy) * (to_f(y) > 0.f ? 1.f : DC_SLOPE);
}
template <typename T> __device__ __forceinline__ Frag<T> frag_g(const Frag<T>& dy, const Frag<T>& y) {
  Frag<T> g;
#pragma unroll
  for (int j = 0; j < 8; ++j) g.e[j] = from_f<T>(gval(dy.e[j], y.e[j]));
  return g;
}
__device__ __forceinline__ void decode4(unsigned m, int A, int B, int C, int& n, int& a, int& b, int& c) {
  c = m % (unsigned)C;
  m /= (unsigned)C;
  b = m % (unsigned)B;
  m /= (unsigned)B;
  a = m % (unsigned)A;
  n = m / (unsigned)A;
}
__device__ __forceinline__ bool inr(int v, int n) { return (unsigned)v < (unsigned)n; }
// accumulator register i of lane half h -> row of the 32 x 32 tile (the column is lane & 31)
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// ------------------------------------------------------------------------------------- inner conv, forward
// x [n][Di][Hi][Wi] pitch xp, cin channels; wpk [64][cin / 8][cout][8]; y [n][Do][Ho][Wo] pitch yp.
// grid (ceil(M / 32), ceil(cout / 128), splits); wave w of a block takes co tile 4 * blockIdx.y + w.
template <typename T>
__global__ __launch_bounds__(256) void disc_conv_fwd_kernel(const T* __restrict__ x, int xp, int n, int Di, int Hi,
                                                            int Wi, int cin, const T* __restrict__ wpk,
                                                            const float* __restrict__ bias, T* __restrict__ y, int yp,
                                                            int Do, int Ho, int Wo, int cout, int splits,
                                                            float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int co0 = (blockIdx.y * 4 + wave) * 32;
  if (co0 >= cout) return;
  const unsigned M = (unsigned)n * Do * Ho * Wo;
  const unsigned m = blockIdx.x * 32u + r;
  const bool valid = m < M;
  int nn = 0, od = 0, oh = 0, ow = 0;
  if (valid) decode4(m, Do, Ho, Wo, nn, od, oh, ow);
  const int s = blockIdx.z, tps = 64 / splits, c8 = cin / 8;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int tap = s * tps; tap < (s + 1) * tps; ++tap) {
    const int id = 2 * od - 1 + (tap >> 4), ih = 2 * oh - 1 + ((tap >> 2) & 3), iw = 2 * ow - 1 + (tap & 3);
    const bool inb = valid && inr(id, Di) && inr(ih, Hi) && inr(iw, Wi);
    const T* xa = inb ? x + ((((size_t)nn * Di + id) * Hi + ih) * Wi + iw) * xp + h * 8 : x;
    const T* wb = wpk + ((size_t)(tap * c8 + h) * cout + co0 + r) * 8;
    for (int c = 0; c < cin / 16; ++c) {
      const Frag<T> a = inb ? frag_load(xa + c * 16) : frag_zero<T>();
      const Frag<T> b = frag_load(wb + (size_t)c * 16 * cout);
      mma(acc, a, b);
    }
  }
  const int co = co0 + r;
  const float bv = splits == 1 ? bias[co] : 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const unsigned mo = blockIdx.x * 32u + acc_row(i, h);
    if (mo >= M) continue;
    if (splits == 1)
      y[(size_t)mo * yp + co] = from_f<T>(lrelu(acc[i] + bv));
    else
      part[((size_t)s * M + mo) * cout + co] = acc[i];
  }
}

// y = lrelu(bias + sum over splits in order)
template <typename T>
__global__ __launch_bounds__(256) void disc_conv_combine_kernel(const float* __restrict__ part, int splits, unsigned M,
                                                                int cout, const float* __restrict__ bias,
                                                                T* __restrict__ y, int yp) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)M * cout) return;
  const unsigned m = i / cout;
  const int co = i % cout;
  float v = 0.f;
  for (int s = 0; s < splits; ++s) v += part[(size_t)s * M * cout + i];
  y[(size_t)m * yp + co] = from_f<T>(lrelu(v + bias[co]));
}

// ------------------------------------------------------------------------------------- inner conv, data gradient
// dy, yv [n][Do][Ho][Wo] (pitches dyp, yvp), cout channels; wpk [64][cout / 8][cin][8]; dx [n][Di][Hi][Wi] pitch dxp.
// grid (ceil(Mq / 32), ceil(cin / 128), 8 parity classes), Mq = n * ceil(Di/2) * ceil(Hi/2) * ceil(Wi/2).
template <typename T>
__global__ __launch_bounds__(256) void disc_conv_dgrad_kernel(const T* __restrict__ dy, int dyp,
                                                              const T* __restrict__ yv, int yvp, int n, int Di, int Hi,
                                                              int Wi, int cin, int Do, int Ho, int Wo, int cout,
                                                              const T* __restrict__ wpk, T* __restrict__ dx, int dxp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int ci0 = (blockIdx.y * 4 + wave) * 32;
  if (ci0 >= cin) return;
  const int Qd = (Di + 1) / 2, Qh = (Hi + 1) / 2, Qw = (Wi + 1) / 2;
  const unsigned Mq = (unsigned)n * Qd * Qh * Qw;
  const int pd = blockIdx.z >> 2, ph = (blockIdx.z >> 1) & 1, pw = blockIdx.z & 1;
  const unsigned m = blockIdx.x * 32u + r;
  int nn = 0, qd = 0, qh = 0, qw = 0;
  if (m < Mq) decode4(m, Qd, Qh, Qw, nn, qd, qh, qw);
  const bool valid = m < Mq && 2 * qd + pd < Di && 2 * qh + ph < Hi && 2 * qw + pw < Wi;
  const int c8 = cout / 8;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int t = 0; t < 8; ++t) {
    const int td = t >> 2, th = (t >> 1) & 1, tw = t & 1;
    // p = 0: (k, o) = (1, q), (3, q - 1);  p = 1: (2, q), (0, q + 1)
    const int kd = pd ? 2 - 2 * td : 1 + 2 * td, od = pd ? qd + td : qd - td;
    const int kh = ph ? 2 - 2 * th : 1 + 2 * th, oh = ph ? qh + th : qh - th;
    const int kw = pw ? 2 - 2 * tw : 1 + 2 * tw, ow = pw ? qw + tw : qw - tw;
    const int tap = (kd * 4 + kh) * 4 + kw;
    const bool inb = valid && inr(od, Do) && inr(oh, Ho) && inr(ow, Wo);
    const size_t vox = inb ? (((size_t)nn * Do + od) * Ho + oh) * Wo + ow : 0;
    const T* ga = dy + vox * dyp + h * 8;
    const T* ya = yv + vox * yvp + h * 8;
    const T* wb = wpk + ((size_t)(tap * c8 + h) * cin + ci0 + r) * 8;
    for (int c = 0; c < cout / 16; ++c) {
      const Frag<T> a = inb ? frag_g(frag_load(ga + c * 16), frag_load(ya + c * 16)) : frag_zero<T>();
      const Frag<T> b = frag_load(wb + (size_t)c * 16 * cin);
      mma(acc, a, b);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const unsigned mo = blockIdx.x * 32u + acc_row(i, h);
    if (mo >= Mq) continue;
    int n2, d2, h2, w2;
    decode4(mo, Qd, Qh, Qw, n2, d2, h2, w2);
    const int xd = 2 * d2 + pd, xh = 2 * h2 + ph, xw = 2 * w2 + pw;
    if (xd >= Di || xh >= Hi || xw >= Wi) continue;
    dx[((((size_t)n2 * Di + xd) * Hi + xh) * Wi + xw) * dxp + ci0 + r] = from_f<T>(acc[i]);
  }
}

// ------------------------------------------------------------------------------------- inner conv, weight gradient
// One wave per (co tile, ci tile, kd, kh, split): the four kw taps share the dy fragment. k = voxel: each lane gathers
// its 8 voxels' values of one channel. part [split][64][cout][cin].
template <typename T>
__global__ __launch_bounds__(64) void disc_conv_wgrad_kernel(const T* __restrict__ x, int xp, const T* __restrict__ dy,
                                                             int dyp, const T* __restrict__ yv, int yvp, int n, int Di,
                                                             int Hi, int Wi, int cin, int Do, int Ho, int Wo, int cout,
                                                             unsigned chunk, float* __restrict__ part) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int nci = cin / 32;
  const int co0 = (blockIdx.x / nci) * 32, ci0 = (blockIdx.x % nci) * 32;
  const int kd = blockIdx.y >> 2, kh = blockIdx.y & 3, s = blockIdx.z;
  const unsigned M = (unsigned)n * Do * Ho * Wo;
  const unsigned mbeg = s * chunk, mend = min(M, mbeg + chunk);
  f32x16 acc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[k][i] = 0.f;
  for (unsigned m0 = mbeg; m0 < mend; m0 += 16) {
    Frag<T> a, b[4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned m = m0 + 8 * h + j;
      T av = (T)0, bv[4] = {(T)0, (T)0, (T)0, (T)0};
      if (m < mend) {
        int nn, od, oh, ow;
        decode4(m, Do, Ho, Wo, nn, od, oh, ow);
        av = from_f<T>(gval(dy[(size_t)m * dyp + co0 + r], yv[(size_t)m * yvp + co0 + r]));
        const int id = 2 * od - 1 + kd, ih = 2 * oh - 1 + kh;
        if (inr(id, Di) && inr(ih, Hi)) {
          const T* row = x + (((size_t)nn * Di + id) * Hi + ih) * Wi * xp + ci0 + r;
#pragma unroll
          for (int kw = 0; kw < 4; ++kw) {
            const int iw = 2 * ow - 1 + kw;
            if (inr(iw, Wi)) bv[kw] = row[(size_t)iw * xp];
          }
        }
      }
      a.e[j] = av;
#pragma unroll
      for (int kw = 0; kw < 4; ++kw) b[kw].e[j] = bv[kw];
    }
#pragma unroll
    for (int kw = 0; kw < 4; ++kw) mma(acc[kw], a, b[kw]);
  }
#pragma unroll
  for (int kw = 0; kw < 4; ++kw) {
    const int tap = (kd * 4 + kh) * 4 + kw;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      part[(((size_t)s * 64 + tap) * cout + co0 + acc_row(i, h)) * cin + ci0 + r] = acc[kw][i];
  }
}

// out[(co * I + ci) * K + tap] = sum over parts of part[p][tap][..]; the slab's inner two axes are [ci][co] (co_inner)
// or [co][ci]. Eight lanes share an output: lane j sums parts j, j + 8, ... in order, then the eight sums combine in a
// fixed tree (a + b and b + a are the same bits, so every lane of the group ends with the same value).
__global__ __launch_bounds__(256) void disc_reduce_unpack_kernel(const float* __restrict__ part, int nparts, int K, int I,
                                                                 int O, int co_inner, float* __restrict__ out) {
  const size_t len = (size_t)K * I * O;
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int j = threadIdx.x & 7;
  float v = 0.f;
  if (i < len)
    for (int p = j; p < nparts; p += 8) v += part[(size_t)p * len + i];
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  if (i >= len || j != 0) return;
  int tap, ci, co;
  if (co_inner) {
    co = i % O;
    ci = (i / O) % I;
    tap = i / ((size_t)O * I);
  } else {
    ci = i % I;
    co = (i / I) % O;
    tap = i / ((size_t)O * I);
  }
  out[((size_t)co * I + ci) * K + tap] = v;
}

// ------------------------------------------------------------------------------------- bias gradient
// part [blockIdx.x][C] = sum of dy * lrelu'(y) over the block's rows: eight row classes m = sub (mod 8), combined in
// sub order through LDS
template <typename T>
__global__ __launch_bounds__(256) void disc_bias_grad_kernel(const T* __restrict__ dy, int dyp, const T* __restrict__ yv,
                                                             int yvp, unsigned M, int C, unsigned rows,
                                                             float* __restrict__ part) {
  const int c = blockIdx.y * 32 + (threadIdx.x & 31), sub = threadIdx.x >> 5;
  const unsigned mend = min(M, (blockIdx.x + 1) * rows);
  float acc = 0.f;
  for (unsigned m = blockIdx.x * rows + sub; m < mend; m += 8) acc += gval(dy[(size_t)m * dyp + c], yv[(size_t)m * yvp + c]);
  __shared__ float s_acc[8][32];
  s_acc[sub][threadIdx.x & 31] = acc;
  __syncthreads();
  if (sub == 0) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += s_acc[k][threadIdx.x];
    part[(size_t)blockIdx.x * C + c] = v;
  }
}

// ------------------------------------------------------------------------------------- first layer (cin <= 4)
// x fp32 NCDHW [n][C][Di][Hi][Wi]; w1 fp32 [64][C][cout]; 8 output voxels x 32 channels per block.
template <typename T>
__global__ __launch_bounds__(256) void disc_first_fwd_kernel(const float* __restrict__ x, int n, int C, int Di, int Hi,
                                                             int Wi, const float* __restrict__ w1,
                                                             const float* __restrict__ bias, T* __restrict__ y, int yp,
                                                             int Do, int Ho, int Wo, int cout) {
  const int co = blockIdx.y * 32 + (threadIdx.x & 31);
  const unsigned M = (unsigned)n * Do * Ho * Wo;
  const unsigned m = blockIdx.x * 8u + (threadIdx.x >> 5);
  if (m >= M) return;
  int nn, od, oh, ow;
  decode4(m, Do, Ho, Wo, nn, od, oh, ow);
  float acc = bias[co];
  for (int tap = 0; tap < 64; ++tap) {
    const int id = 2 * od - 1 + (tap >> 4), ih = 2 * oh - 1 + ((tap >> 2) & 3), iw = 2 * ow - 1 + (tap & 3);
    if (!(inr(id, Di) && inr(ih, Hi) && inr(iw, Wi))) continue;
    for (int ci = 0; ci < C; ++ci)
      acc = fmaf(x[((((size_t)nn * C + ci) * Di + id) * Hi + ih) * Wi + iw], w1[(size_t)(tap * C + ci) * cout + co], acc);
  }
  y[(size_t)m * yp + co] = from_f<T>(lrelu(acc));
}

// dx fp32 NCDHW; one thread per (n, ci, input voxel)
template <typename T>
__global__ __launch_bounds__(256) void disc_first_dgrad_kernel(const T* __restrict__ dy, int dyp,
                                                               const T* __restrict__ yv, int yvp, int n, int C, int Di,
                                                               int Hi, int Wi, int Do, int Ho, int Wo, int cout,
                                                               const float* __restrict__ w1, float* __restrict__ dx) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t vol = (size_t)Di * Hi * Wi;
  if (i >= (size_t)n * C * vol) return;
  const int xw = i % Wi, xh = (i / Wi) % Hi, xd = (i / ((size_t)Wi * Hi)) % Di;
  const int ci = (i / vol) % C, nn = i / (vol * C);
  float acc = 0.f;
  for (int kd = (xd + 1) & 1; kd < 4; kd += 2) {
    const int od = (xd + 1 - kd) / 2;  // xd + 1 - kd is even
    if (xd + 1 - kd < 0 || od >= Do) continue;
    for (int kh = (xh + 1) & 1; kh < 4; kh += 2) {
      const int oh = (xh + 1 - kh) / 2;
      if (xh + 1 - kh < 0 || oh >= Ho) continue;
      for (int kw = (xw + 1) & 1; kw < 4; kw += 2) {
        const int ow = (xw + 1 - kw) / 2;
        if (xw + 1 - kw < 0 || ow >= Wo) continue;
        const size_t vox = (((size_t)nn * Do + od) * Ho + oh) * Wo + ow;
        const float* wr = w1 + (size_t)(((kd * 4 + kh) * 4 + kw) * C + ci) * cout;
        for (int c = 0; c < cout; c += 8) {
          const Frag<T> g = frag_load(dy + vox * dyp + c), yy = frag_load(yv + vox * yvp + c);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc = fmaf(gval(g.e[j], yy.e[j]), wr[c + j], acc);
        }
      }
    }
  }
  dx[i] = acc;
}

// part [blockIdx.x][64][C][cout]; thread (co, group of 8 taps: kd, kh pair)
template <typename T>
__global__ __launch_bounds__(256) void disc_first_wgrad_kernel(const float* __restrict__ x, const T* __restrict__ dy,
                                                               int dyp, const T* __restrict__ yv, int yvp, int n, int C,
                                                               int Di, int Hi, int Wi, int Do, int Ho, int Wo, int cout,
                                                               unsigned rows, float* __restrict__ part) {
  const int co = blockIdx.y * 32 + (threadIdx.x & 31), tg = threadIdx.x >> 5;
  const int kd = tg >> 1, kh0 = (tg & 1) * 2;
  const unsigned M = (unsigned)n * Do * Ho * Wo;
  const unsigned mend = min(M, (blockIdx.x + 1) * rows);
  float acc[8][4];
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) acc[t][ci] = 0.f;
  for (unsigned m = blockIdx.x * rows; m < mend; ++m) {
    int nn, od, oh, ow;
    decode4(m, Do, Ho, Wo, nn, od, oh, ow);
    const float g = gval(dy[(size_t)m * dyp + co], yv[(size_t)m * yvp + co]);
    const int id = 2 * od - 1 + kd;
    if (!inr(id, Di)) continue;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int ih = 2 * oh - 1 + kh0 + (t >> 2), iw = 2 * ow - 1 + (t & 3);
      if (!(inr(ih, Hi) && inr(iw, Wi))) continue;
#pragma unroll
      for (int ci = 0; ci < 4; ++ci)
        if (ci < C) acc[t][ci] = fmaf(g, x[((((size_t)nn * C + ci) * Di + id) * Hi + ih) * Wi + iw], acc[t][ci]);
    }
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int tap = (kd * 4 + kh0 + (t >> 2)) * 4 + (t & 3);
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
      if (ci < C) part[(((size_t)blockIdx.x * 64 + tap) * C + ci) * cout + co] = acc[t][ci];
  }
}

// ------------------------------------------------------------------------------------- side conv (1 -> C, 3^3, s1, p1)
// f fp32 [n][D][H][W]; ws fp32 [27][C]
template <typename T>
__global__ __launch_bounds__(256) void disc_side_fwd_kernel(const float* __restrict__ f, int n, int D, int H, int W,
                                                            const float* __restrict__ ws, const float* __restrict__ bias,
                                                            T* __restrict__ y, int yp, int C) {
  const int co = blockIdx.y * 32 + (threadIdx.x & 31);
  const unsigned M = (unsigned)n * D * H * W;
  const unsigned m = blockIdx.x * 8u + (threadIdx.x >> 5);
  if (m >= M) return;
  int nn, d, hh, w;
  decode4(m, D, H, W, nn, d, hh, w);
  float acc = bias[co];
  for (int tap = 0; tap < 27; ++tap) {
    const int id = d - 1 + tap / 9, ih = hh - 1 + (tap / 3) % 3, iw = w - 1 + tap % 3;
    if (inr(id, D) && inr(ih, H) && inr(iw, W))
      acc = fmaf(f[(((size_t)nn * D + id) * H + ih) * W + iw], ws[tap * C + co], acc);
  }
  y[(size_t)m * yp + co] = from_f<T>(lrelu(acc));
}

template <typename T>
__global__ __launch_bounds__(256) void disc_side_dgrad_kernel(const T* __restrict__ dy, int dyp, const T* __restrict__ yv,
                                                              int yvp, int n, int D, int H, int W, int C,
                                                              const float* __restrict__ ws, float* __restrict__ df) {
  const unsigned M = (unsigned)n * D * H * W;
  const unsigned m = blockIdx.x * 256u + threadIdx.x;
  if (m >= M) return;
  int nn, d, hh, w;
  decode4(m, D, H, W, nn, d, hh, w);
  float acc = 0.f;
  for (int tap = 0; tap < 27; ++tap) {
    const int od = d + 1 - tap / 9, oh = hh + 1 - (tap / 3) % 3, ow = w + 1 - tap % 3;
    if (!(inr(od, D) && inr(oh, H) && inr(ow, W))) continue;
    const size_t vox = (((size_t)nn * D + od) * H + oh) * W + ow;
    for (int c = 0; c < C; c += 8) {
      const Frag<T> g = frag_load(dy + vox * dyp + c), yy = frag_load(yv + vox * yvp + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = fmaf(gval(g.e[j], yy.e[j]), ws[tap * C + c + j], acc);
    }
  }
  df[m] = acc;
}

// part [blockIdx.x][27][C]; thread (co, tap group g: taps g, g + 8, g + 16, g + 24)
template <typename T>
__global__ __launch_bounds__(256) void disc_side_wgrad_kernel(const float* __restrict__ f, const T* __restrict__ dy,
                                                              int dyp, const T* __restrict__ yv, int yvp, int n, int D,
                                                              int H, int W, int C, unsigned rows,
                                                              float* __restrict__ part) {
  const int co = blockIdx.y * 32 + (threadIdx.x & 31), tg = threadIdx.x >> 5;
  const unsigned M = (unsigned)n * D * H * W;
  const unsigned mend = min(M, (blockIdx.x + 1) * rows);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (unsigned m = blockIdx.x * rows; m < mend; ++m) {
    int nn, d, hh, w;
    decode4(m, D, H, W, nn, d, hh, w);
    const float g = gval(dy[(size_t)m * dyp + co], yv[(size_t)m * yvp + co]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int tap = tg + 8 * q;
      if (tap >= 27) continue;
      const int id = d - 1 + tap / 9, ih = hh - 1 + (tap / 3) % 3, iw = w - 1 + tap % 3;
      if (inr(id, D) && inr(ih, H) && inr(iw, W)) acc[q] = fmaf(g, f[(((size_t)nn * D + id) * H + ih) * W + iw], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int tap = tg + 8 * q;
    if (tap < 27) part[((size_t)blockIdx.x * 27 + tap) * C + co] = acc[q];
  }
}

// ------------------------------------------------------------------------------------- host helpers
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int odim(int d) { return d / 2; }
static long long vox4(int n, int d, int h, int w) { return (long long)n * d * h * w; }
constexpr long long DC_MAXM = (1LL << 31) - 64;

// blocks and rows per block of the partial-sum kernels (first / side weight gradient, bias gradient)
static void part_blocks(long long M, int max_blocks, unsigned* nblk, unsigned* rows) {
  long long r = std::max<long long>(64, (M + max_blocks - 1) / max_blocks);
  *rows = (unsigned)r;
  *nblk = (unsigned)((M + r - 1) / r);
}
constexpr int DC_BIAS_BLOCKS = 2048, DC_FIRST_BLOCKS = 4096, DC_SIDE_BLOCKS = 4096;

static int view_ok(const char* what, const void* p, int pitch, int off, int C) {
  U3D_REQUIRE(p && pitch >= off + C && off >= 0 && pitch % 8 == 0 && off % 8 == 0 && aligned16(p),
              "%s: bad view (pitch %d, offset %d, %d channels; pitch and offset must be multiples of 8)", what, pitch,
              off, C);
  return U3D_OK;
}
#define DC_VIEW(what, p, pitch, off, C)                         \
  do {                                                          \
    int rc_ = view_ok(what, p, pitch, off, C);            \
    if (rc_) return rc_;                                        \
  } while (0)
#define DC_DISPATCH(dt, ...)                      \
  do {                                            \
    if ((dt) == U3D_BF16) {                       \
      typedef bf16 T;                             \
      __VA_ARGS__;                                \
    } else {                                      \
      typedef float T;                            \
      __VA_ARGS__;                                \
    }                                             \
  } while (0)

}  // namespace u3d

using namespace u3d;

extern "C" int u3d_disc_conv_fwd_splits(int n, int d, int h, int w, int cin, int cout) {
  // d, h, w: input dims. Aim at ~1024 waves; a split owns whole taps (64 / splits each).
  const long long M = vox4(n, odim(d), odim(h), odim(w));
  if (M <= 0 || cout <= 0) return 1;
  const long long waves = (M + 31) / 32 * (cout / 32);
  int s = 1;
  while (s < 64 && waves * s < 1024) s *= 2;
  return s;
}

extern "C" long long u3d_disc_conv_fwd_ws_bytes(int n, int d, int h, int w, int cout, int splits) {
  if (splits <= 1) return 0;
  return vox4(n, odim(d), odim(h), odim(w)) * cout * splits * (long long)sizeof(float);
}

extern "C" int u3d_disc_conv_fwd(int dt, const void* x, int xp, int xo, int n, int d, int h, int w, int cin,
                                 const void* wpk, const float* bias, void* y, int yp, int yo, int cout, int splits,
                                 float* ws, u3d_stream_t stream) {
  U3D_REQUIRE(dt == U3D_F32 || dt == U3D_BF16, "disc_conv_fwd: dtype");
  U3D_REQUIRE(n > 0 && d >= 2 && h >= 2 && w >= 2, "disc_conv_fwd: every spatial dim must be >= 2 (got %dx%dx%d)", d, h,
              w);
  U3D_REQUIRE(cin > 0 && cout > 0 && cin % 32 == 0 && cout % 32 == 0,
              "disc_conv_fwd: cin and cout must be multiples of 32 (got %d -> %d)", cin, cout);
  U3D_REQUIRE(splits >= 1 && splits <= 64 && (splits & (splits - 1)) == 0, "disc_conv_fwd: splits must be 1..64, 2^k");
  U3D_REQUIRE(wpk && bias && aligned16(wpk) && (splits == 1 || ws), "disc_conv_fwd: null / unaligned buffer");
  DC_VIEW("disc_conv_fwd x", x, xp, xo, cin);
  DC_VIEW("disc_conv_fwd y", y, yp, yo, cout);
  const int Do = odim(d), Ho = odim(h), Wo = odim(w);
  const long long M = vox4(n, Do, Ho, Wo);
  U3D_REQUIRE(M < DC_MAXM && vox4(n, d, h, w) < DC_MAXM, "disc_conv_fwd: more than 2^31 voxels");
  const dim3 grid((unsigned)((M + 31) / 32), (unsigned)((cout + 127) / 128), (unsigned)splits);
  DC_DISPATCH(dt, {
    hipLaunchKernelGGL(disc_conv_fwd_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)x + xo, xp, n, d, h, w,
                       cin, (const T*)wpk, bias, (T*)y + yo, yp, Do, Ho, Wo, cout, splits, ws);
    if (splits > 1) {
      const long long tot = M * cout;
      hipLaunchKernelGGL(disc_conv_combine_kernel<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                         (hipStream_t)stream, ws, splits, (unsigned)M, cout, bias, (T*)y + yo, yp);
    }
  });
  return check_launch("disc_conv_fwd");
}

extern "C" int u3d_disc_conv_dgrad(int dt, const void* dy, int dyp, int dyo, const void* y, int yp, int yo, int n, int d,
                                   int h, int w, int cin, int cout, const void* wpk, void* dx, int dxp, int dxo,
                                   u3d_stream_t stream) {
  U3D_REQUIRE(dt == U3D_F32 || dt == U3D_BF16, "disc_conv_dgrad: dtype");
  U3D_REQUIRE(n > 0 && d >= 2 && h >= 2 && w >= 2, "disc_conv_dgrad: every spatial dim must be >= 2");
  U3D_REQUIRE(cin > 0 && cout > 0 && cin % 32 == 0 && cout % 32 == 0,
              "disc_conv_dgrad: cin and cout must be multiples of 32 (got %d -> %d)", cin, cout);
  U3D_REQUIRE(wpk && aligned16(wpk), "disc_conv_dgrad: null / unaligned weights");
  DC_VIEW("disc_conv_dgrad dy", dy, dyp, dyo, cout);
  DC_VIEW("disc_conv_dgrad y", y, yp, yo, cout);
  DC_VIEW("disc_conv_dgrad dx", dx, dxp, dxo, cin);
  U3D_REQUIRE(vox4(n, d, h, w) < DC_MAXM, "disc_conv_dgrad: more than 2^31 voxels");
  const long long Mq = vox4(n, (d + 1) / 2, (h + 1) / 2, (w + 1) / 2);
  const dim3 grid((unsigned)((Mq + 31) / 32), (unsigned)((cin + 127) / 128), 8);
  DC_DISPATCH(dt, {
    hipLaunchKernelGGL(disc_conv_dgrad_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)dy + dyo, dyp,
                       (const T*)y + yo, yp, n, d, h, w, cin, odim(d), odim(h), odim(w), cout, (const T*)wpk,
                       (T*)dx + dxo, dxp);
  });
  return check_launch("disc_conv_dgrad");
}

extern "C" int u3d_disc_conv_wgrad_splits(int n, int d, int h, int w, int cin, int cout) {
  const long long M = vox4(n, odim(d), odim(h), odim(w));
  if (M <= 0 || cin <= 0 || cout <= 0) return 1;
  const long long waves = 16LL * (cin / 32) * (cout / 32);
  long long s = (2048 + waves - 1) / waves;
  s = std::min<long long>(s, (M + 255) / 256);  // at least 256 voxels per split
  return (int)std::max<long long>(1, std::min<long long>(s, 64));
}

extern "C" long long u3d_disc_conv_wgrad_ws_bytes(int cin, int cout, int splits) {
  return (long long)std::max(splits, 1) * 64 * cin * cout * (long long)sizeof(float);
}

extern "C" int u3d_disc_conv_wgrad(int dt, const void* x, int xp, int xo, const void* dy, int dyp, int dyo,
                                   const void* y, int yp, int yo, int n, int d, int h, int w, int cin, int cout,
                                   int splits, float* ws, float* dw, u3d_stream_t stream) {
  U3D_REQUIRE(dt == U3D_F32 || dt == U3D_BF16, "disc_conv_wgrad: dtype");
  U3D_REQUIRE(n > 0 && d >= 2 && h >= 2 && w >= 2, "disc_conv_wgrad: every spatial dim must be >= 2");
  U3D_REQUIRE(cin > 0 && cout > 0 && cin % 32 == 0 && cout % 32 == 0,
              "disc_conv_wgrad: cin and cout must be multiples of 32 (got %d -> %d)", cin, cout);
  U3D_REQUIRE(splits >= 1 && splits <= 64 && ws && dw, "disc_conv_wgrad: splits must be 1..64, buffers non-null");
  DC_VIEW("disc_conv_wgrad x", x, xp, xo, cin);
  DC_VIEW("disc_conv_wgrad dy", dy, dyp, dyo, cout);
  DC_VIEW("disc_conv_wgrad y", y, yp, yo, cout);
  const int Do = odim(d), Ho = odim(h), Wo = odim(w);
  const long long M = vox4(n, Do, Ho, Wo);
  U3D_REQUIRE(M < DC_MAXM && vox4(n, d, h, w) < DC_MAXM, "disc_conv_wgrad: more than 2^31 voxels");
  const unsigned chunk = (unsigned)(((M + splits - 1) / splits + 15) / 16 * 16);
  const dim3 grid((unsigned)((cin / 32) * (cout / 32)), 16, (unsigned)splits);
  DC_DISPATCH(dt, {
    hipLaunchKernelGGL(disc_conv_wgrad_kernel<T>, grid, dim3(64), 0, (hipStream_t)stream, (const T*)x + xo, xp,
                       (const T*)dy + dyo, dyp, (const T*)y + yo, yp, n, d, h, w, cin, Do, Ho, Wo, cout, chunk, ws);
  });
  const long long len = 64LL * cin * cout;
  hipLaunchKernelGGL(disc_reduce_unpack_kernel, dim3((unsigned)((len * 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ws, splits, 64, cin, cout, 0, dw);
  return check_launch("disc_conv_wgrad");
}

extern "C" long long u3d_disc_bias_grad_ws_bytes(long long M, int C) {
  unsigned nblk, rows;
  part_blocks(std::max<long long>(M, 1), DC_BIAS_BLOCKS, &nblk, &rows);
  return (long long)nblk * C * (long long)sizeof(float);
}

extern "C" int u3d_disc_bias_grad(int dt, const void* dy, int dyp, int dyo, const void* y, int yp, int yo, long long M,
                                  int C, float* ws, float* db, u3d_stream_t stream) {
  U3D_REQUIRE(dt == U3D_F32 || dt == U3D_BF16, "disc_bias_grad: dtype");
  U3D_REQUIRE(M > 0 && M < DC_MAXM && C > 0 && C % 32 == 0 && ws && db, "disc_bias_grad: bad arguments");
  DC_VIEW("disc_bias_grad dy", dy, dyp, dyo, C);
  DC_VIEW("disc_bias_grad y", y, yp, yo, C);
  unsigned nblk, rows;
  part_blocks(M, DC_BIAS_BLOCKS, &nblk, &rows);
  DC_DISPATCH(dt, {
    hipLaunchKernelGGL(disc_bias_grad_kernel<T>, dim3(nblk, (unsigned)(C / 32)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)dy + dyo, dyp, (const T*)y + yo, yp, (unsigned)M, C, rows, ws);
  });
  hipLaunchKernelGGL(disc_reduce_unpack_kernel, dim3((unsigned)((C * 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ws, (int)nblk, 1, 1, C, 1, db);
  return check_launch("disc_bias_grad");
}

static int first_args(const char* what, int dt, int n, int C, int d, int h, int w, int cout) {
  U3D_REQUIRE(dt == U3D_F32 || dt == U3D_BF16, "%s: dtype", what);
  U3D_REQUIRE(n > 0 && d >= 2 && h >= 2 && w >= 2, "%s: every spatial dim must be >= 2 (got %dx%dx%d)", what, d, h, w);
  U3D_REQUIRE(C >= 1 && C <= 4, "%s: 1 <= num_classes <= 4 (got %d)", what, C);
  U3D_REQUIRE(cout > 0 && cout % 32 == 0, "%s: ndf must be a multiple of 32 (got %d)", what, cout);
  U3D_REQUIRE(vox4(n, d, h, w) * C < DC_MAXM, "%s: more than 2^31 input elements", what);
  return U3D_OK;
}

extern "C" int u3d_disc_first_fwd(int dt, const float* x, int n, int C, int d, int h, int w, const float* w1,
                                  const float* bias, void* y, int yp, int yo, int cout, u3d_stream_t stream) {
  if (int rc = first_args("disc_first_fwd", dt, n, C, d, h, w, cout)) return rc;
  U3D_REQUIRE(x && w1 && bias, "disc_first_fwd: null buffer");
  DC_VIEW("disc_first_fwd y", y, yp, yo, cout);
  const long long M = vox4(n, odim(d), odim(h), odim(w));
  const dim3 grid((unsigned)((M + 7) / 8), (unsigned)(cout / 32));
  DC_DISPATCH(dt, {
    hipLaunchKernelGGL(disc_first_fwd_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, x, n, C, d, h, w, w1, bias,
                       (T*)y + yo, yp, odim(d), odim(h), odim(w), cout);
  });
  return check_launch("disc_first_fwd");
}

extern "C" int u3d_disc_first_dgrad(int dt, const void* dy, int dyp, int dyo, const void* y, int yp, int yo, int n, int C,
                                    int d, int h, int w, int cout, const float* w1, float* dx, u3d_stream_t stream) {
  if (int rc = first_args("disc_first_dgrad", dt, n, C, d, h, w, cout)) return rc;
  U3D_REQUIRE(w1 && dx, "disc_first_dgrad: null buffer");
  DC_VIEW("disc_first_dgrad dy", dy, dyp, dyo, cout);
  DC_VIEW("disc_first_dgrad y", y, yp, yo, cout);
  const long long tot = vox4(n, d, h, w) * C;
  DC_DISPATCH(dt, {
    hipLaunchKernelGGL(disc_first_dgrad_kernel<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)dy + dyo, dyp, (const T*)y + yo, yp, n, C, d, h, w, odim(d), odim(h), odim(w), cout, w1,
                       dx);
  });
  return check_launch("disc_first_dgrad");
}

extern "C" long long u3d_disc_first_wgrad_ws_bytes(int n, int d, int h, int w, int C, int cout) {
  unsigned nblk, rows;
  part_blocks(std::max<long long>(vox4(n, odim(d), odim(h), odim(w)), 1), DC_FIRST_BLOCKS, &nblk, &rows);
  return (long long)nblk * 64 * C * cout * (long long)sizeof(float);
}

extern "C" int u3d_disc_first_wgrad(int dt, const float* x, const void* dy, int dyp, int dyo, const void* y, int yp,
                                    int yo, int n, int C, int d, int h, int w, int cout, float* ws, float* dw,
                                    u3d_stream_t stream) {
  if (int rc = first_args("disc_first_wgrad", dt, n, C, d, h, w, cout)) return rc;
  U3D_REQUIRE(x && ws && dw, "disc_first_wgrad: null buffer");
  DC_VIEW("disc_first_wgrad dy", dy, dyp, dyo, cout);
  DC_VIEW("disc_first_wgrad y", y, yp, yo, cout);
  const long long M = vox4(n, odim(d), odim(h), odim(w));
  unsigned nblk, rows;
  part_blocks(M, DC_FIRST_BLOCKS, &nblk, &rows);
  DC_DISPATCH(dt, {
    hipLaunchKernelGGL(disc_first_wgrad_kernel<T>, dim3(nblk, (unsigned)(cout / 32)), dim3(256), 0, (hipStream_t)stream,
                       x, (const T*)dy + dyo, dyp, (const T*)y + yo, yp, n, C, d, h, w, odim(d), odim(h), odim(w), cout,
                       rows, ws);
  });
  const long long len = 64LL * C * cout;
  hipLaunchKernelGGL(disc_reduce_unpack_kernel, dim3((unsigned)((len * 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ws, (int)nblk, 64, C, cout, 1, dw);
  return check_launch("disc_first_wgrad");
}

static int side_args(const char* what, int dt, int n, int d, int h, int w, int C) {
  U3D_REQUIRE(dt == U3D_F32 || dt == U3D_BF16, "%s: dtype", what);
  U3D_REQUIRE(n > 0 && d >= 1 && h >= 1 && w >= 1 && vox4(n, d, h, w) < DC_MAXM, "%s: bad volume %dx%dx%dx%d", what, n,
              d, h, w);
  U3D_REQUIRE(C > 0 && C % 32 == 0, "%s: channels must be a multiple of 32 (got %d)", what, C);
  return U3D_OK;
}

extern "C" int u3d_disc_side_fwd(int dt, const float* f, int n, int d, int h, int w, const float* wsd, const float* bias,
                                 void* y, int yp, int yo, int C, u3d_stream_t stream) {
  if (int rc = side_args("disc_side_fwd", dt, n, d, h, w, C)) return rc;
  U3D_REQUIRE(f && wsd && bias, "disc_side_fwd: null buffer");
  DC_VIEW("disc_side_fwd y", y, yp, yo, C);
  const long long M = vox4(n, d, h, w);
  DC_DISPATCH(dt, {
    hipLaunchKernelGGL(disc_side_fwd_kernel<T>, dim3((unsigned)((M + 7) / 8), (unsigned)(C / 32)), dim3(256), 0,
                       (hipStream_t)stream, f, n, d, h, w, wsd, bias, (T*)y + yo, yp, C);
  });
  return check_launch("disc_side_fwd");
}

extern "C" int u3d_disc_side_dgrad(int dt, const void* dy, int dyp, int dyo, const void* y, int yp, int yo, int n, int d,
                                   int h, int w, int C, const float* wsd, float* df, u3d_stream_t stream) {
  if (int rc = side_args("disc_side_dgrad", dt, n, d, h, w, C)) return rc;
  U3D_REQUIRE(wsd && df, "disc_side_dgrad: null buffer");
  DC_VIEW("disc_side_dgrad dy", dy, dyp, dyo, C);
  DC_VIEW("disc_side_dgrad y", y, yp, yo, C);
  const long long M = vox4(n, d, h, w);
  DC_DISPATCH(dt, {
    hipLaunchKernelGGL(disc_side_dgrad_kernel<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)dy + dyo, dyp, (const T*)y + yo, yp, n, d, h, w, C, wsd, df);
  });
  return check_launch("disc_side_dgrad");
}

extern "C" long long u3d_disc_side_wgrad_ws_bytes(int n, int d, int h, int w, int C) {
  unsigned nblk, rows;
  part_blocks(std::max<long long>(vox4(n, d, h, w), 1), DC_SIDE_BLOCKS, &nblk, &rows);
  return (long long)nblk * 27 * C * (long long)sizeof(float);
}

extern "C" int u3d_disc_side_wgrad(int dt, const float* f, const void* dy, int dyp, int dyo, const void* y, int yp, int yo,
                                   int n, int d, int h, int w, int C, float* ws, float* dw, u3d_stream_t stream) {
  if (int rc = side_args("disc_side_wgrad", dt, n, d, h, w, C)) return rc;
  U3D_REQUIRE(f && ws && dw, "disc_side_wgrad: null buffer");
  DC_VIEW("disc_side_wgrad dy", dy, dyp, dyo, C);
  DC_VIEW("disc_side_wgrad y", y, yp, yo, C);
  const long long M = vox4(n, d, h, w);
  unsigned nblk, rows;
  part_blocks(M, DC_SIDE_BLOCKS, &nblk, &rows);
  DC_DISPATCH(dt, {
    hipLaunchKernelGGL(disc_side_wgrad_kernel<T>, dim3(nblk, (unsigned)(C / 32)), dim3(256), 0, (hipStream_t)stream, f,
                       (const T*)dy + dyo, dyp, (const T*)y + yo, yp, n, d, h, w, C, rows, ws);
  });
  const long long len = 27LL * C;
  hipLaunchKernelGGL(disc_reduce_unpack_kernel, dim3((unsigned)((len * 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ws, (int)nblk, 27, 1, C, 1, dw);
  return check_launch("disc_side_wgrad");
}
