// Weight gradient of the 3^3 convolutions on bf16 NDHWC tensors, halo-brick form (gfx950).
//
//   dW[t][co][ci] = sum_{n, q}  dy[n, q, co] * A[n, q*s + t - 1, ci],   A = relu(gn(x)) (prologue)
//
// One workgroup (8 waves) owns a (32 co) x (32 ci) tile for ALL 27 taps and a range of output bricks
// (BD x BH x BW voxels). Per brick the dy brick and the input halo brick ((BD-1)s+3 x (BH-1)s+3 x (BW-1)s+3
// voxels, GroupNorm+ReLU applied once per element) sit in LDS in their natural channel-contiguous layout;
// the next brick's dy + halo are prefetched into registers while the MFMAs run. Both MFMA operands need
// the voxel index as the k dimension, i.e. a transposed read of channel-contiguous rows:
// ds_read_b64_tr_b16 gives it, and because every lane supplies its own row address the 27 shifted tap
// windows of the halo are read with no data movement (row address = brick voxel row + tap offset). The dy
// fragment is shared by all taps of a wave. Reference: autograd of F.conv3d in Conv3d.forward (unet3D.py:27).
#include "wgrad_brick_body.h"

namespace u3d {

// one workgroup = one run of the body (wgrad_brick_body.h); grid (cin_p / 32, cout_p / 32 / NCO, splits)
template <int BD, int BH, int BW, int S, int NCO = 1, bool BUF = false>
__global__ __launch_bounds__(512, 1) void wgrad_brick_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                            const float* __restrict__ gstat,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ part,
                                                            WBGeom g) {
  __shared__ __attribute__((aligned(16))) char lds[wb_lds_bytes<BD, BH, BW, S, NCO>()];
  wgrad_brick_body<BD, BH, BW, S, NCO, BUF>(lds, (int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)),
                                            (int)(gridDim.x * gridDim.y * gridDim.z), (int)gridDim.x, (int)gridDim.y, dy, x, gstat, gamma, beta, part, g);
}


// ------------------------------------------------------------------------------------------------------
// 1^3 weight gradient (downsample convs, fusion / classifier heads): dW[co][ci] = sum_q dy[q][co] A[q*s][ci].
// No halo: a workgroup streams chunks of 512 output voxels (linear order) of its split; the dy chunk and
// the (strided) A chunk are staged channel-contiguous in LDS, read transposed (ds_read_b64_tr_b16), and the
// 32 k16 steps of a chunk are spread over the 8 waves; the 8 per-wave partial tiles are summed in LDS in
// fixed order at the end (deterministic). Memory-bound by design (16-32 flop/B): the next chunk is
// prefetched into registers while the current one is consumed.
#ifndef U3D_W1_NV
#define U3D_W1_NV 512
#endif
constexpr int W1_NV = U3D_W1_NV;  // output voxels per chunk

struct W1Geom {
  int cin, cout, cin_p, cout_p;
  int id, ih, iw;
  int od, oh, ow;
  long long nvox;  // n * od * oh * ow
  long long per_split;
  int gn_groups;
};

template <int S, bool BUF = false>
__global__ __launch_bounds__(512, 1) void wgrad1_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                       const float* __restrict__ gstat,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ part,
                                                       W1Geom g) {
  constexpr int ROWB = 64, NT = 512, RPP = NT / 4, LD = W1_NV / RPP;  // 4 loads per operand per thread
  __shared__ __attribute__((aligned(16))) char lds[2 * W1_NV * ROWB];
  char* dyt = lds;
  char* at = lds + W1_NV * ROWB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ch = tid & 3, row0 = tid >> 2;
  const TileSplit ts = xcd_tile_split();
  const int ci0 = ts.tx * 32, co0 = ts.ty * 32;
  const long long v0 = (long long)ts.split * g.per_split;
  const long long v1 = min(g.nvox, v0 + g.per_split);
  const bool has_gn = gstat != nullptr;
  const int h = lane >> 5, gq = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int colb = (16 * (gq & 1) + 4 * p) * 2;

  u32x4 pdy[LD], pa[LD];
  int pn[LD];
  f32x2 sc[4], sh[4];
  int gn_n = -1;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;

  // BUF (operands below 2 GiB): branch-free buffer loads with 32-bit offsets and indices (a divergent branch around
  // each prefetch load pulls its wait ahead of the MFMAs it should overlap)
  const auto yrs = __builtin_amdgcn_make_buffer_rsrc((void*)dy, 0, BUF ? (int)(g.nvox * g.cout * 2) : 0, 0x00020000);
  const auto xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)x, 0, BUF ? (int)((long long)g.nvox / ((long long)g.od * g.oh * g.ow) * g.id * g.ih * g.iw * g.cin * 2) : 0,
      0x00020000);
  auto prefetch = [&](long long c0) {
#pragma unroll
    for (int i = 0; i < LD; ++i) {
      const long long v = c0 + row0 + i * RPP;
      if constexpr (BUF) {
        const int vi = (int)v, co = co0 + ch * 8, ci = ci0 + ch * 8;
        const bool ok = v < v1;
        int n, src;
        if (S == 1) {
          n = vi / (g.od * g.oh * g.ow);
          src = vi;
        } else {
          int t = vi;
          const int qw = t % g.ow; t /= g.ow;
          const int qh = t % g.oh; t /= g.oh;
          const int qd = t % g.od;
          n = t / g.od;
          src = ((n * g.id + 2 * qd) * g.ih + 2 * qh) * g.iw + 2 * qw;
        }
        const unsigned ob = ok && co < g.cout ? (unsigned)((vi * g.cout + co) * 2) : 0xFFFFFFF0u;
        const unsigned oa = ok && ci < g.cin ? (unsigned)((src * g.cin + ci) * 2) : 0xFFFFFFF0u;
        pdy[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(yrs, ob, 0, 0));
        pa[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, oa, 0, 0));
        pn[i] = ok ? n : -1;
        continue;
      }
      u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
      int n = -1;
      if (v < v1) {
        const int co = co0 + ch * 8, ci = ci0 + ch * 8;
        if (co < g.cout) b = *reinterpret_cast<const u32x4*>(dy + v * g.cout + co);
        long long src;
        if (S == 1) {
          src = v;
          n = (int)(v / ((long long)g.od * g.oh * g.ow));
        } else {
          long long t = v;
          const int qw = (int)(t % g.ow); t /= g.ow;
          const int qh = (int)(t % g.oh); t /= g.oh;
          const int qd = (int)(t % g.od);
          n = (int)(t / g.od);
          src = (((long long)n * g.id + 2 * qd) * g.ih + 2 * qh) * g.iw + 2 * qw;
        }
        if (ci < g.cin) a = *reinterpret_cast<const u32x4*>(x + src * g.cin + ci);
      }
      pdy[i] = b;
      pa[i] = a;
      pn[i] = n;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < LD; ++i) {
      const int v = row0 + i * RPP;
      u32x4 a = pa[i];
      if (has_gn && pn[i] >= 0) {
        if (pn[i] != gn_n) {
          gn_n = pn[i];
          gn_coef8(gstat, gamma, beta, g.gn_groups, g.cin, gn_n, ci0 + ch * 8, sc, sh);
          if (ci0 + ch * 8 >= g.cin) {  // a chunk of the cin_p padding (gn_coef8 clamps to channel cin - 1): stays zero
#pragma unroll
            for (int k = 0; k < 4; ++k) sc[k] = sh[k] = f32x2{0.f, 0.f};
          }
        }
        a = gn_relu8(a, sc, sh);
      }
      *reinterpret_cast<u32x4*>(dyt + v * ROWB + ch * 16) = pdy[i];
      *reinterpret_cast<u32x4*>(at + v * ROWB + ch * 16) = a;
    }
  };

  if (v0 < v1) {
    prefetch(v0);
    commit();
  }
  __syncthreads();
  for (long long c0 = v0; c0 < v1; c0 += W1_NV) {
    const bool more = c0 + W1_NV < v1;
    prefetch(more ? c0 + W1_NV : c0);
#pragma unroll
    for (int j = 0; j < W1_NV / 16 / 8; ++j) {
      const int ks = wave + 8 * j;
      const int k0 = (ks * 16 + 8 * h + q) * ROWB + colb, k1 = k0 + 4 * ROWB;
      const bf16x8 a = frag_from(tr_read(dyt, k0), tr_read(dyt, k1));
      const bf16x8 b = frag_from(tr_read(at, k0), tr_read(at, k1));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
    __syncthreads();
    if (more) commit();
    __syncthreads();
  }
  // fixed-order sum of the 8 per-wave tiles: D[row = co][col = ci], lane col = lane&31, rows (i&3)+8(i>>2)+4h
  float* red = reinterpret_cast<float*>(lds);
  const int r = lane & 31;
#pragma unroll
  for (int i = 0; i < 16; ++i) red[(wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = acc[i];
  __syncthreads();
  float* pp = part + (long long)ts.split * g.cout_p * g.cin_p;
  for (int e = tid; e < 1024; e += NT) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) s += red[w * 1024 + e];
    const int co = e >> 5, ci = e & 31;
    pp[(long long)(co0 + co) * g.cin_p + ci0 + ci] = s;
  }
}

}  // namespace u3d

using namespace u3d;

static int wgrad_bd() { return opt(OPT_WGRAD_BD) == 2 ? 2 : 3; }  // brick depth of the stride-1 kernel

// stride 2: a workgroup covers two 32-wide output-channel tiles, so the 8x-larger input halo of a stride-2 brick is
// staged (and GroupNorm'd) once for 64 output channels
static int wb_nco(int stride, int cout) { return stride == 2 && opt(OPT_WB_S2CO64) != 0 && round_up(cout, 32) % 64 == 0 ? 2 : 1; }

static void brick_dims(int stride, int* bd, int* bh, int* bw) {
  if (stride == 1) { *bd = wgrad_bd(); *bh = 8; *bw = 16; }
  else { *bd = opt(OPT_WB_S2BD) == 2 ? 2 : 3; *bh = 4; *bw = 8; }
}

extern "C" int u3d_conv_wgrad_brick_splits(int n, int cin, int d, int h, int w, int cout, int stride) {
  int bd, bh, bw;
  brick_dims(stride, &bd, &bh, &bw);
  const int od = (d - 1) / stride + 1, oh = (h - 1) / stride + 1, ow = (w - 1) / stride + 1;
  const long long nb = (long long)n * cdiv(od, bd) * cdiv(oh, bh) * cdiv(ow, bw);
  const long long tiles = (long long)cdiv(cin, 32) * (cdiv(cout, 32) / wb_nco(stride, cout));
  const long long target = std::max(1, opt(OPT_WB_WGS));  // workgroups aimed at
  long long want = std::max(1LL, target / tiles);
  const long long ns = std::max(1LL, std::min(want, nb));
  const long long per = (nb + ns - 1) / ns;
  return (int)((nb + per - 1) / per);  // splits that all receive bricks: no zero-filled slabs
}

extern "C" int u3d_conv_wgrad_brick(const void* dy, const void* x, int n, int cin, int d, int h, int w, int cout,
                                    int stride, const float* gn_stats, const float* gn_gamma, const float* gn_beta,
                                    int gn_groups, float* partials, int nsplit, u3d_stream_t stream) {
  U3D_REQUIRE(dy && x && partials && nsplit >= 1, "wgrad_brick: null pointer");
  U3D_REQUIRE(stride == 1 || stride == 2, "wgrad_brick: stride %d", stride);
  U3D_REQUIRE(cin % 8 == 0 && cout % 8 == 0, "wgrad_brick: channels must be multiples of 8");
  U3D_REQUIRE((long long)nsplit * 27 * round_up(cin, 32) * round_up(cout, 32) * 4 < (1LL << 31),
              "wgrad_brick: partial slabs beyond the 2 GiB offset range");
  U3D_REQUIRE(!gn_stats || (gn_gamma && gn_beta && gn_groups > 0 && cin % gn_groups == 0),
              "wgrad_brick: bad GroupNorm prologue");
  int bd, bh, bw;
  brick_dims(stride, &bd, &bh, &bw);
  WBGeom g;
  wb_geom(n, cin, d, h, w, cout, stride, bd, bh, bw, nsplit, gn_groups, g);
  const int ns_eff = (int)((g.nbricks + g.per_split - 1) / g.per_split);
  hipStream_t s = (hipStream_t)stream;
  if (ns_eff < nsplit)  // trailing slabs would stay unwritten
    U3D_HIP(hipMemsetAsync(partials + (long long)ns_eff * 27 * g.cout_p * g.cin_p, 0,
                           (size_t)(nsplit - ns_eff) * 27 * g.cout_p * g.cin_p * 4, s));
  const int nco = wb_nco(stride, cout);
  dim3 grid(g.cin_p / 32, g.cout_p / 32 / nco, ns_eff);
  // buffer loads where both operands fit the 32-bit offset range (the > 2 GiB whole-volume case keeps 64-bit loads)
  const bool buf = fits_buffer_offsets((long long)n * g.od * g.oh * g.ow * cout * 2) &&
                   fits_buffer_offsets((long long)n * d * h * w * cin * 2);
#define U3D_WB(BD_, BH_, BW_, S_, NCO_)                                                                            \
  do {                                                                                                             \
    if (buf)                                                                                                       \
      hipLaunchKernelGGL((wgrad_brick_kernel<BD_, BH_, BW_, S_, NCO_, true>), grid, dim3(512), 0, s,               \
                         (const bf16*)dy, (const bf16*)x, gn_stats, gn_gamma, gn_beta, partials, g);               \
    else                                                                                                           \
      hipLaunchKernelGGL((wgrad_brick_kernel<BD_, BH_, BW_, S_, NCO_, false>), grid, dim3(512), 0, s,              \
                         (const bf16*)dy, (const bf16*)x, gn_stats, gn_gamma, gn_beta, partials, g);               \
  } while (0)
  if (stride == 2 && bd == 3 && nco == 2) U3D_WB(3, 4, 8, 2, 2);
  else if (stride == 2 && bd == 3) U3D_WB(3, 4, 8, 2, 1);
  else if (stride == 2 && nco == 2) U3D_WB(2, 4, 8, 2, 2);
  else if (stride == 1 && bd == 2) U3D_WB(2, 8, 16, 1, 1);
  else if (stride == 1) U3D_WB(3, 8, 16, 1, 1);
  else U3D_WB(2, 4, 8, 2, 1);
#undef U3D_WB
  return check_launch("wgrad_brick_kernel");
}

extern "C" int u3d_conv_wgrad1_splits(int n, int cin, int d, int h, int w, int cout, int stride) {
  const int od = (d - 1) / stride + 1, oh = (h - 1) / stride + 1, ow = (w - 1) / stride + 1;
  const long long chunks = ((long long)n * od * oh * ow + W1_NV - 1) / W1_NV;
  const long long tiles = (long long)cdiv(cin, 32) * cdiv(cout, 32);
  long long want = std::max(1LL, 256 / tiles);
  const long long ns = std::max(1LL, std::min(want, chunks));
  const long long per = (chunks + ns - 1) / ns;
  return (int)((chunks + per - 1) / per);  // splits that all receive voxels: no zero-filled slabs
}

extern "C" int u3d_conv_wgrad1(const void* dy, const void* x, int n, int cin, int d, int h, int w, int cout, int stride,
                               const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_groups,
                               float* partials, int nsplit, u3d_stream_t stream) {
  U3D_REQUIRE(dy && x && partials && nsplit >= 1, "wgrad1: null pointer");
  U3D_REQUIRE(stride == 1 || stride == 2, "wgrad1: stride %d", stride);
  U3D_REQUIRE(cin % 8 == 0 && cout % 8 == 0, "wgrad1: channels must be multiples of 8");
  U3D_REQUIRE(!gn_stats || (gn_gamma && gn_beta && gn_groups > 0 && cin % gn_groups == 0), "wgrad1: bad GN");
  W1Geom g{};
  g.cin = cin; g.cout = cout; g.cin_p = round_up(cin, 32); g.cout_p = round_up(cout, 32);
  g.id = d; g.ih = h; g.iw = w;
  g.od = (d - 1) / stride + 1; g.oh = (h - 1) / stride + 1; g.ow = (w - 1) / stride + 1;
  g.nvox = (long long)n * g.od * g.oh * g.ow;
  const long long chunks = (g.nvox + W1_NV - 1) / W1_NV;
  g.per_split = (chunks + nsplit - 1) / nsplit * W1_NV;
  g.gn_groups = gn_groups;
  const int ns_eff = (int)((g.nvox + g.per_split - 1) / g.per_split);
  hipStream_t s = (hipStream_t)stream;
  if (ns_eff < nsplit)
    U3D_HIP(hipMemsetAsync(partials + (long long)ns_eff * g.cout_p * g.cin_p, 0,
                           (size_t)(nsplit - ns_eff) * g.cout_p * g.cin_p * 4, s));
  dim3 grid(g.cin_p / 32, g.cout_p / 32, ns_eff);
  // buffer loads and 32-bit indices where both operands fit the 32-bit offset range
  const bool buf = fits_buffer_offsets(g.nvox * cout * 2) && fits_buffer_offsets((long long)n * d * h * w * cin * 2);
#define U3D_W1(S_)                                                                                                \
  do {                                                                                                            \
    if (buf)                                                                                                      \
      hipLaunchKernelGGL((wgrad1_kernel<S_, true>), grid, dim3(512), 0, s, (const bf16*)dy, (const bf16*)x,        \
                         gn_stats, gn_gamma, gn_beta, partials, g);                                               \
    else                                                                                                          \
      hipLaunchKernelGGL((wgrad1_kernel<S_, false>), grid, dim3(512), 0, s, (const bf16*)dy, (const bf16*)x,       \
                         gn_stats, gn_gamma, gn_beta, partials, g);                                               \
  } while (0)
  if (stride == 1) U3D_W1(1);
  else U3D_W1(2);
#undef U3D_W1
  return check_launch("wgrad1_kernel");
}
