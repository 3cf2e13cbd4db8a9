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
//
// This header holds the workgroup body, callable from more than one kernel: wgrad_brick_kernel (wgrad_brick.hip) and
// the paired backward launch (small_pair.hip). The body never reads blockIdx / gridDim: the caller passes the
// workgroup's linear index in the body's own sub-grid (channel tiles x splits, x fastest), that sub-grid's size and
// the LDS base (wb_lds_bytes<BD, BH, BW, S, NCO>() bytes, 16-B aligned).
#pragma once
#include <cstdlib>
#include <type_traits>

#include "common.h"

namespace u3d {

typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
struct WBGeom {
  int n;
  int cin, cout, cin_p, cout_p;
  int id, ih, iw;
  int od, oh, ow;
  int nbd, nbh, nbw;  // bricks per dim
  long long nbricks;  // n * nbd * nbh * nbw
  long long per_split;
  int gn_groups;
};

__device__ __forceinline__ v4i16 tr_read(const char* lds_base, int byte_off) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_v4i16*)((__attribute__((address_space(3))) char*)lds_base + byte_off));
}

__device__ __forceinline__ bf16x8 frag_from(v4i16 lo, v4i16 hi) {
  typedef short v8i16 __attribute__((ext_vector_type(8)));
  v8i16 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// BUF: operands below 2 GiB -> branch-free buffer loads with 32-bit offsets (a masked piece reads zeros at the
// sentinel offset; a divergent branch around each prefetch load pulls its wait ahead of the MFMAs it should overlap)
// the body's LDS: the dy brick and the input halo brick, rows channel-contiguous
template <int BD, int BH, int BW, int S, int NCO>
constexpr int wb_lds_bytes() {
  return BD * BH * BW * 64 * NCO + ((BD - 1) * S + 3) * ((BH - 1) * S + 3) * ((BW - 1) * S + 3) * 64;
}

// bricks and the brick range per split of a launch (host); bd x bh x bw = the kernel's output brick
inline void wb_geom(int n, int cin, int d, int h, int w, int cout, int stride, int bd, int bh, int bw, int nsplit,
                    int gn_groups, WBGeom& g) {
  g = WBGeom{};
  g.n = n;
  g.cin = cin; g.cout = cout; g.cin_p = round_up(cin, 32); g.cout_p = round_up(cout, 32);
  g.id = d; g.ih = h; g.iw = w;
  g.od = (d - 1) / stride + 1; g.oh = (h - 1) / stride + 1; g.ow = (w - 1) / stride + 1;
  g.nbd = cdiv(g.od, bd); g.nbh = cdiv(g.oh, bh); g.nbw = cdiv(g.ow, bw);
  g.nbricks = (long long)n * g.nbd * g.nbh * g.nbw;
  g.per_split = (g.nbricks + nsplit - 1) / nsplit;
  g.gn_groups = gn_groups;
}

// wg: this workgroup's index in [0, nwg), nwg = gx * gy * splits with gx = cin_p / 32 and gy = cout_p / 32 / NCO the
// channel tiles
template <int BD, int BH, int BW, int S, int NCO, bool BUF>
__device__ __forceinline__ void wgrad_brick_body(char* const lds, const int wg, const int nwg, const int gx,
                                                 const int gy,
                                                 const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                 const float* __restrict__ gstat, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float* __restrict__ part,
                                                 const WBGeom& g) {
  constexpr int NV = BD * BH * BW, NKS = NV / 16;
  constexpr int HD = (BD - 1) * S + 3, HH = (BH - 1) * S + 3, HW = (BW - 1) * S + 3, NH = HD * HH * HW;
  constexpr int ROWB = 64;           // 32 bf16 channels per LDS halo row
  constexpr int DROWB = 64 * NCO;    // dy rows: the NCO output-channel tiles of the workgroup side by side
  constexpr int NT = 512;
  constexpr int RPP = NT / 4;                       // halo rows per pass (thread t: chunk t&3 of row t>>2)
  constexpr int DCH = 4 * NCO, DRPP = NT / DCH;     // dy: 8-channel chunks per row, rows per pass
  constexpr int DYL = (NV + DRPP - 1) / DRPP;       // dy loads per thread
  constexpr int HLL = (NH + RPP - 1) / RPP;         // halo loads per thread
  static_assert(NV % 32 == 0, "brick voxels (an even number of 16-voxel k-steps)");
  static_assert(NV * DROWB + NH * ROWB == wb_lds_bytes<BD, BH, BW, S, NCO>(), "LDS size");
  char* dyt = lds;
  char* hal = lds + NV * DROWB;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __builtin_assume((unsigned)tid < (unsigned)NT);  // (the kernels' launch bound, known while the body is optimised alone)
  const int ch = tid & 3, row0 = tid >> 2;  // fixed halo channel chunk per thread
  const int dch = tid % DCH, drow0 = tid / DCH;
  // XCD-aware: the channel tiles of neighbouring brick ranges share an L2
  const TileSplit ts = xcd_tile_split(wg, gx, gy, nwg);
  const int ci0 = ts.tx * 32, co0 = ts.ty * 32 * NCO;
  const long long b0 = (long long)ts.split * g.per_split;
  const long long b1 = min(g.nbricks, b0 + g.per_split);
  const bool has_gn = gstat != nullptr;

  constexpr int MAXT = 4;  // taps per wave: t = wave + 8j
  f32x16 acc[MAXT][NCO];
#pragma unroll
  for (int j = 0; j < MAXT; ++j)
#pragma unroll
    for (int c = 0; c < NCO; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][c][e] = 0.f;
  // stride 2: every halo w line is stored parity-split (even w first, then odd), so the lanes of a fragment read,
  // for any tap, CONSECUTIVE rows (w = 2 vw + tw -> vw, HWE + vw, vw + 1 for tw = 0, 1, 2) instead of every other row
  // (2-way bank conflicts)
  constexpr int HWE = S == 2 ? (HW + 1) / 2 : 0;
  auto wpos = [&](int hw) { return S == 2 ? ((hw & 1) ? HWE + (hw >> 1) : (hw >> 1)) : hw; };
  // tap j's halo row offset, formed where it is used (an array of 4 held across the loop cost 4 VGPRs)
  auto tap_off_of = [&](int j) {
    const int t = min(wave + 8 * j, 26);
    const int td = t / 9, th = (t / 3) % 3, tw = t % 3;
    return ((td * HH + th) * HW + (S == 2 ? (tw == 1 ? HWE : tw >> 1) : tw)) * ROWB;
  };
  const int ntap = (27 - wave + 7) / 8;  // 4 for waves 0-2, 3 for 3-7

  // fragment lane geometry: group gq = lane>>4, in-group lane i = lane&15 -> (q = i>>2, p = i&3)
  const int h = lane >> 5, gq = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int colb = (16 * (gq & 1) + 4 * p) * 2;  // byte offset of this lane's 4 columns

  u32x4 pdy[DYL], phl[HLL];
  // the GroupNorm coefficients of the current sample in LDS (per 8-channel chunk), read only inside commit: held in
  // registers across the MFMA loop they pushed the 3-plane stride-2 form past 256 VGPRs
  __shared__ f32x2 gsc[4][4], gsh[4][4];
  int gn_n = -1;

  auto decode = [&](long long b, int& n, int& od0, int& oh0, int& ow0) {
    long long t = b;
    const int bw_ = (int)(t % g.nbw); t /= g.nbw;
    const int bh_ = (int)(t % g.nbh); t /= g.nbh;
    const int bd_ = (int)(t % g.nbd);
    n = (int)(t / g.nbd);
    od0 = bd_ * BD; oh0 = bh_ * BH; ow0 = bw_ * BW;
  };
  const auto yrs = __builtin_amdgcn_make_buffer_rsrc((void*)dy, 0, BUF ? g.n * g.od * g.oh * g.ow * g.cout * 2 : 0,
                                                     0x00020000);
  const auto xrs = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, BUF ? g.n * g.id * g.ih * g.iw * g.cin * 2 : 0,
                                                     0x00020000);
  auto prefetch = [&](long long b) {
    int n, od0, oh0, ow0;
    decode(b, n, od0, oh0, ow0);
#pragma unroll
    for (int i = 0; i < DYL; ++i) {
      const int v = drow0 + i * DRPP;
      const int vw = v % BW, vh = (v / BW) % BH, vd = v / (BW * BH);
      const int zd = od0 + vd, zh = oh0 + vh, zw = ow0 + vw, co = co0 + dch * 8;
      const bool ok = v < NV && zd < g.od && zh < g.oh && zw < g.ow && co < g.cout;
      if constexpr (BUF) {
        const unsigned off = ok ? (unsigned)(((((n * g.od + zd) * g.oh + zh) * g.ow + zw) * g.cout + co) * 2) : 0xFFFFFFF0u;
        pdy[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(yrs, off, 0, 0));
      } else {
        u32x4 val = {0u, 0u, 0u, 0u};
        if (ok)
          val = *reinterpret_cast<const u32x4*>(dy + ((((long long)n * g.od + zd) * g.oh + zh) * g.ow + zw) * g.cout + co);
        pdy[i] = val;
      }
    }
    const int id0 = od0 * S - 1, ih0 = oh0 * S - 1, iw0 = ow0 * S - 1, c = ci0 + ch * 8;
#pragma unroll
    for (int i = 0; i < HLL; ++i) {
      const int v = row0 + i * RPP;
      const int hw = v % HW, hh = (v / HW) % HH, hd = v / (HW * HH);
      const int zd = id0 + hd, zh = ih0 + hh, zw = iw0 + hw;
      const bool ok = v < NH && (unsigned)zd < (unsigned)g.id && (unsigned)zh < (unsigned)g.ih &&
                      (unsigned)zw < (unsigned)g.iw && c < g.cin;
      if constexpr (BUF) {
        const unsigned off = ok ? (unsigned)(((((n * g.id + zd) * g.ih + zh) * g.iw + zw) * g.cin + c) * 2) : 0xFFFFFFF0u;
        phl[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0));
      } else {
        u32x4 val = {0u, 0u, 0u, 0u};
        if (ok)
          val = *reinterpret_cast<const u32x4*>(x + ((((long long)n * g.id + zd) * g.ih + zh) * g.iw + zw) * g.cin + c);
        phl[i] = val;
      }
    }
  };
  auto commit = [&](long long b) {
    int n, od0, oh0, ow0;
    decode(b, n, od0, oh0, ow0);
    if (has_gn && n != gn_n) {  // n is uniform over the workgroup: the barrier is reached by all or none
      gn_n = n;
      if (tid < 4) {
        f32x2 sc[4], sh[4];
        gn_coef8(gstat, gamma, beta, g.gn_groups, g.cin, n, ci0 + tid * 8, sc, sh);
        // a chunk past cin (cin_p padding) holds zeros and must stay zero: gn_coef8 clamps to channel cin - 1, whose
        // relu(sh) > 0 would put sum(dy) * relu(sh) into the slab's padded ci columns
        const bool pad = ci0 + tid * 8 >= g.cin;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          gsc[tid][k] = pad ? f32x2{0.f, 0.f} : sc[k];
          gsh[tid][k] = pad ? f32x2{0.f, 0.f} : sh[k];
        }
      }
      __syncthreads();
    }
    f32x2 sc[4], sh[4];
    if (has_gn) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        sc[k] = gsc[ch][k];
        sh[k] = gsh[ch][k];
      }
    }
#pragma unroll
    for (int i = 0; i < DYL; ++i) {
      const int v = drow0 + i * DRPP;
      if (v < NV) *reinterpret_cast<u32x4*>(dyt + v * DROWB + dch * 16) = pdy[i];
    }
    const int id0 = od0 * S - 1, ih0 = oh0 * S - 1, iw0 = ow0 * S - 1;
#pragma unroll
    for (int i = 0; i < HLL; ++i) {
      const int v = row0 + i * RPP;
      if (v < NH) {
        u32x4 val = phl[i];
        const int hw = v % HW, hl = v - hw;  // hl = (hd * HH + hh) * HW
        if (has_gn) {
          const int hh = (v / HW) % HH, hd = v / (HW * HH);
          const int zd = id0 + hd, zh = ih0 + hh, zw = iw0 + hw;
          if ((unsigned)zd < (unsigned)g.id && (unsigned)zh < (unsigned)g.ih && (unsigned)zw < (unsigned)g.iw)
            val = gn_relu8(val, sc, sh);
        }
        *reinterpret_cast<u32x4*>(hal + (hl + wpos(hw)) * ROWB + ch * 16) = val;
      }
    }
  };

  if (b0 < b1) {
    prefetch(b0);
    commit(b0);
  }
  __syncthreads();
  for (long long b = b0; b < b1; ++b) {
    const bool more = b + 1 < b1;
    prefetch(more ? b + 1 : b);
    // K loop over the brick's voxels, 16 per MFMA; software-pipelined: the fragments of step ks+1 are read
    // while step ks's MFMAs run, and the tap count is a compile-time constant per wave (4 or 3) so the loop
    // has no divergent branches between the LDS reads and the MFMAs
    auto kloop = [&](auto ntc) {
      constexpr int NT = decltype(ntc)::value;
      auto rows = [&](int ks, int (&ar)[2], int (&hr)[2]) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const int k = ks * 16 + 8 * h + 4 * m + q;
          const int vw = k % BW, vh = (k / BW) % BH, vd = k / (BW * BH);
          ar[m] = k * DROWB + colb;
          hr[m] = ((vd * S * HH + vh * S) * HW + (S == 2 ? vw : vw * S)) * ROWB + colb;
        }
      };
      auto frags = [&](int ks, bf16x8 (&a)[NCO], bf16x8 (&bb)[NT]) {
        int ar[2], hr[2];
        rows(ks, ar, hr);
#pragma unroll
        for (int c = 0; c < NCO; ++c) a[c] = frag_from(tr_read(dyt, ar[0] + 64 * c), tr_read(dyt, ar[1] + 64 * c));
#pragma unroll
        for (int j = 0; j < NT; ++j)
          bb[j] = frag_from(tr_read(hal, hr[0] + tap_off_of(j)), tr_read(hal, hr[1] + tap_off_of(j)));
      };
      auto mfmas = [&](const bf16x8 (&a)[NCO], const bf16x8 (&bb)[NT]) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int c = 0; c < NCO; ++c)
            acc[j][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[c], bb[j], acc[j][c], 0, 0, 0);
      };
      if constexpr (NCO == 1) {
        bf16x8 a0[NCO], a1[NCO], b0[NT], b1[NT];
        frags(0, a0, b0);
#pragma unroll 1
        for (int ks = 0; ks < NKS; ks += 2) {
          frags(ks + 1, a1, b1);  // NKS is even
          mfmas(a0, b0);
          if (ks + 2 < NKS) frags(ks + 2, a0, b0);
          mfmas(a1, b1);
        }
      } else {  // twice the accumulators: no fragment lookahead (the other wave of the SIMD covers the LDS reads)
#pragma unroll 1
        for (int ks = 0; ks < NKS; ++ks) {
          int ar[2], hr[2];
          rows(ks, ar, hr);
          bf16x8 a0[NCO];
#pragma unroll
          for (int c = 0; c < NCO; ++c) a0[c] = frag_from(tr_read(dyt, ar[0] + 64 * c), tr_read(dyt, ar[1] + 64 * c));
          // one tap's halo fragment at a time (4 VGPRs live instead of 16: the 3-plane stride-2 form fits 256)
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            const bf16x8 bj = frag_from(tr_read(hal, hr[0] + tap_off_of(j)), tr_read(hal, hr[1] + tap_off_of(j)));
#pragma unroll
            for (int c = 0; c < NCO; ++c)
              acc[j][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[c], bj, acc[j][c], 0, 0, 0);
          }
        }
      }
    };
    if (ntap == 4)
      kloop(std::integral_constant<int, 4>{});
    else
      kloop(std::integral_constant<int, 3>{});
    __syncthreads();  // everyone done with this brick's LDS
    if (more) commit(b + 1);
    __syncthreads();
  }
  // D[row = co][col = ci]: lane col ci0 + (lane&31), rows co0 + (i&3) + 8(i>>2) + 4h. Buffer stores with 32-bit
  // offsets computed here (the host keeps the slabs below 2 GiB): no 64-bit addresses held across the brick loop.
  int t0 = tid;
  asm volatile("" : "+v"(t0));
  const int r = t0 & 31, w8 = t0 >> 6, h8 = (t0 >> 5) & 1;
  const auto prs = __builtin_amdgcn_make_buffer_rsrc((void*)part, 0, 0x7FFFFFFF, 0x00020000);
#pragma unroll
  for (int j = 0; j < MAXT; ++j) {
    if (j < ntap) {
      const int tt = w8 + 8 * j;
#pragma unroll
      for (int c = 0; c < NCO; ++c) {
        const int base = ((ts.split * 27 + tt) * g.cout_p + co0 + 32 * c + 4 * h8) * g.cin_p + ci0 + r;
        // (the whole accumulator is bit-cast first: a bit_cast of a single element of the fp32 vector fed to
        // raw_buffer_store_b32 is miscompiled by ROCm 7.2 clang into stores of element 0)
        typedef __attribute__((ext_vector_type(16))) uint32_t u32x16;
        const u32x16 ua = __builtin_bit_cast(u32x16, acc[j][c]);
#pragma unroll
        for (int i = 0; i < 16; ++i)
          __builtin_amdgcn_raw_buffer_store_b32(ua[i], prs, (unsigned)((base + ((i & 3) + 8 * (i >> 2)) * g.cin_p) * 4),
                                                0, 0);
      }
    }
  }
}

}  // namespace u3d
