// 3^3 stride-1 convolution (forward / data gradient) for the small deep-level volumes (24^3, 12^3, 6^3 of the
// 96^3 U-Net: 128 / 256 channels), bf16, halo-brick form sized for PARALLELISM rather than reuse.
// The workgroup body, callable from more than one kernel: conv_small_kernel (conv_small.hip) and the paired backward
// launch (small_pair.hip). It never reads blockIdx / gridDim: the caller passes the workgroup's linear index in the
// body's own sub-grid, that sub-grid's size and the LDS base (SC_SMEM bytes, 16-B aligned).
//
// Reference: F.conv3d in Conv3d.forward (unet3D.py:27) through NoBottleneck (:56-73) at layer2..4, fusion and
// x8/x4 decoder blocks, and its autograd data gradient.
//
// At 12^3 x 2 samples a layer is 3456 output voxels x 256 channels = 864 output tiles of 32x32 with a
// 6912-deep contraction: the implicit GEMM's 128x128 tiles leave most CUs idle or need split-K slabs, and
// re-read every tap's operands through L2. Here:
//   * one workgroup (8 waves) = one brick of up to 256 output voxels x one 32-channel output tile; each wave
//     owns one 32-voxel row tile and the full contraction (27 taps x cin) -> no split-K, no slab traffic;
//   * the brick's extents divide the volume evenly (3x6x12 at 12^3, 6^3 whole at 6^3) so few rows idle;
//   * K loop = 32-channel input chunks: the input halo ((bd+2)(bh+2)(bw+2) voxels) is staged once per chunk
//     into LDS with GroupNorm + ReLU applied once per element, the 27 taps' weights of the chunk beside it;
//     the 27 taps are 27 shifted windows of the halo (per-lane row + tap offset); the next chunk is prefetched
//     into registers while the MFMAs run;
//   * epilogue through LDS: coalesced 64-B voxel rows, residual added on the way out.
// FLIP = data gradient: flipped tap offsets with the [t][ci][co] pack, no prologue.
#pragma once
#include "common.h"
#include "diag.h"

namespace u3d {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

// U3D_SC_NT = 512: one 8-wave workgroup of up to 256 output voxels per CU (105 KB of LDS); 256: 4-wave workgroups
// of up to 128 voxels, two per CU (<= 80 KB each: smaller halo, GN table for cin <= 640)
#ifndef U3D_SC_NT
#define U3D_SC_NT 512
#endif
constexpr int SC_NT = U3D_SC_NT;
constexpr int SC_MAXV = SC_NT / 2;               // output voxels per brick (32 per wave)
constexpr int SC_HMAX = SC_NT == 512 ? 640 : 320;  // halo rows (max)
constexpr int SC_PS = SC_HMAX * 16 + 64;         // halo plane stride (+64 B: conflict-free staging writes)
constexpr int SC_NWR = 27 * 32;                  // weight rows (tap, co)
constexpr int SC_WPS = SC_NWR * 16 + 64;         // weight plane stride
constexpr int SC_HLD = SC_HMAX * 4 / SC_NT;      // 5 halo loads per thread
constexpr int SC_WLD = (SC_NWR * 4 + SC_NT - 1) / SC_NT;  // 7 weight loads per thread
constexpr int SC_LDS = 4 * SC_PS + 4 * SC_WPS;
constexpr int SC_MAXC = SC_NT == 512 ? 1024 : 640;  // GN prologue: cin_p <= SC_MAXC (per-channel table after SC_LDS)
constexpr int SC_SMEM = SC_LDS + SC_MAXC * 8;  // the body's LDS
static_assert(SC_NT == 512 || SC_SMEM <= 81920, "two workgroups per CU");

struct SCGeom {
  int n, d, h, w;
  int cin, cin_p, cout, cout_p;
  int bd, bh, bw;          // output brick
  int hh, hw, nh;          // halo pitch (bh+2, bw+2) and rows
  int nbd, nbh, nbw, nct;  // bricks per dim, 32-wide output channel tiles
  int nv;                  // voxels per brick (<= 256)
  int gn_groups;
  int nks, cpk;            // K split: workgroups per output tile, 32-channel chunks per split
  float* slab;             // fp32 partials [nks][n][d][h][w][cout] when nks > 1
  // round 5: in-kernel split-K combine (cnt != nullptr, nks > 1) and optional output GroupNorm(16) statistics
  unsigned* cnt;           // [tiles + 1] zeroed arrival counters (per output tile, then one for the statistics)
  float* spart;            // [n][nbd*nbh*nbw][16][2] fp32 partials of the output statistics (stats != nullptr)
  float* stats;            // [n][16][2] (mean, rstd) of the output, or nullptr
  int cpg;                 // output channels per GroupNorm group (cout / 16; 4, 8 or 16)
  // round 5, data gradient (flip) through the combine: the backward of the GroupNorm + ReLU on x (the forward's input,
  // channels = this launch's cout) — per (sample, brick, channel) (sum g, sum g*xhat) of g = relu-mask * dA, then the
  // apply coefficients coef[n][5][cout] and dgamma / dbeta by the workgroup completing the last tile
  const bf16* gbx;
  const float *gbstat, *gbgamma, *gbbeta;
  int gbgroups;
  float* gbparts;          // [n][bricks][cout][2]
  float *coef, *dgamma, *dbeta;
};

// Geometry and contraction split of one launch (host): the brick, the tiles and nks from the workgroup target
// (OPT_SMALL_WGS) and the split-K workspace (ws / ws_bytes). The one copy: the paired launch plans its data-gradient
// half here too, so both forms split alike. Returns the output tiles; the grid is tiles * g.nks workgroups.
inline long long sc_plan(int n, int cin, int d, int h, int w, int cout, int gn_groups, float* ws, long long ws_bytes,
                         SCGeom& g) {
  g = SCGeom{};
  g.n = n; g.d = d; g.h = h; g.w = w;
  g.cin = cin; g.cin_p = round_up(cin, 32); g.cout = cout; g.cout_p = round_up(cout, 32);
  g.gn_groups = gn_groups;
  auto even = [](int q, int mx) { return cdiv(q, cdiv(q, std::max(1, mx))); };
  g.bw = even(w, 16);
  g.bh = even(h, SC_MAXV / (g.bw * 2));
  g.bd = even(d, std::min(d, SC_MAXV / (g.bw * g.bh)));
  while ((g.bd + 2) * (g.bh + 2) * (g.bw + 2) > SC_HMAX && g.bd > 1) --g.bd;
  while ((g.bd + 2) * (g.bh + 2) * (g.bw + 2) > SC_HMAX && g.bh > 1) --g.bh;
  while ((g.bd + 2) * (g.bh + 2) * (g.bw + 2) > SC_HMAX && g.bw > 1) --g.bw;
  g.nv = g.bd * g.bh * g.bw;
  g.hh = g.bh + 2; g.hw = g.bw + 2;
  g.nh = (g.bd + 2) * g.hh * g.hw;
  g.nbd = cdiv(d, g.bd); g.nbh = cdiv(h, g.bh); g.nbw = cdiv(w, g.bw);
  g.nct = g.cout_p / 32;
  const long long tiles = (long long)n * g.nbd * g.nbh * g.nbw * g.nct;
  // split the contraction over workgroups until ~2 workgroups per CU: the per-CU operand stream (55 KB of
  // weights + the halo per 32-channel chunk), not the MFMAs, bounds these small layers
  const int nchunk = g.cin_p / 32;
  const long long target = std::max(1, opt(OPT_SMALL_WGS));  // workgroups aimed at
  int nks = (int)std::min<long long>(nchunk, std::max<long long>(1, (target + tiles - 1) / tiles));
  const long long slab1 = (long long)n * d * h * w * cout * 4;
  if (cout % 4) nks = 1;
  while (nks > 1 && (!ws || nks * slab1 > ws_bytes)) --nks;
  g.cpk = cdiv(nchunk, nks);
  g.nks = cdiv(nchunk, g.cpk);
  g.slab = g.nks > 1 ? ws : nullptr;
  g.cpg = cout / 16;
  return tiles;
}

// -DU3D_STAMPS phases (diag.h): 0 a chunk's MFMAs, 1 the next chunk's commit (GN + LDS writes) and its barrier, 2 the
// barrier after the MFMAs; "other" = the first chunk's loads and commit (the epilogue is after the last stamp).
// stamps / tail: the calling kernel's stamp buffers (null: none kept).
//
// wg: this workgroup's index in [0, nwg), nwg = tiles * g.nks the body's sub-grid; workgroups wg and wg + 8 must run on
// one XCD (a sub-grid that starts at a multiple of 8 of the launch's linear block index).
template <bool FLIP>
__device__ __forceinline__ void conv_small_body(char* const smem, const int wg, const int nwg,
                                                const bf16* __restrict__ x, const bf16* __restrict__ wpk,
                                                bf16* __restrict__ y, const bf16* __restrict__ res,
                                                const float* __restrict__ gstat, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, const SCGeom& g,
                                                unsigned long long* stamps, unsigned long long* tail) {
  char* const hal = smem;
  char* const wts = smem + 4 * SC_PS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  PhaseStamps ps;
  ps.begin();
  const int r = lane & 31, hh = lane >> 5;

  int bid;  // XCD-aware: each XCD owns a contiguous range of (brick, co tile)
  {
    const int q = nwg >> 3, rr = nwg & 7, xcd = wg & 7, loc = wg >> 3;
    bid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + loc;
  }
  const int ks = bid % g.nks;
  int b = bid / g.nks;
  const int co0 = (b % g.nct) * 32;
  b /= g.nct;
  const int bw_ = b % g.nbw; b /= g.nbw;
  const int bh_ = b % g.nbh; b /= g.nbh;
  const int bd_ = b % g.nbd;
  const int nn = b / g.nbd;
  const int o0d = bd_ * g.bd, o0h = bh_ * g.bh, o0w = bw_ * g.bw;

  const int v = min(wave * 32 + r, g.nv - 1);
  const int vw = v % g.bw, vh = (v / g.bw) % g.bh, vd = v / (g.bw * g.bh);
  const int arow = (vd * g.hh + vh) * g.hw + vw;  // halo row of tap (0,0,0)
  const bool active = wave * 32 < g.nv;
  const bool has_gn = gstat != nullptr;

  const int sch = tid & 3, srow0 = tid >> 2;
  u32x4 hpre[SC_HLD], wpre[SC_WLD];
  unsigned hmask = 0;
  // buffer loads with 32-bit offsets (host: operands below 2 GiB); a masked piece gets the out-of-range sentinel and
  // reads zeros with no branch around the load (a branch merge pulls the prefetch's wait up ahead of the MFMAs)
  const auto xrs = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, g.n * g.d * g.h * g.w * g.cin * 2, 0x00020000);
  const auto wrs = __builtin_amdgcn_make_buffer_rsrc((void*)wpk, 0, 27 * g.cout_p * g.cin_p * 2, 0x00020000);
  auto halo_load = [&](int c) {
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < SC_HLD; ++i) {
      const int row = srow0 + i * (SC_NT / 4);
      const int xw = row % g.hw, xh = (row / g.hw) % g.hh, xd = row / (g.hw * g.hh);
      const int zd = o0d - 1 + xd, zh = o0h - 1 + xh, zw = o0w - 1 + xw, cc = c * 32 + sch * 8;
      const bool ok = row < g.nh && (unsigned)zd < (unsigned)g.d && (unsigned)zh < (unsigned)g.h &&
                      (unsigned)zw < (unsigned)g.w && cc < g.cin;
      const unsigned off = ok ? (unsigned)(((((nn * g.d + zd) * g.h + zh) * g.w + zw) * g.cin + cc) * 2) : 0xFFFFFFF0u;
      hpre[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0));
      m |= (ok ? 1u : 0u) << i;
    }
    hmask = m;
  };
  auto w_load = [&](int c) {
#pragma unroll
    for (int i = 0; i < SC_WLD; ++i) {
      const int id = tid + i * SC_NT;
      const int row = id >> 2, t = row >> 5, co = co0 + (row & 31);
      const bool ok = id < SC_NWR * 4 && co < g.cout_p;
      const unsigned off = ok ? (unsigned)(((t * g.cout_p + co) * g.cin_p + c * 32 + (id & 3) * 8) * 2) : 0xFFFFFFF0u;
      wpre[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, off, 0, 0));
    }
  };
  // GN scale/shift of this workgroup's sample per input channel, in LDS (filled once): the staging reads its 8
  // channels there at commit time. (Computing them from global loads next to the chunk prefetch made the wait for
  // those loads drain the halo/weight prefetch before the MFMAs.)
  f32x2* const gtab = reinterpret_cast<f32x2*>(smem + SC_LDS);
  int stg_c = 0;  // chunk of the staged prefetch
  auto commit = [&]() {
    f32x2 sc[4], sh[4];
    if (has_gn) {
      const f32x2* t = gtab + stg_c * 32 + sch * 8;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x2 a0 = t[2 * e], a1 = t[2 * e + 1];
        sc[e] = f32x2{a0[0], a1[0]};
        sh[e] = f32x2{a0[1], a1[1]};
      }
    }
#pragma unroll
    for (int i = 0; i < SC_HLD; ++i) {
      const int row = srow0 + i * (SC_NT / 4);
      if (row < g.nh) {
        u32x4 val = hpre[i];
        if (has_gn && ((hmask >> i) & 1u)) val = gn_relu8(val, sc, sh);
        *reinterpret_cast<u32x4*>(hal + sch * SC_PS + row * 16) = val;
      }
    }
#pragma unroll
    for (int i = 0; i < SC_WLD; ++i) {
      const int id = tid + i * SC_NT;
      if (id < SC_NWR * 4) *reinterpret_cast<u32x4*>(wts + (id & 3) * SC_WPS + (id >> 2) * 16) = wpre[i];
    }
  };

  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;

  const int c0 = ks * g.cpk, c1 = min(g.cin_p / 32, c0 + g.cpk);
  halo_load(c0);
  w_load(c0);
  stg_c = c0;
  if (has_gn) {
    for (int i = tid; i < min(g.cin_p, SC_MAXC); i += SC_NT) {
      const int c = min(i, g.cin - 1), gg = c / (g.cin / g.gn_groups);
      const float mean = gstat[(nn * g.gn_groups + gg) * 2], rstd = gstat[(nn * g.gn_groups + gg) * 2 + 1];
      const float sc_ = rstd * gamma[c];
      gtab[i] = f32x2{sc_, beta[c] - mean * sc_};
    }
    __syncthreads();
  }
  commit();
  __syncthreads();
  for (int c = c0; c < c1; ++c) {
    const bool more = c + 1 < c1;
    if (more) {
      halo_load(c + 1);
      w_load(c + 1);
      stg_c = c + 1;
    }
    ps.mark_now();
    ps.step(true);
    if (active) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int plane = 2 * s + hh;
        const char* ab = hal + plane * SC_PS + arow * 16;
        const char* bb = wts + plane * SC_WPS + r * 16;
#pragma unroll
        for (int t = 0; t < 27; ++t) {
          const int td = t / 9, th = (t / 3) % 3, tw = t % 3;
          const int od = FLIP ? 2 - td : td, oh = FLIP ? 2 - th : th, ow = FLIP ? 2 - tw : tw;
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(ab + ((od * g.hh + oh) * g.hw + ow) * 16);
          const bf16x8 bv = *reinterpret_cast<const bf16x8*>(bb + t * 32 * 16);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bv, acc, 0, 0, 0);
        }
      }
    }
    ps.lap(0);
    __syncthreads();
    ps.lap(2);
    if (more) {
      commit();
      __syncthreads();
      ps.lap(1);
    }
  }
  ps.end(stamps, wg & 1023, wave, lane);
  TailStamps ts(tail, wg & 1023, tid == 0);
  if (g.nks > 1) {  // fp32 partial through the wave's LDS tile: 128-B rows, coalesced
    float* const ept = reinterpret_cast<float*>(smem + wave * 4096);
    if (active) {
#pragma unroll
      for (int i = 0; i < 16; ++i) ept[((i & 3) + 8 * (i >> 2) + 4 * hh) * 32 + r] = acc[i];
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    const long long per = (long long)g.n * g.d * g.h * g.w * g.cout;  // floats per slab
    // (write-through sc1 16-B stores where the combine runs in this launch: the last-arriving workgroup of the tile
    // reads them with sc1 loads, MI355X_MICROARCH.md visibility table, counter row)
    const auto srs = __builtin_amdgcn_make_buffer_rsrc((void*)g.slab, 0, (int)(g.nks * per * 4), 0x00020000);
    if (active) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int qi = lane + 64 * u, part = qi & 7, row = qi >> 3;
        const int vv = wave * 32 + row;
        const int uw = vv % g.bw, uh = (vv / g.bw) % g.bh, ud = vv / (g.bw * g.bh);
        const int zd = o0d + ud, zh = o0h + uh, zw = o0w + uw, co = co0 + part * 4;
        if (vv < g.nv && zd < g.d && zh < g.h && zw < g.w && co < g.cout) {
          const long long e = ks * per + ((((long long)nn * g.d + zd) * g.h + zh) * g.w + zw) * g.cout + co;
          const f32x4 val = *reinterpret_cast<const f32x4*>(ept + qi * 4);
          if (g.cnt)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, val), srs, (int)(e * 4), 0, 16);
          else
            *reinterpret_cast<f32x4*>(g.slab + e) = val;
        }
      }
    }
    ts.mark<1>();
    if (!g.cnt) return;  // the separate small_reduce_kernel sums the slabs
    // ---- in-kernel split-K combine (round 5): the workgroup that completes its output tile last sums the tile's
    // nks slabs in slab order (bitwise the small_reduce_kernel sums), adds the residual and stores y
    ts.mark<2>();
    const int tile = bid / g.nks;
    const bool tile_last = last_arriver(g.cnt + tile, (unsigned)g.nks);
    ts.mark<3>();
    if (!tile_last) return;
    float ls[8], lq[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) ls[k] = lq[k] = 0.f;
    const int cpg = g.stats ? g.cpg : 32;
    // GroupNorm-backward partials (flip with gbx): this thread's 4 channels are fixed (part = tid & 7)
    float bsc[4], bsh[4], bmu[4], brs[4], b1[4], b2[4];
    if (g.gbx) {
      const int gcpg = g.cout / g.gbgroups;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = min(co0 + (tid & 7) * 4 + e, g.cout - 1), gr = c / gcpg;
        bmu[e] = g.gbstat[(nn * g.gbgroups + gr) * 2];
        brs[e] = g.gbstat[(nn * g.gbgroups + gr) * 2 + 1];
        bsc[e] = brs[e] * g.gbgamma[c];
        bsh[e] = g.gbbeta[c] - bmu[e] * bsc[e];
        b1[e] = b2[e] = 0.f;
      }
    }
    // every load of the thread's 4 output pieces (nks slabs, residual, x) in flight before the first add: one memory
    // round trip; then the adds in slab order
    const int ypb = g.n * g.d * g.h * g.w * g.cout * 2;  // bytes of y / residual / x (host: < 2 GiB)
    const auto rrs = __builtin_amdgcn_make_buffer_rsrc((void*)res, 0, res ? ypb : 0, 0x00020000);
    const auto xrs2 = __builtin_amdgcn_make_buffer_rsrc((void*)g.gbx, 0, g.gbx ? ypb : 0, 0x00020000);
    // with a second hand-off (statistics / GroupNorm-backward partials) the y stores wait until this workgroup's
    // partials are published: its vmcnt(0) drain then covers only the partial store, not the tile's y stores
    const bool defer_y = g.stats || g.gbx;
    uint2 yv[4];
    long long yoff[4];
    bool yok[4];
    auto store_y = [&]() {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (yok[k]) *reinterpret_cast<uint2*>(y + yoff[k]) = yv[k];
    };
    auto combine = [&](auto nsc) {
      constexpr int NS = decltype(nsc)::value;
      static_assert(4 * SC_NT / 8 == SC_MAXV, "4 pieces of 4 channels per thread cover the brick's 32-channel tile");
      f32x4 t[4][NS];
      u32x2 rq[4], xq[4];
      long long vo[4];
      bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int q = tid + SC_NT * k, vv = q >> 3, part = q & 7;
        const int uw = vv % g.bw, uh = (vv / g.bw) % g.bh, ud = vv / (g.bw * g.bh);
        const int zd = o0d + ud, zh = o0h + uh, zw = o0w + uw, co = co0 + part * 4;
        ok[k] = vv < g.nv && zd < g.d && zh < g.h && zw < g.w && co < g.cout;
        vo[k] = ok[k] ? ((((long long)nn * g.d + zd) * g.h + zh) * g.w + zw) * g.cout + co : 0;
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_) {
          const bool in = ok[k] && s_ < g.nks;
          t[k][s_] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                   srs, in ? (int)((s_ * per + vo[k]) * 4) : (int)0xFFFFFFF0u, 0, 16));
        }
        const int yo = ok[k] ? (int)(vo[k] * 2) : (int)0xFFFFFFF0u;
        if (res) rq[k] = __builtin_amdgcn_raw_buffer_load_b64(rrs, yo, 0, 0);
        if (g.gbx) xq[k] = __builtin_amdgcn_raw_buffer_load_b64(xrs2, yo, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        yok[k] = false;
        if (!ok[k]) continue;
        const int part = (tid + SC_NT * k) & 7;
        f32x4 v = t[k][0];
#pragma unroll
        for (int s_ = 1; s_ < NS; ++s_)
          if (s_ < g.nks) v += t[k][s_];
        if (res) {
          v[0] += __uint_as_float(rq[k][0] << 16);
          v[1] += __uint_as_float(rq[k][0] & 0xffff0000u);
          v[2] += __uint_as_float(rq[k][1] << 16);
          v[3] += __uint_as_float(rq[k][1] & 0xffff0000u);
        }
        uint2 o;
        o.x = (uint32_t)from_f<bf16>(v[0]) | ((uint32_t)from_f<bf16>(v[1]) << 16);
        o.y = (uint32_t)from_f<bf16>(v[2]) | ((uint32_t)from_f<bf16>(v[3]) << 16);
        if (defer_y) {
          yv[k] = o;
          yoff[k] = vo[k];
          yok[k] = true;
        } else {
          *reinterpret_cast<uint2*>(y + vo[k]) = o;
        }
        if (g.gbx) {  // exactly gn_bwd_partial's per-element terms on the stored bf16 dA and x
          const float xv[4] = {__uint_as_float(xq[k][0] << 16), __uint_as_float(xq[k][0] & 0xffff0000u),
                               __uint_as_float(xq[k][1] << 16), __uint_as_float(xq[k][1] & 0xffff0000u)};
          const float dv[4] = {__uint_as_float(o.x << 16), __uint_as_float(o.x & 0xffff0000u),
                               __uint_as_float(o.y << 16), __uint_as_float(o.y & 0xffff0000u)};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float xh = (xv[e] - bmu[e]) * brs[e];
            const float gd = fmaf(xv[e], bsc[e], bsh[e]) > 0.f ? dv[e] : 0.f;
            b1[e] += gd;
            b2[e] = fmaf(gd, xh, b2[e]);
          }
        }
        if (g.stats) {  // the stored values' group sums (4 channels of one group: cpg >= 4)
          const float a0 = __uint_as_float(o.x << 16), a1 = __uint_as_float(o.x & 0xffff0000u);
          const float a2 = __uint_as_float(o.y << 16), a3 = __uint_as_float(o.y & 0xffff0000u);
          const float ss = (a0 + a1) + (a2 + a3), qq = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
          const int gi = (part * 4) / cpg;
#pragma unroll
          for (int k2 = 0; k2 < 8; ++k2) {
            ls[k2] += gi == k2 ? ss : 0.f;
            lq[k2] += gi == k2 ? qq : 0.f;
          }
        }
      }
    };
    if (g.nks <= 2)
      combine(std::integral_constant<int, 2>{});
    else if (g.nks <= 4)
      combine(std::integral_constant<int, 4>{});
    else
      combine(std::integral_constant<int, 8>{});
    ts.mark<4>();
    const int ntiles = (int)((unsigned)nwg / g.nks);  // the second hand-off's counter follows the per-tile ones
    if (g.gbx) {
      // per channel of the tile over the workgroup: lanes with the same tid & 7 (xor 8, 16, 32), then the waves in order
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int o2 = 8; o2 < 64; o2 <<= 1) {
          b1[e] += __shfl_xor(b1[e], o2);
          b2[e] += __shfl_xor(b2[e], o2);
        }
      float* const red = reinterpret_cast<float*>(smem);  // [wave][32 channels][2]
      __syncthreads();
      if (lane < 8)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          red[(wave * 32 + lane * 4 + e) * 2] = b1[e];
          red[(wave * 32 + lane * 4 + e) * 2 + 1] = b2[e];
        }
      __syncthreads();
      const int nbr = g.nbd * g.nbh * g.nbw, brick = (bd_ * g.nbh + bh_) * g.nbw + bw_;
      if (tid < 64 && co0 + (tid >> 1) < g.cout) {
        float t2 = 0.f;
#pragma unroll
        for (int wv = 0; wv < SC_NT / 64; ++wv) t2 += red[wv * 64 + tid];
        __hip_atomic_store(g.gbparts + (((long long)nn * nbr + brick) * g.cout + co0) * 2 + tid, t2, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);  // sc1
      }
      ts.mark<5>();
      const bool last = last_arriver(g.cnt + ntiles, (unsigned)ntiles);
      ts.mark<6>();
      store_y();
      if (!last) return;
      // gn_bwd_parts_finalize: per (n, c) fp64 sums over the bricks in order, then the coefficients
      double* const cs = reinterpret_cast<double*>(smem);  // [n * cout][2] (<= 8192 doubles: host-checked)
      lastarriver_rowsum<SC_NT>(g.gbparts, g.n, nbr, 2 * g.cout, cs);
      __syncthreads();
      const double M = (double)g.d * g.h * g.w * (g.cout / g.gbgroups);
      gn_bwd_coefs<SC_NT>(cs, g.n, g.cout, g.gbgroups, M, g.gbstat, g.gbgamma, g.gbbeta, g.coef, g.dgamma, g.dbeta, 0);
      ts.mark<7>();
      return;
    }
    if (!g.stats) return;
    // ---- output GroupNorm(16) statistics: this tile's groups reduced over the workgroup (fixed order), one partial
    // row per (sample, brick); the workgroup completing the last tile combines them in fp64 (one launch, no pass)
    float sv[16];
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
      sv[2 * k2] = ls[k2];
      sv[2 * k2 + 1] = lq[k2];
    }
    const float tot = wave_sum_transposed<16>(sv, lane);  // lane l: value l >> 2 = (group slot, sum | square)
    float* const red = reinterpret_cast<float*>(smem);     // (LDS free: the MFMA loop is done)
    __syncthreads();
    if ((lane & 3) == 0) red[wave * 16 + (lane >> 2)] = tot;
    __syncthreads();
    const int gpt = 32 / cpg, nbr = g.nbd * g.nbh * g.nbw, brick = (bd_ * g.nbh + bh_) * g.nbw + bw_;
    if (tid < 2 * gpt) {
      float t2 = 0.f;
#pragma unroll
      for (int wv = 0; wv < SC_NT / 64; ++wv) t2 += red[wv * 16 + tid];
      const int gr = co0 / cpg + (tid >> 1);
      __hip_atomic_store(g.spart + ((long long)nn * nbr + brick) * 32 + gr * 2 + (tid & 1), t2, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);  // sc1
    }
    ts.mark<5>();
    const bool last = last_arriver(g.cnt + ntiles, (unsigned)ntiles);
    ts.mark<6>();
    store_y();
    if (!last) return;
    double* const cs = reinterpret_cast<double*>(smem) + 64;  // [n * 16][2] (past the wave rows in `red`)
    lastarriver_rowsum<SC_NT>(g.spart, g.n, nbr, 32, cs);
    __syncthreads();
    const double m = (double)g.cpg * g.d * g.h * g.w;
    for (int p = tid; p < g.n * 16; p += SC_NT) gn_store_stats(g.stats + p * 2, cs[2 * p], cs[2 * p + 1], m);
    ts.mark<7>();
    return;
  }

  // epilogue: wave tile [32 rows][32 co] bf16 (2 KB) -> 16-B chunks, 4 lanes per output voxel
  char* const ept = smem + wave * 2048;
  if (active) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
      *reinterpret_cast<bf16*>(ept + (row * 32 + r) * 2) = from_f<bf16>(acc[i]);
    }
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  if (active) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int qi = lane + 64 * u, part = qi & 3, row = qi >> 2;
      const int vv = wave * 32 + row;
      const int uw = vv % g.bw, uh = (vv / g.bw) % g.bh, ud = vv / (g.bw * g.bh);
      const int zd = o0d + ud, zh = o0h + uh, zw = o0w + uw, co = co0 + part * 8;
      if (vv < g.nv && zd < g.d && zh < g.h && zw < g.w && co < g.cout) {
        const long long off = ((((long long)nn * g.d + zd) * g.h + zh) * g.w + zw) * g.cout + co;
        u32x4 val = *reinterpret_cast<const u32x4*>(ept + qi * 16);
        if (res) {
          float a[8], q[8];
          load16<bf16>(reinterpret_cast<const bf16*>(&val), a);
          load16<bf16>(res + off, q);
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] += q[e];
          store16<bf16>(reinterpret_cast<bf16*>(&val), a);
        }
        *reinterpret_cast<u32x4*>(y + off) = val;
      }
    }
  }
}

}  // namespace u3d
