// Generic 3^3 stride-1 convolution (forward / data gradient), bf16, halo-brick form, for the layers with
// cin >= 64 or spatial extents that are not multiples of 32 (48^3, 24^3, 12^3, 6^3 levels of the U-Net).
//
//   * one workgroup (8 waves) = one output brick of 4 x 8 x 16 voxels x one 64- (or 32-) channel co tile;
//   * K loop = 32-channel input chunks x 3 tap planes (td): per chunk the input halo (6 x 10 x 18 voxels) is
//     staged once into LDS with the GroupNorm + ReLU prologue applied once per element; per tap plane the
//     9 taps' weights (9 x 64 x 32 bf16 = 36 KB) are streamed into a double-buffered LDS slot;
//   * each wave owns 2 row tiles (32 voxels = 2 h-rows x 16 w) x the co tile (TN = CO/32 MFMA columns):
//     per k16 step 2 A reads + TN B reads feed 2*TN MFMAs (1 KB of LDS per MFMA at CO = 64);
//   * LDS images are chunk-planar (plane = 8 channels), and the 32 rows of an MFMA tile are ordered so that
//     each 16-lane ds_read_b128 group reads 16 consecutive halo rows (conflict-free for any halo pitch);
//   * the next chunk's halo and the next tap plane's weights are prefetched into registers while the MFMAs
//     of the current plane run.
// Reference: F.conv3d in Conv3d.forward (unet3D.py:27) through NoBottleneck (:56-73), fusion/decoder blocks.
#include "common.h"

namespace u3d {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int GB_BD = 4, GB_BH = 8, GB_BW = 16;
constexpr int GB_HD = GB_BD + 2, GB_HH = GB_BH + 2, GB_HW = GB_BW + 2;
constexpr int GB_NH = GB_HD * GB_HH * GB_HW;  // 1080 halo rows
constexpr int GB_NT = 512;
constexpr int GB_HLD = (GB_NH + GB_NT / 4 - 1) / (GB_NT / 4);  // 9 halo loads per thread
constexpr int GB_PS = GB_NH * 16 + 64;  // LDS plane stride (+64 B: conflict-free staging writes)
constexpr int GB_MAXN = 16;
constexpr int GB_MAXC = 256;  // persistent kernel with a GN prologue: cin_p <= GB_MAXC

struct GBGeom {
  int n, d, h, w;
  int cin, cout, cin_p, cout_p;
  int nbd, nbh, nbw;
  int gn_groups;
  int nct;
  float* fstats;   // round 5: forward output statistics finalized in-kernel (with fcnt), else nullptr
  unsigned* fcnt;  // zeroed arrival counter (left zeroed)
};

// MFMA row r (0..31) -> (segment = which of the 2 h-rows, position = w): the 16 lanes of each ds_read_b128
// group ({0-3,12-15,20-27} and {4-11,16-19,28-31}) get 16 consecutive w of one h-row.
__device__ __forceinline__ int gb_seg(int r) {
  return (r < 4 || (r >= 12 && r < 16) || (r >= 20 && r < 28)) ? 0 : 1;
}
__device__ __forceinline__ int gb_pos(int r) {
  if (r < 4) return r;
  if (r < 12) return r - 4;
  if (r < 16) return r - 8;
  if (r < 20) return r - 8;
  if (r < 28) return r - 12;
  return r - 16;
}

template <int CO, bool FLIP>
__global__ __launch_bounds__(GB_NT, 1) void convg_brick_kernel(const bf16* __restrict__ x, const bf16* __restrict__ wpk,
                                                              bf16* __restrict__ y, const bf16* __restrict__ res,
                                                              const float* __restrict__ gstat,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, GBGeom g) {
  constexpr int TN = CO / 32;
  constexpr int WROWS = 9 * CO;                            // weight rows per tap plane
  constexpr int WLD = (WROWS * 4 + GB_NT - 1) / GB_NT;     // weight loads per thread (5 at CO=64)
  __shared__ __attribute__((aligned(16))) char hal[4 * GB_PS];
  __shared__ __attribute__((aligned(16))) char wbuf[2][4 * WROWS * 16];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  // XCD-aware order: linear id i runs on XCD i % 8; remap so each XCD owns a contiguous range of
  // (brick, co tile) pairs -> concurrently running neighbours share halo rows through that XCD's L2.
  const int nwg = gridDim.x, nct = g.nct;
  int bid;
  {
    const int q = nwg >> 3, rr = nwg & 7, xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    bid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + loc;
  }
  int b = bid / nct;
  const int bw_ = b % g.nbw; b /= g.nbw;
  const int bh_ = b % g.nbh; b /= g.nbh;
  const int bd_ = b % g.nbd;
  const int nn = b / g.nbd;
  const int d0 = bd_ * GB_BD, h0 = bh_ * GB_BH, w0 = bw_ * GB_BW;
  const int co0 = (bid - (bid / nct) * nct) * CO;
  const bool has_gn = gstat != nullptr;
  const int nchunk = g.cin_p / 32;
  const int nsteps = nchunk * 3;

  u32x4 hpre[GB_HLD];
  u32x4 wpre[WLD];

  // staging: fixed 8-channel chunk per thread (4 threads = one voxel's 32 channels, coalesced)
  const int sch = tid & 3, srow0 = tid >> 2;
  f32x2 sc[4], sh[4];
  auto halo_load = [&](int c) {
#pragma unroll
    for (int i = 0; i < GB_HLD; ++i) {
      const int row = srow0 + i * (GB_NT / 4);
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row < GB_NH) {
        const int hw = row % GB_HW, hr = (row / GB_HW) % GB_HH, hd = row / (GB_HW * GB_HH);
        const int zd = d0 - 1 + hd, zh = h0 - 1 + hr, zw = w0 - 1 + hw;
        const int cc = c * 32 + sch * 8;
        if ((unsigned)zd < (unsigned)g.d && (unsigned)zh < (unsigned)g.h && (unsigned)zw < (unsigned)g.w && cc < g.cin)
          v = *reinterpret_cast<const u32x4*>(x + ((((long long)nn * g.d + zd) * g.h + zh) * g.w + zw) * g.cin + cc);
      }
      hpre[i] = v;
    }
  };
  auto gn_table = [&](int c) {  // scale/shift of this thread's 8 channels of chunk c
    if (has_gn) gn_coef8(gstat, gamma, beta, g.gn_groups, g.cin, nn, c * 32 + sch * 8, sc, sh);
  };
  auto halo_commit = [&]() {
#pragma unroll
    for (int i = 0; i < GB_HLD; ++i) {
      const int row = srow0 + i * (GB_NT / 4);
      if (row < GB_NH) {
        u32x4 v = hpre[i];
        if (has_gn) {
          const int hw = row % GB_HW, hr = (row / GB_HW) % GB_HH, hd = row / (GB_HW * GB_HH);
          const int zd = d0 - 1 + hd, zh = h0 - 1 + hr, zw = w0 - 1 + hw;
          if ((unsigned)zd < (unsigned)g.d && (unsigned)zh < (unsigned)g.h && (unsigned)zw < (unsigned)g.w)
            v = gn_relu8(v, sc, sh);
        }
        *reinterpret_cast<u32x4*>(hal + sch * GB_PS + row * 16) = v;
      }
    }
  };
  // weights of step s = (chunk c, tap plane td): rows (j, co) for t = td*9 + j
  auto w_load = [&](int s) {
    const int c = s / 3, td = s % 3;
#pragma unroll
    for (int i = 0; i < WLD; ++i) {
      const int ci = tid + i * GB_NT;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (ci < WROWS * 4) {
        const int ch = ci / WROWS, row = ci % WROWS;
        const int j = row / CO, co = co0 + row % CO;
        const int t = td * 9 + j;
        if (co < g.cout_p)
          v = *reinterpret_cast<const u32x4*>(wpk + ((long long)t * g.cout_p + co) * g.cin_p + c * 32 + ch * 8);
      }
      wpre[i] = v;
    }
  };
  auto w_commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < WLD; ++i) {
      const int ci = tid + i * GB_NT;
      if (ci < WROWS * 4) {
        const int ch = ci / WROWS, row = ci % WROWS;
        *reinterpret_cast<u32x4*>(wbuf[buf] + (ch * WROWS + row) * 16) = wpre[i];
      }
    }
  };

  // prologue: chunk 0 halo + plane 0 weights
  gn_table(0);
  halo_load(0);
  w_load(0);
  __syncthreads();
  halo_commit();
  w_commit(0);
  __syncthreads();

  f32x16 acc[2][TN];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[tm][tn][e] = 0.f;

  // per-lane A row of tap (0,0,0) for row tile tm: rt = 2*wave + tm -> (d = rt >> 2, h-pair = rt & 3)
  int arow[2];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm) {
    const int rt = 2 * wave + tm, vd = rt >> 2, vh = 2 * (rt & 3) + gb_seg(r);
    arow[tm] = (vd * GB_HH + vh) * GB_HW + gb_pos(r);
  }

  for (int s = 0; s < nsteps; ++s) {
    const int td = s % 3;
    const bool last_plane = td == 2;
    if (s + 1 < nsteps) w_load(s + 1);
    if (last_plane && s + 1 < nsteps) halo_load(s / 3 + 1);
    const char* wb = wbuf[s & 1];
    const int od = FLIP ? 2 - td : td;
#pragma unroll 3
    for (int j = 0; j < 9; ++j) {
      const int th = j / 3, tw = j % 3;
      const int oh = FLIP ? 2 - th : th, ow = FLIP ? 2 - tw : tw;
      const int toff = (od * GB_HH + oh) * GB_HW + ow;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int plane = 2 * k + hh;
        bf16x8 a[2], bb[TN];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
          a[tm] = *reinterpret_cast<const bf16x8*>(hal + plane * GB_PS + (arow[tm] + toff) * 16);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          bb[tn] = *reinterpret_cast<const bf16x8*>(wb + (plane * WROWS + j * CO + tn * 32 + r) * 16);
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[tm], bb[tn], acc[tm][tn], 0, 0, 0);
      }
    }
    if (s + 1 < nsteps) {
      w_commit((s + 1) & 1);  // the other buffer: its readers finished before the previous barrier
      if (last_plane) {
        gn_table(s / 3 + 1);
        __syncthreads();  // everyone done with this chunk's halo
        halo_commit();
      }
    }
    __syncthreads();
  }

  // epilogue through LDS (the halo image is free now): the wave's tile [tm][h-row seg][w pos][co] bf16 is
  // written by MFMA lane layout and read back as 16-B chunks, 8 lanes per voxel: coalesced stores / residual.
  constexpr int VB = CO * 2;  // bytes per voxel in the tile
  char* const ept = hal + wave * (2 * 32 * VB);
  u32x4 rv[2][VB / 32];
  long long obase[2];
  bool dok[2];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm) {
    const int rt = 2 * wave + tm, zd = d0 + (rt >> 2);
    dok[tm] = zd < g.d;
    obase[tm] = (((long long)nn * g.d + zd) * g.h + h0 + 2 * (rt & 3)) * g.w + w0;
  }
  auto chunk_ok = [&](int tm, int q, long long& off) {
    const int v = q / (VB / 16), c = q % (VB / 16);
    const int seg = v >> 4, pos = v & 15;
    const int rt = 2 * wave + tm, zh = h0 + 2 * (rt & 3) + seg, zw = w0 + pos, co = co0 + c * 8;
    off = (obase[tm] + (long long)seg * g.w + pos) * g.cout + co;
    return dok[tm] && zh < g.h && zw < g.w && co < g.cout;
  };
  if (res) {
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int u = 0; u < VB / 32; ++u) {
        long long off;
        rv[tm][u] = chunk_ok(tm, lane + 64 * u, off) ? *reinterpret_cast<const u32x4*>(res + off)
                                                      : u32x4{0u, 0u, 0u, 0u};
      }
  }
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ri = (i & 3) + 8 * (i >> 2) + 4 * hh;
        const int v = gb_seg(ri) * 16 + gb_pos(ri);
        *reinterpret_cast<bf16*>(ept + (tm * 32 + v) * VB + (tn * 32 + r) * 2) = from_f<bf16>(acc[tm][tn][i]);
      }
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int u = 0; u < VB / 32; ++u) {
      const int q = lane + 64 * u;
      long long off;
      if (!chunk_ok(tm, q, off)) continue;
      u32x4 v = *reinterpret_cast<const u32x4*>(ept + tm * 32 * VB + q * 16);
      if (res) {
        float a[8], c[8];
        load16<bf16>(reinterpret_cast<const bf16*>(&v), a);
        load16<bf16>(reinterpret_cast<const bf16*>(&rv[tm][u]), c);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += c[e];
        store16<bf16>(reinterpret_cast<bf16*>(&v), a);
      }
      *reinterpret_cast<u32x4*>(y + off) = v;
    }
}

// Persistent form of the same brick schedule (round 2): grid = one workgroup per CU (balanced), each walks a
// contiguous run of (brick, co tile) units and treats the concatenated (unit, chunk, tap plane) steps as ONE
// pipeline — the next unit's first halo chunk, its GroupNorm coefficients and its first weight plane are loaded
// during the last tap plane of the current unit, so a unit costs no cold prologue (the one-shot kernel exposes a
// full HBM round trip + the halo/weight staging per workgroup, ~1/3 of its time at 48^3). The MFMA is issued
// transposed (A = weights, B = halo rows): a lane's accumulators are 16 output channels of one voxel, so the
// epilogue is register-only (permlane32 swap, residual add, two 16-B stores per lane and co block) and never
// touches the LDS the next unit's halo is being written into. Same operands, same fp32 accumulation order per
// output (chunk, tap plane, tap, k-half) as convg_brick_kernel: bitwise-equal results.
// GB (data gradient only, round 4): the epilogue also takes the GroupNorm backward's partial sums over the dA it
// stores, as the 96^3 ring does (conv_ring.hip, GB): res = the GN input x (loaded at the stored dA's addresses, not
// added), gstat / gamma / beta = that GroupNorm, spart = parts[n][bricks per sample][cout][2] of (sum g, sum g*xhat),
// g = relu-mask * dA; u3d_gn_bwd_parts finishes (no partial pass over dA and x).
template <int CO, bool FLIP, int BWX = 16, bool GB = false>
__global__ __launch_bounds__(GB_NT, 1) void convg_pbrick_kernel(const bf16* __restrict__ x, const bf16* __restrict__ wpk,
                                                               bf16* __restrict__ y, const bf16* __restrict__ res,
                                                               const float* __restrict__ gstat,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, GBGeom g, int per,
                                                               int nunits, float* __restrict__ spart = nullptr) {
  constexpr int TN = CO / 32;
  constexpr int WROWS = 9 * CO;
  constexpr int WLD = (WROWS * 4 + GB_NT - 1) / GB_NT;
  // brick 4 x 8 x BWX: BWX = 16 -> 16 row tiles of (2 h-rows x 16 w), TM = 2 per wave; BWX = 8 (8- but not 16-multiple
  // planes, e.g. 24^3: no half-empty bricks) -> 8 row tiles of (4 h-rows x 8 w), TM = 1 per wave
  constexpr int BW = BWX, HH = GB_BH + 2, HW = BW + 2, NH = (GB_BD + 2) * HH * HW;
  constexpr int HLD = (NH + GB_NT / 4 - 1) / (GB_NT / 4), PS = NH * 16 + 64, TM = BW / 8;
  static_assert(BW == 16 || BW == 8, "brick width");
  // MFMA row r of row tile rt -> (d, h, w) inside the brick
  auto tile_vox = [](int rt, int r, int& vd, int& vh, int& vw) {
    if constexpr (BW == 16) {
      vd = rt >> 2; vh = 2 * (rt & 3) + gb_seg(r); vw = gb_pos(r);
    } else {
      vd = rt >> 1; vh = 4 * (rt & 1) + (r >> 3); vw = r & 7;
    }
  };
  __shared__ __attribute__((aligned(16))) char hal[4 * PS];
  // weight planes (8 input channels each) padded by 64 B: the 4 lanes staging one row's 4 chunks write 4 planes
  // conflict-free (plane stride = 64 mod 256 B)
  constexpr int WPS = WROWS * 16 + 64;
  __shared__ __attribute__((aligned(16))) char wbuf[2][4 * WPS];
  // GroupNorm (scale, shift) per input channel of the samples in flight, slot = sample & 1: filled once per sample
  // (the staging reads it from LDS — no global loads whose wait would drain the halo/weight prefetch)
  __shared__ __attribute__((aligned(16))) f32x2 gtab[2][GB_MAXC];
  // GB: (scale, shift, rstd, mean) per dA channel of the samples in flight (the epilogue's relu test and xhat)
  __shared__ __attribute__((aligned(16))) f32x4 gbt[GB ? 2 : 1][GB ? GB_MAXC : 1];
  // output GroupNorm statistics (spart != nullptr): per (wave, lane half, tn, run v, channel pair q) (sum, sum sq), fp64
  __shared__ double sst[8][2][TN * 2 * 4][2];

  // the data gradient never takes a residual or output statistics (convg_impl): dead at compile time, so its
  // epilogue's registers are not reserved (GB: res is the GN input x, spart the GN-backward partials)
  static_assert(!GB || FLIP, "GB: data gradient only");
  constexpr int GB_EARLY = TM == 1 ? TN : 1;  // GB: co blocks whose x loads go out in the last step (VGPR budget)
  if constexpr (FLIP && !GB) {
    res = nullptr;
    spart = nullptr;
  }
  float* const gbpart = GB ? spart : nullptr;
  if constexpr (GB) spart = nullptr;  // (the forward's output-statistics path stays dead)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  int bid;
  {
    const int nwg = gridDim.x, q = nwg >> 3, rr = nwg & 7, xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    bid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + loc;
  }
  const int u_begin = bid * per, u_end = min(nunits, u_begin + per);
  const int nct = g.nct;
  const bool has_gn = gstat != nullptr;
  const bool pro_gn = !FLIP && has_gn;             // GN + ReLU prologue on the staged input (forward only)
  const int gtc = FLIP ? g.cout : g.cin, gtc_p = FLIP ? g.cout_p : g.cin_p;  // channels of the LDS GN table
  const int nchunk = g.cin_p / 32;
  const int nsteps = nchunk * 3;

  struct Unit {
    int nn, d0, h0, w0, co0;
  };
  auto unit_geo = [&](int u) {
    Unit q;
    int b = u / nct;
    q.co0 = (u - b * nct) * CO;
    const int bw_ = b % g.nbw; b /= g.nbw;
    const int bh_ = b % g.nbh; b /= g.nbh;
    const int bd_ = b % g.nbd;
    q.nn = b / g.nbd;
    q.d0 = bd_ * GB_BD; q.h0 = bh_ * GB_BH; q.w0 = bw_ * BW;
    return q;
  };

  u32x4 hpre[HLD];
  unsigned hmask = 0;  // bit i: staged piece i is inside the volume (GroupNorm'd; padding stays zero)
  u32x4 wpre[WLD];
  const int sch = tid & 3, srow0 = tid >> 2;
  int stg_nn = 0, stg_c = 0;  // sample and chunk of the staged halo (GN table lookup at commit)
  // (buffer loads: 32-bit offsets from scalar bases, no per-lane 64-bit addresses held across the unit loop)
  const auto srs = __builtin_amdgcn_make_buffer_rsrc((void*)gstat, 0, has_gn ? 0x7FFFFFFF : 0, 0x00020000);
  const auto grs = __builtin_amdgcn_make_buffer_rsrc((void*)gamma, 0, has_gn ? 0x7FFFFFFF : 0, 0x00020000);
  const auto brs = __builtin_amdgcn_make_buffer_rsrc((void*)beta, 0, has_gn ? 0x7FFFFFFF : 0, 0x00020000);
  auto gtab_fill = [&](int nn) {
    if (has_gn && tid < gtc_p) {
      int t = tid;
      asm volatile("" : "+v"(t));  // recompute channel and group here (once per sample), not held across the loop
      const int c = min(t, gtc - 1), gg = c / (gtc / g.gn_groups);
      const int so = (nn * g.gn_groups + gg) * 8;
      const float mean = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srs, so, 0, 0));
      const float rstd = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srs, so + 4, 0, 0));
      const float sc_ = rstd * __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grs, c * 4, 0, 0));
      const float sh_ = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(brs, c * 4, 0, 0)) - mean * sc_;
      if constexpr (GB)
        gbt[nn & 1][tid] = f32x4{sc_, sh_, rstd, mean};
      else
        gtab[nn & 1][tid] = f32x2{sc_, sh_};
    }
  };
  // buffer loads with 32-bit offsets (the host guarantees x, y / the residual and the weight pack below 2 GiB): the
  // records are the tensors' exact byte sizes, so the sentinel offset 0xFFFFFFF0 of a masked piece is out of range and
  // returns zeros with no branch around the load; an offset needs one register, not a 64-bit address
  const int xbytes = g.n * g.d * g.h * g.w * g.cin * 2, ybytes = g.n * g.d * g.h * g.w * g.cout * 2;
  const auto xrs = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, xbytes, 0x00020000);
  const auto wrs = __builtin_amdgcn_make_buffer_rsrc((void*)wpk, 0, 27 * g.cout_p * g.cin_p * 2, 0x00020000);
  const auto rrs = __builtin_amdgcn_make_buffer_rsrc((void*)res, 0, res ? ybytes : 0, 0x00020000);
  const auto yrs = __builtin_amdgcn_make_buffer_rsrc((void*)y, 0, ybytes, 0x00020000);
  const auto prs = __builtin_amdgcn_make_buffer_rsrc((void*)spart, 0, spart ? 0x7FFFFFFF : 0, 0x00020000);
  auto halo_load = [&](const Unit& q, int c) {
    hmask = 0;
    stg_nn = q.nn;
    stg_c = c;
    const int cc = c * 32 + sch * 8;
#pragma unroll
    for (int i = 0; i < HLD; ++i) {
      const int row = srow0 + i * (GB_NT / 4);
      const int hw = row % HW, hr = (row / HW) % HH, hd = row / (HW * HH);
      const int zd = q.d0 - 1 + hd, zh = q.h0 - 1 + hr, zw = q.w0 - 1 + hw;
      const bool in = row < NH && (unsigned)zd < (unsigned)g.d && (unsigned)zh < (unsigned)g.h &&
                      (unsigned)zw < (unsigned)g.w;
      hmask |= (in ? 1u : 0u) << i;
      const unsigned off =
          in && cc < g.cin ? (unsigned)(((((q.nn * g.d + zd) * g.h + zh) * g.w + zw) * g.cin + cc) * 2) : 0xFFFFFFF0u;
      hpre[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0));
    }
  };
  auto halo_commit = [&]() {
    f32x2 sc[4], sh[4];
    if (pro_gn) {
      const f32x2* t = &gtab[stg_nn & 1][stg_c * 32 + sch * 8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x2 a0 = t[2 * e], a1 = t[2 * e + 1];
        sc[e] = f32x2{a0[0], a1[0]};
        sh[e] = f32x2{a0[1], a1[1]};
      }
    }
#pragma unroll
    for (int i = 0; i < HLD; ++i) {
      const int row = srow0 + i * (GB_NT / 4);
      if (row < NH) {
        u32x4 v = hpre[i];
        if (pro_gn && ((hmask >> i) & 1u)) v = gn_relu8(v, sc, sh);
        *reinterpret_cast<u32x4*>(hal + sch * PS + row * 16) = v;
      }
    }
  };
  auto w_load = [&](int co0, int s) {
    const int c = s / 3, td = s % 3;
#pragma unroll
    for (int i = 0; i < WLD; ++i) {
      const int ci = tid + i * GB_NT;
      // 4 consecutive lanes = one (tap, co) row's 4 chunks: 64 contiguous bytes of the pack per 4 lanes (the chunk-
      // major order read 16 B per cache line and lane)
      const int ch = ci & 3, row = ci >> 2;
      const int j = row / CO, co = co0 + row % CO;
      const int t = td * 9 + j;
      const unsigned off = ci < WROWS * 4 && co < g.cout_p
                               ? (unsigned)(((t * g.cout_p + co) * g.cin_p + c * 32 + ch * 8) * 2) : 0xFFFFFFF0u;
      wpre[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, off, 0, 0));
    }
  };
  auto w_commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < WLD; ++i) {
      const int ci = tid + i * GB_NT;
      if (ci < WROWS * 4) {
        const int ch = ci & 3, row = ci >> 2;
        *reinterpret_cast<u32x4*>(wbuf[buf] + ch * WPS + row * 16) = wpre[i];
      }
    }
  };

  // per-lane A row of tap (0,0,0) for row tile tm (rt = 2*wave + tm -> (d = rt >> 2, h-pair = rt & 3)) and the
  // output voxel of MFMA column r
  int arow[TM];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    int vd, vh, vw;
    tile_vox(TM * wave + tm, r, vd, vh, vw);
    arow[tm] = (vd * HH + vh) * HW + vw;
  }

  Unit cu = unit_geo(u_begin);
  gtab_fill(cu.nn);
  __syncthreads();
  halo_load(cu, 0);
  w_load(cu.co0, 0);
  halo_commit();
  w_commit(0);
  __syncthreads();
  int par = 0;

  for (int u = u_begin; u < u_end; ++u) {
    const bool more = u + 1 < u_end;
    const Unit nu = more ? unit_geo(u + 1) : cu;
    // the next unit's sample table: its slot was last read before this unit's first barrier, and is first read at
    // the commit in this unit's last step (>= 1 barrier later)
    if (more && nu.nn != cu.nn) gtab_fill(nu.nn);
    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[tm][tn][e] = 0.f;
    // epilogue from registers: lane (r, hh) holds channels tn*32 + 8q + 4hh + e (acc[tm][tn][4q + e]) of voxel
    // ovox[tm]; after the swap it holds channels tn*32 + 8hh .. +7 and tn*32 + 16 + 8hh .. +7
    // this lane's output voxels (MFMA column r of row tiles 0, 1)
    int ovox[TM];  // < 2^31 voxels x channels (host check): 32-bit buffer offsets
    bool ook[TM];
    auto out_vox = [&]() {
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        int vd, vh, vw;
        tile_vox(TM * wave + tm, r, vd, vh, vw);
        const int zd = cu.d0 + vd, zh = cu.h0 + vh, zw = cu.w0 + vw;
        ook[tm] = zd < g.d && zh < g.h && zw < g.w;
        ovox[tm] = ((cu.nn * g.d + zd) * g.h + zh) * g.w + zw;
      }
    };
    // (GB: before the walk, its x loads go out in the last step; otherwise after it: nothing held across the MFMAs)
    if constexpr (GB) out_vox();
    u32x4 rv[TM][TN][2];
    auto res_load = [&](int tn) {  // the residual of co block tn (buffer loads: zeros where res is null)
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const int co = cu.co0 + tn * 32 + 16 * v + 8 * hh;
          const unsigned ro = (ook[tm] && co < g.cout) ? (unsigned)((ovox[tm] * g.cout + co) * 2) : 0xFFFFFFF0u;
          rv[tm][tn][v] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rrs, ro, 0, 0));
        }
    };
    for (int s = 0; s < nsteps; ++s) {
      const int td = s % 3;
      const bool last = s + 1 == nsteps;
      const bool next = !last || more;
      if (next) {  // one call site each (the next step is (u, s + 1) or (u + 1, 0))
        const Unit& lq = last ? nu : cu;
        w_load(lq.co0, last ? 0 : s + 1);
        if (td == 2) halo_load(lq, last ? 0 : s / 3 + 1);
      }
      if constexpr (GB) {  // the GN input x (first co block; all with 8-wide bricks) flies under the last tap plane
        if (last)
#pragma unroll
          for (int tn = 0; tn < GB_EARLY; ++tn) res_load(tn);
      }
      const char* wb = wbuf[par];
      const int od = FLIP ? 2 - td : td;
      // the tap plane's 18 k16 steps (tap j, k-half k), the fragments of step i + 1 read before the MFMAs of step
      // i (one scheduling region per step): two fragment sets in flight, so the 64-channel variants keep the
      // accumulators and the staging prefetch within 256 VGPRs
      bf16x8 fa[2][TM], fb[2][TN];
      auto rd = [&](int j, int k, int slot) {
        const int th = j / 3, tw = j % 3;
        const int oh = FLIP ? 2 - th : th, ow = FLIP ? 2 - tw : tw;
        const int toff = (od * HH + oh) * HW + ow;
        const int plane = 2 * k + hh;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
          fa[slot][tm] = *reinterpret_cast<const bf16x8*>(hal + plane * PS + (arow[tm] + toff) * 16);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          fb[slot][tn] = *reinterpret_cast<const bf16x8*>(wb + plane * WPS + (j * CO + tn * 32 + r) * 16);
      };
      rd(0, 0, 0);
#pragma unroll 1
      for (int j0 = 0; j0 < 9; j0 += 3) {
        static_for<0, 6>([&](auto ic) {
          constexpr int i = decltype(ic)::value, slot = i & 1;
          const int j = j0 + (i >> 1);
          if (i < 5 || j0 < 6) rd(i < 5 ? j + ((i & 1) ? 1 : 0) : j0 + 3, (i + 1) & 1, slot ^ 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
              acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[slot][tn], fa[slot][tm], acc[tm][tn], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        });
      }
      if (last) break;  // the last step's staging commit runs after the residual loads are issued (below)
      w_commit(par ^ 1);  // the other buffer: its readers finished before the previous barrier
      if (td == 2) {
        __syncthreads();  // everyone done with this chunk's halo
        halo_commit();
      }
      __syncthreads();
      par ^= 1;
    }

    // the first co block's residual flies under the last step's staging commit (the next unit's first weights and
    // halo); the other blocks' are issued after it, when the staging registers are free
    if constexpr (!GB) out_vox();
    if (!GB && res) res_load(0);
    if (more) {
      w_commit(par ^ 1);
      __syncthreads();
      halo_commit();
    }
    if (res) {  // (GB: the x of the blocks not loaded early, under the first block's epilogue)
#pragma unroll
      for (int tn = GB ? GB_EARLY : 1; tn < TN; ++tn) res_load(tn);
    }
    __syncthreads();
    par ^= 1;
    // (statistics of the stored bf16 outputs, per channel pair: the GN(16) groups of every cout % 32 == 0 hold
    // whole pairs. Unshifted fp32 E[x^2] - mean^2 loses |mean|^2 / var digits to cancellation: ~1e-3 relative rstd at
    // |mean| / std = 50 with the rounds 2-3 fp32 partials (ADVICE r2 / VERDICT r3). Sums of x - shift in fp32 (the
    // shift: the pair's first channel at the half-wave's first voxel, so |x - shift| ~ std), reduced transposed over
    // the half-wave, then un-shifted in fp64 for the fixed-order reductions over waves and units
    // (tests/test_gpu_pbrick.py, |mean| / std ~ 50 cases). An fp64 shuffle reduction of unshifted sums (round 4,
    // first form) cost 7 us per 2x48^3 launch (kbench fwd48st 76.5 -> 83.2 us).)
    // per co block tn: (sum, sum sq) of the 4 channel pairs q of each v half, over this lane's voxels; reduced over the
    // lane half (32 voxels) and stored per wave into the LDS before the next co block (8 pairs live, not 16)
    f32x2 ps[2 * 4];
    float shv[2 * 4];  // output statistics: per channel pair of the co block, the shift of its sums
    float* const gred = reinterpret_cast<float*>(&sst[0][0][0][0]);  // GB: [wave][tn][hh][32] (sst is idle in FLIP)
    static_assert(!GB || sizeof(sst) >= 8 * TN * 2 * 32 * sizeof(float), "GB reduction buffer");
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      if constexpr (GB) {
        // per channel half v: (sum g, sum g*xhat) of this lane's 8 channels e over its voxels tm, from the stored bf16
        // dA and x at the same address (as gn_bwd_partial reads them); v outer so that 16 sums are live, not 32
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const int co = cu.co0 + tn * 32 + 16 * v + 8 * hh;
          u32x4 o[TM];
#pragma unroll
          for (int tm = 0; tm < TM; ++tm) {
            uint32_t pk[2][2];
#pragma unroll
            for (int qq = 0; qq < 2; ++qq)
#pragma unroll
              for (int e = 0; e < 2; ++e)
                pk[qq][e] = pack_bf16x2(acc[tm][tn][4 * (2 * v + qq) + 2 * e], acc[tm][tn][4 * (2 * v + qq) + 2 * e + 1]);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const auto sw = __builtin_amdgcn_permlane32_swap(pk[0][e], pk[1][e], false, false);
              pk[0][e] = sw[0];
              pk[1][e] = sw[1];
            }
            o[tm] = u32x4{pk[0][0], pk[0][1], pk[1][0], pk[1][1]};
            if (ook[tm] && co < g.cout)
              __builtin_amdgcn_raw_buffer_store_b128(o[tm], yrs, (unsigned)((ovox[tm] * g.cout + co) * 2), 0, 0);
          }
          // two passes of 4 channels (8 sums live), channel outer (one table entry live): holding more spilled
          const f32x4* tb = &gbt[cu.nn & 1][co];
          // dA of voxels past the volume / padded channels -> 0 (their x reads returned zeros: all terms finite)
#pragma unroll
          for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int k = 0; k < 4; ++k) o[tm][k] = (ook[tm] && co < g.cout) ? o[tm][k] : 0u;
#pragma unroll
          for (int eh = 0; eh < 2; ++eh) {
            float gbs[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) gbs[i] = 0.f;
#pragma unroll
            for (int el = 0; el < 4; ++el) {
              const int e = eh * 4 + el;
              const f32x4 t = tb[e];
#pragma unroll
              for (int tm = 0; tm < TM; ++tm) {
                const uint32_t ow = o[tm][e >> 1], xw = rv[tm][tn][v][e >> 1];
                const float a = __builtin_bit_cast(float, (e & 1) ? (ow & 0xFFFF0000u) : (ow << 16));
                const float xv = __builtin_bit_cast(float, (e & 1) ? (xw & 0xFFFF0000u) : (xw << 16));
                const float gd = fmaf(xv, t[0], t[1]) > 0.f ? a : 0.f;  // the forward prologue's relu test
                gbs[el * 2] += gd;
                gbs[el * 2 + 1] = fmaf(gd, xv - t[3], gbs[el * 2 + 1]);  // sum g (x - mean); x rstd at the end
              }
            }
            half_sum8_transposed(gbs, r);
            if ((r & 3) == 0) gred[((wave * TN + tn) * 2 + hh) * 32 + v * 16 + eh * 8 + (r >> 2)] = gbs[0];
          }
        }
        continue;
      }
#pragma unroll
      for (int i = 0; i < 2 * 4; ++i) ps[i] = f32x2{0.f, 0.f};
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        uint32_t pk[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int e = 0; e < 2; ++e)
            pk[q][e] = pack_bf16x2(acc[tm][tn][4 * q + 2 * e], acc[tm][tn][4 * q + 2 * e + 1]);
#pragma unroll
        for (int q = 0; q < 4; q += 2)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const auto sw = __builtin_amdgcn_permlane32_swap(pk[q][e], pk[q + 1][e], false, false);
            pk[q][e] = sw[0];
            pk[q + 1][e] = sw[1];
          }
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const int co = cu.co0 + tn * 32 + 16 * v + 8 * hh;
          u32x4 o = {pk[2 * v][0], pk[2 * v][1], pk[2 * v + 1][0], pk[2 * v + 1][1]};
          if (res) {
            float a8[8], c8[8];
            load16<bf16>(reinterpret_cast<const bf16*>(&o), a8);
            load16<bf16>(reinterpret_cast<const bf16*>(&rv[tm][tn][v]), c8);
#pragma unroll
            for (int e = 0; e < 8; ++e) a8[e] += c8[e];
            store16<bf16>(reinterpret_cast<bf16*>(&o), a8);
          }
          if (ook[tm] && co < g.cout)
            __builtin_amdgcn_raw_buffer_store_b128(o, yrs, (unsigned)((ovox[tm] * g.cout + co) * 2), 0, 0);
          if (spart != nullptr) {
            float f8[8];
            load16<bf16>(reinterpret_cast<const bf16*>(&o), f8);
            const bool on = ook[tm] && co < g.cout;
            if (tm == 0)  // the pair's shift: its first channel at the half-wave's lane 0 voxel (a brick origin: inside)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int xb = __builtin_bit_cast(int, f8[2 * q]);
                shv[v * 4 + q] = __builtin_bit_cast(float, hh ? __builtin_amdgcn_readlane(xb, 32)
                                                                : __builtin_amdgcn_readlane(xb, 0));
              }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float a0 = f8[2 * q] - shv[v * 4 + q], a1 = f8[2 * q + 1] - shv[v * 4 + q];
              f32x2& t = ps[v * 4 + q];
              t[0] += on ? a0 + a1 : 0.f;
              t[1] = on ? fmaf(a0, a0, fmaf(a1, a1, t[1])) : t[1];
            }
          }
        }
      }
      if (spart != nullptr) {  // this tn's pairs: reduce over the 32 voxels of each lane half into the LDS
        // shifted fp32 sums (|x - shift| ~ std, not |mean|), transposed over the half-wave (lane r ends with pair
        // (r >> 2) & 7), then un-shifted in fp64: S = sum + n s, Q = sumsq + 2 s sum + n s^2 with n the pair's valid
        // values in this half-wave (2 channels x the voxels inside the volume)
        float s1[8], s2[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          s1[i] = ps[i][0];
          s2[i] = ps[i][1];
        }
        const float t1 = half_sum8_transposed(s1, r), t2 = half_sum8_transposed(s2, r);
        unsigned nvox = 0;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
          const unsigned long long b = __ballot(ook[tm]);
          nvox += __builtin_popcount(hh ? (unsigned)(b >> 32) : (unsigned)b);
        }
        if ((r & 3) == 0) {
          const int i = r >> 2, v = i >> 2;
          float shi = shv[0];  // (select, not a dynamic index: that would put shv in scratch)
#pragma unroll
          for (int j = 1; j < 8; ++j) shi = i == j ? shv[j] : shi;
          const double sh = (double)shi;
          const double nn = cu.co0 + tn * 32 + 16 * v + 8 * hh < g.cout ? 2.0 * nvox : 0.0;
          sst[wave][hh][tn * 8 + i][0] = (double)t1 + nn * sh;
          sst[wave][hh][tn * 8 + i][1] = (double)t2 + 2.0 * sh * (double)t1 + nn * sh * sh;
        }
      }
    }
    if constexpr (GB) {  // the 8 waves in order, per (channel, sum) of the tile -> parts[brick][cout][2]
      __syncthreads();
      if (tid < CO * 2) {
        const int cl = tid >> 1, k = tid & 1, tn = cl >> 5, v = (cl >> 4) & 1, h_ = (cl >> 3) & 1, e = cl & 7;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) t += gred[((w * TN + tn) * 2 + h_) * 32 + (v * 8 + e) * 2 + k];
        const int co = cu.co0 + cl;
        if (co < g.cout) gbpart[((long long)(u / nct) * g.cout + co) * 2 + k] = k ? t * gbt[cu.nn & 1][co][2] : t;
      }
    }
    if (spart != nullptr) {  // the 8 waves in order, per channel pair of the tile
      __syncthreads();
      if (tid < CO / 2) {  // channel pair tid of the tile: c = 2 tid -> (tn, v, hh, q)
        const int c = 2 * tid, tn = c >> 5, w32 = c & 31, v = w32 >> 4, h_ = (w32 >> 3) & 1, q = (w32 & 7) >> 1;
        double t0 = 0.0, t1 = 0.0;
        for (int w = 0; w < 8; ++w) {
          t0 += sst[w][h_][(tn * 2 + v) * 4 + q][0];
          t1 += sst[w][h_][(tn * 2 + v) * 4 + q][1];
        }
        typedef __attribute__((ext_vector_type(2))) double f64x2;
        if (g.fcnt)  // (write-through: the finalizing workgroup reads them in this launch)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (f64x2){t0, t1}), prs, (u * CO + c) * 8, 0,
                                                 16);
        else
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (f64x2){t0, t1}), prs, (u * CO + c) * 8, 0,
                                                 0);
      }
    }
    cu = nu;
  }
  if constexpr (!GB) {
    if (spart != nullptr && g.fcnt != nullptr) {
      // Round 5: the GroupNorm(16) finalize (pbrick_gn_finalize_kernel's sums, one launch less) by the workgroup that
      // arrives last (last_arriver; the partials above are its sc1 stores). 16 lanes per (sample, group), strided over
      // the sample's bricks, the pairs in order, then an xor tree over the 16 lanes in fixed order: deterministic.
      if (last_arriver(g.fcnt, gridDim.x)) {
        const int bps = g.nbd * g.nbh * g.nbw, cpg = g.cout / 16, l16 = tid & 15;
        const double m = (double)cpg * g.d * g.h * g.w;
        for (int p0 = 0; p0 < g.n * 16; p0 += GB_NT / 16) {
          const int p = p0 + (tid >> 4);
          double s1 = 0, s2 = 0;
          if (p < g.n * 16) {
            // this lane's (brick, channel pair) items in the order b = l16, l16 + 16, ..., pairs inner; 8 sc1 loads
            // in flight (a dependent load per item cost the launch ~10 us)
            typedef __attribute__((ext_vector_type(2))) double f64x2;
            const int nn = p >> 4, gr = p & 15, ncp = cpg >> 1, nk = (bps - l16 + 15) / 16 * ncp;
            for (int k0 = 0; k0 < nk; k0 += 8) {
              f64x2 q[8];
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const int k = k0 + u, bi = k / ncp, c = gr * cpg + 2 * (k - bi * ncp), ct = c / CO, cl = c - ct * CO;
                const long long brick = (long long)nn * bps + l16 + 16 * bi;
                q[u] = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(
                                                     prs, k < nk ? (int)(((brick * g.nct + ct) * CO + cl) * 8)
                                                                 : (int)0xFFFFFFF0u, 0, 16));
              }
#pragma unroll
              for (int u = 0; u < 8; ++u)
                if (k0 + u < nk) {
                  s1 += q[u][0];
                  s2 += q[u][1];
                }
            }
          }
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) {
            s1 += __shfl_xor(s1, o);
            s2 += __shfl_xor(s2, o);
          }
          if (p < g.n * 16 && l16 == 0) gn_store_stats(g.fstats + p * 2, s1, s2, m);
        }
      }
    }
  }
}

// GroupNorm(16) (mean, rstd) of the persistent brick conv's output from its per-unit channel-pair partials
// spart[unit][CO / 2][2] (unit = brick * nct + co tile): one 256-thread block per (sample, group), item k = (brick
// k / npg, pair k % npg) of the sample, threads strided over the items with 8 loads in flight (r05: one wave with a
// dependent load per item), the wave butterflies, then the 4 waves in order (fixed order: deterministic)
__global__ __launch_bounds__(256) void pbrick_gn_finalize_kernel(const double* __restrict__ spart, int co_tile, int nct,
                                                                int bricks_per_sample, int cout, double m,
                                                                float* __restrict__ stats) {
  __shared__ double red[4][2];
  const int p = blockIdx.x, nn = p / 16, gr = p % 16, cpg = cout / 16, npg = cpg / 2, tid = threadIdx.x;
  const int nk = bricks_per_sample * npg;
  double s1 = 0, s2 = 0;
  for (int k0 = tid; k0 < nk; k0 += 8 * 256) {
    double2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + u * 256;
      if (k < nk) {
        const int b = k / npg, c = gr * cpg + 2 * (k - b * npg), ct = c / co_tile, cl = c - ct * co_tile;
        v[u] = *reinterpret_cast<const double2*>(spart + ((((long long)nn * bricks_per_sample + b) * nct + ct) * co_tile + cl));
      } else {
        v[u] = make_double2(0.0, 0.0);
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s1 += v[u].x;
      s2 += v[u].y;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = s1;
    red[tid >> 6][1] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    const double t1 = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    const double t2 = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    gn_store_stats(stats + p * 2, t1, t2, m);
  }
}


}  // namespace u3d

using namespace u3d;

static int convg_num_cus() {
  static int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      v = 256;
    return v > 0 ? v : 256;
  }();
  return n;
}

// 8-wide bricks where the plane width is a multiple of 8 but not of 16 (24^3: the 16-wide bricks' second column is
// half empty); CONVG_BW8 = 0 / 1 forces the choice (A/B)
static bool pbrick_bw8(int w) {
  const int e8 = opt(OPT_CONVG_BW8);
  return e8 >= 0 ? e8 != 0 : (w % 16 != 0 && w % 8 == 0);
}

// 64-channel co tiles, unless they give fewer than 128 workgroups and 32-channel tiles give at least 128 (the 24^3 x
// 64-channel decoder convs: 72 -> 144 workgroups, fwd 49 -> 25 us, dgrad 40 -> 20 us). Not below that: at 24^3 x 128
// channels (144 workgroups with 64-channel tiles) 32-channel tiles measured slower (63.5 -> 78.7 us).
// U3D_CONVG_CO32 = 0 / 1 forces the choice (experiments).
static bool gb_co64(long long units, int cout, int cout_p) {
  const int env_co32 = opt(OPT_CONVG_CO32);
  if (cout_p < 64 || env_co32 == 1) return false;
  return !(env_co32 < 0 && units * cdiv(cout, 64) < 128 && units * cdiv(cout, 32) >= 128);
}

struct GBPlan {
  bool pers, bw8, co64;  // the persistent form, its 8-wide bricks, 64-channel co tiles
  int nunits, per, nwg;  // (brick, co tile) units, units per workgroup (1 in the one-shot form), workgroups
};

// The launch plan of the generic brick conv: which form runs, brick width and co tile, and the grid. Fills g's shape
// fields for the chosen form (nbw and nct depend on it). The launcher and u3d_convg_brick_gn_nparts both plan here, so
// `parts` is never laid out for another form than the one that writes it. cin / cout are the launch's own (a data
// gradient contracts over cin = the forward's cout); gn: a GroupNorm prologue (or, with gbparts, the fused backward).
static GBPlan gb_plan(bool flip, int n, int cin, int d, int h, int w, int cout, bool gn, bool residual, bool gbparts,
                      GBGeom& g) {
  g = GBGeom{};
  g.n = n; g.d = d; g.h = h; g.w = w;
  g.cin = cin; g.cout = cout; g.cin_p = round_up(cin, 32); g.cout_p = round_up(cout, 32);
  GBPlan p{};
  // the persistent form runs unless CONVG_PERSIST = 0 (the one-shot kernel; u3d_set_option lets a test compare both
  // in-process), x or the weight pack is beyond its 32-bit buffer offsets, the GroupNorm has more than GB_MAXC
  // channels, or a data gradient adds a residual (not a trunk routing, kept for the ABI: the persistent data gradient
  // has no residual path, so its epilogue reserves no registers for one)
  p.pers = opt(OPT_CONVG_PERSIST) != 0 && n >= 1 && n <= GB_MAXN &&
           fits_buffer_offsets((long long)n * d * h * w * std::max(cin, cout) * 2) &&
           fits_buffer_offsets(27LL * g.cout_p * g.cin_p * 2) &&
           (!gn || (gbparts ? g.cout_p : g.cin_p) <= GB_MAXC) && !(flip && residual);
  p.bw8 = p.pers && pbrick_bw8(w);
  g.nbd = cdiv(d, GB_BD); g.nbh = cdiv(h, GB_BH); g.nbw = cdiv(w, p.bw8 ? 8 : GB_BW);
  const long long bricks = (long long)n * g.nbd * g.nbh * g.nbw;
  p.co64 = gb_co64(bricks, cout, g.cout_p);
  g.nct = cdiv(cout, p.co64 ? 64 : 32);
  p.nunits = (int)(bricks * g.nct);
  p.per = p.pers ? cdiv(p.nunits, convg_num_cus()) : 1;
  p.nwg = cdiv(p.nunits, p.per);
  return p;
}

// Not the plan's own size but an upper bound over both brick widths and co tiles, so a caller's workspace holds
// whatever gb_plan chooses: units x 32 channel pairs x 2 doubles (= 128 floats)
extern "C" long long u3d_convg_brick_stats_ws_floats(int n, int d, int h, int w, int cout) {
  return (long long)n * cdiv(d, GB_BD) * cdiv(h, GB_BH) * cdiv(w, 8) * cdiv(cout, 32) * 128;
}

// what a launch passes besides the plan and the geometry (res: the residual, or the GN input x of the fused GroupNorm
// backward; spart: the forward's statistics partials, or that backward's parts)
struct GBArgs {
  const void *x, *wpk;
  void* y;
  const void* res;
  const float *gstat, *gamma, *beta;
  float* spart;
  hipStream_t s;
};

template <int CO, bool FLIP, int BWX, bool GB>
static void gb_launch(const GBPlan& p, const GBGeom& g, const GBArgs& a) {
  if (p.pers)
    hipLaunchKernelGGL((convg_pbrick_kernel<CO, FLIP, BWX, GB>), dim3(p.nwg), dim3(GB_NT), 0, a.s, (const bf16*)a.x,
                       (const bf16*)a.wpk, (bf16*)a.y, (const bf16*)a.res, a.gstat, a.gamma, a.beta, g, p.per, p.nunits,
                       a.spart);
  else
    hipLaunchKernelGGL((convg_brick_kernel<CO, FLIP>), dim3(p.nwg), dim3(GB_NT), 0, a.s, (const bf16*)a.x,
                       (const bf16*)a.wpk, (bf16*)a.y, (const bf16*)a.res, a.gstat, a.gamma, a.beta, g);
}

// the one ladder from the plan to the kernels' template arguments (GB: on the data gradient only)
template <int CO>
static void gb_dispatch(bool flip, bool gb, const GBPlan& p, const GBGeom& g, const GBArgs& a) {
  if (!flip) p.bw8 ? gb_launch<CO, false, 8, false>(p, g, a) : gb_launch<CO, false, 16, false>(p, g, a);
  else if (gb) p.bw8 ? gb_launch<CO, true, 8, true>(p, g, a) : gb_launch<CO, true, 16, true>(p, g, a);
  else p.bw8 ? gb_launch<CO, true, 8, false>(p, g, a) : gb_launch<CO, true, 16, false>(p, g, a);
}

static int convg_impl(int flip, const void* x, int n, int cin, int d, int h, int w, const void* wpk, int cout,
                      const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_groups,
                      const void* residual, void* y, float* spart, float* stats_out, u3d_stream_t stream,
                      const void* gbx = nullptr, float* gbparts = nullptr, unsigned* fcnt = nullptr) {
  U3D_REQUIRE(x && wpk && y && n >= 1 && n <= GB_MAXN, "convg_brick: bad args");
  U3D_REQUIRE(!gbparts || (flip && gbx && gn_stats && !residual && !spart && cout % gn_groups == 0),
              "convg_brick_dgrad_gn: bad args");
  U3D_REQUIRE(cin % 8 == 0 && cout % 8 == 0, "convg_brick: channels must be multiples of 8");
  U3D_REQUIRE(!gn_stats || (gn_gamma && gn_beta && gn_groups > 0 && (gbparts ? cout : cin) % gn_groups == 0),
              "convg_brick: bad GN");
  GBGeom g;
  const GBPlan p = gb_plan(flip, n, cin, d, h, w, cout, gn_stats, residual, gbparts, g);
  g.gn_groups = gn_groups;
  U3D_REQUIRE(!spart || (p.pers && !flip && cout % 32 == 0), "convg_brick_stats: needs the persistent forward, cout %% 32 == 0");
  U3D_REQUIRE(!gbparts || p.pers, "convg_brick_dgrad_gn: needs the persistent data gradient (u3d_convg_brick_gn_nparts)");
  if (spart && fcnt) {
    g.fstats = stats_out;
    g.fcnt = fcnt;
  }
  hipStream_t s = (hipStream_t)stream;
  const GBArgs a{x, wpk, y, gbparts ? gbx : residual, gn_stats, gn_gamma, gn_beta, gbparts ? gbparts : spart, s};
  if (p.co64) gb_dispatch<64>(flip, gbparts, p, g, a);
  else gb_dispatch<32>(flip, gbparts, p, g, a);
  int rc = check_launch(p.pers ? "convg_pbrick_kernel" : "convg_brick_kernel");
  if (rc || !spart || fcnt) return rc;  // (fcnt: finalized by the kernel's last-arriving workgroup)
  hipLaunchKernelGGL(pbrick_gn_finalize_kernel, dim3(n * 16), dim3(256), 0, s, (const double*)spart, p.co64 ? 64 : 32, g.nct,
                     g.nbd * g.nbh * g.nbw, cout, (double)(cout / 16) * d * h * w, stats_out);
  return check_launch("pbrick_gn_finalize_kernel");
}

extern "C" int u3d_convg_brick(int flip, const void* x, int n, int cin, int d, int h, int w, const void* wpk, int cout,
                               const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_groups,
                               const void* residual, void* y, u3d_stream_t stream) {
  return convg_impl(flip, x, n, cin, d, h, w, wpk, cout, gn_stats, gn_gamma, gn_beta, gn_groups, residual, y, nullptr,
                    nullptr, stream);
}

// Data gradient of conv(relu(gn(x))) with gn_bwd's partial pass fused into the persistent brick's epilogue
// (convg_pbrick_kernel<.., GB>): dx = the data gradient dA (as u3d_convg_brick(flip = 1)), parts[n][nparts][cin][2]
// (nparts = u3d_convg_brick_gn_nparts) = per brick (sum g, sum g*xhat) of g = relu-mask * dA for u3d_gn_bwd_parts.
// Here cin / cout are the FORWARD conv's channels: dy has cout, x / dA have cin; gn_* is the GroupNorm on x.
extern "C" int u3d_convg_brick_gn_nparts(int n, int cin, int d, int h, int w, int cout) {
  GBGeom g;
  return gb_plan(true, n, cout, d, h, w, cin, true, false, true, g).pers ? g.nbd * g.nbh * g.nbw : 0;
}

extern "C" int u3d_convg_brick_dgrad_gn(const void* dy, int n, int cout, int d, int h, int w, const void* wpk_dgrad,
                                        int cin, const void* x, const float* gn_stats, const float* gn_gamma,
                                        const float* gn_beta, int gn_groups, void* dx, float* parts, int nparts,
                                        u3d_stream_t stream) {
  U3D_REQUIRE(parts && x && nparts == u3d_convg_brick_gn_nparts(n, cin, d, h, w, cout) && nparts > 0,
              "convg_brick_dgrad_gn: parts layout (u3d_convg_brick_gn_nparts) mismatch");
  return convg_impl(1, dy, n, cout, d, h, w, wpk_dgrad, cin, gn_stats, gn_gamma, gn_beta, gn_groups, nullptr, dx,
                    nullptr, nullptr, stream, x, parts);
}

extern "C" int u3d_convg_brick_stats(const void* x, int n, int cin, int d, int h, int w, const void* wpk, int cout,
                                     const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_groups,
                                     const void* residual, void* y, float* stats_ws, long long ws_floats,
                                     float* stats_out, u3d_stream_t stream) {
  U3D_REQUIRE(stats_ws && stats_out, "convg_brick_stats: null statistics buffers");
  U3D_REQUIRE(ws_floats >= u3d_convg_brick_stats_ws_floats(n, d, h, w, cout), "convg_brick_stats: workspace too small");
  return convg_impl(0, x, n, cin, d, h, w, wpk, cout, gn_stats, gn_gamma, gn_beta, gn_groups, residual, y, stats_ws,
                    stats_out, stream);
}

// Round 5: u3d_convg_brick_stats with the statistics finalized inside the conv launch by its last-arriving workgroup
// (no pbrick_gn_finalize_kernel launch). cnt: one ZEROED unsigned (left zeroed by every launch).
extern "C" int u3d_convg_brick_stats_fused(const void* x, int n, int cin, int d, int h, int w, const void* wpk, int cout,
                                           const float* gn_stats, const float* gn_gamma, const float* gn_beta,
                                           int gn_groups, const void* residual, void* y, float* stats_ws,
                                           long long ws_floats, float* stats_out, unsigned* cnt, u3d_stream_t stream) {
  U3D_REQUIRE(stats_ws && stats_out && cnt, "convg_brick_stats_fused: null statistics buffers");
  U3D_REQUIRE(ws_floats >= u3d_convg_brick_stats_ws_floats(n, d, h, w, cout), "convg_brick_stats: workspace too small");
  return convg_impl(0, x, n, cin, d, h, w, wpk, cout, gn_stats, gn_gamma, gn_beta, gn_groups, residual, y, stats_ws,
                    stats_out, stream, nullptr, nullptr, cnt);
}
