// 3^3 stride-1 convolution (forward / data gradient) for the small deep-level volumes (24^3, 12^3, 6^3 of the
// 96^3 U-Net: 128 / 256 channels), bf16, halo-brick form sized for PARALLELISM rather than reuse.
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
#include "conv_small_body.h"

namespace u3d {

U3D_STAMP_BUFFER(sc_stamps, 1024, u3d_diag_small_stamps)
U3D_STAMP_BUFFER(sc_tail, 256, u3d_diag_small_tail)  // TailStamps: 16 per workgroup

// one workgroup = one run of the body (conv_small_body.h) on the launch's own 1-D grid
template <bool FLIP>
__global__ __launch_bounds__(SC_NT, 512 / SC_NT) void conv_small_kernel(const bf16* __restrict__ x, const bf16* __restrict__ wpk,
                                                             bf16* __restrict__ y, const bf16* __restrict__ res,
                                                             const float* __restrict__ gstat,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, SCGeom g) {
  __shared__ __attribute__((aligned(16))) char smem[SC_SMEM];
  conv_small_body<FLIP>(smem, (int)blockIdx.x, (int)gridDim.x, x, wpk, y, res, gstat, gamma, beta, g, sc_stamps, sc_tail);
}


// y = bf16(sum_s slab[s] (+ residual)), 4 channels per thread, splits summed in fixed order
__global__ __launch_bounds__(256) void small_reduce_kernel(const float* __restrict__ slab, int nks, long long per4,
                                                           const bf16* __restrict__ res, bf16* __restrict__ y) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < per4; i += (long long)gridDim.x * 256) {
    f32x4 v = reinterpret_cast<const f32x4*>(slab)[i];
    for (int s = 1; s < nks; ++s) v += reinterpret_cast<const f32x4*>(slab)[s * per4 + i];
    if (res) {
      const uint2 q = reinterpret_cast<const uint2*>(res)[i];
      v[0] += __uint_as_float(q.x << 16);
      v[1] += __uint_as_float(q.x & 0xffff0000u);
      v[2] += __uint_as_float(q.y << 16);
      v[3] += __uint_as_float(q.y & 0xffff0000u);
    }
    uint2 o;
    o.x = (uint32_t)from_f<bf16>(v[0]) | ((uint32_t)from_f<bf16>(v[1]) << 16);
    o.y = (uint32_t)from_f<bf16>(v[2]) | ((uint32_t)from_f<bf16>(v[3]) << 16);
    reinterpret_cast<uint2*>(y)[i] = o;
  }
}

}  // namespace u3d

using namespace u3d;

struct SCGb {  // the GroupNorm-backward partials of the data gradient (u3d_conv_small_dgrad_gn)
  const void* x;
  const float *stats, *gamma, *beta;
  int groups;
  float *parts, *coef, *dgamma, *dbeta;
};
static int conv_small_impl(int flip, const void* x, int n, int cin, int d, int h, int w, const void* wpk, int cout,
                           const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_groups,
                           const void* residual, void* y, float* ws, long long ws_bytes, unsigned* cnt,
                           float* spart, float* stats_out, int* nks_out, u3d_stream_t stream,
                           const SCGb* gb = nullptr, bool plan_only = false);

extern "C" int u3d_conv_small(int flip, const void* x, int n, int cin, int d, int h, int w, const void* wpk, int cout,
                              const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_groups,
                              const void* residual, void* y, float* ws, long long ws_bytes, u3d_stream_t stream) {
  return conv_small_impl(flip, x, n, cin, d, h, w, wpk, cout, gn_stats, gn_gamma, gn_beta, gn_groups, residual, y, ws,
                         ws_bytes, nullptr, nullptr, nullptr, nullptr, stream);
}

// Round 5 form: the split-K slabs are combined inside the conv launch by the last-arriving workgroup of each output
// tile (no small_reduce_kernel), and with stats_out the output's GroupNorm(16) statistics come from that combine (no
// statistics pass). cnt: u3d_conv_small_cnt_bytes() of ZEROED memory (left zeroed); spart: u3d_conv_small_spart_floats.
// Statistics need the contraction split (nks > 1) and cout in {64, 128, 256} (4..16 channels per group); where a
// launch cannot produce them it returns 0 with *stats_made = 0 and the caller takes the statistics pass.
extern "C" long long u3d_conv_small_cnt_bytes(int n, int d, int h, int w, int cout) {
  return 4LL * (n * cdiv(d, 1) * cdiv(h, 1) * cdiv(w, 1) * cdiv(cout, 32) + 1);  // >= tiles + 1 (bricks >= 1 voxel)
}
extern "C" long long u3d_conv_small_spart_floats(int n, int d, int h, int w) {
  return 32LL * n * d * h * w;  // >= n * bricks * 32
}
extern "C" int u3d_conv_small2(int flip, const void* x, int n, int cin, int d, int h, int w, const void* wpk, int cout,
                               const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_groups,
                               const void* residual, void* y, float* ws, long long ws_bytes, unsigned* cnt,
                               float* spart, float* stats_out, int* stats_made, u3d_stream_t stream) {
  U3D_REQUIRE(cnt && stats_made, "conv_small2: needs the counter workspace and stats_made");
  int nks = 0;
  // the statistics form's own limits (one thread per (sample, group) in the finalize, 31-bit slab offsets): past
  // them the launch declines with *stats_made = 0 and the caller runs the statistics pass
  const bool want = stats_out && spart && !flip && cout % 16 == 0 &&
                    (cout / 16 == 4 || cout / 16 == 8 || cout / 16 == 16) && n * 16 <= SC_NT &&
                    8LL * n * d * h * w * cout * 4 < (1LL << 31);
  const int rc = conv_small_impl(flip, x, n, cin, d, h, w, wpk, cout, gn_stats, gn_gamma, gn_beta, gn_groups, residual,
                                 y, ws, ws_bytes, cnt, want ? spart : nullptr, want ? stats_out : nullptr, &nks, stream);
  *stats_made = rc == 0 && want && nks > 1 && nks <= 8;
  return rc;
}

static int conv_small_impl(int flip, const void* x, int n, int cin, int d, int h, int w, const void* wpk, int cout,
                           const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_groups,
                           const void* residual, void* y, float* ws, long long ws_bytes, unsigned* cnt,
                           float* spart, float* stats_out, int* nks_out, u3d_stream_t stream,
                           const SCGb* gb, bool plan_only) {
  U3D_REQUIRE(x && wpk && y && n >= 1 && d >= 1 && h >= 1 && w >= 1, "conv_small: bad args");
  U3D_REQUIRE(cin % 8 == 0 && cout % 8 == 0, "conv_small: channels must be multiples of 8");
  U3D_REQUIRE(!gn_stats || (!flip && gn_gamma && gn_beta && gn_groups > 0 && cin % gn_groups == 0),
              "conv_small: bad GN prologue");
  U3D_REQUIRE(!gn_stats || round_up(cin, 32) <= SC_MAXC, "conv_small: GN prologue supports cin <= %d", SC_MAXC);
  SCGeom g;
  const long long tiles = sc_plan(n, cin, d, h, w, cout, gn_groups, ws, ws_bytes, g);
  const long long slab1 = (long long)n * d * h * w * cout * 4;
  if (nks_out) *nks_out = g.nks;
  g.cnt = g.nks > 1 && g.nks <= 8 ? cnt : nullptr;  // in-kernel combine where there are (<= 8) slabs to combine
  g.stats = g.cnt ? stats_out : nullptr;
  g.spart = g.stats ? spart : nullptr;
  if (plan_only) return 0;
  if (gb && g.cnt) {
    U3D_REQUIRE(flip && !residual && gb->groups > 0 && cout % gb->groups == 0 && (long long)n * cout * 2 <= 8192,
                "conv_small_dgrad_gn: bad GroupNorm-backward args");
    g.gbx = (const bf16*)gb->x;
    g.gbstat = gb->stats; g.gbgamma = gb->gamma; g.gbbeta = gb->beta; g.gbgroups = gb->groups;
    g.gbparts = gb->parts; g.coef = gb->coef; g.dgamma = gb->dgamma; g.dbeta = gb->dbeta;
    g.stats = nullptr;
  }
  U3D_REQUIRE(!g.stats || (n * 16 <= SC_NT && g.nks * (long long)n * d * h * w * cout * 4 < (1LL << 31)),
              "conv_small2: statistics form limits");
  const long long nwg = tiles * g.nks;
  U3D_REQUIRE(nwg < (1LL << 31), "conv_small: grid too large");
  U3D_REQUIRE(fits_buffer_offsets((long long)n * d * h * w * std::max(cin, cout) * 2) &&
                  fits_buffer_offsets(27LL * g.cout_p * g.cin_p * 2),
              "conv_small: operands beyond the 2 GiB buffer-offset range");
  hipStream_t s = (hipStream_t)stream;
  if (flip)
    hipLaunchKernelGGL(conv_small_kernel<true>, dim3((unsigned)nwg), dim3(SC_NT), 0, s, (const bf16*)x,
                       (const bf16*)wpk, (bf16*)y, (const bf16*)residual, gn_stats, gn_gamma, gn_beta, g);
  else
    hipLaunchKernelGGL(conv_small_kernel<false>, dim3((unsigned)nwg), dim3(SC_NT), 0, s, (const bf16*)x,
                       (const bf16*)wpk, (bf16*)y, (const bf16*)residual, gn_stats, gn_gamma, gn_beta, g);
  int rc = check_launch("conv_small_kernel");
  if (rc || g.nks == 1 || g.cnt) return rc;
  const long long per4 = slab1 / 16;
  hipLaunchKernelGGL(small_reduce_kernel, dim3((unsigned)std::min<long long>(4096, (per4 + 255) / 256)), dim3(256), 0,
                     s, ws, g.nks, per4, (const bf16*)residual, (bf16*)y);
  return check_launch("small_reduce_kernel");
}

// Round 5: data gradient of conv(relu(gn(x))) for the small deep-level volumes with the GroupNorm backward's partial
// pass AND its coefficient finalize inside the launch (the split-K combine computes the bf16 dA, reads x at the same
// addresses, sums g = relu-mask * dA and g * xhat per (sample, brick, channel); the workgroup completing the last tile
// forms the apply coefficients coef[n][5][cin] and dgamma / dbeta as gn_bwd_parts_finalize does). Then only
// u3d_gn_bwd_apply_coef runs. cin / cout are the FORWARD conv's: dy has cout, dx / x have cin; wpk = the dgrad pack.
// parts: u3d_conv_small_gb_parts_floats floats; cnt: u3d_conv_small_cnt_bytes(n, d, h, w, cin) zeroed bytes.
// *made = 0 (nothing launched; the caller takes the separate passes) where the launch would not split its
// contraction over 2..8 workgroups.
extern "C" long long u3d_conv_small_gb_parts_floats(int n, int d, int h, int w, int cin) {
  return 2LL * n * d * h * w * cin;  // >= n * bricks * cin * 2
}
extern "C" int u3d_conv_small_dgrad_gn(const void* dy, int n, int cout, int d, int h, int w, const void* wpk_dgrad,
                                       int cin, const void* x, const float* gn_stats, const float* gn_gamma,
                                       const float* gn_beta, int gn_groups, void* dx, float* ws, long long ws_bytes,
                                       unsigned* cnt, float* parts, float* coef, float* dgamma, float* dbeta,
                                       int* made, u3d_stream_t stream) {
  U3D_REQUIRE(dy && x && dx && cnt && parts && coef && made && gn_stats && gn_gamma && gn_beta,
              "conv_small_dgrad_gn: bad args");
  *made = 0;
  int nks = 0;
  int rc = conv_small_impl(1, dy, n, cout, d, h, w, wpk_dgrad, cin, nullptr, nullptr, nullptr, 0, nullptr, dx, ws,
                           ws_bytes, cnt, nullptr, nullptr, &nks, stream, nullptr, true);
  if (rc) return rc;
  if (nks < 2 || nks > 8 || (long long)n * cin * 2 > 8192) return 0;
  const SCGb gb{x, gn_stats, gn_gamma, gn_beta, gn_groups, parts, coef, dgamma, dbeta};
  rc = conv_small_impl(1, dy, n, cout, d, h, w, wpk_dgrad, cin, nullptr, nullptr, nullptr, 0, nullptr, dx, ws,
                       ws_bytes, cnt, nullptr, nullptr, &nks, stream, &gb);
  if (rc == 0) *made = 1;
  return rc;
}
