// Backward of a stride-1 3^3 conv behind GroupNorm + ReLU at the 12^3 / 6^3 levels: data gradient and weight gradient
// in ONE launch (horizontal fusion: two independent sub-grids, no barrier and no spin between them).
//
// Both gradients read the same dy and neither needs the other's result. As two launches they run one after the other,
// and the data gradient (conv_small_body.h, flip, with the GroupNorm-backward partials and the coefficient finalize)
// ends in a serial tail of hand-offs (slab drain, tile counter, combine, statistics counter, the last workgroup's
// finalize) during which almost every CU is idle; at 6^3 its 128 workgroups leave half the CUs idle throughout. Here
//   blocks [0, nA)           run the data-gradient body (first: it carries the serial tail),
//   blocks [nA, nApad)       exit at once (nApad = nA rounded up to 8: blocks b and b + 8 of a launch share an XCD,
//                            so the second sub-grid keeps the XCD grouping its tile mapping assumes),
//   blocks [nApad, nApad+nB) run the weight-gradient body: the 12 x 12-tile ring (wgrad_ring_body.h) or the
//                            3 x 8 x 16 brick (wgrad_brick_body.h),
// and the dispatcher hands weight-gradient workgroups to the CUs the data gradient has left. The bodies are the ones
// the separate kernels run, with the same geometry, split counts and slab layout: every output is bitwise what
// u3d_conv_small_dgrad_gn + u3d_conv_wgrad_ring / u3d_conv_wgrad_brick write. A workgroup runs one body to its end and
// exits; the data gradient's last-arriver hand-offs count its own nA workgroups only.
// Reference: autograd of NoBottleneck's relu(gn(x)) -> conv3x3x3 (unet3D.py:44-73) and of F.conv3d (unet3D.py:27).
#include "conv_small_body.h"
#include "wgrad_brick_body.h"
#include "wgrad_ring_body.h"

namespace u3d {
namespace {

constexpr int cmax(int a, int b) { return a > b ? a : b; }
constexpr int PAIR_RING_LDS = wr_lds_bytes<true, 12, 12>();
constexpr int PAIR_BRICK_LDS = wb_lds_bytes<3, 8, 16, 1, 1>();
static_assert(cmax(SC_SMEM, cmax(PAIR_RING_LDS, PAIR_BRICK_LDS)) + 1024 <= 160 * 1024, "LDS");
static_assert(SC_NT == 512 && WR_NT == 512, "one workgroup shape for both bodies");

// weight-gradient half: the ring's or the brick's geometry
struct PairRing {
  static constexpr int LDS = PAIR_RING_LDS;
  typedef WRGeom Geom;
  static __device__ __forceinline__ void run(char* lds, int wg, int nwg, const bf16* dy, const bf16* x,
                                             const float* gstat, const float* gamma, const float* beta, float* part,
                                             const Geom& g) {
    wgrad_ring_body<true, 12, 12>(lds, wg, nwg, g.cin_p / 32, g.cout_p / 32, dy, x, gstat, gamma, beta, part, g, nullptr);
  }
};
struct PairBrick {
  static constexpr int LDS = PAIR_BRICK_LDS;
  typedef WBGeom Geom;
  static __device__ __forceinline__ void run(char* lds, int wg, int nwg, const bf16* dy, const bf16* x,
                                             const float* gstat, const float* gamma, const float* beta, float* part,
                                             const Geom& g) {
    wgrad_brick_body<3, 8, 16, 1, 1, true>(lds, wg, nwg, g.cin_p / 32, g.cout_p / 32, dy, x, gstat, gamma, beta, part, g);
  }
};

}  // namespace

// dy: the output gradient (both halves' operand); wpk: the data-gradient pack; dx: the data gradient (ga.gb*: the
// GroupNorm backward on x); x, gstat / gamma / beta: the weight gradient's operand and its GroupNorm + ReLU prologue
template <typename W>
__global__ __launch_bounds__(512, 1) void small_bwd_pair_kernel(const bf16* __restrict__ dy,
                                                               const bf16* __restrict__ wpk, bf16* __restrict__ dx,
                                                               SCGeom ga, int nA, int nApad,
                                                               const bf16* __restrict__ x,
                                                               const float* __restrict__ gstat,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta,
                                                               float* __restrict__ part, typename W::Geom gb, int nB) {
  __shared__ __attribute__((aligned(16))) char smem[cmax(SC_SMEM, W::LDS)];
  const int b = (int)blockIdx.x;
  if (b < nA) {
    conv_small_body<true>(smem, b, nA, dy, wpk, dx, nullptr, nullptr, nullptr, nullptr, ga, nullptr, nullptr);
    return;
  }
  if (b < nApad) return;
  W::run(smem, b - nApad, nB, dy, x, gstat, gamma, beta, part, gb);
}

}  // namespace u3d

using namespace u3d;

namespace {
struct PairPlan {
  SCGeom ga;
  long long nA;
  bool ring;
  WRGeom gr;
  WBGeom gk;
  int nsplit;
  long long nB;
};
}  // namespace

// The plan of both halves, or false where either would not take the path the separate launches take (see u3d.h).
// cin / cout are the FORWARD conv's: dy has cout channels, x and dx have cin.
static bool pair_plan(int n, int cout, int d, int h, int w, int cin, int ring, float* ws, long long ws_bytes,
                      PairPlan& p) {
  if (n < 1 || d < 1 || h < 1 || w < 1 || cin < 8 || cout < 8 || cin % 8 || cout % 8) return false;
  // ---- the data gradient: u3d_conv_small_dgrad_gn's conditions (contraction = cout, output = cin)
  const long long tiles = sc_plan(n, cout, d, h, w, cin, 0, ws, ws_bytes, p.ga);
  if (p.ga.nks < 2 || p.ga.nks > 8 || (long long)n * cin * 2 > 8192) return false;
  p.nA = tiles * p.ga.nks;
  const long long vox = (long long)n * d * h * w;
  const int cin_p = round_up(cin, 32), cout_p = round_up(cout, 32);
  if (!fits_buffer_offsets(vox * std::max(cin, cout) * 2) || !fits_buffer_offsets(27LL * cout_p * cin_p * 2) ||
      !fits_buffer_offsets(p.ga.nks * vox * cin * 4))
    return false;  // 32-bit buffer offsets: operands, weight pack, split-K slabs
  // ---- the weight gradient: the kernel u3d_conv_wgrad_ring / u3d_conv_wgrad_brick would launch
  p.ring = ring != 0;
  long long wtiles;
  if (p.ring) {
    wr_geom(n, cin, d, h, w, cout, p.gr);
    if (p.gr.ph != 12 || p.gr.pw != 12) return false;  // the 12 x 24 tile or the 16 x 16 DMA ring
    p.nsplit = u3d_conv_wgrad_ring_splits(n, cin, d, h, w, cout);
    p.gr.per = (int)((p.gr.planes + p.nsplit - 1) / p.nsplit);
    if ((p.gr.planes + p.gr.per - 1) / p.gr.per != p.nsplit) return false;  // (a zero-filled trailing slab)
    wtiles = (long long)(p.gr.cin_p / 32) * (p.gr.cout_p / 32);
  } else {
    if (opt(OPT_WGRAD_BD) == 2) return false;  // the 2 x 8 x 16 brick
    p.nsplit = u3d_conv_wgrad_brick_splits(n, cin, d, h, w, cout, 1);
    wb_geom(n, cin, d, h, w, cout, 1, 3, 8, 16, p.nsplit, 0, p.gk);
    if ((p.gk.nbricks + p.gk.per_split - 1) / p.gk.per_split != p.nsplit) return false;
    wtiles = (long long)(p.gk.cin_p / 32) * (p.gk.cout_p / 32);
  }
  if ((long long)p.nsplit * 27 * cout_p * cin_p * 4 >= (1LL << 31)) return false;  // partial slabs
  p.nB = wtiles * p.nsplit;
  return p.nA + 8 + p.nB < (1LL << 31);
}

// The weight gradient's split count (> 0) where u3d_conv_small_bwd_pair would launch, else 0. ring: the caller routes
// this conv's weight gradient to u3d_conv_wgrad_ring (else to u3d_conv_wgrad_brick).
extern "C" int u3d_conv_small_bwd_pair_ok(int n, int cout, int d, int h, int w, int cin, int ring,
                                          long long ws_bytes) {
  PairPlan p;
  float dummy;  // (the plan only asks whether a workspace exists)
  return pair_plan(n, cout, d, h, w, cin, ring, ws_bytes > 0 ? &dummy : nullptr, ws_bytes, p) ? p.nsplit : 0;
}

extern "C" int u3d_conv_small_bwd_pair(const void* dy, int n, int cout, int d, int h, int w, const void* wpk_dgrad,
                                       int cin, const void* x, const float* gn_stats, const float* gn_gamma,
                                       const float* gn_beta, int gn_groups, void* dx, float* ws, long long ws_bytes,
                                       unsigned* cnt, float* parts, float* coef, float* dgamma, float* dbeta,
                                       int ring, float* partials, int nsplit, int* made, u3d_stream_t stream) {
  U3D_REQUIRE(dy && wpk_dgrad && x && dx && cnt && parts && coef && made && gn_stats && gn_gamma && gn_beta &&
                  partials,
              "conv_small_bwd_pair: bad args");
  *made = 0;
  PairPlan p;
  if (!pair_plan(n, cout, d, h, w, cin, ring, ws, ws_bytes, p)) return 0;
  U3D_REQUIRE(gn_groups > 0 && cin % gn_groups == 0, "conv_small_bwd_pair: bad GroupNorm args");
  U3D_REQUIRE(nsplit == p.nsplit, "conv_small_bwd_pair: nsplit %d, the weight gradient splits %d ways", nsplit,
              p.nsplit);
  SCGeom& g = p.ga;  // as conv_small_impl sets it for u3d_conv_small_dgrad_gn
  g.cnt = cnt;
  g.gbx = (const bf16*)x;
  g.gbstat = gn_stats; g.gbgamma = gn_gamma; g.gbbeta = gn_beta; g.gbgroups = gn_groups;
  g.gbparts = parts; g.coef = coef; g.dgamma = dgamma; g.dbeta = dbeta;
  const int nA = (int)p.nA, nApad = round_up(nA, 8), nB = (int)p.nB;
  const dim3 grid((unsigned)(nApad + nB));
  hipStream_t s = (hipStream_t)stream;
  if (p.ring) {
    p.gr.gn_groups = gn_groups;
    hipLaunchKernelGGL(small_bwd_pair_kernel<PairRing>, grid, dim3(512), 0, s, (const bf16*)dy,
                       (const bf16*)wpk_dgrad, (bf16*)dx, g, nA, nApad, (const bf16*)x, gn_stats, gn_gamma, gn_beta,
                       partials, p.gr, nB);
  } else {
    p.gk.gn_groups = gn_groups;
    hipLaunchKernelGGL(small_bwd_pair_kernel<PairBrick>, grid, dim3(512), 0, s, (const bf16*)dy,
                       (const bf16*)wpk_dgrad, (bf16*)dx, g, nA, nApad, (const bf16*)x, gn_stats, gn_gamma, gn_beta,
                       partials, p.gk, nB);
  }
  const int rc = check_launch("small_bwd_pair_kernel");
  if (rc == 0) *made = 1;
  return rc;
}
