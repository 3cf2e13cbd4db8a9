// Stand-alone host exerciser of csrc/resample_core.h (the per-voxel routines of csrc/resample.hip), built by
// tests/test_resample_core_host.py with the host address and undefined-behaviour sanitizers as a plain executable.
//
//   resample_core_host <cases.bin>
//
// cases.bin: int32 count, then per case
//   int32 dtype (0 uint8, 1 int16, 2 int32, 3 float32), C, hostile; int32 src_n[3], n_out[3] (per output axis);
//   int64 stride[3] (elements, per output axis), chan_stride, elems (of the whole source);
//   per output axis a: int32 i0[n_out[a]], float64 frac[n_out[a]], int32 near[n_out[a]];  the source's elems elements
// (written by the test from resample_cases.py and u3d.data's plans). The source is held in a buffer of exactly elems
// elements, so an offset outside it is a sanitizer report. Per case every output voxel of every channel goes through
// pair_offsets / trilinear (int16 and float32 sources) and nearest_offset (all), as the kernels call them, and is
// compared with a direct evaluation: the eight-term weighted sum of the taps (i0, min(i0 + 1, n - 1)) with weights
// (1 - frac, frac) in fp64, bound 64 eps sum |w v|; the nearest tap exactly. A hostile case carries table entries
// outside [0, n - 1]: it is only run, the clamp must keep every access inside the buffer. Exit status 0 when all agree.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "resample_core.h"

using namespace u3d::rs;

struct Case {
  int32_t dtype, C, hostile, src_n[3], n_out[3];
  int64_t stride[3], chan_stride, elems;
  std::vector<int32_t> i0[3], near[3];
  std::vector<double> frac[3];
  std::vector<unsigned char> bytes;
};

template <typename T>
static bool rd(std::FILE* f, T* p, size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}

static bool read_case(std::FILE* f, Case& c) {
  int32_t h[3];
  if (!rd(f, h, 3) || !rd(f, c.src_n, 3) || !rd(f, c.n_out, 3) || !rd(f, c.stride, 3) || !rd(f, &c.chan_stride, 1) ||
      !rd(f, &c.elems, 1))
    return false;
  c.dtype = h[0], c.C = h[1], c.hostile = h[2];
  for (int a = 0; a < 3; ++a) {
    const size_t n = (size_t)c.n_out[a];
    c.i0[a].resize(n), c.frac[a].resize(n), c.near[a].resize(n);
    if (!rd(f, c.i0[a].data(), n) || !rd(f, c.frac[a].data(), n) || !rd(f, c.near[a].data(), n)) return false;
  }
  const size_t es = c.dtype == DT_U8 ? 1 : c.dtype == DT_I16 ? 2 : 4;
  c.bytes.resize((size_t)c.elems * es);
  return rd(f, c.bytes.data(), c.bytes.size());
}

// the taps and weights of one axis, straight from the contract
struct Direct {
  long long off[2];
  double w[2];
};
static Direct direct_axis(const Case& c, int a, int k) {
  const int lo = c.i0[a][k], hi = lo + 1 < c.src_n[a] ? lo + 1 : c.src_n[a] - 1;
  return Direct{{lo * (long long)c.stride[a], hi * (long long)c.stride[a]}, {1.0 - c.frac[a][k], c.frac[a][k]}};
}

template <typename T>
static long long run_case(const Case& c, bool linear) {
  // a copy of exactly elems elements: the allocation's end is the source's end
  std::vector<T> src((const T*)c.bytes.data(), (const T*)c.bytes.data() + c.elems);
  long long bad = 0;
  volatile double sink = 0;
  for (int ch = 0; ch < c.C; ++ch) {
    const T* base = src.data() + ch * c.chan_stride;
    for (int k0 = 0; k0 < c.n_out[0]; ++k0)
      for (int k1 = 0; k1 < c.n_out[1]; ++k1)
        for (int k2 = 0; k2 < c.n_out[2]; ++k2) {
          const long long o = nearest_offset(c.near[0][k0], c.src_n[0], c.stride[0]) +
                              nearest_offset(c.near[1][k1], c.src_n[1], c.stride[1]) +
                              nearest_offset(c.near[2][k2], c.src_n[2], c.stride[2]);
          const T got_near = base[o];
          double got = 0;
          if (linear)
            got = trilinear(base, pair_offsets(c.i0[0][k0], c.src_n[0], c.stride[0]),
                            pair_offsets(c.i0[1][k1], c.src_n[1], c.stride[1]),
                            pair_offsets(c.i0[2][k2], c.src_n[2], c.stride[2]), c.frac[0][k0], c.frac[1][k1],
                            c.frac[2][k2]);
          if (c.hostile) {
            sink = sink + got + (double)got_near;
            continue;
          }
          const long long want_o = c.near[0][k0] * (long long)c.stride[0] + c.near[1][k1] * (long long)c.stride[1] +
                                   c.near[2][k2] * (long long)c.stride[2];
          bad += got_near != src.at((size_t)(ch * c.chan_stride + want_o));
          if (!linear) continue;
          const Direct d0 = direct_axis(c, 0, k0), d1 = direct_axis(c, 1, k1), d2 = direct_axis(c, 2, k2);
          double want = 0, mag = 0;
          for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j)
              for (int l = 0; l < 2; ++l) {
                const double v = (double)src.at((size_t)(ch * c.chan_stride + d0.off[i] + d1.off[j] + d2.off[l]));
                const double w = d0.w[i] * d1.w[j] * d2.w[l];
                want += w * v;
                mag += std::fabs(w * v);
              }
          bad += !(std::fabs(got - want) <= 64 * std::numeric_limits<double>::epsilon() * mag);
        }
  }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 2) return std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]), 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int32_t count = 0;
  if (!rd(f, &count, 1)) return 2;
  int failed = 0;
  for (int i = 0; i < count; ++i) {
    Case c;
    if (!read_case(f, c)) return std::fprintf(stderr, "case %d: short file\n", i), 2;
    long long bad = 0;
    switch (c.dtype) {
      case DT_U8: bad = run_case<uint8_t>(c, false); break;
      case DT_I16: bad = run_case<int16_t>(c, true); break;
      case DT_I32: bad = run_case<int32_t>(c, false); break;
      case DT_F32: bad = run_case<float>(c, true); break;
      default: return std::fprintf(stderr, "case %d: dtype %d\n", i, c.dtype), 2;
    }
    if (bad) ++failed;
    std::printf("case %d (dtype %d, C %d, %d x %d x %d%s): %lld voxels differ\n", i, c.dtype, c.C, c.n_out[0],
                c.n_out[1], c.n_out[2], c.hostile ? ", hostile" : "", bad);
  }
  std::fclose(f);
  std::printf("%s\n", failed ? "FAILED" : "ok");
  return failed ? 1 : 0;
}
