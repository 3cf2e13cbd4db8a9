// Stand-alone host exerciser of rs::argmax_trilinear (csrc/resample_core.h, the per-voxel routine of
// u3d_grid_resample_argmax), built by tests/test_resample_argmax_core_host.py with the host address and
// undefined-behaviour sanitizers as a plain executable.
//
//   resample_argmax_core_host <cases.bin>
//
// cases.bin: int32 count, then per case
//   int32 C, src_n[3], n_out[3] (per output axis); int64 stride[3] (elements, per output axis), chan_stride, elems;
//   per output axis a: int32 i0[n_out[a]], float64 frac[n_out[a]];  the source's elems float32 elements
// (written by the test from resample_cases.py and u3d.data's plans). The source is held in a buffer of exactly elems
// elements, so an offset outside it is a sanitizer report. For every output voxel argmax_trilinear, called with
// pair_offsets as the kernel calls it, must equal a direct evaluation written here from the contract: per channel the
// taps (i0, min(i0 + 1, n - 1)), a + f (b - a) in fp64 along axis 2, then 1, then 0, rounded to fp32; then the first
// NaN if there is one, otherwise the first channel holding the maximum (torch.argmax's rule). Exit status 0 when all
// agree; per case the program also prints how many voxels were decided by a tie and by a NaN.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "resample_core.h"

using namespace u3d::rs;

struct Case {
  int32_t C, src_n[3], n_out[3];
  int64_t stride[3], chan_stride, elems;
  std::vector<int32_t> i0[3];
  std::vector<double> frac[3];
  std::vector<float> src;
};

template <typename T>
static bool rd(std::FILE* f, T* p, size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}

static bool read_case(std::FILE* f, Case& c) {
  if (!rd(f, &c.C, 1) || !rd(f, c.src_n, 3) || !rd(f, c.n_out, 3) || !rd(f, c.stride, 3) || !rd(f, &c.chan_stride, 1) ||
      !rd(f, &c.elems, 1))
    return false;
  for (int a = 0; a < 3; ++a) {
    const size_t n = (size_t)c.n_out[a];
    c.i0[a].resize(n), c.frac[a].resize(n);
    if (!rd(f, c.i0[a].data(), n) || !rd(f, c.frac[a].data(), n)) return false;
  }
  c.src.resize((size_t)c.elems);  // exactly elems elements: the allocation's end is the source's end
  return rd(f, c.src.data(), c.src.size());
}

static float direct_value(const Case& c, int ch, const int* k) {
  long long off[3][2];
  double f[3];
  for (int a = 0; a < 3; ++a) {
    const int lo = c.i0[a][k[a]], hi = lo + 1 < c.src_n[a] ? lo + 1 : c.src_n[a] - 1;
    off[a][0] = lo * (long long)c.stride[a], off[a][1] = hi * (long long)c.stride[a];
    f[a] = c.frac[a][k[a]];
  }
  double plane[2];
  for (int i = 0; i < 2; ++i) {
    double line[2];
    for (int j = 0; j < 2; ++j) {
      const double a = (double)c.src.at((size_t)(ch * c.chan_stride + off[0][i] + off[1][j] + off[2][0]));
      const double b = (double)c.src.at((size_t)(ch * c.chan_stride + off[0][i] + off[1][j] + off[2][1]));
      line[j] = a + f[2] * (b - a);
    }
    plane[i] = line[0] + f[1] * (line[1] - line[0]);
  }
  return (float)(plane[0] + f[0] * (plane[1] - plane[0]));
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
    long long bad = 0, ties = 0, nans = 0;
    std::vector<float> v((size_t)c.C);
    int k[3];
    for (k[0] = 0; k[0] < c.n_out[0]; ++k[0])
      for (k[1] = 0; k[1] < c.n_out[1]; ++k[1])
        for (k[2] = 0; k[2] < c.n_out[2]; ++k[2]) {
          const int got = argmax_trilinear(c.src.data(), c.C, c.chan_stride,
                                           pair_offsets(c.i0[0][k[0]], c.src_n[0], c.stride[0]),
                                           pair_offsets(c.i0[1][k[1]], c.src_n[1], c.stride[1]),
                                           pair_offsets(c.i0[2][k[2]], c.src_n[2], c.stride[2]), c.frac[0][k[0]],
                                           c.frac[1][k[1]], c.frac[2][k[2]]);
          int want = -1;
          for (int ch = 0; ch < c.C; ++ch) {
            v[ch] = direct_value(c, ch, k);
            if (want < 0 && std::isnan(v[ch])) want = ch;
          }
          if (want >= 0) {
            ++nans;
          } else {
            float m = v[0];
            for (int ch = 1; ch < c.C; ++ch) m = v[ch] > m ? v[ch] : m;
            int holders = 0;
            for (int ch = c.C - 1; ch >= 0; --ch)
              if (v[ch] == m) want = ch, ++holders;
            ties += holders > 1;
          }
          bad += got != want;
        }
    if (bad) ++failed;
    std::printf("case %d (C %d, %d x %d x %d): %lld voxels differ, %lld ties, %lld nans\n", i, c.C, c.n_out[0],
                c.n_out[1], c.n_out[2], bad, ties, nans);
  }
  std::fclose(f);
  std::printf("%s\n", failed ? "FAILED" : "ok");
  return failed ? 1 : 0;
}
