// Stand-alone host exerciser of csrc/edt_core.h (the per-line routines of csrc/edt.hip), built by
// tests/test_edt_core_host.py with the host address and undefined-behaviour sanitizers as a plain executable.
//
//   edt_core_host <volumes.bin>
//
// volumes.bin: int32 count, then per volume int32 Z, Y, X, three float64 spacings (sz, sy, sx) and Z * Y * X mask bytes
// (written by the test from surface_cases.py). Per volume the three passes run serially as the kernels run them: the
// row pass from the row's feature words, the y and z passes on tiles of tile_cols(n) adjacent lines copied to a
// scratch tile (the kernels' LDS image, +inf in the columns past the volume), the y pass in place. Every voxel is
// compared with a brute force over all features, sum of w d^2 in the kernel's order of the axes; with integer spacings
// both are exact and must be equal, otherwise they agree to 4 fp64 ulps. A volume without a feature is +inf everywhere.
// Then lines of length 1, 2 and MAX_EXTENT through row_value and line_min. Exit status 0 when all agree.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "edt_core.h"

using namespace u3d::edt;

struct Vol {
  int Z, Y, X;
  double s[3];
  std::vector<uint8_t> m;
  size_t V() const { return (size_t)Z * Y * X; }
};

static void axis_pass(std::vector<double>& D, long long outer, int n, long long inner, double w) {
  const int cols = tile_cols(n);
  std::vector<double> tile((size_t)cols * n), res((size_t)cols * n);
  for (long long o = 0; o < outer; ++o)
    for (long long c0 = 0; c0 < inner; c0 += cols) {
      const int live = inner - c0 < cols ? (int)(inner - c0) : cols;
      for (int i = 0; i < n; ++i)
        for (int c = 0; c < cols; ++c)
          tile[(size_t)i * cols + c] = c < live ? D[(size_t)((o * n + i) * inner + c0 + c)] : infinity();
      for (int j = 0; j < n; ++j)
        for (int c = 0; c < live; ++c) res[(size_t)j * cols + c] = line_min(tile.data() + c, cols, n, j, w);
      for (int j = 0; j < n; ++j)
        for (int c = 0; c < live; ++c) D[(size_t)((o * n + j) * inner + c0 + c)] = res[(size_t)j * cols + c];
    }
}

static std::vector<double> transform(const Vol& v) {
  std::vector<double> D(v.V());
  const int nw = (v.X + 63) / 64;
  std::vector<unsigned long long> words(nw);
  for (long long r = 0; r < (long long)v.Z * v.Y; ++r) {
    for (int k = 0; k < nw; ++k) words[k] = 0;
    for (int x = 0; x < v.X; ++x)
      if (v.m[(size_t)r * v.X + x]) words[x >> 6] |= 1ull << (x & 63);
    for (int x = 0; x < v.X; ++x) D[(size_t)r * v.X + x] = row_value(words.data(), nw, x, v.s[2] * v.s[2]);
  }
  axis_pass(D, v.Z, v.Y, v.X, v.s[1] * v.s[1]);
  axis_pass(D, 1, v.Z, (long long)v.Y * v.X, v.s[0] * v.s[0]);
  return D;
}

static std::vector<double> brute(const Vol& v) {
  std::vector<int> fz, fy, fx;
  for (int z = 0; z < v.Z; ++z)
    for (int y = 0; y < v.Y; ++y)
      for (int x = 0; x < v.X; ++x)
        if (v.m[((size_t)z * v.Y + y) * v.X + x]) fz.push_back(z), fy.push_back(y), fx.push_back(x);
  std::vector<double> D(v.V(), infinity());
  const double wz = v.s[0] * v.s[0], wy = v.s[1] * v.s[1], wx = v.s[2] * v.s[2];
  for (int z = 0; z < v.Z; ++z)
    for (int y = 0; y < v.Y; ++y)
      for (int x = 0; x < v.X; ++x) {
        double best = infinity();
        for (size_t k = 0; k < fz.size(); ++k) {
          const double dz = z - fz[k], dy = y - fy[k], dx = x - fx[k];
          const double d = wx * (dx * dx) + wy * (dy * dy) + wz * (dz * dz);
          if (d < best) best = d;
        }
        D[((size_t)z * v.Y + y) * v.X + x] = best;
      }
  return D;
}

static bool integral(const Vol& v) {
  for (double s : v.s)
    if (s != std::floor(s)) return false;
  return true;
}

static bool close(double got, double want, bool exact) {
  if (got == want) return true;  // +inf included
  if (exact || !std::isfinite(got) || !std::isfinite(want)) return false;
  return std::fabs(got - want) <= 4 * std::numeric_limits<double>::epsilon() * std::fabs(want);
}

// one feature at index f of a line of n: both routines against (j - f)^2 w
static int line_case(int n, int f, double w) {
  int bad = 0;
  const int nw = (n + 63) / 64;
  std::vector<unsigned long long> words(nw, 0);
  std::vector<double> line(n, infinity());
  if (f >= 0) {
    words[f >> 6] |= 1ull << (f & 63);
    line[f] = 0;
  }
  for (int j = 0; j < n; ++j) {
    const double want = f < 0 ? infinity() : w * ((double)(j - f) * (j - f));
    bad += row_value(words.data(), nw, j, w) != want;
    bad += line_min(line.data(), 1, n, j, w) != want;
  }
  if (bad) std::printf("line n=%d feature=%d w=%g: %d values differ\n", n, f, w, bad);
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 2) return std::fprintf(stderr, "usage: %s volumes.bin\n", argv[0]), 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  int bad = 0;
  for (int c = 0; c < count; ++c) {
    int32_t d[3];
    Vol v{};
    if (std::fread(d, 4, 3, f) != 3 || std::fread(v.s, 8, 3, f) != 3) return 2;
    v.Z = d[0], v.Y = d[1], v.X = d[2];
    v.m.resize(v.V());
    if (std::fread(v.m.data(), 1, v.m.size(), f) != v.m.size()) return 2;
    const std::vector<double> got = transform(v), want = brute(v);
    const bool exact = integral(v);
    int diff = 0;
    for (size_t i = 0; i < v.V(); ++i) diff += !close(got[i], want[i], exact);
    if (diff) {
      std::printf("volume %d (%d x %d x %d, spacing %g %g %g): %d voxels differ\n", c, v.Z, v.Y, v.X, v.s[0], v.s[1],
                  v.s[2], diff);
      ++bad;
    }
    std::printf("volume %d (%d x %d x %d): %s\n", c, v.Z, v.Y, v.X, exact ? "exact" : "4 ulp");
  }
  std::fclose(f);
  for (int n : {1, 2, MAX_EXTENT})
    for (int fpos : {-1, 0, n - 1, n / 2})
      for (double w : {1.0, 9.0, 0.49}) bad += line_case(n, fpos, w) != 0;
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
