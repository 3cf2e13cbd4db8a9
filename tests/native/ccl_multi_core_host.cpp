// Stand-alone host exerciser of the multi-label forms in csrc/ccl_core.h (local_unite_codes, seam_unite_codes and the
// shared flatten, the lock-free core of u3d_ccl_keep_largest), built by tests/test_ccl_multi_core_host.py with the
// host address and undefined-behaviour sanitizers as a plain executable.
//
//   ccl_multi_core_host <volumes.bin>
//
// volumes.bin: int32 count, then per volume int32 Z, Y, X, num_labels and Z * Y * X code bytes (written by the test
// from postproc_cases.py). A voxel takes part when its code is in 1..num_labels. Per volume the three phases run as
// the kernels run them (tile-local unions on per-tile parents and codes, seam unions and the flatten on the global
// parents), with the voxels of every phase taken once in C order, once in reverse order (one thread each) and once in
// a seeded shuffled order dealt over 8 threads. Every run must give, for every voxel that takes part, the smallest
// linear index of its component among the voxels of its own code (a serial flood fill per code), and -1 for every
// other voxel. Exit status 0 when all agree.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

#include "ccl_core.h"

using namespace u3d::ccl;

struct Vol {
  int Z, Y, X, num_labels;
  std::vector<uint8_t> c;
  int V() const { return Z * Y * X; }
  uint8_t code(int i) const { return c[i] != 0 && c[i] <= num_labels ? c[i] : 0; }
};

static std::vector<int> flood(const Vol& v) {
  std::vector<int> root(v.V(), -1), stack;
  const int sy = v.X, sz = v.X * v.Y;
  for (int i = 0; i < v.V(); ++i) {
    const uint8_t code = v.code(i);
    if (!code || root[i] >= 0) continue;
    root[i] = i;  // the first voxel met in C order is the smallest index of its component
    stack.push_back(i);
    while (!stack.empty()) {
      const int c = stack.back();
      stack.pop_back();
      const int x = c % v.X, y = (c / v.X) % v.Y, z = c / sz;
      const int nb[6] = {x > 0 ? c - 1 : -1,        x + 1 < v.X ? c + 1 : -1,   y > 0 ? c - sy : -1,
                         y + 1 < v.Y ? c + sy : -1, z > 0 ? c - sz : -1,        z + 1 < v.Z ? c + sz : -1};
      for (int k : nb)
        if (k >= 0 && v.code(k) == code && root[k] < 0) {
          root[k] = i;
          stack.push_back(k);
        }
    }
  }
  return root;
}

enum Order { FORWARD, REVERSE, SHUFFLED };

template <typename F>
static void for_each(int n, Order order, unsigned seed, F f) {
  std::vector<int> idx(n);
  std::iota(idx.begin(), idx.end(), 0);
  if (order == REVERSE) {
    for (int i = 0; i < n / 2; ++i) std::swap(idx[i], idx[n - 1 - i]);
  } else if (order == SHUFFLED) {
    std::mt19937 g(seed);
    for (int i = n - 1; i > 0; --i) std::swap(idx[i], idx[g() % (unsigned)(i + 1)]);
  }
  const int nt = order == SHUFFLED ? 8 : 1;
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (int k = t; k < n; k += nt) f(idx[k]);
    });
  for (auto& t : th) t.join();
}

static std::vector<int> run(const Vol& v, Order order, int* roots) {
  const int ntx = (v.X + TX - 1) / TX, nty = (v.Y + TY - 1) / TY, ntz = (v.Z + TZ - 1) / TZ;
  const int tiles = ntx * nty * ntz;
  std::vector<int> lp((size_t)tiles * TILE), parent(v.V(), -2);
  std::vector<uint8_t> lc((size_t)tiles * TILE);
  // the seam phase reads the volume's codes as given: a voxel that takes no part is known by its parent, -1
  const std::vector<uint8_t> codes(v.c);
  auto origin = [&](int t, int& z0, int& y0, int& x0) {
    x0 = (t % ntx) * TX, y0 = ((t / ntx) % nty) * TY, z0 = (t / (ntx * nty)) * TZ;
  };
  for (int t = 0; t < tiles; ++t) {
    int z0, y0, x0;
    origin(t, z0, y0, x0);
    for (int l = 0; l < TILE; ++l) {
      const int x = x0 + l % TX, y = y0 + (l / TX) % TY, z = z0 + l / (TX * TY);
      const uint8_t c = x < v.X && y < v.Y && z < v.Z ? v.code((z * v.Y + y) * v.X + x) : 0;
      lc[(size_t)t * TILE + l] = c;
      lp[(size_t)t * TILE + l] = c ? l : -1;
    }
  }
  for_each(tiles * TILE, order, 1u, [&](int w) {
    const int l = w % TILE;
    const size_t base = (size_t)(w / TILE) * TILE;
    local_unite_codes(&lp[base], &lc[base], l, l % TX, (l / TX) % TY, l / (TX * TY));
  });
  for_each(tiles * TILE, order, 2u, [&](int w) {
    const int t = w / TILE, l = w % TILE;
    int z0, y0, x0;
    origin(t, z0, y0, x0);
    const int x = x0 + l % TX, y = y0 + (l / TX) % TY, z = z0 + l / (TX * TY);
    if (x < v.X && y < v.Y && z < v.Z)
      parent[(z * v.Y + y) * v.X + x] = local_result(&lp[(size_t)t * TILE], l, z0, y0, x0, v.Y, v.X);
  });
  for_each(v.V(), order, 3u, [&](int i) {
    seam_unite_codes(parent.data(), codes.data(), i, i / (v.X * v.Y), (i / v.X) % v.Y, i % v.X, v.Y, v.X);
  });
  std::vector<int> isroot(v.V(), 0);
  for_each(v.V(), order, 4u, [&](int i) { isroot[i] = flatten(parent.data(), i); });
  *roots = std::accumulate(isroot.begin(), isroot.end(), 0);
  return parent;
}

int main(int argc, char** argv) {
  if (argc != 2) return std::fprintf(stderr, "usage: %s volumes.bin\n", argv[0]), 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  int bad = 0;
  for (int c = 0; c < count; ++c) {
    int32_t d[4];
    if (std::fread(d, 4, 4, f) != 4) return 2;
    Vol v{d[0], d[1], d[2], d[3], {}};
    v.c.resize((size_t)v.V());
    if (std::fread(v.c.data(), 1, v.c.size(), f) != v.c.size()) return 2;
    const std::vector<int> want = flood(v);
    int nroots = 0;
    for (int i = 0; i < v.V(); ++i) nroots += want[i] == i;
    for (Order o : {FORWARD, REVERSE, SHUFFLED}) {
      int roots = -1;
      const std::vector<int> got = run(v, o, &roots);
      int diff = 0;
      for (int i = 0; i < v.V(); ++i) diff += got[i] != want[i];
      if (diff || roots != nroots) {
        std::printf("volume %d (%d x %d x %d, %d labels) order %d: %d voxels differ, %d roots (want %d)\n", c, v.Z, v.Y,
                    v.X, v.num_labels, (int)o, diff, roots, nroots);
        ++bad;
      }
    }
    std::printf("volume %d (%d x %d x %d, %d labels): %d components\n", c, v.Z, v.Y, v.X, v.num_labels, nroots);
  }
  std::fclose(f);
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
