// The lock-free core of the 3-D connected-component labelling (csrc/ccl.hip), written so that it also compiles as
// plain host C++ (tests/native/ccl_core_host.cpp runs it under the host sanitizers, in several orders and from several
// threads, before any kernel runs: a mistake in a lock-free union-find shows as a hang).
//
// parent[] is int32, indexed by the linear (C order) voxel index; background is -1. INVARIANT: parent[i] <= i for
// every foreground voxel, so the root of a tree (parent[r] == r) is its smallest index, and once all unions are made
// the root of a component is the smallest linear index of the component: the result is a pure function of the mask,
// whatever the launch geometry and the order in which the unions arrive.
//  * find   follows parents, which strictly decrease: it terminates.
//  * unite  links the larger root onto the smaller with an atomic min and continues from the value it displaced
//           (the link that the min may have cut). Values only decrease: it terminates. A stale read in find only
//           yields an ancestor that is no longer a root; the atomic min then returns the real parent and the loop
//           goes on from there.
// The tile-local phase runs the same code on a tile's parents in LDS (local linear indices, which order the voxels of
// a tile as the global indices do), the seam phase on the global parents.
#pragma once

#if defined(__HIPCC__)
#define CCL_HD __host__ __device__ __forceinline__
#else
#define CCL_HD inline
#endif

namespace u3d {
namespace ccl {

// one workgroup's tile (x contiguous); the local index is (lz * TY + ly) * TX + lx
constexpr int TX = 64, TY = 8, TZ = 8;
constexpr int TILE = TX * TY * TZ;

enum Scope : int { WORKGROUP = 0, AGENT = 1 };

template <int S>
CCL_HD int load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (S == WORKGROUP)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}

template <int S>
CCL_HD void store(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (S == WORKGROUP)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  __atomic_store_n(p, v, __ATOMIC_RELAXED);
#endif
}

// *p = min(*p, v); returns the value before
template <int S>
CCL_HD int fetch_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (S == WORKGROUP)
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  int old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
  return old;
#endif
}

// the root above foreground voxel i (parents strictly decrease up to the root)
template <int S>
CCL_HD int find(const int* parent, int i) {
  int p;
  while ((p = load<S>(parent + i)) < i && p >= 0) i = p;
  return i;
}

// join the trees of foreground voxels a and b
template <int S>
CCL_HD void unite(int* parent, int a, int b) {
  for (;;) {
    a = find<S>(parent, a);
    b = find<S>(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = fetch_min<S>(parent + a, b);  // a > b
    if (old == a) return;                         // a was a root and now hangs below b
    a = old;                                      // a had a parent already: that tree and b's remain to be joined
  }
}

// tile-local phase, one voxel: local index l = (lz * TY + ly) * TX + lx of a tile whose parents lp[TILE] hold l for
// foreground and -1 for background and for voxels past the volume. Unions with the three predecessors inside the tile.
CCL_HD void local_unite(int* lp, int l, int lx, int ly, int lz) {
  if (load<WORKGROUP>(lp + l) < 0) return;
  if (lx > 0 && load<WORKGROUP>(lp + l - 1) >= 0) unite<WORKGROUP>(lp, l, l - 1);
  if (ly > 0 && load<WORKGROUP>(lp + l - TX) >= 0) unite<WORKGROUP>(lp, l, l - TX);
  if (lz > 0 && load<WORKGROUP>(lp + l - TX * TY) >= 0) unite<WORKGROUP>(lp, l, l - TX * TY);
}

// the global linear index of local index l of the tile whose first voxel is (z0, y0, x0), volume rows Y x X
CCL_HD int local_to_global(int l, int z0, int y0, int x0, int Y, int X) {
  const int lx = l % TX, ly = (l / TX) % TY, lz = l / (TX * TY);
  return ((z0 + lz) * Y + (y0 + ly)) * X + (x0 + lx);
}

// the global parent of local voxel l after the tile-local unions (call after every local_unite of the tile)
CCL_HD int local_result(const int* lp, int l, int z0, int y0, int x0, int Y, int X) {
  if (load<WORKGROUP>(lp + l) < 0) return -1;
  return local_to_global(find<WORKGROUP>(lp, l), z0, y0, x0, Y, X);
}

// seam phase, one voxel v = (z * Y + y) * X + x: unions across the tile's low faces
CCL_HD void seam_unite(int* parent, int v, int z, int y, int x, int Y, int X) {
  if (load<AGENT>(parent + v) < 0) return;
  if (x > 0 && x % TX == 0 && load<AGENT>(parent + v - 1) >= 0) unite<AGENT>(parent, v, v - 1);
  if (y > 0 && y % TY == 0 && load<AGENT>(parent + v - X) >= 0) unite<AGENT>(parent, v, v - X);
  if (z > 0 && z % TZ == 0 && load<AGENT>(parent + v - X * Y) >= 0) unite<AGENT>(parent, v, v - X * Y);
}

// Multi-label forms (u3d_ccl_keep_largest): a voxel carries a code, 0 for a voxel that takes no part (its parent is
// -1), and joins a predecessor only when both hold the same nonzero code. The unions are the ones above, so the
// invariants hold unchanged and a component's root is still its smallest linear index; flatten is shared.
// Tile-local phase, one voxel: lc[TILE] are the codes of the tile next to its parents lp[TILE].
CCL_HD void local_unite_codes(int* lp, const unsigned char* lc, int l, int lx, int ly, int lz) {
  const unsigned char c = lc[l];
  if (c == 0) return;
  if (lx > 0 && lc[l - 1] == c) unite<WORKGROUP>(lp, l, l - 1);
  if (ly > 0 && lc[l - TX] == c) unite<WORKGROUP>(lp, l, l - TX);
  if (lz > 0 && lc[l - TX * TY] == c) unite<WORKGROUP>(lp, l, l - TX * TY);
}

// seam phase, one voxel: codes[] is the volume as given; a voxel takes part when its parent is not -1, and a
// predecessor with the same code then takes part too
CCL_HD void seam_unite_codes(int* parent, const unsigned char* codes, int v, int z, int y, int x, int Y, int X) {
  if (load<AGENT>(parent + v) < 0) return;
  const unsigned char c = codes[v];
  if (x > 0 && x % TX == 0 && codes[v - 1] == c) unite<AGENT>(parent, v, v - 1);
  if (y > 0 && y % TY == 0 && codes[v - X] == c) unite<AGENT>(parent, v, v - X);
  if (z > 0 && z % TZ == 0 && codes[v - X * Y] == c) unite<AGENT>(parent, v, v - X * Y);
}

// flatten, one voxel: parent[v] = its root. Returns 1 when v is a root. Safe next to concurrent flattens: a voxel's
// parent only moves to an ancestor, and roots never change once the unions are complete.
CCL_HD int flatten(int* parent, int v) {
  const int p = load<AGENT>(parent + v);
  if (p < 0) return 0;
  if (p == v) return 1;
  const int r = find<AGENT>(parent, p);
  if (r != p) store<AGENT>(parent + v, r);
  return 0;
}

}  // namespace ccl
}  // namespace u3d
