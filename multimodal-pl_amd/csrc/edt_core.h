// The per-line routines of the exact Euclidean distance transform (csrc/edt.hip), written so that they also compile as
// plain host C++ (tests/native/edt_core_host.cpp runs the three passes serially under the host sanitizers and compares
// every voxel with a brute force before any kernel runs).
//
// The transform is separable. With w = spacing^2 per axis and squared distances carried in fp64:
//  * pass 1 (x rows)   D(x) = wx dx^2, dx the distance in voxels to the nearest feature of the row (row_value, from the
//                      row's feature bits, 64 voxels per word); +inf for a row without a feature.
//  * passes 2, 3       D'(j) = min_i D(i) + w (j - i)^2 along y, then z (line_min: a search outward from j that stops
//                      once w k^2 reaches the best value so far; every candidate farther out is at least w k^2 because
//                      D >= 0, so the result is the exact minimum over the whole line).
// Every candidate is one fp64 product and one fp64 sum; with integer spacings both are exact (V < 2^31 bounds the
// sums far below 2^53). A minimum does not depend on the order of its operands: the result is a pure function of the
// mask and the spacing.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EDT_HD __host__ __device__ __forceinline__
#else
#define EDT_HD inline
#endif

namespace u3d {
namespace edt {

constexpr int MAX_EXTENT = 2048;            // per axis: the row bits of pass 1 and a two-column tile of passes 2, 3
constexpr int ROW_WORDS = MAX_EXTENT / 64;  // feature words of one row
constexpr int MAX_COLS = 64;                // adjacent lines one workgroup solves together (at most)
constexpr int TILE_BYTES = 32768;           // LDS of one workgroup's tile of lines: cols * n * 8 <= TILE_BYTES

// adjacent lines of length n solved together: the largest power of two <= MAX_COLS whose tile fits TILE_BYTES
EDT_HD int tile_cols(int n) {
  int c = MAX_COLS;
  while (c > 1 && (long long)c * n * 8 > TILE_BYTES) c >>= 1;
  return c;
}

EDT_HD double infinity() { return __builtin_huge_val(); }

// pass 1, voxel x of a row whose feature bits are words[0 .. nwords) (bit b of word k = voxel 64 k + b; bits past the
// row are 0): w dx^2 for the nearest feature at distance dx, +inf when the row has none
EDT_HD double row_value(const unsigned long long* words, int nwords, int x, double w) {
  const int wi = x >> 6, b = x & 63;
  int d = -1;
  unsigned long long m = words[wi] & (~0ull >> (63 - b));  // voxels <= x of its word
  int k = wi;
  while (m == 0 && k > 0) m = words[--k];
  if (m != 0) d = x - (k * 64 + 63 - __builtin_clzll(m));
  m = words[wi] & (~0ull << b);                             // voxels >= x of its word
  k = wi;
  while (m == 0 && k + 1 < nwords) m = words[++k];
  if (m != 0) {
    const int r = k * 64 + __builtin_ctzll(m) - x;
    if (d < 0 || r < d) d = r;
  }
  if (d < 0) return infinity();
  return w * ((double)d * (double)d);
}

// passes 2 and 3, element j of a line of n values line[i * stride]: min_i line[i * stride] + w (j - i)^2
EDT_HD double line_min(const double* line, int stride, int n, int j, double w) {
  double best = line[j * stride];
  const int kmax = j > n - 1 - j ? j : n - 1 - j;
  for (int k = 1; k <= kmax; ++k) {
    const double p = w * ((double)k * (double)k);
    if (p >= best) break;
    if (j - k >= 0) {
      const double a = line[(j - k) * stride] + p;
      if (a < best) best = a;
    }
    if (j + k < n) {
      const double a = line[(j + k) * stride] + p;
      if (a < best) best = a;
    }
  }
  return best;
}

// the fp32 output of a squared distance: itself, or its correctly rounded fp64 root, rounded once to fp32
EDT_HD float finish(double d2, int squared) { return (float)(squared ? d2 : sqrt(d2)); }

}  // namespace edt
}  // namespace u3d
