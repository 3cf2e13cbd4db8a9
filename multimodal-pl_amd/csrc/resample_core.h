// The per-voxel routines of the separable grid resampling (csrc/resample.hip), written so that they also compile as
// plain host C++ (tests/native/resample_core_host.cpp runs every voxel of the test cases serially under the host
// sanitizers and compares it with a direct evaluation before any kernel runs).
//
// An output voxel (k0, k1, k2) reads the source through one table entry per output axis (u3d.data.GridPlan forms the
// tables in float64 on the host; orientation, i.e. the permutation and the flips, is already inside them and inside
// the strides):
//  * linear   i0[k] = the lower source index of the axis' pair, frac[k] = the weight of the upper one. The pair is
//             (i0, min(i0 + 1, n - 1)): the tables keep i0 <= max(n - 2, 0), so the bound only acts on an axis of
//             length 1, which reads index 0 twice. Interpolation runs along axis 2, then 1, then 0 in fp64,
//             lerp(a, b, f) = a + f (b - a); the caller rounds once, at the store.
//  * nearest  near[k] = the source index.
// Every index is clamped to [0, n - 1] before it becomes an offset: a table that breaks its contract gives wrong
// values, never an access outside the source. Offsets are 64-bit.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif

namespace u3d {
namespace rs {

// element types of a source (U3D_RS_* of include/u3d.h)
constexpr int DT_U8 = 0, DT_I16 = 1, DT_I32 = 2, DT_F32 = 3;

RS_HD int clamp_index(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// element offsets of the two taps of one axis
struct Pair {
  long long lo, hi;
};

RS_HD Pair pair_offsets(int i0, int n, long long stride) {
  const int a = clamp_index(i0, n);
  const int b = a + 1 < n ? a + 1 : n - 1;
  return Pair{a * stride, b * stride};
}

RS_HD long long nearest_offset(int i, int n, long long stride) { return clamp_index(i, n) * stride; }

RS_HD double lerp(double a, double b, double f) { return a + f * (b - a); }

// the trilinear value at the taps (p0, p1, p2) with upper-tap weights (f0, f1, f2), fp64
template <typename T>
RS_HD double trilinear(const T* src, Pair p0, Pair p1, Pair p2, double f0, double f1, double f2) {
  const long long r00 = p0.lo + p1.lo, r01 = p0.lo + p1.hi, r10 = p0.hi + p1.lo, r11 = p0.hi + p1.hi;
  const double v00 = lerp((double)src[r00 + p2.lo], (double)src[r00 + p2.hi], f2);
  const double v01 = lerp((double)src[r01 + p2.lo], (double)src[r01 + p2.hi], f2);
  const double v10 = lerp((double)src[r10 + p2.lo], (double)src[r10 + p2.hi], f2);
  const double v11 = lerp((double)src[r11 + p2.lo], (double)src[r11 + p2.hi], f2);
  return lerp(lerp(v00, v01, f1), lerp(v10, v11, f1), f0);
}

// the channel, of C channels cstride elements apart, whose trilinear value rounded to fp32 is largest: the lowest
// channel on a tie, and a NaN counts as the maximum with the first NaN winning (torch.argmax's rule). Each channel is
// evaluated by trilinear as the linear kernel evaluates it, so this is the argmax over that kernel's output.
RS_HD int argmax_trilinear(const float* src, int C, long long cstride, Pair p0, Pair p1, Pair p2, double f0, double f1,
                           double f2) {
  int best = 0;
  float bv = (float)trilinear(src, p0, p1, p2, f0, f1, f2);
  for (int c = 1; c < C; ++c) {
    const float v = (float)trilinear(src + c * cstride, p0, p1, p2, f0, f1, f2);
    if (bv == bv && (v > bv || v != v)) {  // once bv is a NaN nothing replaces it
      bv = v;
      best = c;
    }
  }
  return best;
}

}  // namespace rs
}  // namespace u3d
