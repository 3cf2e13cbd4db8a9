// Separable grid resampling on the device: the sampling step of MONAI's Orientationd + Spacingd as the reference's
// preprocess/transforms.py:41-54 applies them (trilinear for the image, nearest for the label, border clamping), and
// the way back for predictions. With Spacing's defaults the map from an output voxel to the source is a permutation and
// flip of the axes followed by an independent scale per axis, so it is three 1-D tables (u3d.data.GridPlan, float64 on
// the host) and the kernels are gathers that know nothing about orientation: per output axis a source stride, a source
// length and the table. The per-voxel routines are csrc/resample_core.h.
//
// Shape: lanes along output axis 2, one wave-uniform output row (k0, k1) per group of 64, 128 or 256 lanes (the
// smallest that covers the row, so short rows do not idle most of a workgroup). A row's four source-row offsets and
// its two weights are uniform (scalar loads of the tables); each lane forms its two column offsets and its weight
// once and walks the channels. When the source's contiguous axis is output axis 2 (no permutation: the AMOS case)
// adjacent lanes read adjacent or equal elements of four source rows and store one contiguous output row.
//
// The way back for scores, grid_resample_argmax_kernel: the same row shape, but a lane keeps only the index of the
// channel whose trilinear value is largest (rs::argmax_trilinear: the linear kernel's arithmetic and rounding, so the
// argmax over its output bit for bit) and stores one byte; voxels outside a box of valid output indices get 0.
#include "common.h"
#include "resample_core.h"

namespace u3d {

constexpr int RS_NT = 256;

struct RsAxes {
  int n_out[3];
  int n_src[3];
  long long stride[3];
};

struct RsTables {
  const int* idx[3];
  const double* frac[3];
};

// lanes of one row: 64, 128 or 256
static int rs_lane_shift(int n2) { return n2 <= 64 ? 6 : n2 <= 128 ? 7 : 8; }

// the wave's output row, or -1 past the end
__device__ __forceinline__ int rs_row(int shift, int rows) {
  const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (RS_NT >> shift) + (threadIdx.x >> shift)));
  return row < rows ? row : -1;
}

template <typename T>
__global__ __launch_bounds__(RS_NT) void grid_resample_linear_kernel(const T* __restrict__ src, int C, long long cstride,
                                                                    RsAxes ax, RsTables tab, float* __restrict__ out,
                                                                    int shift, int rows) {
  const int row = rs_row(shift, rows);
  if (row < 0) return;
  const int k0 = row / ax.n_out[1], k1 = row - k0 * ax.n_out[1];
  const rs::Pair p0 = rs::pair_offsets(tab.idx[0][k0], ax.n_src[0], ax.stride[0]);
  const rs::Pair p1 = rs::pair_offsets(tab.idx[1][k1], ax.n_src[1], ax.stride[1]);
  const double f0 = tab.frac[0][k0], f1 = tab.frac[1][k1];
  const int n2 = ax.n_out[2], lanes = 1 << shift;
  const long long plane = (long long)rows * n2;
  float* orow = out + (long long)row * n2;
  for (int k2 = threadIdx.x & (lanes - 1); k2 < n2; k2 += lanes) {
    const rs::Pair p2 = rs::pair_offsets(tab.idx[2][k2], ax.n_src[2], ax.stride[2]);
    const double f2 = tab.frac[2][k2];
    for (int c = 0; c < C; ++c) orow[c * plane + k2] = (float)rs::trilinear(src + c * cstride, p0, p1, p2, f0, f1, f2);
  }
}

template <typename T>
__global__ __launch_bounds__(RS_NT) void grid_resample_nearest_kernel(const T* __restrict__ src, int C,
                                                                     long long cstride, RsAxes ax, RsTables tab,
                                                                     T* __restrict__ out, int shift, int rows) {
  const int row = rs_row(shift, rows);
  if (row < 0) return;
  const int k0 = row / ax.n_out[1], k1 = row - k0 * ax.n_out[1];
  const long long base = rs::nearest_offset(tab.idx[0][k0], ax.n_src[0], ax.stride[0]) +
                         rs::nearest_offset(tab.idx[1][k1], ax.n_src[1], ax.stride[1]);
  const int n2 = ax.n_out[2], lanes = 1 << shift;
  const long long plane = (long long)rows * n2;
  T* orow = out + (long long)row * n2;
  for (int k2 = threadIdx.x & (lanes - 1); k2 < n2; k2 += lanes) {
    const long long o = base + rs::nearest_offset(tab.idx[2][k2], ax.n_src[2], ax.stride[2]);
    for (int c = 0; c < C; ++c) orow[c * plane + k2] = src[c * cstride + o];
  }
}

struct RsValid {
  int lo[3], hi[3];
};

// out uint8 = the argmax over the channels of what grid_resample_linear_kernel<float> would store, 0 outside the valid
// box. The same row shape: a row outside the box on axis 0 or 1 (wave-uniform) is zeros and reads no table and no source.
__global__ __launch_bounds__(RS_NT) void grid_resample_argmax_kernel(const float* __restrict__ src, int C,
                                                                    long long cstride, RsAxes ax, RsTables tab,
                                                                    RsValid valid, unsigned char* __restrict__ out,
                                                                    int shift, int rows) {
  const int row = rs_row(shift, rows);
  if (row < 0) return;
  const int k0 = row / ax.n_out[1], k1 = row - k0 * ax.n_out[1];
  const int n2 = ax.n_out[2], lanes = 1 << shift;
  unsigned char* orow = out + (long long)row * n2;
  if (k0 < valid.lo[0] || k0 >= valid.hi[0] || k1 < valid.lo[1] || k1 >= valid.hi[1]) {
    for (int k2 = threadIdx.x & (lanes - 1); k2 < n2; k2 += lanes) orow[k2] = 0;
    return;
  }
  const rs::Pair p0 = rs::pair_offsets(tab.idx[0][k0], ax.n_src[0], ax.stride[0]);
  const rs::Pair p1 = rs::pair_offsets(tab.idx[1][k1], ax.n_src[1], ax.stride[1]);
  const double f0 = tab.frac[0][k0], f1 = tab.frac[1][k1];
  for (int k2 = threadIdx.x & (lanes - 1); k2 < n2; k2 += lanes) {
    int best = 0;
    if (k2 >= valid.lo[2] && k2 < valid.hi[2]) {
      const rs::Pair p2 = rs::pair_offsets(tab.idx[2][k2], ax.n_src[2], ax.stride[2]);
      best = rs::argmax_trilinear(src, C, cstride, p0, p1, p2, f0, f1, tab.frac[2][k2]);
    }
    orow[k2] = (unsigned char)best;
  }
}

// the checks both entry points share; fills ax, the row count and the grid
static int rs_geometry(const char* what, const void* src, const void* out, int C, const long long* src_stride,
                       long long src_chan_stride, const int* src_n, const int* n_out, RsAxes& ax, int& rows,
                       int& shift, unsigned& blocks) {
  U3D_REQUIRE(src && out && src_stride && src_n && n_out, "%s: null pointer", what);
  U3D_REQUIRE(C >= 1 && src_chan_stride >= 0, "%s: C=%d, channel stride %lld", what, C, src_chan_stride);
  for (int i = 0; i < 3; ++i) {
    U3D_REQUIRE(n_out[i] >= 1 && src_n[i] >= 1 && src_stride[i] >= 1,
                "%s: axis %d: output size %d, source size %d, source stride %lld must be positive", what, i, n_out[i],
                src_n[i], src_stride[i]);
    ax.n_out[i] = n_out[i];
    ax.n_src[i] = src_n[i];
    ax.stride[i] = src_stride[i];
  }
  const long long r = (long long)n_out[0] * n_out[1];
  U3D_REQUIRE(r < (1LL << 31) - RS_NT, "%s: %lld output rows (fewer than 2^31)", what, r);
  rows = (int)r;
  shift = rs_lane_shift(n_out[2]);
  blocks = (unsigned)cdiv(r, RS_NT >> shift);
  return 0;
}

}  // namespace u3d

using namespace u3d;

extern "C" int u3d_grid_resample_linear(const void* src, int src_dtype, int C, const long long* src_stride,
                                        long long src_chan_stride, const int* src_n, const int* n_out,
                                        const int* i0_0, const int* i0_1, const int* i0_2, const double* frac_0,
                                        const double* frac_1, const double* frac_2, float* out, u3d_stream_t stream) {
  U3D_REQUIRE(src_dtype == U3D_RS_F32 || src_dtype == U3D_RS_I16,
              "grid_resample_linear: source dtype %d (U3D_RS_F32 or U3D_RS_I16)", src_dtype);
  U3D_REQUIRE(i0_0 && i0_1 && i0_2 && frac_0 && frac_1 && frac_2, "grid_resample_linear: null table");
  RsAxes ax;
  int rows, shift;
  unsigned blocks;
  int rc = rs_geometry("grid_resample_linear", src, out, C, src_stride, src_chan_stride, src_n, n_out, ax, rows, shift,
                       blocks);
  if (rc) return rc;
  const RsTables tab{{i0_0, i0_1, i0_2}, {frac_0, frac_1, frac_2}};
  hipStream_t s = (hipStream_t)stream;
  if (src_dtype == U3D_RS_F32)
    hipLaunchKernelGGL(grid_resample_linear_kernel<float>, dim3(blocks), dim3(RS_NT), 0, s, (const float*)src, C,
                       src_chan_stride, ax, tab, out, shift, rows);
  else
    hipLaunchKernelGGL(grid_resample_linear_kernel<int16_t>, dim3(blocks), dim3(RS_NT), 0, s, (const int16_t*)src, C,
                       src_chan_stride, ax, tab, out, shift, rows);
  return check_launch("grid_resample_linear_kernel");
}

extern "C" int u3d_grid_resample_nearest(const void* src, int src_dtype, int C, const long long* src_stride,
                                         long long src_chan_stride, const int* src_n, const int* n_out,
                                         const int* near_0, const int* near_1, const int* near_2, void* out,
                                         u3d_stream_t stream) {
  U3D_REQUIRE(src_dtype == U3D_RS_U8 || src_dtype == U3D_RS_I16 || src_dtype == U3D_RS_I32 || src_dtype == U3D_RS_F32,
              "grid_resample_nearest: source dtype %d (U3D_RS_U8, _I16, _I32 or _F32)", src_dtype);
  U3D_REQUIRE(near_0 && near_1 && near_2, "grid_resample_nearest: null table");
  RsAxes ax;
  int rows, shift;
  unsigned blocks;
  int rc = rs_geometry("grid_resample_nearest", src, out, C, src_stride, src_chan_stride, src_n, n_out, ax, rows,
                       shift, blocks);
  if (rc) return rc;
  const RsTables tab{{near_0, near_1, near_2}, {nullptr, nullptr, nullptr}};
  hipStream_t s = (hipStream_t)stream;
  // a copy of the element's bits: one kernel per element size
  if (src_dtype == U3D_RS_U8)
    hipLaunchKernelGGL(grid_resample_nearest_kernel<uint8_t>, dim3(blocks), dim3(RS_NT), 0, s, (const uint8_t*)src, C,
                       src_chan_stride, ax, tab, (uint8_t*)out, shift, rows);
  else if (src_dtype == U3D_RS_I16)
    hipLaunchKernelGGL(grid_resample_nearest_kernel<uint16_t>, dim3(blocks), dim3(RS_NT), 0, s, (const uint16_t*)src, C,
                       src_chan_stride, ax, tab, (uint16_t*)out, shift, rows);
  else
    hipLaunchKernelGGL(grid_resample_nearest_kernel<uint32_t>, dim3(blocks), dim3(RS_NT), 0, s, (const uint32_t*)src, C,
                       src_chan_stride, ax, tab, (uint32_t*)out, shift, rows);
  return check_launch("grid_resample_nearest_kernel");
}

extern "C" int u3d_grid_resample_argmax(const float* src, int C, const long long* src_stride, long long src_chan_stride,
                                        const int* src_n, const int* n_out, const int* i0_0, const int* i0_1,
                                        const int* i0_2, const double* frac_0, const double* frac_1,
                                        const double* frac_2, const int* valid_lo, const int* valid_hi,
                                        unsigned char* out, u3d_stream_t stream) {
  U3D_REQUIRE(C <= 256, "grid_resample_argmax: C=%d (1..256: the result is a uint8)", C);
  U3D_REQUIRE(i0_0 && i0_1 && i0_2 && frac_0 && frac_1 && frac_2, "grid_resample_argmax: null table");
  U3D_REQUIRE(valid_lo && valid_hi, "grid_resample_argmax: null valid range");
  RsAxes ax;
  int rows, shift;
  unsigned blocks;
  int rc = rs_geometry("grid_resample_argmax", src, out, C, src_stride, src_chan_stride, src_n, n_out, ax, rows, shift,
                       blocks);
  if (rc) return rc;
  RsValid valid;
  for (int i = 0; i < 3; ++i) {
    valid.lo[i] = valid_lo[i];
    valid.hi[i] = valid_hi[i];
  }
  const RsTables tab{{i0_0, i0_1, i0_2}, {frac_0, frac_1, frac_2}};
  hipLaunchKernelGGL(grid_resample_argmax_kernel, dim3(blocks), dim3(RS_NT), 0, (hipStream_t)stream, src, C,
                     src_chan_stride, ax, tab, valid, out, shift, rows);
  return check_launch("grid_resample_argmax_kernel");
}
