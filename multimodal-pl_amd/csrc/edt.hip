// Surface metrics on the device: an exact 3-D Euclidean distance transform and the passes that turn two label maps
// into surface distances (u3d/surface.py: NSD, HD, HD95, ASSD).
//
// u3d_edt, separable (edt_core.h), squared distances in fp64, w = spacing^2:
//  * edt_row_kernel        one wave per x row: the row's feature bits by ballot (64 voxels per word, in LDS), then per
//                          voxel the nearest set bit on either side (clz / ctz over the words): D = wx dx^2, +inf for a
//                          row without a feature. mask (1 B) -> D (8 B).
//  * edt_axis_kernel       min-plus along y, then z: one workgroup stages a tile of `cols` adjacent lines (x fastest, so
//                          the global accesses are contiguous runs of cols doubles) in LDS and every thread searches
//                          outward from its element; lanes of a wave read consecutive LDS doubles at every step. The y
//                          pass works in place (a tile is read whole before it is written); the z pass writes the fp32
//                          result (the distance, or its square).
// No atomics; a minimum over exact candidates: the result does not depend on the launch geometry.
//  * mask_surface_kernel   uint8 surface of (src == value) on a box: the voxel is set and one of its six face neighbours
//                          is not (outside the volume counts as not). One pass.
//  * class_boxes_kernel    per class 1..num_class the bounding box of (pred == c) | (gt == c) and the two voxel counts:
//                          LDS atomics per hit (x bounds, counts), the row's z / y once per row and class, then one
//                          global atomic per block, bound and class.
//  * surf_reduce_kernel    over surf_a != 0: count, fp64 sum, max, count(dist_b <= tol), min of dist_b: block partials
//                          in a fixed geometry, combined in block order by surf_reduce_final_kernel.
#include "common.h"
#include "edt_core.h"

#include <limits.h>

namespace u3d {

using namespace edt;

constexpr int EB = 256;        // threads of the transform's kernels and of the reduction
constexpr int EROW = 128;      // threads of the row-striding kernels
constexpr int EMAXB = 8192;    // blocks of a grid-stride kernel at most
constexpr int ERED = 512;      // blocks of the reduction at most (the fixed geometry of its sum)
constexpr int EMAXC = 64;      // classes of u3d_class_boxes at most
enum { SD_U8 = 0, SD_F32 = 1, SD_I32 = 2, SD_I64 = 3 };

__global__ __launch_bounds__(EB) void edt_row_kernel(const unsigned char* __restrict__ mask, long long rows, int X,
                                                     int invert, double wx, double* __restrict__ D) {
  __shared__ unsigned long long words[EB / 64][ROW_WORDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = (X + 63) >> 6;
  // every wave of a block makes the same number of rounds (the barriers); a wave past the last row idles
  for (long long r0 = (long long)blockIdx.x * (EB / 64); r0 < rows; r0 += (long long)gridDim.x * (EB / 64)) {
    const long long r = r0 + wave;
    const bool live = r < rows;
    for (int c = 0; c < nw; ++c) {
      const int x = c * 64 + lane;
      const bool f = live && x < X && ((mask[r * X + x] != 0) != (invert != 0));
      const unsigned long long b = __ballot(f);
      if (lane == 0) words[wave][c] = b;
    }
    __syncthreads();
    if (live)
      for (int x = lane; x < X; x += 64) D[r * X + x] = row_value(words[wave], nw, x, wx);
    __syncthreads();
  }
}

// [outer][n][inner] fp64, min-plus along n. Workgroup b: outer index b / tiles, columns (b % tiles) * cols ... of inner.
// cols is a power of two (1 << lc) with cols * n * 8 <= TILE_BYTES. LAST: write finish(.) to outf, else to outd (which
// may be `in`).
template <bool LAST>
__global__ __launch_bounds__(EB) void edt_axis_kernel(const double* in, double* outd, float* __restrict__ outf, int n,
                                                      long long inner, int lc, int tiles, double w, int squared) {
  extern __shared__ double line[];
  const int cols = 1 << lc;
  const long long o = blockIdx.x / tiles;
  const long long c0 = (long long)(blockIdx.x % tiles) * cols;
  const int live = inner - c0 < cols ? (int)(inner - c0) : cols;
  const long long base = o * n * inner + c0;
  const int tot = n << lc;
  for (int e = threadIdx.x; e < tot; e += EB) {
    const int i = e >> lc, c = e & (cols - 1);
    line[e] = c < live ? in[base + (long long)i * inner + c] : infinity();
  }
  __syncthreads();
  for (int e = threadIdx.x; e < tot; e += EB) {
    const int j = e >> lc, c = e & (cols - 1);
    if (c >= live) continue;
    const double v = line_min(line + c, cols, n, j, w);
    const long long g = base + (long long)j * inner + c;
    if constexpr (LAST)
      outf[g] = finish(v, squared);
    else
      outd[g] = v;
  }
}

// src[i] == value (nonzero: src[i] != 0, NaN counting as nonzero); value compared in double (exact below 2^53)
__device__ __forceinline__ bool sd_hit(const void* __restrict__ p, int dt, long long i, double value, int nonzero) {
  double v;
  switch (dt) {
    case SD_U8: v = ((const unsigned char*)p)[i]; break;
    case SD_F32: v = ((const float*)p)[i]; break;
    case SD_I32: v = ((const int*)p)[i]; break;
    default: v = (double)((const long long*)p)[i]; break;
  }
  return nonzero ? v != 0.0 : v == value;
}

// the class of voxel i as an int, -1 when it is no int (a fraction, NaN, out of range)
__device__ __forceinline__ int sd_class(const void* __restrict__ p, int dt, long long i) {
  switch (dt) {
    case SD_U8: return ((const unsigned char*)p)[i];
    case SD_I32: return ((const int*)p)[i];
    case SD_F32: {
      const float v = ((const float*)p)[i];
      if (!(v >= 0.f && v <= 65536.f)) return -1;
      const int c = (int)v;
      return (float)c == v ? c : -1;
    }
    default: {
      const long long v = ((const long long*)p)[i];
      return v >= 0 && v <= 65536 ? (int)v : -1;
    }
  }
}

__global__ __launch_bounds__(EROW) void mask_surface_kernel(const void* __restrict__ src, int dt, int Z, int Y, int X,
                                                            double value, int nonzero, int z0, int y0, int x0, int bz,
                                                            int by, int bx, unsigned char* __restrict__ out) {
  const long long rows = (long long)bz * by, sy = X, sz = (long long)Y * X;
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
    const int z = z0 + (int)(r / by), y = y0 + (int)(r % by);
    for (int lx = threadIdx.x; lx < bx; lx += EROW) {
      const int x = x0 + lx;
      const long long i = ((long long)z * Y + y) * X + x;
      bool m = sd_hit(src, dt, i, value, nonzero);
      if (m) {
        const bool inside = x > 0 && x + 1 < X && y > 0 && y + 1 < Y && z > 0 && z + 1 < Z &&
                            sd_hit(src, dt, i - 1, value, nonzero) && sd_hit(src, dt, i + 1, value, nonzero) &&
                            sd_hit(src, dt, i - sy, value, nonzero) && sd_hit(src, dt, i + sy, value, nonzero) &&
                            sd_hit(src, dt, i - sz, value, nonzero) && sd_hit(src, dt, i + sz, value, nonzero);
        m = !inside;
      }
      out[r * bx + lx] = m ? 1 : 0;
    }
  }
}

enum { K_LO = 0, K_HI = 3, K_NP = 6, K_NG = 7 };

__global__ void class_boxes_init_kernel(int* __restrict__ rec, int n) {
  for (int k = threadIdx.x; k < n * U3D_CLASS_RECORD; k += blockDim.x) {
    const int f = k % U3D_CLASS_RECORD;
    rec[k] = f < K_HI ? INT_MAX : f < K_NP ? -1 : 0;
  }
}

__global__ __launch_bounds__(EROW) void class_boxes_kernel(const void* __restrict__ pred, int pdt,
                                                           const void* __restrict__ gt, int gdt, int Z, int Y, int X,
                                                           int nc, int* __restrict__ rec) {
  __shared__ int s[EMAXC][U3D_CLASS_RECORD];
  __shared__ int seen[EMAXC];
  for (int k = threadIdx.x; k < nc * U3D_CLASS_RECORD; k += EROW) {
    const int f = k % U3D_CLASS_RECORD;
    s[k / U3D_CLASS_RECORD][f] = f < K_HI ? INT_MAX : f < K_NP ? -1 : 0;
  }
  for (int c = threadIdx.x; c < nc; c += EROW) seen[c] = 0;
  __syncthreads();
  const long long rows = (long long)Z * Y;
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {  // the same rounds for every thread of the block
    const int z = (int)(r / Y), y = (int)(r - (long long)z * Y);
    for (int x = threadIdx.x; x < X; x += EROW) {
      const int cp = sd_class(pred, pdt, r * X + x) - 1, cg = sd_class(gt, gdt, r * X + x) - 1;
      if (cp >= 0 && cp < nc) {
        atomicMin(&s[cp][K_LO + 2], x), atomicMax(&s[cp][K_HI + 2], x), atomicAdd(&s[cp][K_NP], 1);
        seen[cp] = 1;
      }
      if (cg >= 0 && cg < nc) {
        atomicMin(&s[cg][K_LO + 2], x), atomicMax(&s[cg][K_HI + 2], x), atomicAdd(&s[cg][K_NG], 1);
        seen[cg] = 1;
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < nc; c += EROW)
      if (seen[c]) {  // thread c alone owns the z / y bounds of class c
        s[c][K_LO] = min(s[c][K_LO], z), s[c][K_HI] = max(s[c][K_HI], z);
        s[c][K_LO + 1] = min(s[c][K_LO + 1], y), s[c][K_HI + 1] = max(s[c][K_HI + 1], y);
        seen[c] = 0;
      }
    __syncthreads();
  }
  for (int k = threadIdx.x; k < nc * U3D_CLASS_RECORD; k += EROW) {
    const int c = k / U3D_CLASS_RECORD, f = k % U3D_CLASS_RECORD;
    if (s[c][K_HI] < 0) continue;
    if (f < K_HI)
      atomicMin(&rec[k], s[c][f]);
    else if (f < K_NP)
      atomicMax(&rec[k], s[c][f]);
    else if (s[c][f])
      atomicAdd(&rec[k], s[c][f]);
  }
}

// part[block][5] = count, sum, max, count(<= tol), min over the block's share of the voxels with surf != 0
__global__ __launch_bounds__(EB) void surf_reduce_kernel(const unsigned char* __restrict__ surf,
                                                         const float* __restrict__ dist, long long V, double tol,
                                                         double* __restrict__ part) {
  double n = 0, s = 0, mx = -infinity(), le = 0, mn = infinity();
  for (long long i = blockIdx.x * (long long)EB + threadIdx.x; i < V; i += (long long)gridDim.x * EB) {
    if (surf[i] == 0) continue;
    const double d = dist[i];
    n += 1;
    s += d;
    mx = fmax(mx, d);
    mn = fmin(mn, d);
    le += d <= tol ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_xor(n, o);
    s += __shfl_xor(s, o);
    le += __shfl_xor(le, o);
    mx = fmax(mx, __shfl_xor(mx, o));
    mn = fmin(mn, __shfl_xor(mn, o));
  }
  __shared__ double r[EB / 64][U3D_SURFACE_RECORD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) r[wave][0] = n, r[wave][1] = s, r[wave][2] = mx, r[wave][3] = le, r[wave][4] = mn;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0, b = 0, c = -infinity(), d = 0, e = infinity();
    for (int w = 0; w < EB / 64; ++w) {
      a += r[w][0], b += r[w][1], d += r[w][3];
      c = fmax(c, r[w][2]), e = fmin(e, r[w][4]);
    }
    double* o = part + (long long)blockIdx.x * U3D_SURFACE_RECORD;
    o[0] = a, o[1] = b, o[2] = c, o[3] = d, o[4] = e;
  }
}

__global__ void surf_reduce_final_kernel(const double* __restrict__ part, int nb, double* __restrict__ rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a = 0, b = 0, c = -infinity(), d = 0, e = infinity();
  for (int k = 0; k < nb; ++k) {
    const double* p = part + (long long)k * U3D_SURFACE_RECORD;
    a += p[0], b += p[1], d += p[3];
    c = fmax(c, p[2]), e = fmin(e, p[4]);
  }
  rec[0] = a, rec[1] = b, rec[2] = c, rec[3] = d, rec[4] = e;
}

static inline int edt_row_blocks(long long rows) {
  return (int)std::min<long long>(EMAXB, std::max<long long>(1, rows));
}
static inline int log2i(int p) {
  int l = 0;
  while ((1 << l) < p) ++l;
  return l;
}

}  // namespace u3d

using namespace u3d;

extern "C" int u3d_edt_max_extent(void) { return MAX_EXTENT; }

extern "C" void u3d_edt_tile(int* max_cols, int* tile_bytes) {
  if (max_cols) *max_cols = MAX_COLS;
  if (tile_bytes) *tile_bytes = TILE_BYTES;
}

extern "C" long long u3d_edt_ws_bytes(long long V) {
  if (V < 1 || V >= (1LL << 31)) return -1;
  return 8 * V;
}

extern "C" long long u3d_surface_reduce_ws_bytes(void) { return (long long)ERED * U3D_SURFACE_RECORD * 8; }

extern "C" int u3d_edt(const unsigned char* mask, int Z, int Y, int X, double sz, double sy, double sx, int invert,
                       int squared, float* out, void* ws, u3d_stream_t stream) {
  U3D_REQUIRE(Z >= 1 && Y >= 1 && X >= 1, "edt: bad shape %d x %d x %d", Z, Y, X);
  U3D_REQUIRE(Z <= MAX_EXTENT && Y <= MAX_EXTENT && X <= MAX_EXTENT, "edt: %d x %d x %d: at most %d per axis", Z, Y, X,
              MAX_EXTENT);
  const long long V = (long long)Z * Y * X;
  U3D_REQUIRE(V < (1LL << 31), "edt: %lld voxels (V < 2^31)", V);
  U3D_REQUIRE(sz > 0 && sy > 0 && sx > 0 && sz <= 1e6 && sy <= 1e6 && sx <= 1e6, "edt: spacing (%g, %g, %g) must be "
              "positive and finite", sz, sy, sx);
  U3D_REQUIRE(mask && out && ws, "edt: null pointer");
  hipStream_t s = (hipStream_t)stream;
  double* D = (double*)ws;
  const long long rows = (long long)Z * Y;
  hipLaunchKernelGGL(edt_row_kernel, dim3(edt_row_blocks((rows + EB / 64 - 1) / (EB / 64))), dim3(EB), 0, s, mask, rows,
                     X, invert, sx * sx, D);
  {
    const int cols = tile_cols(Y), tiles = cdiv(X, cols);
    hipLaunchKernelGGL((edt_axis_kernel<false>), dim3((unsigned)((long long)Z * tiles)), dim3(EB),
                       (size_t)cols * Y * 8, s, (const double*)D, D, (float*)nullptr, Y, (long long)X, log2i(cols),
                       tiles, sy * sy, 0);
  }
  {
    const long long inner = (long long)Y * X;
    const int cols = tile_cols(Z), tiles = cdiv(inner, cols);
    hipLaunchKernelGGL((edt_axis_kernel<true>), dim3((unsigned)tiles), dim3(EB), (size_t)cols * Z * 8, s,
                       (const double*)D, (double*)nullptr, out, Z, inner, log2i(cols), tiles, sz * sz, squared);
  }
  return check_launch("edt");
}

extern "C" int u3d_mask_surface(const void* src, int dtype, int Z, int Y, int X, double value, int nonzero, int z0,
                                int y0, int x0, int bz, int by, int bx, unsigned char* out, u3d_stream_t stream) {
  U3D_REQUIRE(Z >= 1 && Y >= 1 && X >= 1 && (long long)Z * Y * X < (1LL << 31), "mask_surface: bad shape %d x %d x %d "
              "(V < 2^31)", Z, Y, X);
  U3D_REQUIRE(dtype >= 0 && dtype <= 3, "mask_surface: dtype=%d (0 uint8, 1 float32, 2 int32, 3 int64)", dtype);
  U3D_REQUIRE(bz >= 1 && by >= 1 && bx >= 1 && z0 >= 0 && y0 >= 0 && x0 >= 0 && z0 <= Z - bz && y0 <= Y - by &&
                  x0 <= X - bx,
              "mask_surface: box (%d, %d, %d) + (%d, %d, %d) outside %d x %d x %d", z0, y0, x0, bz, by, bx, Z, Y, X);
  U3D_REQUIRE(src && out, "mask_surface: null pointer");
  hipLaunchKernelGGL(mask_surface_kernel, dim3(edt_row_blocks((long long)bz * by)), dim3(EROW), 0, (hipStream_t)stream,
                     src, dtype, Z, Y, X, value, nonzero, z0, y0, x0, bz, by, bx, out);
  return check_launch("mask_surface");
}

extern "C" int u3d_class_boxes(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int Z, int Y, int X,
                               int num_class, int* record, u3d_stream_t stream) {
  U3D_REQUIRE(Z >= 1 && Y >= 1 && X >= 1 && (long long)Z * Y * X < (1LL << 31), "class_boxes: bad shape %d x %d x %d "
              "(the counts are int32: V < 2^31)", Z, Y, X);
  U3D_REQUIRE(num_class >= 1 && num_class <= EMAXC, "class_boxes: num_class=%d (1..%d)", num_class, EMAXC);
  U3D_REQUIRE(pred_dtype >= 0 && pred_dtype <= 3 && gt_dtype >= 0 && gt_dtype <= 3,
              "class_boxes: dtypes %d, %d (0 uint8, 1 float32, 2 int32, 3 int64)", pred_dtype, gt_dtype);
  U3D_REQUIRE(pred && gt && record, "class_boxes: null pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(class_boxes_init_kernel, dim3(1), dim3(256), 0, s, record, num_class);
  hipLaunchKernelGGL(class_boxes_kernel, dim3(edt_row_blocks((long long)Z * Y)), dim3(EROW), 0, s, pred, pred_dtype, gt,
                     gt_dtype, Z, Y, X, num_class, record);
  return check_launch("class_boxes");
}

extern "C" int u3d_surface_dist_reduce(const unsigned char* surf_a, const float* dist_b, long long V, double tol,
                                       double* record, void* ws, u3d_stream_t stream) {
  U3D_REQUIRE(V >= 1 && V < (1LL << 31), "surface_dist_reduce: %lld voxels (1 <= V < 2^31)", V);
  U3D_REQUIRE(tol == tol, "surface_dist_reduce: tol is NaN");
  U3D_REQUIRE(surf_a && dist_b && record && ws, "surface_dist_reduce: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)std::min<long long>(ERED, (V + EB - 1) / EB);
  hipLaunchKernelGGL(surf_reduce_kernel, dim3(nb), dim3(EB), 0, s, surf_a, dist_b, V, tol, (double*)ws);
  hipLaunchKernelGGL(surf_reduce_final_kernel, dim3(1), dim3(64), 0, s, (const double*)ws, nb, record);
  return check_launch("surface_dist_reduce");
}
