// Building the probabilistic atlas on the device (preprocess/atlas_gen_mm.py:114-145): per training case and label l,
// ndimage.zoom(label == l, order=0) to the atlas shape summed into plane l - 1 and a per-label case count; then
// plane / count. (The Gaussian filter that follows is data.hip's blur_axis_kernel, three passes over all planes.)
//  * atlas_gather_kernel: the fifteen zooms of a case as ONE gather of the label codes: atlas voxel (a, b, c) reads
//    label[idx0[a]][idx1[b]][idx2[c]] and adds 1 to the plane of the code it finds. The index tables come from the
//    host (u3d.data.zoom_index, scipy's float64 rule; -1 = the coordinate falls outside, the voxel receives nothing),
//    so no floating-point index arithmetic happens here. One thread owns a voxel: plain read-modify-write.
//  * atlas_presence_kernel / atlas_presence_final_kernel: which codes 1..L occur anywhere in the SOURCE volume (the
//    reference tests label_mask.sum() > 0 before the zoom; a shrinking gather skips source voxels): an L-bit word per
//    thread, OR-reduced per block, one atomicOr per block, then counts[l] += bit l.
//  * atlas_normalize_kernel: plane / count in double, rounded once; a plane no case has is written as zeros.
// Sums and counts are integers: every result is independent of the launch geometry and of the order of the calls.
#include "common.h"

namespace u3d {

constexpr int AB = 256;
constexpr int AB_GX = 64;     // blocks along a plane (b, c) of the atlas at most, grid-stride beyond
constexpr int AB_GY = 1024;   // blocks along the slowest atlas axis at most, grid-stride beyond
constexpr int AB_PB = 1024;   // blocks of the presence pass at most
constexpr int AB_LMAX = 31;   // labels: the presence word is 32 bits

// grid.y strides over a, grid.x * AB over the plane index j = b s2 + c (< 2^31); offsets are 64-bit
__global__ __launch_bounds__(AB) void atlas_gather_kernel(const unsigned char* __restrict__ lab, int h, int w, int d,
                                                         const int* __restrict__ idx0, const int* __restrict__ idx1,
                                                         const int* __restrict__ idx2, int L, int s0, int s1, int s2,
                                                         float* __restrict__ acc) {
  const unsigned plane = (unsigned)s1 * (unsigned)s2;
  const long long V = (long long)s0 * plane;
  for (int a = blockIdx.y; a < s0; a += gridDim.y) {
    const int ia = idx0[a];
    if ((unsigned)ia >= (unsigned)h) continue;  // -1: outside (an index past the source is never read either)
    const unsigned char* srow = lab + (long long)ia * w * d;
    float* arow = acc + (long long)a * plane;
    for (unsigned j = blockIdx.x * AB + threadIdx.x; j < plane; j += gridDim.x * AB) {
      const unsigned b = j / (unsigned)s2, c = j - b * (unsigned)s2;
      const int ib = idx1[b], ic = idx2[c];
      if ((unsigned)ib >= (unsigned)w || (unsigned)ic >= (unsigned)d) continue;
      const unsigned l = srow[(long long)ib * d + ic];
      if (l - 1u < (unsigned)L) arow[(long long)(l - 1u) * V + j] += 1.f;
    }
  }
}

__device__ __forceinline__ unsigned label_bit(unsigned l, unsigned L) { return l - 1u < L ? 1u << (l - 1u) : 0u; }

// bits of the codes 1..L present in lab[0..N): scalar head up to 16-byte alignment, 16-byte body, scalar tail
__global__ __launch_bounds__(AB) void atlas_presence_kernel(const unsigned char* __restrict__ lab, long long N, int L,
                                                           unsigned* __restrict__ word) {
  __shared__ unsigned blk;
  if (threadIdx.x == 0) blk = 0;
  __syncthreads();
  const long long tid = blockIdx.x * (long long)AB + threadIdx.x, nthr = (long long)gridDim.x * AB;
  const long long mis = (16 - (long long)((uintptr_t)lab & 15)) & 15;
  const long long head = mis < N ? mis : N;
  const long long nvec = (N - head) / 16, tail = head + nvec * 16;
  unsigned bits = 0;
  for (long long i = tid; i < head; i += nthr) bits |= label_bit(lab[i], L);
  const uint4* v = reinterpret_cast<const uint4*>(lab + head);
  for (long long i = tid; i < nvec; i += nthr) {
    const uint4 q = v[i];
    const unsigned x[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int s = 0; s < 32; s += 8) bits |= label_bit((x[k] >> s) & 255u, L);
  }
  for (long long i = tail + tid; i < N; i += nthr) bits |= label_bit(lab[i], L);
  for (int o = 32; o > 0; o >>= 1) bits |= __shfl_xor(bits, o);
  if ((threadIdx.x & 63) == 0 && bits) atomicOr(&blk, bits);
  __syncthreads();
  if (threadIdx.x == 0 && blk) atomicOr(word, blk);
}

__global__ void atlas_presence_final_kernel(const unsigned* __restrict__ word, int L, int* __restrict__ counts) {
  const int l = threadIdx.x;
  if (l < L && ((*word >> l) & 1u)) counts[l] += 1;
}

// grid.y = the plane l; out[l][v] = (float)((double)acc[l][v] / counts[l]), zeros where counts[l] == 0
__global__ __launch_bounds__(AB) void atlas_normalize_kernel(const float* __restrict__ acc,
                                                            const int* __restrict__ counts, long long V,
                                                            float* __restrict__ out) {
  const int l = blockIdx.y;
  const int n = counts[l];
  const float* a = acc + (long long)l * V;
  float* o = out + (long long)l * V;
  for (long long i = blockIdx.x * (long long)AB + threadIdx.x; i < V; i += (long long)gridDim.x * AB)
    o[i] = n > 0 ? (float)((double)a[i] / (double)n) : 0.f;
}

}  // namespace u3d

using namespace u3d;

extern "C" long long u3d_atlas_build_ws_bytes(void) { return 16; }

extern "C" int u3d_atlas_build_add(const unsigned char* label_u8, int h, int w, int d, const int* idx0, const int* idx1,
                                   const int* idx2, int L, int s0, int s1, int s2, float* acc, int* counts, void* ws,
                                   u3d_stream_t stream) {
  U3D_REQUIRE(label_u8 && idx0 && idx1 && idx2 && acc && counts && ws, "atlas_build_add: null pointer");
  U3D_REQUIRE(h >= 1 && w >= 1 && d >= 1 && s0 >= 1 && s1 >= 1 && s2 >= 1, "atlas_build_add: bad shape");
  U3D_REQUIRE(L >= 1 && L <= AB_LMAX, "atlas_build_add: L=%d (1..%d)", L, AB_LMAX);
  U3D_REQUIRE((long long)s1 * s2 < (1LL << 31), "atlas_build_add: atlas plane %d x %d too large", s1, s2);
  hipStream_t s = (hipStream_t)stream;
  U3D_HIP(hipMemsetAsync(ws, 0, 4, s));
  const long long N = (long long)h * w * d;
  const int pb = (int)std::min<long long>(AB_PB, std::max<long long>(1, (N / 16 + AB - 1) / AB));
  hipLaunchKernelGGL(atlas_presence_kernel, dim3(pb), dim3(AB), 0, s, label_u8, N, L, (unsigned*)ws);
  hipLaunchKernelGGL(atlas_presence_final_kernel, dim3(1), dim3(64), 0, s, (const unsigned*)ws, L, counts);
  const long long plane = (long long)s1 * s2;
  const int gx = (int)std::min<long long>(AB_GX, (plane + AB - 1) / AB), gy = std::min(AB_GY, s0);
  hipLaunchKernelGGL(atlas_gather_kernel, dim3(gx, gy), dim3(AB), 0, s, label_u8, h, w, d, idx0, idx1, idx2, L, s0, s1,
                     s2, acc);
  return check_launch("atlas_build_add");
}

extern "C" int u3d_atlas_build_normalize(const float* acc, const int* counts, int L, long long V, float* out,
                                         u3d_stream_t stream) {
  U3D_REQUIRE(acc && counts && out && L >= 1 && L <= AB_LMAX && V >= 1, "atlas_build_normalize: bad args");
  const int gx = (int)std::min<long long>(4096, (V + AB - 1) / AB);
  hipLaunchKernelGGL(atlas_normalize_kernel, dim3(gx, L), dim3(AB), 0, (hipStream_t)stream, acc, counts, V, out);
  return check_launch("atlas_build_normalize");
}
