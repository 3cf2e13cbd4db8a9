// 3-D connected components on the device, and the body mask of preprocess/forward_crop.py:37-82 on top of them.
// Face connectivity (6 neighbours); components numbered 1..n in the C order of their first voxel, background 0:
// scipy.ndimage.label(mask) with its default structure.
//
// Labelling, a single-pass union-find (ccl_core.h: a component's root is its smallest linear index, unions are atomic
// mins, every loop moves to smaller values only; no pass is repeated "until nothing changes"):
//  * ccl_local_kernel         one workgroup per TZ x TY x TX tile: parents in LDS, unions with the three predecessors
//                             inside the tile, global parent = global index of the local root.
//  * ccl_seam_kernel          voxels on a tile's low faces union with the neighbour across the face (device-scope
//                             atomic min on the global parents). Rows off the y / z faces touch every TX-th voxel only.
//  * ccl_flatten_count_kernel parent[v] = root, and the roots (parent[v] == v) of each CH-voxel chunk counted.
// Consecutive numbering, a two-level prefix sum over the root flags:
//  * ccl_scan_kernel          exclusive scan of the chunk counts (one workgroup), n to a device int.
//  * ccl_rank_kernel          labels[root] = 1 + roots before it (chunk offset + ballot prefix inside the chunk).
//  * ccl_relabel_kernel       labels[v] = labels[parent[v]], 0 for background.
// getmaxcomponent (:37-59):
//  * ccl_sizes_kernel         voxels per label 1..num_limit-1: each thread walks 8 consecutive voxels and adds a run's
//                             length when the label changes, into an LDS table; one global add per label and block.
//  * ccl_pick_kernel          the largest label with size >= min_filter, the earliest on a tie; the record.
//  * bbox_kernel<.., SELECT>  the uint8 mask of the chosen label and its bounding box: block-reduced in LDS, one
//                             atomic min / max per block and bound.
// Per-label largest component (u3d_ccl_keep_largest), one labelling for all the organs of a label map:
//  * keep_local_kernel / keep_seam_kernel   the two kernels above with the voxel's code next to its parent: a voxel
//                             joins a predecessor only when both hold the same code in 1..num_labels.
//  * keep_flatten_sizes_kernel  parent[v] = root and sizes[root] += run lengths (integer adds: no arrival order).
//  * keep_best_kernel         per label an atomic max over its roots of (size << 32) | (INT_MAX - root): the largest,
//                             the earliest on a tie; block-reduced in LDS.
//  * keep_filter_kernel       out = code where parent == the label's best root, 0 otherwise; the record.
// Mask helpers: body_threshold_kernel (vol > t, optionally the 2x2x2 erosion in the same pass), mask_window_kernel
// (AND / OR over a window along one axis), bbox_kernel<.., NONZERO> (bounding box and count of the nonzero voxels).
// The helpers take a gate: a device int that, when nonzero, turns the launch into a no-op, so that the fallback route
// of get_body is queued behind the component search without a host read in between.
// The record, int32[U3D_CCL_RECORD]: {found, label, size, lo z y x, hi z y x (inclusive), n, 0, 0}.
#include "common.h"
#include "ccl_core.h"

#include <limits.h>

namespace u3d {

using namespace ccl;

constexpr int CB = 256;          // threads of the tile, chunk and size kernels
constexpr int CH = 2048;         // voxels per chunk of the numbering (8 rounds of CB)
constexpr int CSCAN = 1024;      // threads of the scan kernel
constexpr int CLIM = 1024;       // num_limit at most (the LDS size table)
constexpr int CROW = 128;        // threads of the row kernels
constexpr int CMAXB = 8192;      // blocks of a grid-stride kernel at most
enum { R_FOUND = 0, R_LABEL, R_SIZE, R_LO, R_HI = 6, R_N = 9 };

__global__ __launch_bounds__(CB) void ccl_local_kernel(const unsigned char* __restrict__ mask, int Z, int Y, int X,
                                                       int ntx, int nty, int* __restrict__ parent) {
  __shared__ int lp[TILE];
  const int t = blockIdx.x;
  const int x0 = (t % ntx) * TX, y0 = ((t / ntx) % nty) * TY, z0 = (t / (ntx * nty)) * TZ;
  for (int l = threadIdx.x; l < TILE; l += CB) {
    const int x = x0 + l % TX, y = y0 + (l / TX) % TY, z = z0 + l / (TX * TY);
    const bool fg = x < X && y < Y && z < Z && mask[((long long)z * Y + y) * X + x] != 0;
    lp[l] = fg ? l : -1;
  }
  __syncthreads();
  for (int l = threadIdx.x; l < TILE; l += CB) local_unite(lp, l, l % TX, (l / TX) % TY, l / (TX * TY));
  __syncthreads();
  for (int l = threadIdx.x; l < TILE; l += CB) {
    const int x = x0 + l % TX, y = y0 + (l / TX) % TY, z = z0 + l / (TX * TY);
    if (x < X && y < Y && z < Z) parent[((long long)z * Y + y) * X + x] = local_result(lp, l, z0, y0, x0, Y, X);
  }
}

// blocks stride over the rows (z, y); a row on a y or z face visits every x, any other row x = TX, 2 TX, ...
__global__ __launch_bounds__(CROW) void ccl_seam_kernel(int Z, int Y, int X, int* __restrict__ parent) {
  const long long rows = (long long)Z * Y;
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
    const int z = (int)(r / Y), y = (int)(r - (long long)z * Y);
    const bool face = (y > 0 && y % TY == 0) || (z > 0 && z % TZ == 0);
    const int step = face ? 1 : TX;
    for (int x = face ? threadIdx.x : TX * (1 + threadIdx.x); x < X; x += step * CROW)
      seam_unite(parent, (int)(r * X + x), z, y, x, Y, X);
  }
}

__global__ __launch_bounds__(CB) void ccl_flatten_count_kernel(int* __restrict__ parent, int V, int* __restrict__ bc) {
  __shared__ int tot;
  if (threadIdx.x == 0) tot = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * CH;
  int cnt = 0;
  for (int r = 0; r < CH / CB; ++r) {
    const long long i = base + r * CB + threadIdx.x;
    if (i < V) cnt += flatten(parent, (int)i);
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&tot, cnt);
  __syncthreads();
  if (threadIdx.x == 0) bc[blockIdx.x] = tot;
}

// bc[0..nb): counts -> exclusive prefix sums, in place; *n = their total; record[R_N] too when given
__global__ __launch_bounds__(CSCAN) void ccl_scan_kernel(int* __restrict__ bc, int nb, int* __restrict__ n) {
  __shared__ int wsum[CSCAN / 64];
  __shared__ int carry;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += CSCAN) {
    const int i = base + tid;
    const int v = i < nb ? bc[i] : 0;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int woff = 0, total = 0;
    for (int k = 0; k < CSCAN / 64; ++k) {
      if (k < w) woff += wsum[k];
      total += wsum[k];
    }
    if (i < nb) bc[i] = carry + woff + inc - v;
    __syncthreads();
    if (tid == 0) carry += total;
    __syncthreads();
  }
  if (tid == 0) *n = carry;
}

__global__ __launch_bounds__(CB) void ccl_rank_kernel(const int* __restrict__ parent, int V,
                                                      const int* __restrict__ bo, int* __restrict__ labels) {
  __shared__ int wtot[CH / CB][CB / 64];
  const long long base = (long long)blockIdx.x * CH;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  bool flag[CH / CB];
  int pre[CH / CB];
  for (int r = 0; r < CH / CB; ++r) {
    const long long i = base + r * CB + threadIdx.x;
    flag[r] = i < V && parent[i] == (int)i;
    const unsigned long long b = __ballot(flag[r]);
    pre[r] = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[r][w] = __popcll(b);
  }
  __syncthreads();
  int run = bo[blockIdx.x] + 1;
  for (int r = 0; r < CH / CB; ++r) {
    int woff = 0, total = 0;
    for (int k = 0; k < CB / 64; ++k) {
      if (k < w) woff += wtot[r][k];
      total += wtot[r][k];
    }
    if (flag[r]) labels[base + r * CB + threadIdx.x] = run + woff + pre[r];
    run += total;
  }
}

__global__ __launch_bounds__(CB) void ccl_relabel_kernel(const int* __restrict__ parent, int V, int* labels) {
  for (long long i = blockIdx.x * (long long)CB + threadIdx.x; i < V; i += (long long)gridDim.x * CB) {
    const int p = parent[i];
    if (p < 0)
      labels[i] = 0;
    else if (p != (int)i)
      labels[i] = labels[p];  // a root's label was written by the launch before; only non-roots are written here
  }
}

// sizes[l] += voxels of label l for 1 <= l < lim
__global__ __launch_bounds__(CB) void ccl_sizes_kernel(const int* __restrict__ labels, int V, int lim,
                                                       int* __restrict__ sizes) {
  __shared__ int h[CLIM];
  for (int j = threadIdx.x; j < lim; j += CB) h[j] = 0;
  __syncthreads();
  for (long long i0 = (blockIdx.x * (long long)CB + threadIdx.x) * 8; i0 < V; i0 += (long long)gridDim.x * CB * 8) {
    int cur = 0, cnt = 0;
    for (int k = 0; k < 8 && i0 + k < V; ++k) {
      const int l = labels[i0 + k];
      if (l != cur) {
        if (cnt && cur > 0 && cur < lim) atomicAdd(&h[cur], cnt);
        cur = l;
        cnt = 0;
      }
      ++cnt;
    }
    if (cnt && cur > 0 && cur < lim) atomicAdd(&h[cur], cnt);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < lim; j += CB)
    if (h[j]) atomicAdd(&sizes[j], h[j]);
}

__global__ void ccl_pick_kernel(const int* __restrict__ sizes, const int* __restrict__ n, int lim, double min_filter,
                                int* __restrict__ rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int best = 0, bsize = 0;
  const int last = min(lim - 1, *n);
  for (int l = 1; l <= last; ++l) {
    const int s = sizes[l];
    if ((double)s < min_filter) continue;
    if (s > bsize) {  // strict: the earliest label wins a tie
      bsize = s;
      best = l;
    }
  }
  rec[R_FOUND] = best != 0;
  rec[R_LABEL] = best;
  rec[R_SIZE] = bsize;
  for (int k = 0; k < 3; ++k) {
    rec[R_LO + k] = INT_MAX;
    rec[R_HI + k] = -1;
  }
  rec[R_N] = *n;
  rec[10] = rec[11] = 0;
}

__global__ void record_init_kernel(int* __restrict__ rec) {
  const int k = threadIdx.x;
  if (k < U3D_CCL_RECORD) rec[k] = (k >= R_LO && k < R_LO + 3) ? INT_MAX : (k >= R_HI && k < R_HI + 3) ? -1 : 0;
}

// SELECT: in = labels (int), the voxels of label rec[R_LABEL] (none when rec[R_FOUND] == 0) are written to out as
// 0 / 1 and bound. NONZERO: the voxels in != 0 are bound and counted into rec[R_SIZE]; nothing is written.
enum BboxMode { SELECT, NONZERO };
template <typename T, int MODE>
__global__ __launch_bounds__(CROW) void bbox_kernel(const T* __restrict__ in, int Z, int Y, int X,
                                                    unsigned char* __restrict__ out, int* __restrict__ rec,
                                                    const int* __restrict__ gate) {
  if (gate && *gate != 0) return;
  __shared__ int s[7];  // lo z y x, hi z y x, count
  if (threadIdx.x < 7) s[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : threadIdx.x < 6 ? -1 : 0;
  __syncthreads();
  int want = 0;
  if constexpr (MODE == SELECT) want = rec[R_FOUND] ? rec[R_LABEL] : -1;
  int lz = INT_MAX, ly = INT_MAX, lx = INT_MAX, hz = -1, hy = -1, hx = -1, cnt = 0;
  const long long rows = (long long)Z * Y;
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
    const int z = (int)(r / Y), y = (int)(r - (long long)z * Y);
    for (int x = threadIdx.x; x < X; x += CROW) {
      const T v = in[r * X + x];
      bool hit;
      if constexpr (MODE == SELECT) {
        hit = (int)v == want;
        out[r * X + x] = hit ? 1 : 0;
      } else {
        hit = v != (T)0;
      }
      if (hit) {
        lz = min(lz, z), hz = max(hz, z);
        ly = min(ly, y), hy = max(hy, y);
        lx = min(lx, x), hx = max(hx, x);
        ++cnt;
      }
    }
  }
  if (cnt) {
    atomicMin(&s[0], lz), atomicMin(&s[1], ly), atomicMin(&s[2], lx);
    atomicMax(&s[3], hz), atomicMax(&s[4], hy), atomicMax(&s[5], hx);
    if constexpr (MODE == NONZERO) atomicAdd(&s[6], cnt);
  }
  __syncthreads();
  if (threadIdx.x < 3 && s[3] >= 0) atomicMin(&rec[R_LO + threadIdx.x], s[threadIdx.x]);
  if (threadIdx.x >= 3 && threadIdx.x < 6 && s[3] >= 0) atomicMax(&rec[R_HI + threadIdx.x - 3], s[threadIdx.x]);
  if (MODE == NONZERO && threadIdx.x == 6 && s[6]) atomicAdd(&rec[R_SIZE], s[6]);
}

// out = vol > t (NaN: 0); erode: AND over [z-1..z] x [y-1..y] x [x-1..x], outside false
__global__ __launch_bounds__(CROW) void body_threshold_kernel(const float* __restrict__ vol, int Z, int Y, int X,
                                                             float t, int erode, unsigned char* __restrict__ out,
                                                             const int* __restrict__ gate) {
  if (gate && *gate != 0) return;
  const long long rows = (long long)Z * Y, sy = X, sz = (long long)Y * X;
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
    const int z = (int)(r / Y), y = (int)(r - (long long)z * Y);
    const float* p = vol + r * X;
    for (int x = threadIdx.x; x < X; x += CROW) {
      bool m = p[x] > t;
      if (erode) {
        if (z == 0 || y == 0 || x == 0)
          m = false;
        else
          m = m && p[x - 1] > t && p[x - sy] > t && p[x - sy - 1] > t && p[x - sz] > t && p[x - sz - 1] > t &&
              p[x - sz - sy] > t && p[x - sz - sy - 1] > t;
      }
      out[r * X + x] = m ? 1 : 0;
    }
  }
}

// out[o][i][k] = AND (op 0) / OR (op 1) of in[o][j][k] != 0 over j in [i + lo, i + hi]; a j outside [0, n) is false
__global__ __launch_bounds__(CB) void mask_window_kernel(const unsigned char* __restrict__ in,
                                                         unsigned char* __restrict__ out, long long total, int n,
                                                         long long inner, int lo, int hi, int op,
                                                         const int* __restrict__ gate) {
  if (gate && *gate != 0) return;
  for (long long idx = blockIdx.x * (long long)CB + threadIdx.x; idx < total; idx += (long long)gridDim.x * CB) {
    const long long oi = idx / inner;
    const int i = (int)(oi % n);
    const int j0 = i + lo, j1 = i + hi;
    bool m;
    if (op == 0) {
      m = j0 >= 0 && j1 < n;
      for (int j = j0; m && j <= j1; ++j) m = in[idx + (long long)(j - i) * inner] != 0;
    } else {
      m = false;
      for (int j = max(j0, 0); !m && j <= min(j1, n - 1); ++j) m = in[idx + (long long)(j - i) * inner] != 0;
    }
    out[idx] = m ? 1 : 0;
  }
}

// ---- per-label largest component (u3d_ccl_keep_largest): one labelling of the whole code map, a voxel joining only
// neighbours of its own code, then per root its size, per label the best (size, earliest root) and a filter.
constexpr int KL = 256;  // table rows: the codes a uint8 holds

// the table behind the parents and the sizes in the workspace
struct KeepTable {
  unsigned long long best[KL];  // per label max over its roots of (size << 32) | (INT_MAX - root); 0: label absent
  int ncomp[KL], nvox[KL];
};

__device__ __forceinline__ bool keep_takes_part(unsigned char c, int num_labels) { return c != 0 && c <= num_labels; }

// ccl_local_kernel with the tile's codes next to its parents; also clears the sizes of the tile's voxels
__global__ __launch_bounds__(CB) void keep_local_kernel(const unsigned char* codes, int Z, int Y, int X, int ntx,
                                                        int nty, int num_labels, int* __restrict__ parent,
                                                        int* __restrict__ sizes) {
  __shared__ int lp[TILE];
  __shared__ unsigned char lc[TILE];
  const int t = blockIdx.x;
  const int x0 = (t % ntx) * TX, y0 = ((t / ntx) % nty) * TY, z0 = (t / (ntx * nty)) * TZ;
  for (int l = threadIdx.x; l < TILE; l += CB) {
    const int x = x0 + l % TX, y = y0 + (l / TX) % TY, z = z0 + l / (TX * TY);
    unsigned char c = 0;
    if (x < X && y < Y && z < Z) c = codes[((long long)z * Y + y) * X + x];
    if (!keep_takes_part(c, num_labels)) c = 0;
    lc[l] = c;
    lp[l] = c ? l : -1;
  }
  __syncthreads();
  for (int l = threadIdx.x; l < TILE; l += CB) local_unite_codes(lp, lc, l, l % TX, (l / TX) % TY, l / (TX * TY));
  __syncthreads();
  for (int l = threadIdx.x; l < TILE; l += CB) {
    const int x = x0 + l % TX, y = y0 + (l / TX) % TY, z = z0 + l / (TX * TY);
    if (x < X && y < Y && z < Z) {
      const long long v = ((long long)z * Y + y) * X + x;
      parent[v] = local_result(lp, l, z0, y0, x0, Y, X);
      sizes[v] = 0;
    }
  }
}

// ccl_seam_kernel on codes
__global__ __launch_bounds__(CROW) void keep_seam_kernel(const unsigned char* codes, int Z, int Y, int X,
                                                         int* __restrict__ parent) {
  const long long rows = (long long)Z * Y;
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
    const int z = (int)(r / Y), y = (int)(r - (long long)z * Y);
    const bool face = (y > 0 && y % TY == 0) || (z > 0 && z % TZ == 0);
    const int step = face ? 1 : TX;
    for (int x = face ? threadIdx.x : TX * (1 + threadIdx.x); x < X; x += step * CROW)
      seam_unite_codes(parent, codes, (int)(r * X + x), z, y, x, Y, X);
  }
}

// parent[v] = root, sizes[root] += the voxels below it and nvox[code] += the voxels of the code: each thread walks 8
// consecutive voxels and adds a run's length when the root changes (a run has one code); the codes through an LDS table
__global__ __launch_bounds__(CB) void keep_flatten_sizes_kernel(const unsigned char* codes, int V,
                                                                int* __restrict__ parent, int* __restrict__ sizes,
                                                                KeepTable* __restrict__ tab) {
  __shared__ int h[KL];
  for (int j = threadIdx.x; j < KL; j += CB) h[j] = 0;
  __syncthreads();
  for (long long i0 = (blockIdx.x * (long long)CB + threadIdx.x) * 8; i0 < V; i0 += (long long)gridDim.x * CB * 8) {
    int cur = -1, cnt = 0;
    for (int k = 0; k < 8 && i0 + k < V; ++k) {
      const int i = (int)(i0 + k);
      flatten(parent, i);
      const int r = load<AGENT>(parent + i);  // this thread's own store, or a root's own index, or -1
      if (r != cur) {
        if (cnt && cur >= 0) {
          atomicAdd(&sizes[cur], cnt);
          atomicAdd(&h[codes[cur]], cnt);
        }
        cur = r;
        cnt = 0;
      }
      ++cnt;
    }
    if (cnt && cur >= 0) {
      atomicAdd(&sizes[cur], cnt);
      atomicAdd(&h[codes[cur]], cnt);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < KL; j += CB)
    if (h[j]) atomicAdd(&tab->nvox[j], h[j]);
}

// per label the best key over its roots and the number of roots: block-reduced in LDS, one atomic per block and label
__global__ __launch_bounds__(CB) void keep_best_kernel(const unsigned char* codes, int V,
                                                       const int* __restrict__ parent, const int* __restrict__ sizes,
                                                       KeepTable* __restrict__ tab) {
  __shared__ unsigned long long b[KL];
  __shared__ int n[KL];
  for (int j = threadIdx.x; j < KL; j += CB) b[j] = 0, n[j] = 0;
  __syncthreads();
  for (long long i = blockIdx.x * (long long)CB + threadIdx.x; i < V; i += (long long)gridDim.x * CB) {
    if (parent[i] != (int)i) continue;
    const unsigned long long key = ((unsigned long long)(unsigned)sizes[i] << 32) | (unsigned)(INT_MAX - (int)i);
    const int c = codes[i];
    atomicMax(&b[c], key);
    atomicAdd(&n[c], 1);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < KL; j += CB)
    if (n[j]) {
      atomicMax(&tab->best[j], b[j]);
      atomicAdd(&tab->ncomp[j], n[j]);
    }
}

// out = codes where the voxel takes no part or hangs below its label's best root, 0 otherwise; block 0 writes the record
__global__ __launch_bounds__(CB) void keep_filter_kernel(const unsigned char* codes, int V,
                                                         const int* __restrict__ parent,
                                                         const KeepTable* __restrict__ tab, int num_labels,
                                                         unsigned char* out, int* __restrict__ record) {
  __shared__ int root[KL];
  for (int j = threadIdx.x; j < KL; j += CB) {
    const unsigned long long k = tab->best[j];
    root[j] = k ? INT_MAX - (int)(unsigned)(k & 0xffffffffu) : -1;
    if (blockIdx.x == 0 && j >= 1 && j <= num_labels) {
      int* rec = record + (j - 1) * U3D_KEEP_RECORD;
      rec[0] = tab->ncomp[j];
      rec[1] = tab->nvox[j];
      rec[2] = (int)(k >> 32);
      rec[3] = root[j];
    }
  }
  __syncthreads();
  for (long long i = blockIdx.x * (long long)CB + threadIdx.x; i < V; i += (long long)gridDim.x * CB) {
    const unsigned char c = codes[i];
    const int p = parent[i];
    out[i] = (p < 0 || p == root[c]) ? c : 0;
  }
}

static inline int row_blocks(long long rows) { return (int)std::min<long long>(CMAXB, std::max<long long>(1, rows)); }
static inline long long chunks(long long V) { return (V + CH - 1) / CH; }

}  // namespace u3d

using namespace u3d;

extern "C" void u3d_ccl_tile(int* tz, int* ty, int* tx) {
  if (tz) *tz = TZ;
  if (ty) *ty = TY;
  if (tx) *tx = TX;
}

// parents [V] int32, then the chunk counts / offsets
extern "C" long long u3d_ccl_ws_bytes(long long V) {
  if (V < 1 || V >= (1LL << 31)) return -1;
  return 4 * ((V + 3) / 4 * 4) + 4 * chunks(V) + 16;
}

extern "C" long long u3d_ccl_select_ws_bytes(void) { return 4LL * CLIM; }

extern "C" int u3d_ccl_label(const unsigned char* mask, int Z, int Y, int X, int* labels, int* n, void* ws,
                             u3d_stream_t stream) {
  U3D_REQUIRE(Z >= 1 && Y >= 1 && X >= 1, "ccl_label: bad shape %d x %d x %d", Z, Y, X);
  const long long V = (long long)Z * Y * X;
  U3D_REQUIRE(V < (1LL << 31), "ccl_label: %lld voxels: the parents are int32 (V < 2^31)", V);
  U3D_REQUIRE(mask && labels && n && ws, "ccl_label: null pointer");
  hipStream_t s = (hipStream_t)stream;
  int* parent = (int*)ws;
  int* bc = parent + (V + 3) / 4 * 4;
  const int ntx = cdiv(X, TX), nty = cdiv(Y, TY), ntz = cdiv(Z, TZ);
  const long long tiles = (long long)ntx * nty * ntz;  // <= V: fits the grid's x
  const int nb = (int)chunks(V);
  hipLaunchKernelGGL(ccl_local_kernel, dim3((unsigned)tiles), dim3(CB), 0, s, mask, Z, Y, X, ntx, nty, parent);
  hipLaunchKernelGGL(ccl_seam_kernel, dim3(row_blocks((long long)Z * Y)), dim3(CROW), 0, s, Z, Y, X, parent);
  hipLaunchKernelGGL(ccl_flatten_count_kernel, dim3(nb), dim3(CB), 0, s, parent, (int)V, bc);
  hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(CSCAN), 0, s, bc, nb, n);
  hipLaunchKernelGGL(ccl_rank_kernel, dim3(nb), dim3(CB), 0, s, (const int*)parent, (int)V, (const int*)bc, labels);
  hipLaunchKernelGGL(ccl_relabel_kernel, dim3(std::min(nb * (CH / CB), CMAXB)), dim3(CB), 0, s, (const int*)parent,
                     (int)V, labels);
  return check_launch("ccl_label");
}

extern "C" int u3d_ccl_select(const int* labels, int Z, int Y, int X, const int* n, int num_limit, double min_filter,
                              unsigned char* mask_out, int* record, void* ws, u3d_stream_t stream) {
  U3D_REQUIRE(Z >= 1 && Y >= 1 && X >= 1, "ccl_select: bad shape %d x %d x %d", Z, Y, X);
  const long long V = (long long)Z * Y * X;
  U3D_REQUIRE(V < (1LL << 31), "ccl_select: %lld voxels (V < 2^31)", V);
  U3D_REQUIRE(num_limit >= 1 && num_limit <= CLIM, "ccl_select: num_limit=%d (1..%d)", num_limit, CLIM);
  U3D_REQUIRE(min_filter == min_filter, "ccl_select: min_filter is NaN");
  U3D_REQUIRE(labels && n && mask_out && record && ws, "ccl_select: null pointer");
  hipStream_t s = (hipStream_t)stream;
  int* sizes = (int*)ws;
  U3D_HIP(hipMemsetAsync(sizes, 0, 4 * CLIM, s));
  const int gb = (int)std::min<long long>(CMAXB, (V + CB * 8 - 1) / (CB * 8));
  hipLaunchKernelGGL(ccl_sizes_kernel, dim3(gb), dim3(CB), 0, s, labels, (int)V, num_limit, sizes);
  hipLaunchKernelGGL(ccl_pick_kernel, dim3(1), dim3(64), 0, s, (const int*)sizes, n, num_limit, min_filter, record);
  hipLaunchKernelGGL((bbox_kernel<int, SELECT>), dim3(row_blocks((long long)Z * Y)), dim3(CROW), 0, s, labels, Z, Y, X,
                     mask_out, record, (const int*)nullptr);
  return check_launch("ccl_select");
}

// parents [V] int32, sizes [V] int32, then the table
extern "C" long long u3d_ccl_keep_largest_ws_bytes(long long V) {
  if (V < 1 || V >= (1LL << 31)) return -1;
  return 8 * V + (long long)sizeof(KeepTable);
}

extern "C" int u3d_ccl_keep_largest(const unsigned char* codes, int Z, int Y, int X, int num_labels,
                                    unsigned char* out, int* record, void* ws, u3d_stream_t stream) {
  U3D_REQUIRE(Z >= 1 && Y >= 1 && X >= 1, "ccl_keep_largest: bad shape %d x %d x %d", Z, Y, X);
  const long long V = (long long)Z * Y * X;
  U3D_REQUIRE(V < (1LL << 31), "ccl_keep_largest: %lld voxels: the parents are int32 (V < 2^31)", V);
  U3D_REQUIRE(num_labels >= 1 && num_labels < KL, "ccl_keep_largest: num_labels=%d (1..%d)", num_labels, KL - 1);
  U3D_REQUIRE(codes && out && record && ws, "ccl_keep_largest: null pointer");
  U3D_REQUIRE(((uintptr_t)ws & 7) == 0, "ccl_keep_largest: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int* parent = (int*)ws;
  int* sizes = parent + V;
  KeepTable* tab = (KeepTable*)(sizes + V);
  U3D_HIP(hipMemsetAsync(tab, 0, sizeof(KeepTable), s));
  const int ntx = cdiv(X, TX), nty = cdiv(Y, TY), ntz = cdiv(Z, TZ);
  const long long tiles = (long long)ntx * nty * ntz;  // <= V: fits the grid's x
  const int gb8 = (int)std::min<long long>(CMAXB, (V + CB * 8 - 1) / (CB * 8));
  const int gb = (int)std::min<long long>(CMAXB, (V + CB - 1) / CB);
  hipLaunchKernelGGL(keep_local_kernel, dim3((unsigned)tiles), dim3(CB), 0, s, codes, Z, Y, X, ntx, nty, num_labels,
                     parent, sizes);
  hipLaunchKernelGGL(keep_seam_kernel, dim3(row_blocks((long long)Z * Y)), dim3(CROW), 0, s, codes, Z, Y, X, parent);
  hipLaunchKernelGGL(keep_flatten_sizes_kernel, dim3(gb8), dim3(CB), 0, s, codes, (int)V, parent, sizes, tab);
  hipLaunchKernelGGL(keep_best_kernel, dim3(gb), dim3(CB), 0, s, codes, (int)V, (const int*)parent,
                     (const int*)sizes, tab);
  hipLaunchKernelGGL(keep_filter_kernel, dim3(gb), dim3(CB), 0, s, codes, (int)V, (const int*)parent,
                     (const KeepTable*)tab, num_labels, out, record);
  return check_launch("ccl_keep_largest");
}

extern "C" int u3d_body_threshold(const float* vol, int Z, int Y, int X, float t, int erode, unsigned char* out,
                                  const int* gate, u3d_stream_t stream) {
  U3D_REQUIRE(vol && out && Z >= 1 && Y >= 1 && X >= 1, "body_threshold: bad args");
  hipLaunchKernelGGL(body_threshold_kernel, dim3(row_blocks((long long)Z * Y)), dim3(CROW), 0, (hipStream_t)stream,
                     vol, Z, Y, X, t, erode, out, gate);
  return check_launch("body_threshold");
}

extern "C" int u3d_mask_window_axis(const unsigned char* in, unsigned char* out, long long outer, int n,
                                    long long inner, int lo, int hi, int op, const int* gate, u3d_stream_t stream) {
  U3D_REQUIRE(in && out && in != out, "mask_window_axis: null or aliased pointers");
  U3D_REQUIRE(outer >= 1 && n >= 1 && inner >= 1 && lo <= hi && (op == 0 || op == 1), "mask_window_axis: bad args");
  U3D_REQUIRE(lo > -(1 << 20) && hi < (1 << 20), "mask_window_axis: window [%d, %d] too wide", lo, hi);
  const long long total = outer * n * inner;
  const int gb = (int)std::min<long long>(CMAXB * 4, (total + CB - 1) / CB);
  hipLaunchKernelGGL(mask_window_kernel, dim3(gb), dim3(CB), 0, (hipStream_t)stream, in, out, total, n, inner, lo, hi,
                     op, gate);
  return check_launch("mask_window_axis");
}

extern "C" int u3d_nonzero_bbox(const void* x, int dtype, int Z, int Y, int X, int* record, int accumulate,
                                const int* gate, u3d_stream_t stream) {
  U3D_REQUIRE(x && record && Z >= 1 && Y >= 1 && X >= 1, "nonzero_bbox: bad args");
  U3D_REQUIRE((long long)Z * Y * X < (1LL << 31), "nonzero_bbox: the count is int32 (V < 2^31)");
  U3D_REQUIRE(dtype >= 0 && dtype <= 2, "nonzero_bbox: dtype=%d (0 uint8, 1 float32, 2 int32)", dtype);
  hipStream_t s = (hipStream_t)stream;
  if (!accumulate) hipLaunchKernelGGL(record_init_kernel, dim3(1), dim3(64), 0, s, record);
  const dim3 g(row_blocks((long long)Z * Y)), b(CROW);
  unsigned char* none = nullptr;
  if (dtype == 0)
    hipLaunchKernelGGL((bbox_kernel<unsigned char, NONZERO>), g, b, 0, s, (const unsigned char*)x, Z, Y, X, none, record,
                       gate);
  else if (dtype == 1)
    hipLaunchKernelGGL((bbox_kernel<float, NONZERO>), g, b, 0, s, (const float*)x, Z, Y, X, none, record, gate);
  else
    hipLaunchKernelGGL((bbox_kernel<int, NONZERO>), g, b, 0, s, (const int*)x, Z, Y, X, none, record, gate);
  return check_launch("nonzero_bbox");
}
