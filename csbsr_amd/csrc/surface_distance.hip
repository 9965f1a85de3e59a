// Surface-distance metrics of the evaluation loop (model/engine/inference.py:293-336 over the vendored surface_distance package): for one
// image and every threshold t_j, the distances between the contour of gt = (mask > 0.5) and the contour of pred_j = (pred - t_j > 0), as
// INTEGER counts keyed by (squared distance, contour-length class).  HD / MSD are an fp64 function of those counts (utils/estimate_metrics.py).
//
// Everything lives on the corner grid (H+1) x (W+1): corner (i, x) sees the pixels (i-1, x-1), (i-1, x), (i, x-1), (i, x) (zero outside the
// image), code = 8 a + 4 b + 2 c + d, and is a border corner when its four pixels are not all equal.  Its contour length is the
// marching-squares length of the code, one of four values, so a class index 0..3 is carried instead of a float:
//   one or three pixels set -> 1 (one diagonal half-cell segment), two adjacent -> 2 (one straight segment), two opposite -> 3 (two diagonals).
// A pixel's prediction exceeds exactly the first k thresholds (ascending; the binary search of csbsr_iou_sweep, bit-identical to
// `pred - t > 0`), so ONE byte plane of levels k holds all the thresholded masks: pred_j = (k > j), and a corner is a border corner of pred_j
// for  min k <= j < max k  of its four pixels.
//
//   prepare: levels + gt bytes, border-corner counts (gt; pred as a difference array over j), the exact squared EDT to the gt contour
//            (column scan, then the lower envelope over a row held in LDS: edt_cols_kernel / edt_rows_kernel of image_ops.hip in integers).
//   gather : pred -> gt   every pred_j border corner looks its distance up in that one gt map;
//            gt -> pred   the column scan runs per threshold (uint16 planes, a chunk of thresholds at a time), the row pass is evaluated
//                         ONLY at the gt border corners of rows that have any -- a few thousand queries per plane instead of (H+1)(W+1).
//            Both insert  key = d^2 * 4 + class  into a per-(threshold, direction) open-addressing table with integer atomics (atomicCAS on
//            the key, atomicAdd on the count).  The slot a key lands in depends on arrival order; the (key, count) SET does not, and the
//            finish sorts it -- no floating-point atomics, results are run-to-run bit-identical.  A last kernel compacts the occupied slots
//            into rows (table, key, count), so the host reads the few thousand distinct bins, not the tables.
#include "common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define SD_BIG 0x3FFFFFFF        // "no border corner in this column": BIG + dx^2 (dx < 2^13) stays below 2^31
#define SD_NONE 0xFFFF           // the same in a uint16 column-scan plane
#define SD_MAX_SIDE 8191         // corner rows of <= 8192 ints in LDS; d^2 <= 2 * 8192^2 = 2^27, key < 2^29

static inline int sd_grid(long work, int block, int cap = 16384) {
  long b = (work + block - 1) / block;
  if (b < 1) b = 1;
  return (int)(b > cap ? cap : b);
}

__device__ __forceinline__ int sd_px(const uint8_t* p, int H, int W, int y, int x) {
  return ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? (int)p[(long)y * W + x] : 0;
}
// contour-length class of a neighbour code
__device__ __forceinline__ int sd_class(int code) {
  const int n = __popc(code);
  if (n == 0 || n == 4) return 0;
  if (n != 2) return 1;
  return (code == 6 || code == 9) ? 3 : 2;
}
__device__ __forceinline__ int sd_gt_code(const uint8_t* gt, int H, int W, int i, int x) {
  return 8 * sd_px(gt, H, W, i - 1, x - 1) + 4 * sd_px(gt, H, W, i - 1, x) + 2 * sd_px(gt, H, W, i, x - 1) + sd_px(gt, H, W, i, x);
}

// ------------------------------------------------------------------------------------------- prepare
__global__ __launch_bounds__(256) void sd_levels_kernel(const float* pred, const float* mask, const float* ths, int T, long hw, uint8_t* lvl,
                                                        uint8_t* gt) {
  __shared__ float sth[256];
  for (int i = threadIdx.x; i < T; i += 256) sth[i] = ths[i];
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
    const float p = pred[i];
    int lo = 0, hi = T;                  // number of thresholds strictly below p
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (p - sth[mid] > 0.f) lo = mid + 1; else hi = mid; }
    lvl[i] = (uint8_t)lo;
    gt[i] = mask[i] > 0.5f ? 1 : 0;
  }
}
// counts[0] = gt border corners; counts[1 + k] = difference array of the pred border-corner counts (+1 at min k, -1 at max k: the count for
// threshold j is the prefix sum up to j); rowflag[i] = 1 where corner row i holds a gt border corner
__global__ __launch_bounds__(256) void sd_count_kernel(const uint8_t* lvl, const uint8_t* gt, int H, int W, int T, int* counts, int* rowflag) {
  __shared__ int sc[258];
  const int Wc = W + 1;
  const long total = (long)(H + 1) * Wc;
  for (int i = threadIdx.x; i < T + 2; i += 256) sc[i] = 0;
  __syncthreads();
  for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < total; c += (long)gridDim.x * 256) {
    const int i = (int)(c / Wc), x = (int)(c - (long)i * Wc);
    const int code = sd_gt_code(gt, H, W, i, x);
    if (code != 0 && code != 15) { atomicAdd(&sc[0], 1); rowflag[i] = 1; }
    const int a = sd_px(lvl, H, W, i - 1, x - 1), b = sd_px(lvl, H, W, i - 1, x), cc = sd_px(lvl, H, W, i, x - 1), d = sd_px(lvl, H, W, i, x);
    const int kmin = min(min(a, b), min(cc, d)), kmax = max(max(a, b), max(cc, d));
    if (kmin < kmax) { atomicAdd(&sc[1 + kmin], 1); atomicAdd(&sc[1 + kmax], -1); }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T + 2; i += 256)
    if (sc[i]) atomicAdd(&counts[i], sc[i]);
}

// Column scan of the EDT to the border corners of plane jj (one thread per (plane, corner column)): g[i][x] = vertical distance from corner
// (i, x) to the nearest border corner of column x, SD_NONE if the column has none.  j0 < 0: the gt plane (bit = gt byte); else plane jj is
// threshold j0 + jj (bit = level > j) and planes whose gt -> pred table is absent (cap == 0: a degenerate cell) are skipped.
__global__ __launch_bounds__(64) void sd_cols_kernel(const uint8_t* src, int H, int W, int j0, int nj, const int* cap, uint16_t* g) {
  const int Hc = H + 1, Wc = W + 1;
  const long total = (long)nj * Wc;
  for (long t = (long)blockIdx.x * 64 + threadIdx.x; t < total; t += (long)gridDim.x * 64) {
    const int jj = (int)(t / Wc), x = (int)(t - (long)jj * Wc);
    if (j0 >= 0 && cap[2 * jj] == 0) continue;
    const int j = j0 < 0 ? 0 : j0 + jj;      // gt bytes are 0 / 1: bit = byte > 0
    uint16_t* gp = g + (long)jj * Hc * Wc + x;
    int pa = 0, pb = 0;                      // bits of the pixel row above the corner row
    int d = SD_NONE;
    for (int i = 0; i < Hc; ++i) {
      const int ca = sd_px(src, H, W, i, x - 1) > j, cb = sd_px(src, H, W, i, x) > j;
      const int s = pa + pb + ca + cb;
      d = (s != 0 && s != 4) ? 0 : (d >= SD_NONE ? SD_NONE : d + 1);
      gp[(long)i * Wc] = (uint16_t)d;
      pa = ca; pb = cb;
    }
    d = SD_NONE;
    for (int i = Hc - 1; i >= 0; --i) {
      const int cur = gp[(long)i * Wc];
      d = cur == 0 ? 0 : (d >= SD_NONE ? SD_NONE : d + 1);
      if (d < cur) gp[(long)i * Wc] = (uint16_t)d;
    }
  }
}

// min over x' of sq[x'] + (x - x')^2 : blocks of 32 columns, their minima as lower bounds (edt_rows_kernel's search, in integers)
__device__ __forceinline__ int sd_row_min(const int* sq, const int* bmin, int nb, int Wc, int x) {
  int best = sq[x];
  const int bx = x >> 5;
  auto scan = [&](int b) {
    const int x1 = min(Wc, 32 * b + 32);
    for (int xx = 32 * b; xx < x1; ++xx) {
      const int d = x - xx;
      best = min(best, sq[xx] + d * d);
    }
  };
  if (bmin[bx] < best) scan(bx);
  for (int d = 1; d < nb; ++d) {
    const int bl = bx - d, br = bx + d;
    const int gl = x - (32 * bl + 31), gr = 32 * br - x;       // gap to the nearest column of the block (>= 1)
    const bool lin = bl >= 0 && gl * gl < best, rin = br < nb && gr * gr < best;
    if (!lin && !rin) break;                                   // the gaps only grow and ``best`` only shrinks
    if (lin && bmin[bl] + gl * gl < best) scan(bl);
    if (rin && bmin[br] + gr * gr < best) scan(br);
  }
  return best;
}
__device__ __forceinline__ void sd_stage_row(const uint16_t* gp, int Wc, int nb, int* sq, int* bmin) {
  for (int x = threadIdx.x; x < Wc; x += 256) { const int v = gp[x]; sq[x] = v >= SD_NONE ? SD_BIG : v * v; }
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += 256) {
    int m = SD_BIG;
    const int x1 = min(Wc, 32 * b + 32);
    for (int x = 32 * b; x < x1; ++x) m = min(m, sq[x]);
    bmin[b] = m;
  }
  __syncthreads();
}
// dense row pass (the gt plane, once per image): d2[i][x] = squared distance from corner (i, x) to the nearest gt border corner
__global__ __launch_bounds__(256) void sd_rows_dense_kernel(const uint16_t* g, int Wc, int* d2) {
  extern __shared__ int srow[];          // [Wc] squares, then [nb] block minima
  const int nb = (Wc + 31) >> 5;
  const long row = blockIdx.x;
  sd_stage_row(g + row * Wc, Wc, nb, srow, srow + Wc);
  for (int x = threadIdx.x; x < Wc; x += 256) d2[row * Wc + x] = sd_row_min(srow, srow + Wc, nb, Wc, x);
}

// ------------------------------------------------------------------------------------------- gather
// count of ``key`` += 1 in the table [off, off + cap) (cap a power of two, > the number of distinct keys; keys start at -1)
__device__ __forceinline__ void sd_insert(int* keys, unsigned* cnts, int off, int cap, int key, int* err) {
  unsigned h = (unsigned)key * 2654435761u;
  h = (h ^ (h >> 15)) & (unsigned)(cap - 1);
  for (int probe = 0; probe < cap; ++probe) {
    const int old = atomicCAS(&keys[off + h], -1, key);
    if (old == -1 || old == key) { atomicAdd(&cnts[off + h], 1u); return; }
    h = (h + 1) & (unsigned)(cap - 1);
  }
  atomicAdd(err, 1);                     // table full: the caller sized it wrongly
}
// pred -> gt: one pass over the corner grid serves every threshold of the chunk
__global__ __launch_bounds__(256) void sd_gather_p2g_kernel(const uint8_t* lvl, const int* dgt, int H, int W, int j0, int nj, const int* off,
                                                            const int* cap, int* keys, unsigned* cnts, int* err) {
  const int Wc = W + 1;
  const long total = (long)(H + 1) * Wc;
  for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < total; c += (long)gridDim.x * 256) {
    const int i = (int)(c / Wc), x = (int)(c - (long)i * Wc);
    const int a = sd_px(lvl, H, W, i - 1, x - 1), b = sd_px(lvl, H, W, i - 1, x), cc = sd_px(lvl, H, W, i, x - 1), d = sd_px(lvl, H, W, i, x);
    const int kmin = min(min(a, b), min(cc, d)), kmax = max(max(a, b), max(cc, d));
    const int lo = max(kmin, j0), hi = min(kmax, j0 + nj);
    if (lo >= hi) continue;
    const int d2 = dgt[c];
    for (int j = lo; j < hi; ++j) {
      const int t = 2 * (j - j0) + 1;
      if (cap[t] == 0) continue;
      const int code = 8 * (a > j) + 4 * (b > j) + 2 * (cc > j) + (d > j);
      sd_insert(keys, cnts, off[t], cap[t], d2 * 4 + sd_class(code), err);
    }
  }
}
// gt -> pred: workgroup = (corner row i, plane jj); the row pass at the gt border corners of the row only
__global__ __launch_bounds__(256) void sd_gather_g2p_kernel(const uint8_t* gt, const int* rowflag, const uint16_t* g, int H, int W, int nj,
                                                            const int* off, const int* cap, int* keys, unsigned* cnts, int* err) {
  extern __shared__ int srow[];
  const int i = blockIdx.x, jj = blockIdx.y;
  const int t = 2 * jj;
  if (!rowflag[i] || cap[t] == 0) return;          // uniform over the workgroup
  const int Hc = H + 1, Wc = W + 1, nb = (Wc + 31) >> 5;
  sd_stage_row(g + ((long)jj * Hc + i) * Wc, Wc, nb, srow, srow + Wc);
  const int o = off[t], cp = cap[t];
  for (int x = threadIdx.x; x < Wc; x += 256) {
    const int code = sd_gt_code(gt, H, W, i, x);
    if (code == 0 || code == 15) continue;
    sd_insert(keys, cnts, o, cp, sd_row_min(srow, srow + Wc, nb, Wc, x) * 4 + sd_class(code), err);
  }
}

// occupied slots of every table of the chunk -> rows (table index, key, count), in arrival order (the finish sorts them)
__global__ __launch_bounds__(256) void sd_compact_kernel(const int* off, const int* cap, const int* keys, const unsigned* cnts, int* rows,
                                                         int max_rows, int* meta) {
  const int t = blockIdx.y, o = off[t], cp = cap[t];
  const int lane = threadIdx.x & 63;
  for (int base = blockIdx.x * 256; base < cp; base += gridDim.x * 256) {          // uniform trip count: one atomic per wave and step
    const int sidx = base + threadIdx.x;
    const int k = sidx < cp ? keys[o + sidx] : -1;
    const unsigned long long m = __ballot(k != -1);
    if (m == 0) continue;
    int r = 0;
    if (lane == __ffsll((long long)m) - 1) r = atomicAdd(&meta[1], __popcll(m));
    r = __shfl(r, __ffsll((long long)m) - 1, 64) + __popcll(m & ((1ull << lane) - 1));
    if (k == -1) continue;
    if (r >= max_rows) { atomicAdd(&meta[0], 1); continue; }
    rows[3 * (long)r] = t; rows[3 * (long)r + 1] = k; rows[3 * (long)r + 2] = (int)cnts[o + sidx];
  }
}

static int sd_check_size(int H, int W, const char* what) {
  CSBSR_CHECK(H >= 1 && W >= 1 && H <= SD_MAX_SIDE && W <= SD_MAX_SIDE, "%s: %d x %d is outside 1 .. %d per side (int32 keys d^2 * 4 + class, "
              "corner rows in LDS)", what, H, W, SD_MAX_SIDE);
  return 0;
}

extern "C" int csbsr_surface_prepare(const float* pred, const float* mask, const float* thresholds, int32_t H, int32_t W, int32_t T, uint8_t* lvl,
                                     uint8_t* gt, int32_t* counts /* [T+2] zeroed */, int32_t* rowflag /* [H+1] zeroed */,
                                     uint16_t* gcol /* [(H+1)(W+1)] */, int32_t* dgt /* [(H+1)(W+1)] */, csbsr_stream_t s) {
  CSBSR_CHECK(pred && mask && thresholds && lvl && gt && counts && rowflag && gcol && dgt, "surface_prepare: null");
  CSBSR_CHECK(T >= 1 && T <= 255, "surface_prepare: 1 .. 255 thresholds (levels are bytes), got %d", T);
  if (sd_check_size(H, W, "surface_prepare")) return 1;
  const int Hc = H + 1, Wc = W + 1;
  hipStream_t st = ST(s);
  hipLaunchKernelGGL(sd_levels_kernel, dim3(sd_grid((long)H * W, 256)), dim3(256), 0, st, pred, mask, thresholds, T, (long)H * W, lvl, gt);
  hipLaunchKernelGGL(sd_count_kernel, dim3(sd_grid((long)Hc * Wc, 256, 2048)), dim3(256), 0, st, lvl, gt, H, W, T, counts, rowflag);
  hipLaunchKernelGGL(sd_cols_kernel, dim3(sd_grid(Wc, 64)), dim3(64), 0, st, gt, H, W, -1, 1, nullptr, gcol);
  hipLaunchKernelGGL(sd_rows_dense_kernel, dim3(Hc), dim3(256), (size_t)(Wc + (Wc + 31) / 32) * sizeof(int), st, gcol, Wc, dgt);
  CSBSR_LAUNCH_CHECK("csbsr_surface_prepare");
  return 0;
}

extern "C" int csbsr_surface_gather(const uint8_t* lvl, const uint8_t* gt, const int32_t* dgt, const int32_t* rowflag, int32_t H, int32_t W,
                                    int32_t j0, int32_t nj, uint16_t* gcol /* [nj][(H+1)(W+1)] */, const int32_t* tab_off /* [nj][2] */,
                                    const int32_t* tab_cap /* [nj][2] */, int32_t* tab_keys /* -1 */, uint32_t* tab_cnt /* 0 */,
                                    int32_t max_cap, int32_t* rows /* [max_rows][3] */, int32_t max_rows, int32_t* meta /* [2] zeroed */,
                                    csbsr_stream_t s) {
  CSBSR_CHECK(lvl && gt && dgt && rowflag && gcol && tab_off && tab_cap && tab_keys && tab_cnt && rows && meta, "surface_gather: null");
  CSBSR_CHECK(max_cap >= 1 && max_rows >= 1, "surface_gather: empty tables");
  int32_t* err = meta;
  CSBSR_CHECK(j0 >= 0 && nj >= 1 && j0 + nj <= 255 && nj <= 65535, "surface_gather: bad threshold range %d + %d", j0, nj);
  if (sd_check_size(H, W, "surface_gather")) return 1;
  const int Hc = H + 1, Wc = W + 1;
  hipStream_t st = ST(s);
  hipLaunchKernelGGL(sd_gather_p2g_kernel, dim3(sd_grid((long)Hc * Wc, 256)), dim3(256), 0, st, lvl, dgt, H, W, j0, nj, tab_off, tab_cap, tab_keys,
                     tab_cnt, err);
  hipLaunchKernelGGL(sd_cols_kernel, dim3(sd_grid((long)nj * Wc, 64)), dim3(64), 0, st, lvl, H, W, j0, nj, tab_cap, gcol);
  hipLaunchKernelGGL(sd_gather_g2p_kernel, dim3(Hc, nj), dim3(256), (size_t)(Wc + (Wc + 31) / 32) * sizeof(int), st, gt, rowflag, gcol, H, W, nj,
                     tab_off, tab_cap, tab_keys, tab_cnt, err);
  hipLaunchKernelGGL(sd_compact_kernel, dim3(sd_grid(max_cap, 256, 1024), 2 * nj), dim3(256), 0, st, tab_off, tab_cap, tab_keys, tab_cnt, rows,
                     max_rows, meta);
  CSBSR_LAUNCH_CHECK("csbsr_surface_gather");
  return 0;
}
