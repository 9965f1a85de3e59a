// Tolerance-matched precision / recall counts of the evaluation loop for every threshold t_j in ONE pass over the map.
//
// A pixel's prediction exceeds exactly the first k thresholds (ascending; the binary search of csbsr_iou_sweep, bit-identical to
// `pred - t > 0`, NaN -> 0), so one plane of levels k holds all the thresholded masks: pred_j = (k > j), and the masks are nested.  With
// gt = (mask > 0.5), the disk D = {(dy, dx): dy^2 + dx^2 <= tol2}, and zero (level and gt) outside the image:
//   near(p) = any gt pixel in p + D          m(p) = max level in p + D
//   n_pred[j]  = #{level > j}                a predicted pixel of pred_j
//   tp_pred[j] = #{level > j and near}       ... that has a gt pixel within the tolerance
//   tp_gt[j]   = #{gt and m > j}             a gt pixel that has a pixel of pred_j within the tolerance
//   n_gt       = #gt
// i.e. three histograms -- of level over all pixels, of level over the near pixels, of m over the gt pixels -- and their suffix sums.
//
//   pr_hist_kernel : a workgroup walks 32 x 64 output tiles of one image.  Per tile it builds level | gt << 8 of the tile plus a halo of
//                    R = floor(sqrt(tol2)) as uint16 cells in LDS straight from pred / mask (neither plane ever exists in global memory),
//                    then scans the disk row by row (half-width floor(sqrt(tol2 - dy^2)) per row offset) -- only at pixels with level > 0
//                    (near) or gt (m), and not at all when the tile plus halo holds no gt pixel.  The histograms live in LDS for all the
//                    tiles of the workgroup (integer atomics; bin 0 of the two level histograms is never read and never written), and go
//                    out with one global integer atomicAdd per non-zero bin.
//   pr_finish_kernel: suffix sums -> counts [N][4][T], one lane per threshold.
// Integer atomics only: the counts do not depend on arrival order and are run-to-run identical.
#include "common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define PR_TH 32
#define PR_TW 64
#define PR_MAXR 16                       // tol2 <= 256
#define PR_MAX_SIDE 8192                 // 8192^2 = 2^26 pixels: every count fits an int32
#define PR_BINS 256                      // T + 1 <= 256

__global__ __launch_bounds__(256) void pr_hist_kernel(const float* pred, const float* mask, const float* ths, int H, int W, int T, int tol2,
                                                      int R, int tiles_x, int ntiles, unsigned* hist) {
  __shared__ uint16_t cell[(PR_TH + 2 * PR_MAXR) * (PR_TW + 2 * PR_MAXR)];       // level | gt << 8, zero outside the image
  __shared__ unsigned sh[3 * PR_BINS];                                         // level (all), level (near), m (gt)
  __shared__ float sth[PR_BINS];
  __shared__ int shw[2 * PR_MAXR + 1];                                         // half-width of the disk at row offset dy = i - R
  __shared__ int sflag[2];                                                     // "this tile plus halo holds a gt pixel", alternating
  const int tid = threadIdx.x, n = blockIdx.y;
  const int PH = PR_TH + 2 * R, PW = PR_TW + 2 * R;
  const long base = (long)n * H * W;
  for (int i = tid; i < 3 * PR_BINS; i += 256) sh[i] = 0;
  for (int i = tid; i < T; i += 256) sth[i] = ths[i];
  if (tid < 2 * R + 1) {
    const int dy = tid - R, rem = tol2 - dy * dy;
    int w = (int)sqrtf((float)rem);
    while (w * w > rem) --w;
    while ((w + 1) * (w + 1) <= rem) ++w;
    shw[tid] = w;
  }
  if (tid < 2) sflag[tid] = 0;
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6;
  int cur = 0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x, cur ^= 1) {
    const int y0 = (t / tiles_x) * PR_TH, x0 = (t % tiles_x) * PR_TW;
    int anyg = 0;
    for (int idx = tid; idx < PH * PW; idx += 256) {
      const int pr = idx / PW, pc = idx - pr * PW;
      const int y = y0 - R + pr, x = x0 - R + pc;
      int v = 0;
      if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
        const long o = base + (long)y * W + x;
        const float p = pred[o];
        int lo = 0, hi = T;              // number of thresholds strictly below p
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (p - sth[mid] > 0.f) lo = mid + 1; else hi = mid; }
        const int g = mask[o] > 0.5f ? 1 : 0;
        v = lo | (g << 8);
        anyg |= g;
      }
      cell[idx] = (uint16_t)v;
    }
    if (anyg) sflag[cur] = 1;
    __syncthreads();
    if (tid == 0) sflag[cur ^ 1] = 0;     // the next tile's flag: read only after the next barrier
    const int has_gt = sflag[cur];
    for (int k = 0; k < PR_TH / 4; ++k) {
      const int r = wv + 4 * k;
      const uint16_t* c0 = cell + (r + R) * PW + lane + R;
      const int v = *c0;
      const int lv = v & 255, g = v >> 8;
      // level histogram: a wave whose 64 pixels share one level (flat regions of the map) adds once
      const int l0 = __builtin_amdgcn_readfirstlane(lv);
      if (__all(lv == l0)) {
        if (l0 > 0 && lane == 0) atomicAdd(&sh[l0], 64u);
      } else if (lv > 0) {
        atomicAdd(&sh[lv], 1u);
      }
      if (has_gt && (lv > 0 || g)) {
        int any = 0, mx = 0;
        for (int dy = -R; dy <= R; ++dy) {
          const int w = shw[dy + R];
          const uint16_t* row = c0 + dy * PW;
          for (int dx = -w; dx <= w; ++dx) {
            const int u = row[dx];
            any |= u;
            mx = max(mx, u & 255);
          }
        }
        if (lv > 0 && (any >> 8)) atomicAdd(&sh[PR_BINS + lv], 1u);
        if (g) atomicAdd(&sh[2 * PR_BINS + mx], 1u);
      }
    }
    __syncthreads();                      // the cells are rewritten by the next tile
  }
  unsigned* hn = hist + (long)n * 3 * (T + 1);
  for (int i = tid; i < 3 * (T + 1); i += 256) {
    const unsigned c = sh[(i / (T + 1)) * PR_BINS + i % (T + 1)];
    if (c) atomicAdd(&hn[i], c);
  }
}

// one workgroup per image; lane j sums the bins above j of the three histograms out of LDS (T^2 / 2 reads of LDS instead of one lane walking
// global memory)
__global__ __launch_bounds__(256) void pr_finish_kernel(const unsigned* hist, int T, int* counts) {
  __shared__ unsigned sh[3 * PR_BINS];
  const int n = blockIdx.x;
  const unsigned* h = hist + (long)n * 3 * (T + 1);
  for (int i = threadIdx.x; i < 3 * (T + 1); i += 256) sh[(i / (T + 1)) * PR_BINS + i % (T + 1)] = h[i];
  __syncthreads();
  int* c = counts + (long)n * 4 * T;
  for (int j = threadIdx.x; j < T; j += 256) {
    unsigned s0 = 0, s1 = 0, s2 = 0, ngt = 0;
    for (int k = 0; k <= T; ++k) {
      const unsigned g = sh[2 * PR_BINS + k];
      ngt += g;
      if (k > j) { s0 += sh[k]; s1 += sh[PR_BINS + k]; s2 += g; }
    }
    c[j] = (int)s0; c[T + j] = (int)s1; c[2 * T + j] = (int)s2; c[3 * T + j] = (int)ngt;
  }
}

extern "C" int csbsr_pr_sweep(const float* pred, const float* mask, const float* thresholds, int32_t N, int32_t H, int32_t W, int32_t T,
                              int32_t tol2, uint32_t* hist /* [N][3][T+1] zeroed */, int32_t* counts /* [N][4][T] */, csbsr_stream_t s) {
  CSBSR_CHECK(pred && mask && thresholds && hist && counts, "pr_sweep: null");
  CSBSR_CHECK(N >= 1 && N <= 65535, "pr_sweep: 1 .. 65535 images, got %d", N);
  CSBSR_CHECK(T >= 1 && T <= 255, "pr_sweep: 1 .. 255 thresholds (levels are bytes), got %d", T);
  CSBSR_CHECK(H >= 1 && W >= 1 && H <= PR_MAX_SIDE && W <= PR_MAX_SIDE, "pr_sweep: %d x %d is outside 1 .. %d per side (int32 counts)", H, W,
              PR_MAX_SIDE);
  CSBSR_CHECK(tol2 >= 0 && tol2 <= PR_MAXR * PR_MAXR, "pr_sweep: squared tolerance %d is outside 0 .. %d", tol2, PR_MAXR * PR_MAXR);
  int R = 0;
  while ((R + 1) * (R + 1) <= tol2) ++R;
  const int tiles_x = (W + PR_TW - 1) / PR_TW, ntiles = tiles_x * ((H + PR_TH - 1) / PR_TH);
  int per = (4096 + N - 1) / N;          // workgroups per image: a few thousand in all, each keeps its histograms over its tiles
  if (per > ntiles) per = ntiles;
  hipLaunchKernelGGL(pr_hist_kernel, dim3(per, N), dim3(256), 0, ST(s), pred, mask, thresholds, H, W, T, tol2, R, tiles_x, ntiles, hist);
  hipLaunchKernelGGL(pr_finish_kernel, dim3(N), dim3(256), 0, ST(s), hist, T, counts);
  CSBSR_LAUNCH_CHECK("csbsr_pr_sweep");
  return 0;
}
