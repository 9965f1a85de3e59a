// Local crack width: the exact squared distance from every centerline pixel to the nearest background pixel of its plane.
//
// A plane is binarised as in skel_init_kernel and ccl_local_kernel: a pixel is in the region R iff  x - threshold > 0  in fp32 (NaN -> not
// in R).  The background is the pixels OF THE PLANE that are not in R: nothing outside the plane, in the next plane of the batch or in the
// padding bits of a packed row is background, so a crack that runs off the image is not narrowed by the border.  For a skeleton pixel p
//   d2(p) = min(r^2 + 1, min over background q of |p - q|^2)          (integers; r^2 + 1 = "wider than the search radius", saturated)
// and d2 = 0 where the skeleton is 0.  A skeleton pixel that is itself background gets 0 as well (legal input; it counts in bin 0).
//
//   width_kernel : a workgroup owns WD_TH x WD_TW pixels.
//     1. It compacts the tile's skeleton pixels into an LDS list (ballot + one LDS atomic per wave) and writes d2 = 0 at every other pixel
//        of the tile.  A tile without skeleton pixels -- nearly all of a crack map -- ends here, having read one byte and written one
//        int32 per pixel.
//     2. It builds the bit-packed region of the tile plus a halo of r rows and ceil(r / 32) words per side in LDS, straight from the fp32
//        plane with wave ballots (the way pr_sweep builds its halo).  Positions outside the plane enter as SET.  At r = 128 the halo spans
//        two tiles above and below and one beside: 320 rows x 12 words.
//     3. A lane takes one skeleton pixel and walks the rows dy = 0, -1, +1, -2, +2, ...  In a row the nearest clear bit to the left and to the
//        right is found with count-leading / count-trailing zeros on the inverted words, a word at a time, and only while a word can
//        still hold a closer pixel.  The walk stops as soon as dy^2 reaches the best so far (which starts at r^2 + 1, so dy <= r and
//        every row and word it touches lies inside the halo).
//     4. d2 is stored and counted: the bins below WD_LBINS and the saturated bin in an LDS histogram that the workgroup flushes with one
//        global integer atomic per bin it filled, the bins between with a global atomic each.  (One global atomic per pixel serialises on
//        the bin of d2 = 1 when a plane is thresholded noise: measured 17.0 ms against 0.43 ms for 6.7 M skeleton pixels at r = 64)
//
//   component_width : per root pixel i = label - 1 of csbsr_ccl_label's labels, wacc[n][0][i] = max d2 over the component, wacc[n][1][i] = the
//     smallest linear index that attains it (-1 when the maximum is 0).  Three launches: reset the root slots; integer max; integer min of
//     the indices whose d2 equals the finished maximum.  Both are defined by an extremum, so every order gives the same bits.
#include "common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define WD_TH 64                          // owned rows of a workgroup
#define WD_TWW 4                          // owned words per row
#define WD_TW (32 * WD_TWW)
#define WD_MAX_R 128
#define WD_MAX_HW ((WD_MAX_R + 31) / 32)  // halo words per side
#define WD_ROWS (WD_TH + 2 * WD_MAX_R)    // 320
#define WD_WPR (WD_TWW + 2 * WD_MAX_HW)   // 12
#define WD_MAX_SIDE 8192                  // 8192^2 = 2^26 pixels: every index fits an int32
#define WD_LBINS 64                       // d2 < 64 (and the saturated bin) are counted in LDS first

__global__ __launch_bounds__(256) void width_kernel(const float* x, float th, const uint8_t* skel, int H, int W, int r, int cap, int* d2,
                                                    int* hist) {
  __shared__ uint32_t bits[WD_ROWS * WD_WPR];                                       // 15 KB
  __shared__ uint16_t list[WD_TH * WD_TW];                                          // 16 KB: tile-local index of each skeleton pixel
  __shared__ int lhist[WD_LBINS + 1];                                               // [WD_LBINS]: the saturated bin
  __shared__ int count;
  const int tid = threadIdx.x, lane = tid & 63;
  const int y0 = blockIdx.y * WD_TH, x0 = blockIdx.x * WD_TW;
  const long base = (long)blockIdx.z * H * W;
  if (tid == 0) count = 0;
  if (tid <= WD_LBINS) lhist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < WD_TH * WD_TW; i += 256) {                                  // every lane makes every trip: the ballots are whole
    const int ly = i / WD_TW, lx = i - ly * WD_TW;
    const int gy = y0 + ly, gx = x0 + lx;
    bool sk = false;
    if (gy < H && gx < W) {
      const long o = base + (long)gy * W + gx;
      sk = skel[o] != 0;
      if (!sk) d2[o] = 0;
    }
    const unsigned long long m = __ballot(sk);
    if (m) {                                                                        // wave-uniform
      int b = 0;
      if (lane == 0) b = atomicAdd(&count, __popcll(m));
      b = __shfl(b, 0);
      if (sk) list[b + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)i;
    }
  }
  __syncthreads();
  const int n = count;
  if (n == 0) return;                                                               // the whole workgroup
  const int hw = (r + 31) >> 5, wpr = WD_TWW + 2 * hw, rows = WD_TH + 2 * r;
  const int rowpx = wpr * 32, total = rows * rowpx;                                 // a multiple of 32, <= 320 * 384
  const int gy0 = y0 - r, gx0 = x0 - 32 * hw;
  for (int i = tid; i < ((total + 255) & ~255); i += 256) {
    bool v = true;                                                                  // outside the plane: set, never background
    if (i < total) {
      const int rr = i / rowpx, c = i - rr * rowpx;
      const int gy = gy0 + rr, gx = gx0 + c;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = x[base + (long)gy * W + gx] - th > 0.f;      // NaN compares false
    }
    const unsigned long long b = __ballot(v);
    if ((tid & 31) == 0 && i < total) bits[i >> 5] = (uint32_t)(b >> (tid & 32));
  }
  __syncthreads();
  for (int k = tid; k < n; k += 256) {
    const int p = list[k];
    const int ly = p / WD_TW, lx = p - ly * WD_TW;
    const int row = ly + r, bx = lx + 32 * hw;
    const int cw = bx >> 5, b = bx & 31;
    int best = cap;
    for (int dy = 0; dy * dy < best; ++dy) {                                        // best <= r^2 + 1: dy <= r, the row is inside the halo
      for (int s = 0; s < (dy ? 2 : 1); ++s) {
        const uint32_t* R = bits + (s ? row + dy : row - dy) * wpr;
        const int dy2 = dy * dy;
        const uint32_t inv = ~R[cw];
        // to the left: bits 0 .. b of this word, then whole words while their nearest pixel could still win
        const uint32_t l = inv & (0xFFFFFFFFu >> (31 - b));
        if (l) {
          const int dx = b - 31 + __builtin_clz(l);
          best = min(best, dy2 + dx * dx);
        } else {
          for (int j = 1; j <= hw; ++j) {
            const int nearest = 32 * (j - 1) + b + 1;
            if (dy2 + nearest * nearest >= best) break;
            const uint32_t w = ~R[cw - j];
            if (w) {
              const int dx = 32 * j + b - 31 + __builtin_clz(w);
              best = min(best, dy2 + dx * dx);
              break;
            }
          }
        }
        const uint32_t g = inv & (0xFFFFFFFFu << b);
        if (g) {
          const int dx = __builtin_ctz(g) - b;
          best = min(best, dy2 + dx * dx);
        } else {
          for (int j = 1; j <= hw; ++j) {
            const int nearest = 32 * j - b;
            if (dy2 + nearest * nearest >= best) break;
            const uint32_t w = ~R[cw + j];
            if (w) {
              const int dx = 32 * j + __builtin_ctz(w) - b;
              best = min(best, dy2 + dx * dx);
              break;
            }
          }
        }
      }
    }
    d2[base + (long)(y0 + ly) * W + x0 + lx] = best;
    if (best < WD_LBINS) atomicAdd(&lhist[best], 1);
    else if (best == cap) atomicAdd(&lhist[WD_LBINS], 1);
    else atomicAdd(hist + (long)blockIdx.z * (cap + 1) + best, 1);                  // WD_LBINS <= best < cap
  }
  __syncthreads();
  if (tid <= WD_LBINS) {
    const int v = lhist[tid], bin = tid < WD_LBINS ? tid : cap;
    if (v && bin <= cap) atomicAdd(hist + (long)blockIdx.z * (cap + 1) + bin, v);   // a filled bin is <= cap: best never exceeds it
  }
}

__global__ __launch_bounds__(256) void cw_roots_init_kernel(const int* labels, int hw, int* wacc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long n = blockIdx.y;
  if (labels[n * hw + i] != i + 1) return;
  int* a = wacc + n * 2 * hw + i;
  a[0] = 0;
  a[hw] = -1;                                                                       // as unsigned: above every index
}

// PASS 0: the maximum; PASS 1: the smallest index that attains the finished maximum (an unsigned minimum under the initial -1)
template <int PASS>
__global__ __launch_bounds__(256) void cw_reduce_kernel(const int* labels, const int* d2, int hw, int* wacc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long n = blockIdx.y;
  const int d = d2[n * hw + i];
  if (d <= 0) return;
  const int lab = labels[n * hw + i];
  if (lab <= 0 || lab > hw) return;                                                 // no label at all: nothing is indexed with it
  int* a = wacc + n * 2 * hw + (lab - 1);
  if (PASS == 0) {
    if (__hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < d) atomicMax(a, d);     // a stale load costs a needless atomic only
  } else if (a[0] == d) {
    atomicMin(reinterpret_cast<unsigned int*>(a + hw), (unsigned int)i);
  }
}

static int wd_dims_ok(const char* what, int32_t N, int32_t H, int32_t W) {
  CSBSR_CHECK(N >= 1 && N <= 65535, "%s: 1 .. 65535 planes, got %d", what, N);
  CSBSR_CHECK(H >= 1 && W >= 1 && H <= WD_MAX_SIDE && W <= WD_MAX_SIDE, "%s: %d x %d is outside 1 .. %d per side (int32 indices)", what, H, W,
              WD_MAX_SIDE);
  return 0;
}

extern "C" int32_t csbsr_width_max_radius(void) { return WD_MAX_R; }

extern "C" int csbsr_width_tile(int32_t* th, int32_t* tw) {
  CSBSR_CHECK(th && tw, "width_tile: null");
  *th = WD_TH;
  *tw = WD_TW;
  return 0;
}

extern "C" int csbsr_skeleton_width(const float* planes, float threshold, const uint8_t* skeleton, int32_t N, int32_t H, int32_t W,
                                    int32_t max_radius, int32_t* d2, int32_t* hist, csbsr_stream_t s) {
  CSBSR_CHECK(planes && skeleton && d2 && hist, "skeleton_width: null");
  if (wd_dims_ok("skeleton_width", N, H, W)) return 1;
  CSBSR_CHECK(max_radius >= 1 && max_radius <= WD_MAX_R, "skeleton_width: the radius is 1 .. %d, got %d", WD_MAX_R, max_radius);
  CSBSR_CHECK(threshold == threshold && threshold - threshold == 0.f, "skeleton_width: the threshold is not finite");
  const int cap = max_radius * max_radius + 1;
  const hipError_t e = hipMemsetAsync(hist, 0, sizeof(int32_t) * (size_t)N * (size_t)(cap + 1), ST(s));
  CSBSR_CHECK(e == hipSuccess, "skeleton_width: clearing the histogram failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(width_kernel, dim3((W + WD_TW - 1) / WD_TW, (H + WD_TH - 1) / WD_TH, N), dim3(256), 0, ST(s), planes, threshold, skeleton,
                     H, W, max_radius, cap, d2, hist);
  CSBSR_LAUNCH_CHECK("csbsr_skeleton_width");
  return 0;
}

extern "C" int csbsr_component_width(const int32_t* labels, const int32_t* d2, int32_t N, int32_t H, int32_t W, int32_t* wacc,
                                     csbsr_stream_t s) {
  CSBSR_CHECK(labels && d2 && wacc, "component_width: null");
  if (wd_dims_ok("component_width", N, H, W)) return 1;
  const int hw = H * W;
  const dim3 grid((hw + 255) / 256, N);
  hipLaunchKernelGGL(cw_roots_init_kernel, grid, dim3(256), 0, ST(s), labels, hw, wacc);
  CSBSR_LAUNCH_CHECK("csbsr_component_width (init)");
  hipLaunchKernelGGL(cw_reduce_kernel<0>, grid, dim3(256), 0, ST(s), labels, d2, hw, wacc);
  CSBSR_LAUNCH_CHECK("csbsr_component_width (max)");
  hipLaunchKernelGGL(cw_reduce_kernel<1>, grid, dim3(256), 0, ST(s), labels, d2, hw, wacc);
  CSBSR_LAUNCH_CHECK("csbsr_component_width (first)");
  return 0;
}
