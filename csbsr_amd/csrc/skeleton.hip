// Guo-Hall parallel thinning of binary planes and the centerline counts of clDice.
//
// A plane lives as one bit per pixel, 32 pixels of a row per uint32 word (bit i of word c = pixel x = 32 c + i; the bits past W are 0).  One
// lane evaluates the deletion predicate for the 32 pixels of a word with boolean algebra: the eight neighbour planes are the word itself,
// the words above and below, each shifted by one bit with the carry of the adjacent word; "C == 1" and "min(N1, N2) in {2, 3}" are
// bit-sliced sums of four one-bit terms.
//
//   P2 = N, P3 = NE, P4 = E, P5 = SE, P6 = S, P7 = SW, P8 = W, P9 = NW; zero outside the image
//   C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
//   N  = min((P9|P2) + (P3|P4) + (P5|P6) + (P7|P8), (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9))
//   m  = (P2 | P3 | !P5) & P4 in the first sub-iteration, (P6 | P7 | !P9) & P8 in the second
//   P is deleted iff C == 1 and 2 <= N <= 3 and m == 0; all deletions of a sub-iteration are simultaneous.
//
//   skel_init_kernel   : fp32 -> bits (x - threshold > 0, NaN -> 0), one wave ballot = two words.
//   skel_passes_kernel : a workgroup owns SK_TH x SK_TW pixels.  It loads them with a halo of 2 SK_K rows and one word (32 >= 2 SK_K pixels)
//                        per side into LDS, runs up to SK_K passes (2 SK_K sub-iterations) there between two LDS buffers, and writes its own
//                        pixels once, to the OTHER global plane (a neighbour reads them as its halo, so a launch never updates in place).
//                        What lies outside the LDS tile is taken as 0: where that is not the image border the error moves inwards by one
//                        pixel per sub-iteration and, after 2 SK_K of them, has not reached the owned pixels.  A tile that is empty, or in
//                        which a whole pass deleted nothing (it is a fixed point: the remaining passes would not change it either), stops
//                        early.  The workgroup adds the number of OWNED pixels it deleted to one int32 counter (one integer atomic per
//                        workgroup); the host decides on convergence from that counter.  No workgroup waits for another.
//   skel_finish_kernel : bits -> uint8 0 / 1.
//   cl_counts_kernel   : (|S_P|, |S_P & V_L|, |S_L|, |S_L & V_P|) per image, wave ballots + integer atomics (run-to-run identical).
#include "common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define SK_TH 64                         // owned rows of a workgroup
#define SK_TWW 4                         // owned words per row: SK_TW = 128 pixels
#define SK_K 8                           // passes per launch at most; 2 SK_K <= 32 = the one-word halo
#define SK_PH (SK_TH + 4 * SK_K)         // LDS rows: the owned ones and 2 SK_K above and below
#define SK_PWW (SK_TWW + 2)              // LDS words per row
#define SK_MAX_SIDE 8192                 // 8192^2 = 2^26 pixels: every count fits an int32

__global__ __launch_bounds__(256) void skel_init_kernel(const float* x, float th, int H, int W, int WW, uint32_t* work) {
  const int px = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const long n = blockIdx.z;
  bool v = false;
  if (px < W) v = x[(n * H + y) * W + px] - th > 0.f;                             // NaN compares false
  const unsigned long long b = __ballot(v);
  const int w = px >> 5;
  if ((threadIdx.x & 31) == 0 && w < WW) work[(n * H + y) * WW + w] = (uint32_t)(b >> (threadIdx.x & 32));
}

// the word of the next state: ``c`` with the pixels deleted that the sub-iteration ``second`` (0 / 1) deletes.  u, c, d: the rows above,
// at and below; l / r: the words to the left / right of each
__device__ __forceinline__ uint32_t skel_step(uint32_t ul, uint32_t u, uint32_t ur, uint32_t cl, uint32_t c, uint32_t cr, uint32_t dl, uint32_t d,
                                              uint32_t dr, int second) {
  const uint32_t p2 = u, p3 = (u >> 1) | (ur << 31), p4 = (c >> 1) | (cr << 31), p5 = (d >> 1) | (dr << 31);
  const uint32_t p6 = d, p7 = (d << 1) | (dl >> 31), p8 = (c << 1) | (cl >> 31), p9 = (u << 1) | (ul >> 31);
  // C == 1: exactly one of four terms
  const uint32_t c1 = ~p2 & (p3 | p4), c2 = ~p4 & (p5 | p6), c3 = ~p6 & (p7 | p8), c4 = ~p8 & (p9 | p2);
  const uint32_t one = ((c1 ^ c2) ^ (c3 ^ c4)) & ~(c1 & c2) & ~(c3 & c4);
  // min(N1, N2) in {2, 3}: both sums >= 2 and not both == 4
  const uint32_t a1 = p9 | p2, a2 = p3 | p4, a3 = p5 | p6, a4 = p7 | p8;
  const uint32_t b1 = p2 | p3, b2 = p4 | p5, b3 = p6 | p7, b4 = p8 | p9;
  const uint32_t ge2a = (a1 & a2) | (a3 & a4) | ((a1 ^ a2) & (a3 ^ a4)), ge2b = (b1 & b2) | (b3 & b4) | ((b1 ^ b2) & (b3 ^ b4));
  const uint32_t n23 = ge2a & ge2b & ~(a1 & a2 & a3 & a4 & b1 & b2 & b3 & b4);
  const uint32_t m = second ? ((p6 | p7 | ~p9) & p8) : ((p2 | p3 | ~p5) & p4);
  return c & ~(one & n23 & ~m);
}

__global__ __launch_bounds__(256) void skel_passes_kernel(const uint32_t* src, uint32_t* dst, int H, int WW, int passes, int* deleted) {
  __shared__ uint32_t buf[2][SK_PH * SK_PWW];
  __shared__ int sdel;
  const int tid = threadIdx.x;
  const int y0 = blockIdx.y * SK_TH - 2 * SK_K, w0 = blockIdx.x * SK_TWW - 1;        // image coordinates of LDS (0, 0)
  const long base = (long)blockIdx.z * H * WW;
  if (tid == 0) sdel = 0;
  uint32_t any = 0;
  int before = 0;                        // set bits among the owned pixels this thread loaded
  for (int i = tid; i < SK_PH * SK_PWW; i += 256) {
    const int r = i / SK_PWW, c = i - r * SK_PWW;
    const int y = y0 + r, w = w0 + c;
    uint32_t v = 0;
    if ((unsigned)y < (unsigned)H && (unsigned)w < (unsigned)WW) v = src[base + (long)y * WW + w];
    buf[0][i] = v;
    any |= v;
    if (r >= 2 * SK_K && r < 2 * SK_K + SK_TH && c >= 1 && c <= SK_TWW) before += __popc(v);
  }
  int cur = 0;
  if (__syncthreads_or(any != 0)) {      // an empty tile stays empty
    for (int p = 0; p < passes; ++p) {
      uint32_t changed = 0;
      for (int second = 0; second < 2; ++second) {
        const uint32_t* a = buf[cur];
        uint32_t* b = buf[cur ^ 1];
        for (int i = tid; i < SK_PH * SK_PWW; i += 256) {
          const int r = i / SK_PWW, c = i - r * SK_PWW;
          const uint32_t v = a[i];
          uint32_t nv = 0;
          if (v) {
            const bool up = r > 0, dn = r < SK_PH - 1, lf = c > 0, rt = c < SK_PWW - 1;
            const uint32_t* q = a + i;
            const uint32_t u = up ? q[-SK_PWW] : 0, d = dn ? q[SK_PWW] : 0;
            const uint32_t ul = up && lf ? q[-SK_PWW - 1] : 0, ur = up && rt ? q[-SK_PWW + 1] : 0;
            const uint32_t cl = lf ? q[-1] : 0, cr = rt ? q[1] : 0;
            const uint32_t dl = dn && lf ? q[SK_PWW - 1] : 0, dr = dn && rt ? q[SK_PWW + 1] : 0;
            nv = skel_step(ul, u, ur, cl, v, cr, dl, d, dr, second);
            changed |= v ^ nv;
          }
          b[i] = nv;
        }
        cur ^= 1;
        if (second == 0) __syncthreads();
      }
      if (!__syncthreads_or(changed != 0)) break;          // a fixed point of the tile: the remaining passes would delete nothing
    }
  }
  int after = 0;
  for (int i = tid; i < SK_TH * SK_TWW; i += 256) {
    const int r = i / SK_TWW, c = i - r * SK_TWW;
    const int y = y0 + 2 * SK_K + r, w = w0 + 1 + c;
    if (y < H && w < WW) {
      const uint32_t v = buf[cur][(r + 2 * SK_K) * SK_PWW + c + 1];
      dst[base + (long)y * WW + w] = v;
      after += __popc(v);
    }
  }
  if (before != after) atomicAdd(&sdel, before - after);   // LDS; threads load and store different words, only the sum is meaningful
  __syncthreads();
  if (tid == 0 && sdel != 0) atomicAdd(deleted, sdel);
}

__global__ __launch_bounds__(256) void skel_finish_kernel(const uint32_t* work, int H, int W, int WW, uint8_t* out) {
  const int px = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const long n = blockIdx.z;
  if (px < W) out[(n * H + y) * W + px] = (uint8_t)((work[(n * H + y) * WW + (px >> 5)] >> (px & 31)) & 1u);
}

__global__ __launch_bounds__(256) void cl_counts_kernel(const uint8_t* sp, const float* pred, float th, const uint8_t* sl, const float* mask,
                                                        long hw, int* counts) {
  __shared__ int sh[4];
  const int tid = threadIdx.x;
  const long n = blockIdx.y;
  if (tid < 4) sh[tid] = 0;
  __syncthreads();
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (long i = (long)blockIdx.x * 256 + tid; i < hw; i += (long)gridDim.x * 256) {
    const long o = n * hw + i;
    const bool a = sp[o] != 0, b = sl[o] != 0;
    const bool vp = pred[o] - th > 0.f, vl = mask[o] > 0.5f;
    c0 += a;
    c1 += a && vl;
    c2 += b;
    c3 += b && vp;
  }
  if (c0) atomicAdd(&sh[0], c0);
  if (c1) atomicAdd(&sh[1], c1);
  if (c2) atomicAdd(&sh[2], c2);
  if (c3) atomicAdd(&sh[3], c3);
  __syncthreads();
  if (tid < 4 && sh[tid]) atomicAdd(&counts[n * 4 + tid], sh[tid]);
}

static int skel_dims_ok(const char* what, int32_t N, int32_t H, int32_t W) {
  CSBSR_CHECK(N >= 1 && N <= 65535, "%s: 1 .. 65535 planes, got %d", what, N);
  CSBSR_CHECK(H >= 1 && W >= 1 && H <= SK_MAX_SIDE && W <= SK_MAX_SIDE, "%s: %d x %d is outside 1 .. %d per side (int32 counts)", what, H, W,
              SK_MAX_SIDE);
  return 0;
}

extern "C" int32_t csbsr_skeleton_max_passes(void) { return SK_K; }

extern "C" int csbsr_skeleton_init(const float* planes, float threshold, int32_t N, int32_t H, int32_t W, uint32_t* work, csbsr_stream_t s) {
  CSBSR_CHECK(planes && work, "skeleton_init: null");
  if (skel_dims_ok("skeleton_init", N, H, W)) return 1;
  CSBSR_CHECK(threshold == threshold && threshold - threshold == 0.f, "skeleton_init: the threshold is not finite");
  const int WW = (W + 31) / 32;
  hipLaunchKernelGGL(skel_init_kernel, dim3((W + 255) / 256, H, N), dim3(256), 0, ST(s), planes, threshold, H, W, WW, work);
  CSBSR_LAUNCH_CHECK("csbsr_skeleton_init");
  return 0;
}

extern "C" int csbsr_skeleton_passes(const uint32_t* src, uint32_t* dst, int32_t N, int32_t H, int32_t W, int32_t passes, int32_t* deleted,
                                     csbsr_stream_t s) {
  CSBSR_CHECK(src && dst && deleted, "skeleton_passes: null");
  CSBSR_CHECK(src != dst, "skeleton_passes: a launch reads one plane set and writes another, never in place");
  if (skel_dims_ok("skeleton_passes", N, H, W)) return 1;
  CSBSR_CHECK(passes >= 1 && passes <= SK_K, "skeleton_passes: 1 .. %d passes per launch, got %d", SK_K, passes);
  const int WW = (W + 31) / 32;
  hipLaunchKernelGGL(skel_passes_kernel, dim3((WW + SK_TWW - 1) / SK_TWW, (H + SK_TH - 1) / SK_TH, N), dim3(256), 0, ST(s), src, dst, H, WW,
                     passes, deleted);
  CSBSR_LAUNCH_CHECK("csbsr_skeleton_passes");
  return 0;
}

extern "C" int csbsr_skeleton_finish(const uint32_t* work, int32_t N, int32_t H, int32_t W, uint8_t* out, csbsr_stream_t s) {
  CSBSR_CHECK(work && out, "skeleton_finish: null");
  if (skel_dims_ok("skeleton_finish", N, H, W)) return 1;
  hipLaunchKernelGGL(skel_finish_kernel, dim3((W + 255) / 256, H, N), dim3(256), 0, ST(s), work, H, W, (W + 31) / 32, out);
  CSBSR_LAUNCH_CHECK("csbsr_skeleton_finish");
  return 0;
}

extern "C" int csbsr_centerline_counts(const uint8_t* skel_pred, const float* pred, float threshold, const uint8_t* skel_gt, const float* mask,
                                       int32_t N, int32_t H, int32_t W, int32_t* counts, csbsr_stream_t s) {
  CSBSR_CHECK(skel_pred && pred && skel_gt && mask && counts, "centerline_counts: null");
  if (skel_dims_ok("centerline_counts", N, H, W)) return 1;
  CSBSR_CHECK(hipMemsetAsync(counts, 0, (size_t)N * 4 * sizeof(int32_t), ST(s)) == hipSuccess, "centerline_counts: memset failed");
  const long hw = (long)H * W;
  long per = (hw + 256 * 16 - 1) / (256 * 16);             // 16 pixels per lane
  if (per > 1024) per = 1024;
  hipLaunchKernelGGL(cl_counts_kernel, dim3((unsigned)per, N), dim3(256), 0, ST(s), skel_pred, pred, threshold, skel_gt, mask, hw, counts);
  CSBSR_LAUNCH_CHECK("csbsr_centerline_counts");
  return 0;
}
