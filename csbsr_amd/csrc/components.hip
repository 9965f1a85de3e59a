// Connected-component labelling of binary planes, per-component sums and the small-component filter.
//
// A plane is binarised as in skel_init_kernel: a pixel is set iff  x - threshold > 0  in fp32 (NaN -> not set).  The label of a set pixel is
// 1 + min(y W + x) over its 4- or 8-connected component, the label of a background pixel 0: the value is defined by a minimum, so every
// correct order of unions gives the same bits and nothing differs from run to run.
//
// The forest.  ``work`` holds one int32 per pixel: -1 for background, else the linear index (within the plane) of the pixel's PARENT.  At
// every moment parent(i) <= i, with equality exactly for a root, so every path descends and ends; when all unions are done a tree is a
// component and its root the component's smallest index.
//
//   ccl_local_kernel   : a workgroup owns CC_TH x CC_TW pixels.  It binarises them with wave ballots into one bit per pixel, labels the tile
//                        in LDS with a union-find over tile-local indices (a lane owns one 32-pixel word of a row: the pixels of a run inside
//                        the word start with the run's first pixel as parent, then one union per pair of touching runs, chosen with word
//                        algebra from the word, the word above and their neighbours) and writes, per set pixel, the GLOBAL index of its
//                        tile-local root.  Local raster order and global raster order agree inside a tile, so that root is the smallest
//                        global index of the tile-local component.
//   ccl_merge_kernel   : one lane per seam pixel, ONE launch for all seams (the "same-launch" form).  A lane of the horizontal seam y = k CC_TH
//                        joins (y, x) to (y-1, x), or, where that is background and the connectivity is 8, to (y-1, x-1) and (y-1, x+1); a
//                        lane of the vertical seam x = k CC_TW joins (y, x) to (y, x-1), or else to (y-1, x-1) and (y+1, x-1).  (A pair that
//                        is skipped is joined through a third pixel by another lane or by the local pass.)
//   ccl_flatten_kernel : every set pixel walks to its root and stores root + 1 into ``labels``; background stores 0.  ``work`` is only read.
//
// cc_union(a, b): find both roots; equal -> done; else atomic-min the LARGER root's slot with the smaller root.  If the value the atomic
// returns is the larger root itself, that slot was a root and now points to the smaller: done.  Otherwise another lane has lowered the slot
// first: the slot now holds min(returned, smaller), and the lane goes on to join ``returned`` with the smaller root.
//
// Coherence (ccl_merge_kernel reads words other workgroups write in the same launch).  The device has one L2 per XCD and a CU's L1 is never
// refreshed by another CU's stores, so a plain load may return an old parent and a plain store need not become visible.  The merge kernel
// therefore reads ``work`` ONLY with relaxed agent-scope atomic loads (they bypass L1) or takes the value an agent-scope atomic min
// returned, and writes it ONLY with that atomic (performed at the memory side, visible to all).  Correctness does not depend on a load being
// fresh: a slot only ever decreases, and every value it has held is an ancestor of the pixel in the final forest -- when a lane replaces
// parent p1 of a by a smaller b, the same lane goes on to join p1 with b -- so a stale parent is an older, larger, still valid ancestor and
// costs one more step.  The decision "a was a root and is now linked" rests on the atomic's return value alone, which is always current.
// ccl_local_kernel's plain stores are complete at the kernel boundary before the merge starts, and ccl_flatten_kernel starts after the
// merge has finished; within ccl_local_kernel the same argument holds for LDS at workgroup scope.
//
// Termination.  Every loop strictly decreases the index it holds: cc_find steps from i to parent(i) < i and stops at parent(i) >= i (or at
// a value that is no index at all); an iteration of cc_union either returns or replaces its larger index by the strictly smaller value the
// atomic returned, and returns on anything else.  No loop polls for a value another lane or workgroup has yet to write: there is no flag,
// no ticket, no spin, and no workgroup waits for another.  (The alternative, a hierarchical merge with one launch per level in which a
// workgroup owns both super-tiles of a seam, shares nothing within a launch but needs about log2(tiles) launches: DESIGN 1.11.)
//
//   component_sums     : per root, with integer atomics only: area_px, skeleton_px, min x, max y, max x (min y is the root's own row).  The
//                        accumulators are indexed by root pixel: acc int32 [N][CC_ACC][H W], of which only the slots of root pixels are
//                        written (cc_roots_init_kernel resets exactly those).  One lane reads one pixel, a wave 64 consecutive pixels of
//                        a row; the set pixels of a horizontal run share a label, so the run's first lane adds the run's length and its
//                        skeleton pixels once (ballots + bit counts), and touches the box only where a relaxed load says it would change.
//   component_keep     : uint8 1 where the pixel's component has >= min_px pixels; optionally the labels with the other components zeroed.
#include "common.h"
#include "union_find.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define CC_TH 64                         // owned rows of a workgroup
#define CC_TWW 4                         // owned words per row: CC_TW = 128 pixels, one lane per word
#define CC_TW (32 * CC_TWW)
#define CC_MAX_SIDE 8192                 // 8192^2 = 2^26 pixels: every index and count fits an int32
#define CC_ACC 5                         // accumulators per root: area_px, skeleton_px, x0, y1, x1

// cc_load / cc_find / cc_union, shared with branches.hip: union_find.h

__global__ __launch_bounds__(256) void ccl_local_kernel(const float* x, float th, int H, int W, int conn8, int* work) {
  __shared__ uint32_t bits[CC_TH * CC_TWW];
  __shared__ int lab[CC_TH * CC_TW];
  const int tid = threadIdx.x;
  const int y0 = blockIdx.y * CC_TH, x0 = blockIdx.x * CC_TW;
  const long base = (long)blockIdx.z * H * W;
  // binarise: 256 lanes = two rows of the tile per step, one ballot = two words
  for (int i = tid; i < CC_TH * CC_TW; i += 256) {
    const int r = i / CC_TW, c = i - r * CC_TW;
    const int gy = y0 + r, gx = x0 + c;
    bool v = false;
    if (gy < H && gx < W) v = x[base + (long)gy * W + gx] - th > 0.f;               // NaN compares false
    const unsigned long long b = __ballot(v);
    if ((tid & 31) == 0) bits[i >> 5] = (uint32_t)(b >> (tid & 32));
  }
  __syncthreads();
  const int r = tid / CC_TWW, w = tid - r * CC_TWW;                                 // this lane's word
  const bool up = r > 0, lf = w > 0, rt = w < CC_TWW - 1;
  const uint32_t c = bits[tid], cl = lf ? bits[tid - 1] : 0, cr = rt ? bits[tid + 1] : 0;
  const uint32_t u = up ? bits[tid - CC_TWW] : 0, ul = up && lf ? bits[tid - CC_TWW - 1] : 0, ur = up && rt ? bits[tid - CC_TWW + 1] : 0;
  const int p0 = r * CC_TW + w * 32;                                                // local index of bit 0
  int start = 0;
  for (int i = 0; i < 32; ++i) {                                                    // a run inside the word hangs on its first pixel
    if ((c >> i) & 1u) {
      if (i == 0 || !((c >> (i - 1)) & 1u)) start = p0 + i;
      lab[p0 + i] = start;
    }
  }
  __syncthreads();
  const uint32_t cw = (c << 1) | (cl >> 31), ce = (c >> 1) | (cr << 31);            // bit i: the pixel to the west / east
  const uint32_t uw = (u << 1) | (ul >> 31), ue = (u >> 1) | (ur << 31);            // bit i: the pixel to the north-west / north-east
  if ((c & 1u) && (cl >> 31)) cc_union<CC_WG>(lab, p0, p0 - 1);                     // a run that continues from the word to the left
  // north: once per pair of touching runs -- not where the western neighbour and its northern neighbour are set too (that pixel, or one
  // further west, makes the same join)
  for (uint32_t m = c & u & ~(cw & uw); m; m &= m - 1) {
    const int p = p0 + __builtin_ctz(m);
    cc_union<CC_WG>(lab, p, p - CC_TW);
  }
  if (conn8) {
    // the diagonals matter only under a background pixel, and only where the western (eastern) neighbour does not make the join itself
    for (uint32_t m = c & ~u & uw & ~cw; m; m &= m - 1) {
      const int p = p0 + __builtin_ctz(m);
      cc_union<CC_WG>(lab, p, p - CC_TW - 1);
    }
    for (uint32_t m = c & ~u & ue & ~ce; m; m &= m - 1) {
      const int p = p0 + __builtin_ctz(m);
      cc_union<CC_WG>(lab, p, p - CC_TW + 1);
    }
  }
  __syncthreads();
  for (uint32_t m = c; m; m &= m - 1) {                                             // flatten in LDS: a root is an ancestor, concurrent walks stay valid
    const int p = p0 + __builtin_ctz(m);
    __hip_atomic_store(lab + p, cc_find<CC_WG>(lab, p), __ATOMIC_RELAXED, CC_WG);
  }
  __syncthreads();
  for (int i = tid; i < CC_TH * CC_TW; i += 256) {
    const int rr = i / CC_TW, cc = i - rr * CC_TW;
    const int gy = y0 + rr, gx = x0 + cc;
    if (gy < H && gx < W) {
      int v = -1;
      if ((bits[i >> 5] >> (i & 31)) & 1u) {
        const int root = lab[i];
        v = (y0 + root / CC_TW) * W + x0 + root % CC_TW;
      }
      work[base + (long)gy * W + gx] = v;
    }
  }
}

#define CC_SET(i) (cc_load<CC_AGENT>(L, (i)) >= 0)
__global__ __launch_bounds__(256) void ccl_merge_kernel(int* work, int H, int W, int conn8, int nhs, int nvs) {
  int* L = work + (long)blockIdx.y * H * W;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int nh = nhs * W;
  if (i < nh) {                                                                     // horizontal seams: y = (k + 1) CC_TH < H
    const int k = i / W, x = i - k * W;
    const int p = (k + 1) * CC_TH * W + x, q = p - W;
    if (!CC_SET(p)) return;
    if (CC_SET(q)) {
      if (!(x > 0 && CC_SET(p - 1) && CC_SET(q - 1))) cc_union<CC_AGENT>(L, p, q);  // else the western lane (or one further west) joins the rows
    } else if (conn8) {
      if (x > 0 && CC_SET(q - 1)) cc_union<CC_AGENT>(L, p, q - 1);
      if (x + 1 < W && CC_SET(q + 1)) cc_union<CC_AGENT>(L, p, q + 1);
    }
  } else if (i < nh + nvs * H) {                                                    // vertical seams: x = (k + 1) CC_TW < W
    const int j = i - nh;
    const int k = j / H, y = j - k * H;
    const int p = y * W + (k + 1) * CC_TW, q = p - 1;
    if (!CC_SET(p)) return;
    if (CC_SET(q)) {
      cc_union<CC_AGENT>(L, p, q);
    } else if (conn8) {
      if (y > 0 && CC_SET(q - W)) cc_union<CC_AGENT>(L, p, q - W);
      if (y + 1 < H && CC_SET(q + W)) cc_union<CC_AGENT>(L, p, q + W);
    }
  }
}
#undef CC_SET

__global__ __launch_bounds__(256) void ccl_flatten_kernel(const int* work, int hw, int* labels) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long base = (long)blockIdx.y * hw;
  const int* L = work + base;
  int r = L[i];
  if (r >= 0) {
    for (;;) {                                                                      // r strictly decreases
      const int p = L[r];
      if ((unsigned)p >= (unsigned)r) break;
      r = p;
    }
  }
  labels[base + i] = r + 1;                                                         // background: -1 + 1
}

__global__ __launch_bounds__(256) void cc_roots_init_kernel(const int* labels, int hw, int W, int* acc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long n = blockIdx.y;
  if (labels[n * hw + i] != i + 1) return;
  int* a = acc + n * CC_ACC * hw + i;
  a[0] = 0;
  a[hw] = 0;
  a[2l * hw] = W;                                                                   // x0: a minimum
  a[3l * hw] = 0;
  a[4l * hw] = 0;
}

__global__ __launch_bounds__(256) void component_sums_kernel(const int* labels, const uint8_t* skel, int H, int W, int* acc) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const long n = blockIdx.z;
  const int hw = H * W;
  const int lane = threadIdx.x & 63;
  int lab = 0;
  bool sk = false;
  if (x < W) {
    const long o = n * hw + (long)y * W + x;
    lab = labels[o];
    if (lab > 0 && skel) sk = skel[o] != 0;
  }
  if (lab < 0 || lab > hw) lab = 0;                                                 // no label at all: nothing is indexed with it
  const unsigned long long set = __ballot(lab != 0), skm = __ballot(sk);
  const bool head = lab != 0 && (lane == 0 || ((set >> (lane - 1)) & 1ull) == 0);
  if (!head) return;
  const unsigned long long rest = ~(set >> lane);                                   // bit j: lane + j is not set (zeros shifted in count as not set)
  const int len = rest ? __builtin_ctzll(rest) : 64;
  const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
  const int nsk = __popcll(skm & run);
  int* a = acc + n * CC_ACC * hw + (lab - 1);
  atomicAdd(a, len);
  if (nsk) atomicAdd(a + hw, nsk);
  const int xe = x + len - 1;
  // the box: an atomic only where a relaxed load says the value would change (a stale load costs a needless atomic, never a wrong one)
  if (__hip_atomic_load(a + 2l * hw, __ATOMIC_RELAXED, CC_AGENT) > x) atomicMin(a + 2l * hw, x);
  if (__hip_atomic_load(a + 3l * hw, __ATOMIC_RELAXED, CC_AGENT) < y) atomicMax(a + 3l * hw, y);
  if (__hip_atomic_load(a + 4l * hw, __ATOMIC_RELAXED, CC_AGENT) < xe) atomicMax(a + 4l * hw, xe);
}

__global__ __launch_bounds__(256) void component_keep_kernel(const int* labels, const int* acc, int hw, int min_px, uint8_t* keep,
                                                             int* labels_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long n = blockIdx.y;
  const int lab = labels[n * hw + i];
  const bool k = lab > 0 && lab <= hw && acc[n * CC_ACC * hw + (lab - 1)] >= min_px;
  keep[n * hw + i] = k ? 1 : 0;
  if (labels_out) labels_out[n * hw + i] = k ? lab : 0;
}

static int cc_dims_ok(const char* what, int32_t N, int32_t H, int32_t W) {
  CSBSR_CHECK(N >= 1 && N <= 65535, "%s: 1 .. 65535 planes, got %d", what, N);
  CSBSR_CHECK(H >= 1 && W >= 1 && H <= CC_MAX_SIDE && W <= CC_MAX_SIDE, "%s: %d x %d is outside 1 .. %d per side (int32 indices)", what, H, W,
              CC_MAX_SIDE);
  return 0;
}

extern "C" int csbsr_ccl_tile(int32_t* th, int32_t* tw) {
  CSBSR_CHECK(th && tw, "ccl_tile: null");
  *th = CC_TH;
  *tw = CC_TW;
  return 0;
}

extern "C" int csbsr_ccl_label(const float* planes, float threshold, int32_t N, int32_t H, int32_t W, int32_t connectivity, int32_t* work,
                               int32_t* labels, csbsr_stream_t s) {
  CSBSR_CHECK(planes && work && labels, "ccl_label: null");
  CSBSR_CHECK(work != labels, "ccl_label: work and labels are two arrays");
  if (cc_dims_ok("ccl_label", N, H, W)) return 1;
  CSBSR_CHECK(connectivity == 4 || connectivity == 8, "ccl_label: the connectivity is 4 or 8, got %d", connectivity);
  CSBSR_CHECK(threshold == threshold && threshold - threshold == 0.f, "ccl_label: the threshold is not finite");
  const int conn8 = connectivity == 8;
  hipLaunchKernelGGL(ccl_local_kernel, dim3((W + CC_TW - 1) / CC_TW, (H + CC_TH - 1) / CC_TH, N), dim3(256), 0, ST(s), planes, threshold, H, W,
                     conn8, work);
  CSBSR_LAUNCH_CHECK("csbsr_ccl_label (local)");
  const int nhs = (H - 1) / CC_TH, nvs = (W - 1) / CC_TW;                            // seams strictly inside the plane
  const int lanes = nhs * W + nvs * H;                                              // < 2 * 128 * 8192
  if (lanes > 0) {
    hipLaunchKernelGGL(ccl_merge_kernel, dim3((lanes + 255) / 256, N), dim3(256), 0, ST(s), work, H, W, conn8, nhs, nvs);
    CSBSR_LAUNCH_CHECK("csbsr_ccl_label (merge)");
  }
  const int hw = H * W;
  hipLaunchKernelGGL(ccl_flatten_kernel, dim3((hw + 255) / 256, N), dim3(256), 0, ST(s), work, hw, labels);
  CSBSR_LAUNCH_CHECK("csbsr_ccl_label (flatten)");
  return 0;
}

extern "C" int csbsr_component_sums(const int32_t* labels, const uint8_t* skeleton, int32_t N, int32_t H, int32_t W, int32_t* acc,
                                    csbsr_stream_t s) {
  CSBSR_CHECK(labels && acc, "component_sums: null");
  if (cc_dims_ok("component_sums", N, H, W)) return 1;
  const int hw = H * W;
  hipLaunchKernelGGL(cc_roots_init_kernel, dim3((hw + 255) / 256, N), dim3(256), 0, ST(s), labels, hw, W, acc);
  CSBSR_LAUNCH_CHECK("csbsr_component_sums (init)");
  hipLaunchKernelGGL(component_sums_kernel, dim3((W + 255) / 256, H, N), dim3(256), 0, ST(s), labels, skeleton, H, W, acc);
  CSBSR_LAUNCH_CHECK("csbsr_component_sums");
  return 0;
}

extern "C" int csbsr_component_keep(const int32_t* labels, const int32_t* acc, int32_t N, int32_t H, int32_t W, int32_t min_px, uint8_t* keep,
                                    int32_t* labels_out, csbsr_stream_t s) {
  CSBSR_CHECK(labels && acc && keep, "component_keep: null");
  if (cc_dims_ok("component_keep", N, H, W)) return 1;
  CSBSR_CHECK(min_px >= 1, "component_keep: min_px is >= 1, got %d", min_px);
  const int hw = H * W;
  hipLaunchKernelGGL(component_keep_kernel, dim3((hw + 255) / 256, N), dim3(256), 0, ST(s), labels, acc, hw, min_px, keep, labels_out);
  CSBSR_LAUNCH_CHECK("csbsr_component_keep");
  return 0;
}
