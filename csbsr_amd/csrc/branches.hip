// Crack branches: one label per centerline segment between junctions, and the per-branch sums of the branch table.
//
// ``topo`` is the byte plane of csbsr_skeleton_topology (topology.hip): bits 0-2 the class, bits 4 .. 7 the owned E, S, SE, SW link.  A BRANCH
// PIXEL has class 1, 2 or 3, a JUNCTION PIXEL class 4.  An INNER link is an owned link whose two ends are branch pixels, an ATTACH link one
// with exactly one junction end.  A branch is a connected component of the branch pixels under the inner links; its label is 1 + the smallest
// linear index y W + x among its pixels, 0 at clear and at junction pixels -- a minimum, so every correct order of unions gives the same bits.
// A diagonal link exists only where no orthogonal two-step path does, so the two arms of a T, whose corner is the junction pixel, are
// never linked: the link graph separates what 8-connectivity of the non-junction pixels leaves joined.  A link bit whose other end lies
// outside the plane or is clear (no topo of csbsr_skeleton_topology has one) is ignored.
//
// The labelling is the forest of components.hip -- ``work`` holds -1 at a pixel that is no branch pixel, else the index of its parent, with
// parent(i) <= i -- with links for adjacency in place of pixel adjacency:
//
//   branch_local_kernel   : a workgroup owns BR_TH x BR_TW pixels.  It packs the branch-pixel mask and the four link planes (each masked by
//                           it) to one bit per pixel in LDS with wave ballots.  A tile without a branch pixel only writes -1 to its slots.
//                           Otherwise a lane owns one 32-pixel word of a row: the pixels of a chain of inner E links inside the word start
//                           with the chain's first pixel as parent, then one union per inner link that stays inside the tile -- the E link
//                           into the next word, and every S, SE and SW link, found with word algebra from the planes and the mask of the
//                           row below.  After a flatten in LDS every branch pixel stores the GLOBAL index of its tile-local root.
//   branch_merge_kernel   : ONE launch with a lane per pixel of the tile seams, for the links that cross a seam: S, SE and SW from a tile's
//                           last row (horizontal seam lanes), E and SE from a tile's last column and SW from the next tile's first column
//                           (vertical seam lanes; on a tile's last row the horizontal lanes make the diagonal joins).
//   branch_flatten_kernel : every branch pixel walks to its root and stores root + 1; every other pixel stores 0.  ``work`` is only read.
//
// Coherence and termination are those of components.hip, whose comment block states them in full: the merge kernel reads ``work`` only
// with relaxed agent-scope atomic loads or through the value an agent-scope atomic min returned, and writes it only with that atomic; a slot
// only ever decreases; unions go to the smaller index; every loop strictly decreases the index it holds; there is no flag, no spin, and no
// workgroup waits for another.  ``topo`` is read-only in all three launches, so plain loads of it are safe.
//
//   branch_sums_kernel    : per root pixel i = blabel - 1, with integer atomics only.  One lane reads one pixel, a wave 64 consecutive
//                           pixels of a row.  Adjacent set pixels of a row always share an E link, so a maximal horizontal run of one non-zero
//                           label lies in one branch: the run's first lane adds the run's ballot counts (px, end, the four link kinds,
//                           attach) once and touches the box.  A link is credited to the branch of its non-junction end: a branch pixel
//                           counts the links it owns (inner and attach), a junction pixel credits each link it owns to the branch found by
//                           reading ``blabels`` at the link's other end.  node_a / node_b, the box and the d2 extremes use min / max atomics
//                           only where a relaxed load says they would change; node_a and min_d2, minima over positive values that are 0 when
//                           there is none, are first set by a compare-and-swap against 0 (the slot never returns to 0 afterwards).
#include "common.h"
#include "union_find.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define BR_TH 64                          // owned rows of a workgroup
#define BR_TWW 4                          // owned words per row, one lane per word
#define BR_TW (32 * BR_TWW)
#define BR_MAX_SIDE 8192                  // 8192^2 = 2^26 pixels: every index and count fits an int32
#define BR_ACC 12                         // per root: px, end, attach, h, v, d_se, d_sw, node_a, node_b, x0, y1, x1
#define BR_ACC_D2 14                      // and with a d2 map: max_d2, min_d2

#define BR_IS(t) ((((uint32_t)(t) & 7u) - 1u) < 3u)                                 // class 1, 2 or 3

__global__ __launch_bounds__(256) void branch_local_kernel(const uint8_t* topo, int H, int W, int* work) {
  __shared__ uint32_t pl[5][BR_TH * BR_TWW];                                        // the branch pixels; their E, S, SE, SW link bits
  __shared__ int lab[BR_TH * BR_TW];
  const int tid = threadIdx.x;
  const int y0 = blockIdx.y * BR_TH, x0 = blockIdx.x * BR_TW;
  const long base = (long)blockIdx.z * H * W;
  bool own = false;
  for (int i = tid; i < BR_TH * BR_TW; i += 256) {                                  // 32 trips, every lane makes every one: the ballots are whole
    const int r = i / BR_TW, c = i - r * BR_TW;
    const int gy = y0 + r, gx = x0 + c;
    uint32_t t = 0;
    if (gy < H && gx < W) t = topo[base + (long)gy * W + gx];
    const bool b = BR_IS(t);
    own |= b;
    const unsigned long long m0 = __ballot(b), m1 = __ballot(b && (t & 16u)), m2 = __ballot(b && (t & 32u)), m3 = __ballot(b && (t & 64u)),
                             m4 = __ballot(b && (t & 128u));
    if ((tid & 31) == 0) {
      const int sh = tid & 32, wi = i >> 5;
      pl[0][wi] = (uint32_t)(m0 >> sh);
      pl[1][wi] = (uint32_t)(m1 >> sh);
      pl[2][wi] = (uint32_t)(m2 >> sh);
      pl[3][wi] = (uint32_t)(m3 >> sh);
      pl[4][wi] = (uint32_t)(m4 >> sh);
    }
  }
  if (!__syncthreads_or(own)) {                                                     // no branch pixel among the owned ones
    for (int i = tid; i < BR_TH * BR_TW; i += 256) {
      const int r = i / BR_TW, c = i - r * BR_TW;
      const int gy = y0 + r, gx = x0 + c;
      if (gy < H && gx < W) work[base + (long)gy * W + gx] = -1;
    }
    return;                                                                         // the whole workgroup
  }
  const int r = tid / BR_TWW, w = tid - r * BR_TWW;                                 // this lane's word
  const bool dn = r < BR_TH - 1, lf = w > 0, rt = w < BR_TWW - 1;
  const uint32_t c = pl[0][tid], cr = rt ? pl[0][tid + 1] : 0;
  const uint32_t d = dn ? pl[0][tid + BR_TWW] : 0, dl = dn && lf ? pl[0][tid + BR_TWW - 1] : 0, dr = dn && rt ? pl[0][tid + BR_TWW + 1] : 0;
  // bit i: the inner link of pixel i of the word that stays inside the tile (a link out of the tile is the merge kernel's)
  const uint32_t mE = pl[1][tid] & ((c >> 1) | (cr << 31)), mS = pl[2][tid] & d;
  const uint32_t mSE = pl[3][tid] & ((d >> 1) | (dr << 31)), mSW = pl[4][tid] & ((d << 1) | (dl >> 31));
  const int p0 = r * BR_TW + w * 32;                                                // local index of bit 0
  int start = 0;
  for (int i = 0; i < 32; ++i) {                                                    // a chain of E links inside the word hangs on its first pixel
    if ((c >> i) & 1u) {
      if (i == 0 || !((mE >> (i - 1)) & 1u)) start = p0 + i;
      lab[p0 + i] = start;
    }
  }
  __syncthreads();
  if (mE >> 31) cc_union<CC_WG>(lab, p0 + 31, p0 + 32);                             // the chain goes on in the word to the right
  for (uint32_t m = mS; m; m &= m - 1) {
    const int p = p0 + __builtin_ctz(m);
    cc_union<CC_WG>(lab, p, p + BR_TW);
  }
  for (uint32_t m = mSE; m; m &= m - 1) {
    const int p = p0 + __builtin_ctz(m);
    cc_union<CC_WG>(lab, p, p + BR_TW + 1);
  }
  for (uint32_t m = mSW; m; m &= m - 1) {
    const int p = p0 + __builtin_ctz(m);
    cc_union<CC_WG>(lab, p, p + BR_TW - 1);
  }
  __syncthreads();
  for (uint32_t m = c; m; m &= m - 1) {                                             // flatten in LDS: a root is an ancestor, concurrent walks stay valid
    const int p = p0 + __builtin_ctz(m);
    __hip_atomic_store(lab + p, cc_find<CC_WG>(lab, p), __ATOMIC_RELAXED, CC_WG);
  }
  __syncthreads();
  for (int i = tid; i < BR_TH * BR_TW; i += 256) {
    const int rr = i / BR_TW, cc = i - rr * BR_TW;
    const int gy = y0 + rr, gx = x0 + cc;
    if (gy < H && gx < W) {
      int v = -1;
      if ((pl[0][i >> 5] >> (i & 31)) & 1u) {
        const int root = lab[i];
        v = (y0 + root / BR_TW) * W + x0 + root % BR_TW;
      }
      work[base + (long)gy * W + gx] = v;
    }
  }
}

__global__ __launch_bounds__(256) void branch_merge_kernel(const uint8_t* topo, int* work, int H, int W, int nhs, int nvs) {
  int* L = work + (long)blockIdx.y * H * W;
  const uint8_t* T = topo + (long)blockIdx.y * H * W;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int nh = nhs * W;
  if (i < nh) {                                                                     // the last row of a tile: y + 1 = (k + 1) BR_TH < H
    const int k = i / W, x = i - k * W;
    const int p = ((k + 1) * BR_TH - 1) * W + x;
    const uint32_t t = T[p];
    if (!BR_IS(t)) return;
    if ((t & 32u) && BR_IS(T[p + W])) cc_union<CC_AGENT>(L, p, p + W);
    if ((t & 64u) && x + 1 < W && BR_IS(T[p + W + 1])) cc_union<CC_AGENT>(L, p, p + W + 1);
    if ((t & 128u) && x > 0 && BR_IS(T[p + W - 1])) cc_union<CC_AGENT>(L, p, p + W - 1);
  } else if (i < nh + nvs * H) {                                                    // the last column of a tile: x + 1 = (k + 1) BR_TW < W
    const int j = i - nh;
    const int k = j / H, y = j - k * H;
    const int p = y * W + (k + 1) * BR_TW - 1;
    const uint32_t t = T[p], u = T[p + 1];
    const bool diag = y + 1 < H && y % BR_TH != BR_TH - 1;                          // on a tile's last row the horizontal lanes join the diagonals
    if (BR_IS(t)) {
      if ((t & 16u) && BR_IS(u)) cc_union<CC_AGENT>(L, p, p + 1);
      if (diag && (t & 64u) && BR_IS(T[p + W + 1])) cc_union<CC_AGENT>(L, p, p + W + 1);
    }
    if (diag && BR_IS(u) && (u & 128u) && BR_IS(T[p + W])) cc_union<CC_AGENT>(L, p + 1, p + W);
  }
}

__global__ __launch_bounds__(256) void branch_flatten_kernel(const int* work, int hw, int* blabels) {
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
  blabels[base + i] = r + 1;                                                        // no branch pixel: -1 + 1
}

__global__ __launch_bounds__(256) void branch_roots_init_kernel(const int* blabels, int hw, int W, int K, int* bacc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long n = blockIdx.y;
  if (blabels[n * hw + i] != i + 1) return;
  int* a = bacc + n * K * hw + i;
  for (int k = 0; k < K; ++k) a[(long)k * hw] = k == 9 ? W : 0;                      // x0 is a minimum
}

// a maximum of values >= 0: the atomic only where a relaxed load says the slot would change (a stale load costs a needless atomic)
__device__ __forceinline__ void br_max(int* a, int v) {
  if (__hip_atomic_load(a, __ATOMIC_RELAXED, CC_AGENT) < v) atomicMax(a, v);
}

// a minimum over values v > 0 in a slot that holds 0 while there is none: the first value enters by a compare-and-swap against 0, and the
// slot is never 0 again; no loop
__device__ __forceinline__ void br_min_pos(int* a, int v) {
  int cur = __hip_atomic_load(a, __ATOMIC_RELAXED, CC_AGENT);
  if (cur == 0) {
    cur = atomicCAS(a, 0, v);
    if (cur == 0) return;
  }
  if (cur > v) atomicMin(a, v);
}

__global__ __launch_bounds__(256) void branch_sums_kernel(const int* blabels, const uint8_t* topo, const int* jlabels, const int* d2, int H, int W,
                                                          int K, int* bacc) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const long n = blockIdx.z;
  const int hw = H * W;
  const int lane = threadIdx.x & 63;
  const int* BL = blabels + n * hw;
  const uint8_t* T = topo + n * hw;
  int* A = bacc + n * K * hw;
  const int i = y * W + x;
  int lab = 0;
  uint32_t t = 0;
  if (x < W) {
    t = T[i];
    lab = BL[i];
  }
  if (lab < 0 || lab > hw) lab = 0;                                                 // no label at all: nothing is indexed with it
  const bool junction = lab == 0 && (t & 7u) == 4u;
  const int jown = junction && jlabels ? jlabels[n * hw + i] : 0;
  // the four owned links: E, S, SE, SW
  const int qy[4] = {y, y + 1, y + 1, y + 1}, qx[4] = {x + 1, x, x + 1, x - 1};
  bool credit[4], attach[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    credit[k] = attach[k] = false;
    if (!((t >> (4 + k)) & 1u) || !(lab != 0 || junction) || qy[k] >= H || qx[k] < 0 || qx[k] >= W) continue;
    const int q = qy[k] * W + qx[k];
    int lq = BL[q];
    if (lq < 0 || lq > hw) lq = 0;
    if (lab != 0) {                                                                 // a branch pixel: its inner and attach links count for its branch
      if (lq != 0) {
        credit[k] = true;
      } else if ((T[q] & 7u) == 4u) {
        credit[k] = attach[k] = true;
        const int jl = jlabels ? jlabels[n * hw + q] : 0;
        if (jl > 0) {
          br_min_pos(A + 7l * hw + (lab - 1), jl);
          br_max(A + 8l * hw + (lab - 1), jl);
        }
      }
    } else if (lq != 0) {                                                           // a junction pixel: the link counts for the branch at its other end
      atomicAdd(A + (3l + k) * hw + (lq - 1), 1);
      atomicAdd(A + 2l * hw + (lq - 1), 1);
      if (jown > 0) {
        br_min_pos(A + 7l * hw + (lq - 1), jown);
        br_max(A + 8l * hw + (lq - 1), jown);
      }
    }
  }
  if (lab != 0 && d2) {
    const int v = d2[n * hw + i];
    if (v > 0) {
      br_max(A + 12l * hw + (lab - 1), v);
      br_min_pos(A + 13l * hw + (lab - 1), v);
    }
  }
  // the order of the ballots: px, end, attach E / S / SE / SW, credited E / S / SE / SW
  const int prev = __shfl_up(lab, 1);
  const bool cont = lane > 0 && lab != 0 && prev == lab;                            // the pixel continues the run of the lane before
  const unsigned long long contm = __ballot(cont);
  const unsigned long long m[10] = {__ballot(lab != 0),  __ballot(lab != 0 && (t & 7u) == 2u),
                                    __ballot(attach[0]), __ballot(attach[1]),
                                    __ballot(attach[2]), __ballot(attach[3]),
                                    __ballot(credit[0]), __ballot(credit[1]),
                                    __ballot(credit[2]), __ballot(credit[3])};
  if (lab == 0 || cont) return;                                                     // not the first lane of a run
  const int len = 1 + (lane == 63 ? 0 : __builtin_ctzll(~(contm >> (lane + 1))));   // zeros shifted in end the run
  const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
  int* a = A + (lab - 1);
  atomicAdd(a, len);
  const int nend = __popcll(m[1] & run), natt = __popcll((m[2] & run)) + __popcll(m[3] & run) + __popcll(m[4] & run) + __popcll(m[5] & run);
  if (nend) atomicAdd(a + hw, nend);
  if (natt) atomicAdd(a + 2l * hw, natt);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = __popcll(m[6 + k] & run);
    if (v) atomicAdd(a + (3l + k) * hw, v);
  }
  const int xe = x + len - 1;
  if (__hip_atomic_load(a + 9l * hw, __ATOMIC_RELAXED, CC_AGENT) > x) atomicMin(a + 9l * hw, x);
  br_max(a + 10l * hw, y);
  br_max(a + 11l * hw, xe);
}

static int br_dims_ok(const char* what, int32_t N, int32_t H, int32_t W) {
  CSBSR_CHECK(N >= 1 && N <= 65535, "%s: 1 .. 65535 planes, got %d", what, N);
  CSBSR_CHECK(H >= 1 && W >= 1 && H <= BR_MAX_SIDE && W <= BR_MAX_SIDE, "%s: %d x %d is outside 1 .. %d per side (int32 indices)", what, H, W,
              BR_MAX_SIDE);
  return 0;
}

extern "C" int csbsr_branch_tile(int32_t* th, int32_t* tw) {
  CSBSR_CHECK(th && tw, "branch_tile: null");
  *th = BR_TH;
  *tw = BR_TW;
  return 0;
}

extern "C" int csbsr_branch_label(const uint8_t* topo, int32_t N, int32_t H, int32_t W, int32_t* work, int32_t* blabels, csbsr_stream_t s) {
  CSBSR_CHECK(topo && work && blabels, "branch_label: null");
  CSBSR_CHECK(work != blabels, "branch_label: work and blabels are two arrays");
  if (br_dims_ok("branch_label", N, H, W)) return 1;
  hipLaunchKernelGGL(branch_local_kernel, dim3((W + BR_TW - 1) / BR_TW, (H + BR_TH - 1) / BR_TH, N), dim3(256), 0, ST(s), topo, H, W, work);
  CSBSR_LAUNCH_CHECK("csbsr_branch_label (local)");
  const int nhs = (H - 1) / BR_TH, nvs = (W - 1) / BR_TW;                            // seams strictly inside the plane
  const int lanes = nhs * W + nvs * H;                                              // < 2 * 128 * 8192
  if (lanes > 0) {
    hipLaunchKernelGGL(branch_merge_kernel, dim3((lanes + 255) / 256, N), dim3(256), 0, ST(s), topo, work, H, W, nhs, nvs);
    CSBSR_LAUNCH_CHECK("csbsr_branch_label (merge)");
  }
  const int hw = H * W;
  hipLaunchKernelGGL(branch_flatten_kernel, dim3((hw + 255) / 256, N), dim3(256), 0, ST(s), work, hw, blabels);
  CSBSR_LAUNCH_CHECK("csbsr_branch_label (flatten)");
  return 0;
}

extern "C" int csbsr_branch_sums(const int32_t* blabels, const uint8_t* topo, const int32_t* jlabels, const int32_t* d2, int32_t N, int32_t H,
                                 int32_t W, int32_t* bacc, csbsr_stream_t s) {
  CSBSR_CHECK(blabels && topo && bacc, "branch_sums: null");
  if (br_dims_ok("branch_sums", N, H, W)) return 1;
  const int hw = H * W, K = d2 ? BR_ACC_D2 : BR_ACC;
  hipLaunchKernelGGL(branch_roots_init_kernel, dim3((hw + 255) / 256, N), dim3(256), 0, ST(s), blabels, hw, W, K, bacc);
  CSBSR_LAUNCH_CHECK("csbsr_branch_sums (init)");
  hipLaunchKernelGGL(branch_sums_kernel, dim3((W + 255) / 256, H, N), dim3(256), 0, ST(s), blabels, topo, jlabels, d2, H, W, K, bacc);
  CSBSR_LAUNCH_CHECK("csbsr_branch_sums");
  return 0;
}
