// Crack topology: node class, owned links and full quads of every pixel of a binary plane, their counts, and the same sums per connected
// component.
//
// S is a plane of bytes, set where the byte is non-zero (a skeleton of csbsr_skeleton_finish, or any uint8 plane).  Everything outside the
// plane is clear: the next plane of a batch and the bits past W of a packed row never link to anything.
//
//   ring    : the 8 neighbours in the order N, NE, E, SE, S, SW, W, NW, cyclically
//   n8      : the set neighbours;  A : the positions where a clear neighbour is followed by a set one (the Rutovitz crossing number, 0 .. 4)
//   class   : 0 clear, 1 isolated (n8 == 0), 2 end (A == 1), 4 junction (A >= 3), 3 path (the rest: A == 2, or A == 0 with n8 == 8)
//   links   : a link belongs to its first pixel in raster order.  E and S: both pixels set.  SE: both set and neither E nor S set;
//             SW: both set and neither W nor S set (a diagonal is dropped where an orthogonal two-step path exists)
//   quad    : the pixel, E, S and SE are all set
//   topo    : bits 0-2 the class, bit 3 the quad, bits 4 .. 7 the E, S, SE, SW link
//
//   topology_kernel : a workgroup owns TP_TH x TP_TW pixels.  It packs them and a halo of one pixel to one bit per pixel in LDS straight from
//     the bytes (wave ballots: 256 lanes = two rows = four words; the halo columns a lane each).  A tile without a set pixel of its own only
//     clears its topo.  Otherwise one lane evaluates one 32-pixel word with boolean algebra: the eight neighbour planes are the words above,
//     at and below, shifted by one bit with the carry of the adjacent word; the eight ring terms ~r[i] & r[i + 1] go through a bit-sliced
//     adder whose three sum planes give the masks A == 1 and A >= 3.  The eight result planes pass through LDS so that the bytes leave
//     in row order, 64 consecutive bytes per wave.  Counts are bit counts of the masks: one LDS atomic per lane and counter that is
//     non-zero, one global integer atomic per workgroup and counter that is non-zero.
//   component_topology : per root pixel i = label - 1 of csbsr_ccl_label's labels, nine sums over the component's pixels.  One lane reads one
//     pixel, a wave 64 consecutive pixels of a row; the set pixels of a horizontal run share a label, so the run's first lane adds the
//     run's bit counts once (the form of component_sums_kernel).
//
// No floating point, no workgroup waits for another, integer atomics only: every order gives the same bits.
#include "common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define TP_TH 64                          // owned rows of a workgroup
#define TP_TWW 4                          // owned words per row, one lane per word
#define TP_TW (32 * TP_TWW)
#define TP_PH (TP_TH + 2)                 // LDS rows: the owned ones and one above and below
#define TP_MAX_SIDE 8192                  // 8192^2 = 2^26 pixels: every index and count fits an int32
#define TP_COUNTS 10                      // V, isolated, end, path, junction_px, h, v, d_se, d_sw, q4
#define TP_ACC 9                          // per root: end, junction_px, h, v, d_se, d_sw, q4, isolated, junctions

__global__ __launch_bounds__(256) void topology_kernel(const uint8_t* skel, int H, int W, uint8_t* topo, int* counts) {
  __shared__ uint32_t bits[TP_PH * TP_TWW];                                         // row rr = image row y0 - 1 + rr
  __shared__ uint32_t lcol[TP_PH], rcol[TP_PH];                                     // 0 / 1: the pixels x0 - 1 and x0 + TP_TW of each row
  __shared__ uint32_t res[8][TP_TH * TP_TWW];                                       // plane k = bit k of topo
  __shared__ int sh[TP_COUNTS];
  const int tid = threadIdx.x;
  const int y0 = blockIdx.y * TP_TH, x0 = blockIdx.x * TP_TW;
  const long base = (long)blockIdx.z * H * W;
  if (tid < TP_COUNTS) sh[tid] = 0;
  bool own = false;
  for (int i = tid; i < TP_PH * TP_TW; i += 256) {                                  // 33 trips, every lane makes every one: the ballots are whole
    const int rr = i / TP_TW, c = i - rr * TP_TW;
    const int gy = y0 - 1 + rr, gx = x0 + c;
    bool v = false;
    if (gy >= 0 && gy < H && gx < W) v = skel[base + (long)gy * W + gx] != 0;
    own |= v && rr >= 1 && rr <= TP_TH;
    const unsigned long long b = __ballot(v);
    if ((tid & 31) == 0) bits[i >> 5] = (uint32_t)(b >> (tid & 32));
  }
  if (tid < 2 * TP_PH) {
    const int side = tid >= TP_PH, rr = tid - side * TP_PH;
    const int gy = y0 - 1 + rr, gx = side ? x0 + TP_TW : x0 - 1;
    uint32_t v = 0;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = skel[base + (long)gy * W + gx] != 0;
    (side ? rcol : lcol)[rr] = v;
  }
  if (!__syncthreads_or(own)) {                                                     // nothing set among the owned pixels: every class and link is 0
    for (int i = tid; i < TP_TH * TP_TW; i += 256) {
      const int r = i / TP_TW, c = i - r * TP_TW;
      const int gy = y0 + r, gx = x0 + c;
      if (gy < H && gx < W) topo[base + (long)gy * W + gx] = 0;
    }
    return;                                                                         // the whole workgroup
  }
  {
    const int r = tid / TP_TWW, w = tid - r * TP_TWW;                               // this lane's word: owned row r, LDS row r + 1
    const uint32_t* q = bits + (r + 1) * TP_TWW + w;
    const uint32_t u = q[-TP_TWW], c = q[0], d = q[TP_TWW];
    const bool lf = w > 0, rt = w < TP_TWW - 1;
    const uint32_t ul = lf ? q[-TP_TWW - 1] >> 31 : lcol[r], cl = lf ? q[-1] >> 31 : lcol[r + 1], dl = lf ? q[TP_TWW - 1] >> 31 : lcol[r + 2];
    const uint32_t ur = rt ? q[-TP_TWW + 1] & 1u : rcol[r], cr = rt ? q[1] & 1u : rcol[r + 1], dr = rt ? q[TP_TWW + 1] & 1u : rcol[r + 2];
    // bit i of a neighbour plane: that neighbour of pixel i of the word
    const uint32_t n = u, ne = (u >> 1) | (ur << 31), e = (c >> 1) | (cr << 31), se = (d >> 1) | (dr << 31);
    const uint32_t s = d, sw = (d << 1) | dl, we = (c << 1) | cl, nw = (u << 1) | ul;
    // A = the sum of the eight ring terms, bit-sliced: two full adders and a half adder, then the ones and the twos
    const uint32_t t0 = ~n & ne, t1 = ~ne & e, t2 = ~e & se, t3 = ~se & s, t4 = ~s & sw, t5 = ~sw & we, t6 = ~we & nw, t7 = ~nw & n;
    const uint32_t s0 = t0 ^ t1 ^ t2, c0 = (t0 & t1) | (t2 & (t0 ^ t1));
    const uint32_t s1 = t3 ^ t4 ^ t5, c1 = (t3 & t4) | (t5 & (t3 ^ t4));
    const uint32_t s2 = t6 ^ t7, c2 = t6 & t7;
    const uint32_t a1 = s0 ^ s1 ^ s2, c3 = (s0 & s1) | (s2 & (s0 ^ s1));               // the ones plane and its carry
    const uint32_t x2 = c0 ^ c1 ^ c2, f0 = (c0 & c1) | (c2 & (c0 ^ c1));
    const uint32_t a2 = x2 ^ c3, a4 = f0 | (x2 & c3);                                 // the twos and the fours plane (A <= 4: one carry at most)
    const uint32_t any = n | ne | e | se | s | sw | we | nw;
    const uint32_t iso = c & ~any, end = c & a1 & ~a2 & ~a4, jun = c & ((a1 & a2) | a4), path = c & ~(iso | end | jun);
    const uint32_t le = c & e, ls = c & s, lse = c & se & ~e & ~s, lsw = c & sw & ~we & ~s, quad = c & e & s & se;
    res[0][tid] = iso | path;                                                       // class 1 and 3
    res[1][tid] = end | path;                                                       // class 2 and 3
    res[2][tid] = jun;                                                              // class 4
    res[3][tid] = quad;
    res[4][tid] = le;
    res[5][tid] = ls;
    res[6][tid] = lse;
    res[7][tid] = lsw;
    const uint32_t m[TP_COUNTS] = {c, iso, end, path, jun, le, ls, lse, lsw, quad};
#pragma unroll
    for (int k = 0; k < TP_COUNTS; ++k)
      if (m[k]) atomicAdd(&sh[k], __popc(m[k]));
  }
  __syncthreads();
  for (int i = tid; i < TP_TH * TP_TW; i += 256) {
    const int r = i / TP_TW, c = i - r * TP_TW;
    const int gy = y0 + r, gx = x0 + c;
    if (gy < H && gx < W) {
      const int wi = i >> 5, b = i & 31;
      uint32_t v = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) v |= ((res[k][wi] >> b) & 1u) << k;
      topo[base + (long)gy * W + gx] = (uint8_t)v;
    }
  }
  if (tid < TP_COUNTS && sh[tid]) atomicAdd(counts + (long)blockIdx.z * TP_COUNTS + tid, sh[tid]);
}

__global__ __launch_bounds__(256) void ct_roots_init_kernel(const int* labels, int hw, int* tacc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long n = blockIdx.y;
  if (labels[n * hw + i] != i + 1) return;
  int* a = tacc + n * TP_ACC * hw + i;
#pragma unroll
  for (int k = 0; k < TP_ACC; ++k) a[(long)k * hw] = 0;
}

__global__ __launch_bounds__(256) void component_topology_kernel(const int* labels, const uint8_t* topo, const int* jlabels, int H, int W,
                                                                 int* tacc) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const long n = blockIdx.z;
  const int hw = H * W;
  const int lane = threadIdx.x & 63;
  int lab = 0;
  uint32_t t = 0;
  bool jr = false;
  if (x < W) {
    const int i = y * W + x;
    const long o = n * hw + i;
    lab = labels[o];
    if (lab > 0) {
      t = topo[o];
      if (jlabels) jr = jlabels[o] == i + 1;
    }
  }
  if (lab < 0 || lab > hw) lab = 0;                                                 // no label at all: nothing is indexed with it
  if (lab == 0) {
    t = 0;
    jr = false;
  }
  const uint32_t cls = t & 7u;
  // the order of the accumulators: end, junction_px, h, v, d_se, d_sw, q4, isolated, junctions
  const unsigned long long m[TP_ACC] = {__ballot(cls == 2u), __ballot(cls == 4u), __ballot((t & 16u) != 0), __ballot((t & 32u) != 0),
                                        __ballot((t & 64u) != 0), __ballot((t & 128u) != 0), __ballot((t & 8u) != 0), __ballot(cls == 1u),
                                        __ballot(jr)};
  const unsigned long long set = __ballot(lab != 0);
  const bool head = lab != 0 && (lane == 0 || ((set >> (lane - 1)) & 1ull) == 0);
  if (!head) return;
  const unsigned long long rest = ~(set >> lane);                                   // bit j: lane + j is not set (zeros shifted in count as not set)
  const int len = rest ? __builtin_ctzll(rest) : 64;
  const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
  int* a = tacc + n * TP_ACC * hw + (lab - 1);
#pragma unroll
  for (int k = 0; k < TP_ACC; ++k) {
    const int v = __popcll(m[k] & run);
    if (v) atomicAdd(a + (long)k * hw, v);
  }
}

static int tp_dims_ok(const char* what, int32_t N, int32_t H, int32_t W) {
  CSBSR_CHECK(N >= 1 && N <= 65535, "%s: 1 .. 65535 planes, got %d", what, N);
  CSBSR_CHECK(H >= 1 && W >= 1 && H <= TP_MAX_SIDE && W <= TP_MAX_SIDE, "%s: %d x %d is outside 1 .. %d per side (int32 indices)", what, H, W,
              TP_MAX_SIDE);
  return 0;
}

extern "C" int csbsr_skeleton_topology(const uint8_t* skeleton, int32_t N, int32_t H, int32_t W, uint8_t* topo, int32_t* counts,
                                       csbsr_stream_t s) {
  CSBSR_CHECK(skeleton && topo && counts, "skeleton_topology: null");
  CSBSR_CHECK(skeleton != topo, "skeleton_topology: the skeleton and topo are two arrays (a workgroup reads its neighbours' pixels)");
  if (tp_dims_ok("skeleton_topology", N, H, W)) return 1;
  const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)N * TP_COUNTS, ST(s));
  CSBSR_CHECK(e == hipSuccess, "skeleton_topology: clearing the counts failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(topology_kernel, dim3((W + TP_TW - 1) / TP_TW, (H + TP_TH - 1) / TP_TH, N), dim3(256), 0, ST(s), skeleton, H, W, topo,
                     counts);
  CSBSR_LAUNCH_CHECK("csbsr_skeleton_topology");
  return 0;
}

extern "C" int csbsr_component_topology(const int32_t* labels, const uint8_t* topo, const int32_t* jlabels, int32_t N, int32_t H, int32_t W,
                                        int32_t* tacc, csbsr_stream_t s) {
  CSBSR_CHECK(labels && topo && tacc, "component_topology: null");
  if (tp_dims_ok("component_topology", N, H, W)) return 1;
  const int hw = H * W;
  hipLaunchKernelGGL(ct_roots_init_kernel, dim3((hw + 255) / 256, N), dim3(256), 0, ST(s), labels, hw, tacc);
  CSBSR_LAUNCH_CHECK("csbsr_component_topology (init)");
  hipLaunchKernelGGL(component_topology_kernel, dim3((W + 255) / 256, H, N), dim3(256), 0, ST(s), labels, topo, jlabels, H, W, tacc);
  CSBSR_LAUNCH_CHECK("csbsr_component_topology");
  return 0;
}
