// Spur pruning of a binary plane: the side branches of up to L pixels go, everything else stays bit for bit.
//
// S is a plane of bytes, set where the byte is non-zero.  Everything outside the plane is clear: the next plane of a batch and the bits past W
// of a packed row are no neighbours.  With the ring N, NE, E, SE, S, SW, W, NW (cyclically), n8 = the set neighbours and A = the positions
// where a clear neighbour is followed by a set one, a set pixel is a TIP iff A == 1 and n8 <= 3, and ISOLATED iff n8 == 0.
//
//   peel  : X_0 = S.  For k = 1 .. L: E = the tips of X_(k-1); D_k = the pixels of E with an 8-neighbour in X_(k-1) \ E; X_k = X_(k-1) \ D_k, all
//           at once; T = k on D_k, 0 where nothing was peeled.  A tip whose set neighbours are all tips stays: no component vanishes.
//   seeds : Z = the tips and isolated pixels of X_L; M(z) = the largest T among z's 8 neighbours.
//   grow  : R starts empty.  For k = L .. 1, R gains every q with T(q) = k that has an 8-neighbour r with (r in Z and M(r) = k) or (r in R and
//           T(r) = k + 1).  The first alternative does not depend on R: it is R's initial value, and the steps L - 1 .. 1 use the second alone.
//   P = X_L | R;  removed = |S| - |P| = the pixels with T > 0 outside R.
//
// A plane lives as one bit per pixel, 32 pixels of a row per uint32 word (bit i of word c = pixel x = 32 c + i; the bits past W are 0), T as
// one byte per pixel in the caller's ``time``.
//
//   prune_pack_kernel   : bytes -> bits, one wave ballot = two words.
//   prune_peel_kernel   : a workgroup owns PR_TH x PR_TW pixels.  It loads them with a halo of 2 PR_KP rows and one word (32 >= 2 PR_KP pixels)
//                         per side into LDS and runs up to PR_KP steps there.  A step is two sweeps with a barrier after each: U = X \ tips(X)
//                         into a second buffer (one lane evaluates 32 pixels: the ring terms and the neighbours through a bit-sliced adder
//                         each), then X &= ~(X & ~U & any8(U)) in place, for a lane reads no other word of X than its own.  What lies outside
//                         the LDS tile is taken as clear: where that is not the plane's border the error moves inwards by two pixels per step
//                         and, after PR_KP steps, has not reached the owned pixels.  The owner stores the global step number into ``time`` for
//                         every owned pixel it deletes (a pixel is deleted once: one byte store each) and writes its own pixels once per
//                         launch to the OTHER global plane.  An empty tile, or one in which a step deleted nothing (a fixed point), stops early.
//   prune_seed_kernel   : one lane per pixel with T > 0 looks at its neighbours' rings in the peeled plane; R's initial value, as bits.
//   prune_grow_kernel   : a workgroup owns the same pixels and loads T | R << 7 of them and of a halo of PR_KG pixels as bytes into LDS -- only
//                         the values of this launch's steps k_hi .. k_lo and of k_hi + 1, the rest as 0.  Each lane remembers in a 64-bit mask
//                         which of its up to 60 bytes can still change, and a step visits those alone: a byte == k with a neighbour
//                         == 0x80 | (k + 1) becomes 0x80 | k (no byte written in step k is read in step k).  The error of the clear surroundings
//                         moves inwards by one pixel per step.  The owner writes its pixels' R bits to the OTHER R plane.
//   prune_finish_kernel : P = X_L | R as bytes, and the removed pixels per plane: wave ballots, one LDS atomic per wave, one integer atomic
//                         per workgroup that removed anything.
//
// The entry enqueues every launch itself -- L is known, nothing is read back --, no workgroup waits for another, there is no floating point
// and atomics are integer only: every order gives the same bits.
#include "common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define PR_TH 64                          // owned rows of a workgroup
#define PR_TWW 4                          // owned words per row
#define PR_TW (32 * PR_TWW)
#define PR_KP 8                           // peel steps per launch at most; 2 PR_KP <= 32 = the one-word halo
#define PR_PH (PR_TH + 4 * PR_KP)         // LDS rows of the peel kernel: the owned ones and 2 PR_KP above and below
#define PR_PWW (PR_TWW + 2)               // LDS words per row
#define PR_KG 16                          // grow steps per launch at most = the halo of the grow kernel in pixels
#define PR_GH (PR_TH + 2 * PR_KG)         // LDS rows and
#define PR_GW (PR_TW + 2 * PR_KG)         // bytes per row of the grow kernel
#define PR_GPER (PR_GH * PR_GW / 256)     // bytes per lane: 60 <= 64, the lane's mask
#define PR_MAX_SPUR 64                    // T fits 7 bits, bit 7 of a byte in LDS is R
#define PR_MAX_SIDE 8192                  // 8192^2 = 2^26 pixels: every index inside a plane and every count fits an int32

static_assert(2 * PR_KP <= 32, "the peel kernel's column halo is one word");
static_assert(PR_GH * PR_GW % 256 == 0 && PR_GPER <= 64, "a lane of the grow kernel keeps one mask bit per byte it owns");
static_assert(PR_MAX_SPUR < 128, "bit 7 is R");

__global__ __launch_bounds__(256) void prune_pack_kernel(const uint8_t* skel, int H, int W, int WW, uint32_t* bits) {
  const int px = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const long n = blockIdx.z;
  bool v = false;
  if (px < W) v = skel[(n * H + y) * W + px] != 0;
  const unsigned long long b = __ballot(v);
  const int w = px >> 5;
  if ((threadIdx.x & 31) == 0 && w < WW) bits[(n * H + y) * WW + w] = (uint32_t)(b >> (threadIdx.x & 32));
}

// the nine words around word i = (r, c) of an LDS tile of PR_PH x PR_PWW words, 0 outside the tile: ul, u, ur, cl, c, cr, dl, d, dr
__device__ __forceinline__ void pr_nine(const uint32_t* a, int i, int r, int c, uint32_t* q9) {
  const bool up = r > 0, dn = r < PR_PH - 1, lf = c > 0, rt = c < PR_PWW - 1;
  const uint32_t* q = a + i;
  q9[0] = up && lf ? q[-PR_PWW - 1] : 0;
  q9[1] = up ? q[-PR_PWW] : 0;
  q9[2] = up && rt ? q[-PR_PWW + 1] : 0;
  q9[3] = lf ? q[-1] : 0;
  q9[4] = q[0];
  q9[5] = rt ? q[1] : 0;
  q9[6] = dn && lf ? q[PR_PWW - 1] : 0;
  q9[7] = dn ? q[PR_PWW] : 0;
  q9[8] = dn && rt ? q[PR_PWW + 1] : 0;
}

// the eight neighbour planes of the middle word, in ring order: bit i of ring[j] = neighbour j of pixel i
__device__ __forceinline__ void pr_ring(const uint32_t* q9, uint32_t* ring) {
  const uint32_t u = q9[1], c = q9[4], d = q9[7];
  ring[0] = u;
  ring[1] = (u >> 1) | (q9[2] << 31);
  ring[2] = (c >> 1) | (q9[5] << 31);
  ring[3] = (d >> 1) | (q9[8] << 31);
  ring[4] = d;
  ring[5] = (d << 1) | (q9[6] >> 31);
  ring[6] = (c << 1) | (q9[3] >> 31);
  ring[7] = (u << 1) | (q9[0] >> 31);
}

// the sum of eight one-bit planes, bit-sliced: two full adders and a half adder for the ones, then the carries.  one = the sum is exactly 1,
// ge4 = the sum is at least 4
__device__ __forceinline__ void pr_sum8(const uint32_t* t, uint32_t& one, uint32_t& ge4) {
  const uint32_t s0 = t[0] ^ t[1] ^ t[2], c0 = (t[0] & t[1]) | (t[2] & (t[0] ^ t[1]));
  const uint32_t s1 = t[3] ^ t[4] ^ t[5], c1 = (t[3] & t[4]) | (t[5] & (t[3] ^ t[4]));
  const uint32_t s2 = t[6] ^ t[7], c2 = t[6] & t[7];
  const uint32_t a1 = s0 ^ s1 ^ s2, c3 = (s0 & s1) | (s2 & (s0 ^ s1));                // the ones plane and its carry
  const uint32_t x2 = c0 ^ c1 ^ c2, f0 = (c0 & c1) | (c2 & (c0 ^ c1));                // the four carries weigh 2 each:
  const uint32_t a2 = x2 ^ c3;                                                      //   the twos plane,
  ge4 = f0 | (x2 & c3);                                                             //   and two or more of them make 4
  one = a1 & ~a2 & ~ge4;
}

// the tips among the 32 pixels of the middle word: A == 1 and n8 <= 3
__device__ __forceinline__ uint32_t pr_tips(const uint32_t* q9) {
  uint32_t ring[8], term[8], a_one, a_ge4, n_one, n_ge4;
  pr_ring(q9, ring);
#pragma unroll
  for (int j = 0; j < 8; ++j) term[j] = ~ring[j] & ring[(j + 1) & 7];
  pr_sum8(term, a_one, a_ge4);
  pr_sum8(ring, n_one, n_ge4);
  return q9[4] & a_one & ~n_ge4;
}

__global__ __launch_bounds__(256) void prune_peel_kernel(const uint32_t* src, uint32_t* dst, int H, int W, int WW, int steps, int k0,
                                                         uint8_t* time) {
  __shared__ uint32_t xb[PR_PH * PR_PWW], ub[PR_PH * PR_PWW];
  const int tid = threadIdx.x;
  const int y0 = blockIdx.y * PR_TH - 2 * PR_KP, w0 = blockIdx.x * PR_TWW - 1;        // plane coordinates of LDS (0, 0)
  const long base = (long)blockIdx.z * H * WW;
  uint32_t any = 0;
  for (int i = tid; i < PR_PH * PR_PWW; i += 256) {
    const int r = i / PR_PWW, c = i - r * PR_PWW;
    const int y = y0 + r, w = w0 + c;
    uint32_t v = 0;
    if ((unsigned)y < (unsigned)H && (unsigned)w < (unsigned)WW) v = src[base + (long)y * WW + w];
    xb[i] = v;
    any |= v;
  }
  if (__syncthreads_or(any != 0)) {       // an empty tile stays empty
    for (int k = 1; k <= steps; ++k) {
      for (int i = tid; i < PR_PH * PR_PWW; i += 256) {
        const uint32_t v = xb[i];
        uint32_t u = 0;
        if (v) {
          const int r = i / PR_PWW, c = i - r * PR_PWW;
          uint32_t q9[9];
          pr_nine(xb, i, r, c, q9);
          u = v & ~pr_tips(q9);
        }
        ub[i] = u;
      }
      __syncthreads();
      uint32_t changed = 0;
      for (int i = tid; i < PR_PH * PR_PWW; i += 256) {
        const uint32_t v = xb[i], e = v & ~ub[i];
        if (e) {
          const int r = i / PR_PWW, c = i - r * PR_PWW;
          uint32_t q9[9], ring[8];
          pr_nine(ub, i, r, c, q9);
          pr_ring(q9, ring);
          uint32_t del = e & (ring[0] | ring[1] | ring[2] | ring[3] | ring[4] | ring[5] | ring[6] | ring[7]);
          if (del) {
            xb[i] = v & ~del;             // only this lane reads xb[i] in this sweep
            changed = 1;
            if (r >= 2 * PR_KP && r < 2 * PR_KP + PR_TH && c >= 1 && c <= PR_TWW) {
              // an owned word: a set bit is a pixel of the plane (rows >= H and the bits past W were loaded as 0)
              uint8_t* row = time + ((long)blockIdx.z * H + (y0 + r)) * W + 32 * (w0 + c);
              while (del) {
                row[__builtin_ctz(del)] = (uint8_t)(k0 + k);
                del &= del - 1;
              }
            }
          }
        }
      }
      if (!__syncthreads_or(changed != 0)) break;            // a fixed point of the tile: the remaining steps would delete nothing
    }
  }
  for (int i = tid; i < PR_TH * PR_TWW; i += 256) {
    const int r = i / PR_TWW, c = i - r * PR_TWW;
    const int y = y0 + 2 * PR_KP + r, w = w0 + 1 + c;
    if (y < H && w < WW) dst[base + (long)y * WW + w] = xb[(r + 2 * PR_KP) * PR_PWW + c + 1];
  }
}

// pixel (y, x) of a packed plane, clear outside it
__device__ __forceinline__ uint32_t pr_bit(const uint32_t* bits, int H, int W, int WW, int y, int x) {
  if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return 0;
  return (bits[(long)y * WW + (x >> 5)] >> (x & 31)) & 1u;
}

__constant__ int pr_dy[8] = {-1, -1, 0, 1, 1, 1, 0, -1};                             // N, NE, E, SE, S, SW, W, NW
__constant__ int pr_dx[8] = {0, 1, 1, 1, 0, -1, -1, -1};

__global__ __launch_bounds__(256) void prune_seed_kernel(const uint32_t* xl, const uint8_t* time, int H, int W, int WW, uint32_t* rbits) {
  const int px = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const long n = blockIdx.z;
  const uint32_t* x = xl + n * H * WW;
  const uint8_t* t = time + n * H * W;
  bool v = false;
  const int tq = px < W ? t[(long)y * W + px] : 0;
  if (tq) {                               // few pixels come here: the peeled ones
    for (int j = 0; j < 8 && !v; ++j) {
      const int zy = y + pr_dy[j], zx = px + pr_dx[j];
      if (!pr_bit(x, H, W, WW, zy, zx)) continue;
      uint32_t ring = 0;
      int m = 0;
      for (int i = 0; i < 8; ++i) {
        const int ny = zy + pr_dy[i], nx = zx + pr_dx[i];
        ring |= pr_bit(x, H, W, WW, ny, nx) << i;
        if ((unsigned)ny < (unsigned)H && (unsigned)nx < (unsigned)W) m = max(m, (int)t[(long)ny * W + nx]);
      }
      const uint32_t rot = ((ring << 1) | (ring >> 7)) & 0xffu;                       // bit i: ring position i - 1
      const int n8 = __popc(ring), a = __popc(~rot & ring & 0xffu);                   // position i - 1 clear and position i set
      v = m == tq && (n8 == 0 || (a == 1 && n8 <= 3));
    }
  }
  const unsigned long long b = __ballot(v);
  const int w = px >> 5;
  if ((threadIdx.x & 31) == 0 && w < WW) rbits[(n * H + y) * WW + w] = (uint32_t)(b >> (threadIdx.x & 32));
}

__global__ __launch_bounds__(256) void prune_grow_kernel(const uint8_t* time, const uint32_t* rsrc, uint32_t* rdst, int H, int W, int WW,
                                                         int k_hi, int k_lo) {
  __shared__ uint8_t tb[PR_GH * PR_GW];                                             // T | R << 7 where k_lo <= T <= k_hi + 1, else 0
  const int tid = threadIdx.x;
  const int y0 = blockIdx.y * PR_TH - PR_KG, x0 = blockIdx.x * PR_TW - PR_KG;         // plane coordinates of LDS (0, 0)
  const uint8_t* t = time + (long)blockIdx.z * H * W;
  const long base = (long)blockIdx.z * H * WW;
  unsigned long long mine = 0;            // bit j: byte tid + 256 j has k_lo <= T <= k_hi and no R yet
#pragma unroll 4
  for (int j = 0; j < PR_GPER; ++j) {
    const int i = tid + 256 * j;
    const int r = i / PR_GW, c = i - r * PR_GW;
    const int y = y0 + r, x = x0 + c;
    uint32_t v = 0;
    if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
      const int tv = t[(long)y * W + x];
      if (tv >= k_lo && tv <= k_hi + 1) {
        const uint32_t rb = (rsrc[base + (long)y * WW + (x >> 5)] >> (x & 31)) & 1u;
        v = tv | (rb << 7);
        if (tv <= k_hi && !rb) mine |= 1ull << j;
      }
    }
    tb[i] = (uint8_t)v;
  }
  if (__syncthreads_or(mine != 0)) {      // otherwise nothing in reach can change: R passes through
    for (int k = k_hi; k >= k_lo; --k) {
      const uint8_t want = (uint8_t)(0x80 | (k + 1));
      unsigned long long m = mine;
      while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        const int i = tid + 256 * j;
        if (tb[i] != k) continue;
        const int r = i / PR_GW, c = i - r * PR_GW;
        bool hit = false;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
          const int rr = r + pr_dy[d], cc = c + pr_dx[d];
          if ((unsigned)rr < (unsigned)PR_GH && (unsigned)cc < (unsigned)PR_GW) hit |= tb[rr * PR_GW + cc] == want;
        }
        if (hit) tb[i] = (uint8_t)(0x80 | k);                // read only by step k - 1, behind the barrier
        mine &= ~(1ull << j);                                // step k was this byte's only chance
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < PR_TH * PR_TW; i += 256) {                                   // 32 trips, every lane makes every one: the ballots are whole
    const int r = i / PR_TW, c = i - r * PR_TW;
    const unsigned long long b = __ballot((tb[(r + PR_KG) * PR_GW + c + PR_KG] & 0x80) != 0);
    const int y = y0 + PR_KG + r, w = (x0 + PR_KG + c) >> 5;
    if ((tid & 31) == 0 && y < H && w < WW) {
      const long o = base + (long)y * WW + w;
      rdst[o] = rsrc[o] | (uint32_t)(b >> (tid & 32));
    }
  }
}

__global__ __launch_bounds__(256) void prune_finish_kernel(const uint32_t* xl, const uint32_t* rbits, const uint8_t* time, int H, int W, int WW,
                                                           uint8_t* out, int* removed) {
  __shared__ int sh;
  const int px = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const long n = blockIdx.z;
  if (threadIdx.x == 0) sh = 0;
  __syncthreads();
  bool gone = false;
  if (px < W) {
    const long o = (n * H + y) * WW + (px >> 5), p = (n * H + y) * W + px;
    const uint32_t r = (rbits[o] >> (px & 31)) & 1u;
    out[p] = (uint8_t)(((xl[o] >> (px & 31)) & 1u) | r);
    gone = time[p] != 0 && !r;
  }
  const unsigned long long b = __ballot(gone);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&sh, __popcll(b));
  __syncthreads();
  if (threadIdx.x == 0 && sh) atomicAdd(removed + n, sh);
}

static int pr_dims_ok(const char* what, int32_t N, int32_t H, int32_t W) {
  CSBSR_CHECK(N >= 1 && N <= 65535, "%s: 1 .. 65535 planes, got %d", what, N);
  CSBSR_CHECK(H >= 1 && W >= 1 && H <= PR_MAX_SIDE && W <= PR_MAX_SIDE, "%s: %d x %d is outside 1 .. %d per side (int32 indices)", what, H, W,
              PR_MAX_SIDE);
  return 0;
}

extern "C" int32_t csbsr_prune_max_spur(void) { return PR_MAX_SPUR; }

extern "C" int csbsr_prune_steps(int32_t* peel, int32_t* grow) {
  CSBSR_CHECK(peel && grow, "prune_steps: null");
  *peel = PR_KP;
  *grow = PR_KG;
  return 0;
}

extern "C" int csbsr_prune_tile(int32_t* th, int32_t* tw) {
  CSBSR_CHECK(th && tw, "prune_tile: null");
  *th = PR_TH;
  *tw = PR_TW;
  return 0;
}

// four bit planes: the two the peel launches alternate between, and the two of R
extern "C" int64_t csbsr_prune_work_bytes(int32_t N, int32_t H, int32_t W) {
  if (N < 1 || N > 65535 || H < 1 || W < 1 || H > PR_MAX_SIDE || W > PR_MAX_SIDE) return 0;
  return 4 * (int64_t)N * H * ((W + 31) / 32) * (int64_t)sizeof(uint32_t);
}

extern "C" int csbsr_skeleton_prune(const uint8_t* skeleton, int32_t N, int32_t H, int32_t W, int32_t spur_px, void* work, uint8_t* time,
                                    uint8_t* out, int32_t* removed, csbsr_stream_t s) {
  CSBSR_CHECK(skeleton && work && time && out && removed, "skeleton_prune: null");
  CSBSR_CHECK(skeleton != out && skeleton != time && time != out, "skeleton_prune: the skeleton, time and out are three arrays");
  if (pr_dims_ok("skeleton_prune", N, H, W)) return 1;
  CSBSR_CHECK(spur_px >= 1 && spur_px <= PR_MAX_SPUR, "skeleton_prune: spur_px is 1 .. %d, got %d", PR_MAX_SPUR, spur_px);
  const int WW = (W + 31) / 32;
  const size_t plane = (size_t)N * H * WW;
  uint32_t* xa = static_cast<uint32_t*>(work);
  uint32_t *xb = xa + plane, *ra = xb + plane, *rb = ra + plane;
  hipError_t e = hipMemsetAsync(removed, 0, sizeof(int32_t) * (size_t)N, ST(s));
  CSBSR_CHECK(e == hipSuccess, "skeleton_prune: clearing the counts failed: %s", hipGetErrorString(e));
  e = hipMemsetAsync(time, 0, (size_t)N * H * W, ST(s));
  CSBSR_CHECK(e == hipSuccess, "skeleton_prune: clearing the peel times failed: %s", hipGetErrorString(e));
  const dim3 rows((W + 255) / 256, H, N), tiles((WW + PR_TWW - 1) / PR_TWW, (H + PR_TH - 1) / PR_TH, N);
  hipLaunchKernelGGL(prune_pack_kernel, rows, dim3(256), 0, ST(s), skeleton, H, W, WW, xa);
  CSBSR_LAUNCH_CHECK("csbsr_skeleton_prune (pack)");
  for (int k0 = 0; k0 < spur_px; k0 += PR_KP) {
    const int steps = spur_px - k0 < PR_KP ? spur_px - k0 : PR_KP;
    hipLaunchKernelGGL(prune_peel_kernel, tiles, dim3(256), 0, ST(s), xa, xb, H, W, WW, steps, k0, time);
    CSBSR_LAUNCH_CHECK("csbsr_skeleton_prune (peel)");
    uint32_t* t = xa;
    xa = xb;
    xb = t;
  }
  hipLaunchKernelGGL(prune_seed_kernel, rows, dim3(256), 0, ST(s), xa, time, H, W, WW, ra);
  CSBSR_LAUNCH_CHECK("csbsr_skeleton_prune (seeds)");
  for (int k_hi = spur_px - 1; k_hi >= 1;) {
    const int k_lo = k_hi - PR_KG + 1 > 1 ? k_hi - PR_KG + 1 : 1;
    hipLaunchKernelGGL(prune_grow_kernel, tiles, dim3(256), 0, ST(s), time, ra, rb, H, W, WW, k_hi, k_lo);
    CSBSR_LAUNCH_CHECK("csbsr_skeleton_prune (grow)");
    uint32_t* t = ra;
    ra = rb;
    rb = t;
    k_hi = k_lo - 1;
  }
  hipLaunchKernelGGL(prune_finish_kernel, rows, dim3(256), 0, ST(s), xa, ra, time, H, W, WW, out, removed);
  CSBSR_LAUNCH_CHECK("csbsr_skeleton_prune (finish)");
  return 0;
}
