// Polyline simplification (Douglas-Peucker) of the ordered points of every branch.
//
// The input is the table of branch_polylines: span j of ``points`` is rows offsets[j] .. offsets[j + 1] - 1, and only y and x are read.  For a
// segment from kept point a to kept point b and a point p strictly between them along the chain, with c2 = |b - a|^2 and t = (p - a).(b - a),
// the KEY is |p - a|^2 (c2 = 0), |p - a|^2 c2 (t <= 0), |p - b|^2 c2 (t >= c2), else cross(b - a, p - a)^2: the squared distance to the
// SEGMENT times c2, an int64 below 2^58 for coordinates in [0, 8192).  The CANDIDATE of a segment is its inner point with the largest key,
// among equal keys the one with the smallest row; it is kept iff 16 key > tol_q^2 c2 (c2 = 0: 16 key > tol_q^2), and then splits the segment
// into two that are treated the same way.  The first and the last row of a span are always kept.  A split depends only on its segment's two
// ends, so the order in which segments are examined does not change the flags: every route below gives the same bits.
//
// Every chain is owned by ONE execution unit for the whole call:
//
//   simplify_wave_kernel  : one wave per span.  A span of up to SP_WAVE_MAX = 64 rows has one point per lane; the state (the two kept ends of
//                           the lane's segment, whether the segment still has to be examined) lives in registers.  One segment per trip: the
//                           first pending lane names it, the key maximum is a wave reduction, the smallest row among the equals is the
//                           lowest lane of a ballot.  Longer spans are left to the other kernel; a span whose offsets descend or leave 0 .. P
//                           gets vcount 0 and nothing else.
//   simplify_group_kernel : a fixed grid; workgroup g owns a contiguous range of spans, scans their offsets 256 at a time and works through
//                           those longer than SP_WAVE_MAX one after the other, all 256 lanes on one chain.  Per point: L and R, the chain
//                           positions of its segment's kept ends (R = -1: the point is kept, R = -2: kept in this round, L = -1: final); per
//                           segment, at the slot of its left end: the best key and the smallest position that has it.  A chain of up to
//                           SP_LDS_MAX = 2048 rows keeps this and a copy of its points in LDS (57 KiB: two workgroups per CU); a longer one
//                           keeps the state in ``work`` at its own rows -- no other workgroup's, as long as spans do not overlap -- and reads the points in place.
//                           A ROUND examines all segments made in the round before: (1) every pending point maxes its key into its segment's
//                           slot -- one atomic per wave where the wave's points share a segment --, (2) the points that hold the maximum min
//                           their position into it, (3) every pending point reads the outcome: the winner marks itself, the others take it as
//                           their new left or right end, and the points of a segment that did not split become final, (4) the new kept
//                           points reset the two slots of the segments they made.  Barriers between the phases; the loop ends when all lanes
//                           read 0 from the one LDS word that a round's winners set.  Rounds are not logarithmic (a saw whose teeth grow needs
//                           one per point); a round costs a pass over the chain's rows, so a chain of n rows costs up to n^2 / 256 steps a lane in
//                           this one launch: the worst case of Douglas-Peucker.  The caller bounds n (a chain of an image has at most H W rows).
//
// Coherence.  For a well-formed table (spans that do not overlap: ascending offsets) no workgroup reads or writes what another writes in the same launch: ``keep`` is zeroed by a memset in front of the kernels and
// a kernel only stores 1 at rows of spans it owns, vcount[j] has one writer, and the rows of ``work`` belong to the chain that covers them.
// With offsets that descend and rise again two spans can share rows of ``keep`` and ``work``: the flags are then unspecified (Bounds).
// There is no flag to wait for and no spin.  Inside a workgroup the state in ``work`` is read with agent-scope loads after a barrier.
//
// Bounds.  Offsets are checked before they are used, every position read back from the state is checked against the chain's length before
// it indexes anything, and the rounds are bounded by the chain's length: overlapping spans (offsets that descend and rise again) or
// coordinates outside [0, 8192) give unspecified flags, never an access outside an array or a loop without end.  No floating point.
#include "common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define SP_MAX_TOL_Q 64
#define SP_MAX_M (1 << 28)
#define SP_MAX_P (1 << 28)                // PL_MAX_P of polylines.hip
#define SP_WAVE_MAX 64                    // the longest span of the wave route
#define SP_LDS_MAX 2048                   // the longest chain whose state lives in LDS
#define SP_GROUPS 2048                    // the largest grid of simplify_group_kernel
#define SP_NONE 0x7fffffff

typedef unsigned long long u64;

// the key of p against the segment a -> b; c2 is returned for the split rule.  Products wrap (unsigned): coordinates out of range are no UB.
__device__ __forceinline__ u64 sp_key(int ay, int ax, int by, int bx, int py, int px, u64& c2) {
  const long long dy = (long long)by - ay, dx = (long long)bx - ax, ey = (long long)py - ay, ex = (long long)px - ax;
  c2 = (u64)dy * (u64)dy + (u64)dx * (u64)dx;
  const u64 pa = (u64)ey * (u64)ey + (u64)ex * (u64)ex;
  if (c2 == 0) return pa;
  const long long t = (long long)((u64)ey * (u64)dy + (u64)ex * (u64)dx);
  if (t <= 0) return pa * c2;
  if ((u64)t >= c2) {
    const long long fy = (long long)py - by, fx = (long long)px - bx;
    return ((u64)fy * (u64)fy + (u64)fx * (u64)fx) * c2;
  }
  const u64 cr = (u64)dx * (u64)ey - (u64)dy * (u64)ex;
  return cr * cr;                                                                    // the square of the wrapped value is the wrapped square
}

__device__ __forceinline__ bool sp_split(u64 key, u64 c2, u64 tq2) { return 16ull * key > tq2 * (c2 ? c2 : 1ull); }

__device__ __forceinline__ u64 sp_shfl_xor(u64 v, int m) {
  const int lo = __shfl_xor((int)(uint32_t)v, m, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), m, 64);
  return (u64)(uint32_t)lo | (u64)(uint32_t)hi << 32;
}

__device__ __forceinline__ u64 sp_wave_max(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 u = sp_shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return v;
}

__device__ __forceinline__ bool sp_span(const int64_t* offsets, int j, int P, long long& o0, long long& n) {
  o0 = offsets[j];
  const long long o1 = offsets[j + 1];
  const bool ok = o0 >= 0 && o1 >= o0 && o1 <= P;
  n = ok ? o1 - o0 : 0;
  return ok;
}

__global__ __launch_bounds__(256) void simplify_wave_kernel(const int64_t* offsets, const int2* points, int M, int P, u64 tq2, uint8_t* keep, int* vcount) {
  const int lane = threadIdx.x & 63;
  const long long jw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);                // wave-uniform
  if (jw >= M) return;
  const int j = (int)jw;
  long long o0, nn;
  if (!sp_span(offsets, j, P, o0, nn)) {
    if (lane == 0) vcount[j] = 0;
    return;
  }
  if (nn > SP_WAVE_MAX) return;                                                      // the other kernel's
  const int n = (int)nn;
  int y = 0, x = 0;
  if (lane < n) {
    const int2 p = points[2 * (o0 + lane)];                                          // y and x: the first 8 bytes of a 16-byte row
    y = p.x;
    x = p.y;
  }
  int L = 0, R = n - 1;
  bool kept = lane < n && (lane == 0 || lane == n - 1);
  bool pending = lane < n && !kept;
  for (int trip = 0; trip < 2 * SP_WAVE_MAX; ++trip) {                               // at most n - 2 splits and n - 1 segments that do not split
    const u64 mask = __ballot(pending);
    if (!mask) break;
    const int lead = __ffsll((long long)mask) - 1;
    const int Ls = __shfl(L, lead, 64) & 63, Rs = __shfl(R, lead, 64) & 63;
    const bool inseg = pending && L == Ls;
    const int ay = __shfl(y, Ls, 64), ax = __shfl(x, Ls, 64), by = __shfl(y, Rs, 64), bx = __shfl(x, Rs, 64);
    u64 c2;
    const u64 key = sp_key(ay, ax, by, bx, y, x, c2);
    const u64 kmax = sp_wave_max(inseg ? key : 0ull);
    const u64 win = __ballot(inseg && key == kmax);
    if (kmax > 0 && win && sp_split(kmax, c2, tq2)) {                                // c2 is the segment's: the same in every lane
      const int w = __ffsll((long long)win) - 1;                                     // the smallest row among the equals
      if (inseg) {
        if (lane == w) {
          kept = true;
          pending = false;
        } else if (lane > w) {
          L = w;
        } else {
          R = w;
        }
      }
    } else if (inseg) {
      pending = false;                                                               // the segment is final
    }
  }
  if (kept) keep[o0 + lane] = 1;
  const int v = __popcll(__ballot(kept));
  if (lane == 0) vcount[j] = v;
}

template <bool G, typename T>
__device__ __forceinline__ T sp_ld(const T* p) {
  if constexpr (G) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}

// one chain of n > 2 rows by the whole workgroup; returns the rows kept (the same value in every lane).  G: the state is in global memory.
// py / px: the coordinates of position i at py[i * ps] and px[i * ps].  ``flag`` and ``total`` are LDS words.
template <bool G>
__device__ __forceinline__ int sp_chain(int n, const int* py, const int* px, int ps, int* L, int* R, u64* best, int* bidx, u64 tq2, uint8_t* keep,
                                        int* flag, int* total) {
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < n; i += 256) {
    const bool end = i == 0 || i == n - 1;
    L[i] = end ? -1 : 0;
    R[i] = end ? -1 : n - 1;
    if (end) keep[i] = 1;
  }
  if (tid == 0) {
    best[0] = 0;
    bidx[0] = SP_NONE;
    *total = 2;
  }
  __syncthreads();
  for (int round = 0; round < n; ++round) {                                          // every round but the last keeps a point
    // (1) the largest key of every pending segment
    for (int i0 = 0; i0 < n; i0 += 256) {
      const int i = i0 + tid;
      int l = -1, r = -1;
      if (i < n) {
        l = sp_ld<G>(L + i);
        r = sp_ld<G>(R + i);
      }
      const bool act = (unsigned)l < (unsigned)n && (unsigned)r < (unsigned)n;
      u64 key = 0, c2;
      if (act) key = sp_key(py[(long)l * ps], px[(long)l * ps], py[(long)r * ps], px[(long)r * ps], py[(long)i * ps], px[(long)i * ps], c2);
      const u64 m = __ballot(act);
      if (!m) continue;                                                              // wave-uniform
      const int lf = __shfl(l, __ffsll((long long)m) - 1, 64);
      if (__ballot(act && l != lf) == 0) {                                           // one segment in this wave: one atomic
        const u64 kmax = sp_wave_max(key);
        if (lane == __ffsll((long long)m) - 1 && kmax > 0) atomicMax(best + l, kmax);
      } else if (act && key > 0) {
        atomicMax(best + l, key);
      }
    }
    __syncthreads();
    // (2) the smallest position among those that have it
    if (tid == 0) *flag = 0;
    for (int i = tid; i < n; i += 256) {
      const int l = sp_ld<G>(L + i), r = sp_ld<G>(R + i);
      if ((unsigned)l >= (unsigned)n || (unsigned)r >= (unsigned)n) continue;
      u64 c2;
      const u64 key = sp_key(py[(long)l * ps], px[(long)l * ps], py[(long)r * ps], px[(long)r * ps], py[(long)i * ps], px[(long)i * ps], c2);
      if (key > 0 && key == sp_ld<G>(best + l)) atomicMin(bidx + l, i);
    }
    __syncthreads();
    // (3) the outcome, read by every pending point; nobody writes a slot here
    for (int i = tid; i < n; i += 256) {
      const int l = sp_ld<G>(L + i), r = sp_ld<G>(R + i);
      if ((unsigned)l >= (unsigned)n || (unsigned)r >= (unsigned)n) continue;
      const u64 k = sp_ld<G>(best + l);
      const int w = sp_ld<G>(bidx + l);
      const long long dy = (long long)py[(long)r * ps] - py[(long)l * ps], dx = (long long)px[(long)r * ps] - px[(long)l * ps];
      const u64 c2 = (u64)dy * (u64)dy + (u64)dx * (u64)dx;
      if (k > 0 && w > l && w < r && sp_split(k, c2, tq2)) {
        if (i == w) {
          R[i] = -2;                                                                 // kept in this round; L stays: the slot to reset
          *flag = 1;
        } else if (i > w) {
          L[i] = w;
        } else {
          R[i] = w;
        }
      } else {
        L[i] = -1;                                                                   // final
      }
    }
    __syncthreads();
    // (4) the new kept points reset the slots of the two segments they made
    int mine = 0;
    for (int i = tid; i < n; i += 256) {
      if (sp_ld<G>(R + i) != -2) continue;
      const int l = sp_ld<G>(L + i);
      R[i] = -1;
      keep[i] = 1;
      ++mine;
      best[i] = 0;
      bidx[i] = SP_NONE;
      if ((unsigned)l < (unsigned)n) {
        best[l] = 0;
        bidx[l] = SP_NONE;
      }
    }
    if (mine) atomicAdd(total, mine);
    __syncthreads();
    if (*flag == 0) break;                                                           // the same word in every lane, after the barrier
  }
  const int v = *total;
  __syncthreads();                                                                   // before the next chain touches flag and total
  return v;
}

__global__ __launch_bounds__(256) void simplify_group_kernel(const int64_t* offsets, const int* points, int M, int P, int per, u64 tq2, int* wL, int* wR,
                                                              u64* wbest, int* wbidx, uint8_t* keep, int* vcount) {
  __shared__ u64 sbest[SP_LDS_MAX];
  __shared__ int sy[SP_LDS_MAX], sx[SP_LDS_MAX], sL[SP_LDS_MAX], sR[SP_LDS_MAX], sbidx[SP_LDS_MAX];
  __shared__ int list[256];
  __shared__ int cnt, flag, total;
  const int tid = threadIdx.x;
  const long long lo = (long long)blockIdx.x * per;
  const long long hi = lo + per < M ? lo + per : M;
  for (long long j0 = lo; j0 < hi; j0 += 256) {                                      // uniform over the workgroup
    if (tid == 0) cnt = 0;
    __syncthreads();
    const long long j = j0 + tid;
    if (j < hi) {
      long long o0, n;
      if (sp_span(offsets, (int)j, P, o0, n) && n > SP_WAVE_MAX) list[atomicAdd(&cnt, 1)] = (int)j;      // the order does not matter
    }
    __syncthreads();
    const int c = cnt;
    for (int k = 0; k < c; ++k) {
      const int js = list[k];
      long long o0, nn;
      sp_span(offsets, js, P, o0, nn);                                               // checked above: 0 <= o0, o0 + nn <= P, nn > SP_WAVE_MAX
      const int n = (int)nn;
      int v;
      if (n <= SP_LDS_MAX) {
        for (int i = tid; i < n; i += 256) {
          const int2 p = *reinterpret_cast<const int2*>(points + 4 * (o0 + i));
          sy[i] = p.x;
          sx[i] = p.y;
        }
        __syncthreads();
        v = sp_chain<false>(n, sy, sx, 1, sL, sR, sbest, sbidx, tq2, keep + o0, &flag, &total);
      } else {
        const int* p = points + 4 * o0;
        v = sp_chain<true>(n, p, p + 1, 4, wL + o0, wR + o0, wbest + o0, wbidx + o0, tq2, keep + o0, &flag, &total);
      }
      if (tid == 0) vcount[js] = v;
    }
    __syncthreads();                                                                 // the list is read before the next batch overwrites it
  }
}

static inline int64_t sp_up(int64_t b) { return (b + 255) / 256 * 256; }

extern "C" int32_t csbsr_simplify_max_tol_q(void) { return SP_MAX_TOL_Q; }

extern "C" int csbsr_simplify_route_limits(int32_t* wave_max, int32_t* lds_max) {
  CSBSR_CHECK(wave_max && lds_max, "simplify_route_limits: null");
  *wave_max = SP_WAVE_MAX;
  *lds_max = SP_LDS_MAX;
  return 0;
}

extern "C" int64_t csbsr_polyline_simplify_work_bytes(int32_t M, int32_t P) {
  if (M < 0 || M > SP_MAX_M || P < 0 || P > SP_MAX_P) return 0;
  return 256 + sp_up(8ll * P) + 3 * sp_up(4ll * P);                                  // best, L, R, bidx: one slot per row
}

extern "C" int csbsr_polyline_simplify(const int64_t* offsets, const int32_t* points, int32_t M, int32_t P, int32_t tol_q, void* work, uint8_t* keep,
                                       int32_t* vcount, csbsr_stream_t s) {
  CSBSR_CHECK(offsets && points && work && keep && vcount, "polyline_simplify: null");
  CSBSR_CHECK((const void*)keep != (const void*)offsets && (const void*)keep != (const void*)points && (void*)keep != work &&
                  (void*)keep != (void*)vcount && (const void*)vcount != (const void*)offsets && (const void*)vcount != (const void*)points &&
                  (void*)vcount != work && (const void*)offsets != work && (const void*)points != work,
              "polyline_simplify: offsets, points, work, keep and vcount are five arrays");
  CSBSR_CHECK(M >= 0 && M <= SP_MAX_M, "polyline_simplify: M = %d spans is outside 0 .. %d", M, SP_MAX_M);
  CSBSR_CHECK(P >= 0 && P <= SP_MAX_P, "polyline_simplify: P = %d rows is outside 0 .. %d", P, SP_MAX_P);
  CSBSR_CHECK(tol_q >= 0 && tol_q <= SP_MAX_TOL_Q, "polyline_simplify: tol_q = %d quarter pixels is outside 0 .. %d", tol_q, SP_MAX_TOL_Q);
  CSBSR_CHECK((reinterpret_cast<uintptr_t>(work) & 15) == 0, "polyline_simplify: work is 16-byte aligned");
  CSBSR_CHECK((reinterpret_cast<uintptr_t>(points) & 15) == 0, "polyline_simplify: points is 16-byte aligned");
  if (P > 0 && hipMemsetAsync(keep, 0, (size_t)P, ST(s)) != hipSuccess) {            // 0 where a row goes and where no span covers it
    csbsr_set_error("polyline_simplify: memset failed");
    return 2;
  }
  if (M == 0) return 0;
  char* w = static_cast<char*>(work) + 256;
  u64* wbest = reinterpret_cast<u64*>(w);
  int* wL = reinterpret_cast<int*>(w + sp_up(8ll * P));
  int* wR = reinterpret_cast<int*>(reinterpret_cast<char*>(wL) + sp_up(4ll * P));
  int* wbidx = reinterpret_cast<int*>(reinterpret_cast<char*>(wR) + sp_up(4ll * P));
  const u64 tq2 = (u64)tol_q * (u64)tol_q;
  hipLaunchKernelGGL(simplify_wave_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, ST(s), offsets, reinterpret_cast<const int2*>(points), M, P, tq2,
                     keep, vcount);
  CSBSR_LAUNCH_CHECK("csbsr_polyline_simplify (wave)");
  const int groups = M < SP_GROUPS ? M : SP_GROUPS;
  const int per = (M + groups - 1) / groups;
  hipLaunchKernelGGL(simplify_group_kernel, dim3(groups), dim3(256), 0, ST(s), offsets, points, M, P, per, tq2, wL, wR, wbest, wbidx, keep, vcount);
  CSBSR_LAUNCH_CHECK("csbsr_polyline_simplify (group)");
  return 0;
}
