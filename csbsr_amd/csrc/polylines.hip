// Crack polylines: the position of every branch pixel along its branch, and the ordered points of every branch.
//
// ``topo`` and ``blabels`` are those of branches.hip: a BRANCH PIXEL has class 1, 2 or 3, an INNER link is an owned E / S / SE / SW link whose
// two ends are branch pixels, a branch is a component of the branch pixels under the inner links and its label 1 + its smallest linear index.
// The DEGREE of a branch pixel is the number of its inner links, those it owns and those its W / N / NW / NE neighbour owns.  A branch is a
// CHAIN when no pixel of it has a degree above 2.  A chain with TERMINALS (degree <= 1) is a path -- it has two of them, or is one pixel --
// and starts at the terminal with the smaller linear index; a chain without one is a cycle, starts at its first pixel in raster order
// (blabel - 1) and is walked from there first to the start's neighbour with the smaller linear index.  rank = the inner links walked from
// the start, diag = the SE / SW links among them; both are -1 at clear pixels, at junction pixels and at every pixel of a branch that is no
// chain.  The values are defined by minima of indices, so every correct execution order gives the same bits.
//
// A walk costs one step per pixel of length; here every pixel learns its position in ceil(log2(P)) rounds of pointer jumping over the
// compact list of the call's P branch pixels (list ranking, Wyllie):
//
//   branch_count_kernel  : P, for the caller to size the list (the call's one host read, 8 bytes).  One integer atomic per workgroup that
//                          holds a branch pixel.
//   order_local_kernel   : a workgroup owns PL_TH x PL_TW pixels and loads their topo bytes with a one-pixel halo into LDS (zero outside the
//                          plane, so a link out of the plane is ignored).  A tile without a branch pixel only writes -1.  Otherwise the branch
//                          pixels are compacted: wave ballots give a lane its place, ONE atomic add per workgroup gives the workgroup its
//                          first slot.  A branch pixel finds its degree and its first two inner neighbours from its own link bits and the
//                          E / S / SE / SW bits of its W / N / NW / NE neighbours, writes its list entry (pixel, plane, the two neighbour
//                          pixels, whether each link is diagonal, degree > 2, degree <= 1) and leaves its SLOT in ``rank`` -- scratch until the
//                          last launch -- and -1 in ``diag``.  The slot order differs from run to run; nothing that is returned depends on it.
//   order_link_kernel    : per slot: the neighbours' slots and the slot of the branch's first pixel (the ROOT slot), read from ``rank``; a
//                          pixel of degree > 2 or <= 1 ORs its flag into flags[root slot].
//   order_init_kernel    : per slot and side s (0, 1) the HALF-STATE of the walk that leaves the pixel through side s after one link:
//                          (the slot reached, links walked, diagonal links walked, the side through which to go on from there or STOP | the
//                          side through which it was entered), 16 bytes.  STOPS are the terminals and, in a branch without one, the root.  A
//                          side without a neighbour, and both sides of a pixel of a branch that is no chain, stay at the pixel with 0 links.
//   order_jump_kernel    : R = ceil(log2(P)) launches.  A half-state that has not stopped appends the half-state of the slot it has reached
//                          on the side it goes on through: one 16-byte load of its own state, one of the other, one 16-byte store.  After k
//                          rounds a half-state has walked min(2^k, links to its stop), and no walk is longer than P - 1 links.
//   order_finish_kernel  : per slot: a path pixel takes the half-state that has reached the terminal with the smaller linear index; a cycle
//                          pixel the one that has entered the root through the side of the root's smaller-index neighbour (it came the
//                          way the walk goes, backwards); the root of a cycle is 0; a pixel of a branch that is no chain writes -1.
//   branch_scatter_kernel: one lane per pixel; a pixel with rank >= 0 writes (y, x, diag, d2) to row offset[root] + rank of the table.  No sort:
//                          rank is the position.
//
// Coherence.  No launch reads a word that another workgroup writes in the same launch, with two exceptions, both integer atomics performed at
// the memory side: the slot counter (atomic add, whose return value alone is used) and the flags (atomic or; read only in later launches).
// Everything else is written by exactly one lane with a plain store and read, with plain loads, only in LATER launches of the same stream, after
// the kernel boundary has made it visible: ``rank`` as the slot map is written by order_local_kernel, read by order_link_kernel and
// overwritten by order_finish_kernel, which reads only the list; a jump round reads one buffer of half-states and writes the other
// (ping-pong), so a round sees only the previous round's state whatever the order of the workgroups.  There is no flag to wait for, no spin,
// no loop whose trip count depends on data (the jump kernel makes one step per launch), and no workgroup waits for another.
//
// Bounds.  Every index is checked before it is used: a slot at or above the caller's P is never written (the pixel then counts as no branch
// pixel), the list kernels run over min(P, the slots handed out), and a label, slot or table row outside its range is ignored -- a wrong P,
// a foreign ``blabels`` or wrong offsets give wrong numbers, never an access outside an array.
#include "common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define PL_TH 64                          // owned rows of a workgroup: the tile of branches.hip
#define PL_TW 128
#define PL_LW (PL_TW + 4)                 // LDS pitch of a row with its halo (PL_TW + 2 used)
#define PL_MAX_SIDE 8192
#define PL_MAX_P (1 << 28)                // 4 P half-states and their indices fit an int32
#define PL_STOP 2
#define PL_HEAD 256                       // bytes in front of ``work``: the slot counter

#define PL_IS(t) ((((uint32_t)(t) & 7u) - 1u) < 3u)                                 // class 1, 2 or 3

__global__ __launch_bounds__(256) void branch_count_kernel(const uint8_t* topo, long total, unsigned long long* count) {
  __shared__ int wsum[4];
  const int tid = threadIdx.x;
  const long i0 = (long)blockIdx.x * (PL_TH * PL_TW);
  int n = 0;
  for (int k = 0; k < PL_TH * PL_TW / 256; ++k) {                                   // every lane makes every trip: the ballots are whole
    const long i = i0 + k * 256 + tid;
    const bool b = i < total && PL_IS(topo[i]);
    n += __popcll(__ballot(b));
  }
  if ((tid & 63) == 0) wsum[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    const int t = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (t) atomicAdd(count, (unsigned long long)t);
  }
}

__global__ __launch_bounds__(256) void order_local_kernel(const uint8_t* topo, int H, int W, int* rank, int* diag, int* counter, int4* ent, int cap) {
  __shared__ uint8_t tb[(PL_TH + 2) * PL_LW];
  __shared__ int wsum[4];
  __shared__ int first;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int y0 = blockIdx.y * PL_TH, x0 = blockIdx.x * PL_TW;
  const long base = (long)blockIdx.z * H * W;
  bool own = false;
  for (int i = tid; i < (PL_TH + 2) * (PL_TW + 2); i += 256) {
    const int r = i / (PL_TW + 2), c = i - r * (PL_TW + 2);
    const int gy = y0 + r - 1, gx = x0 + c - 1;
    uint32_t t = 0;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) t = topo[base + (long)gy * W + gx];
    tb[r * PL_LW + c] = (uint8_t)t;
    own |= r >= 1 && r <= PL_TH && c >= 1 && c <= PL_TW && PL_IS(t);
  }
  if (!__syncthreads_or(own)) {                                                     // no branch pixel among the owned ones
    for (int i = tid; i < PL_TH * PL_TW; i += 256) {
      const int r = i / PL_TW, c = i - r * PL_TW;
      const int gy = y0 + r, gx = x0 + c;
      if (gy < H && gx < W) rank[base + (long)gy * W + gx] = diag[base + (long)gy * W + gx] = -1;
    }
    return;                                                                         // the whole workgroup
  }
  int n = 0;
  for (int i = tid; i < PL_TH * PL_TW; i += 256) {                                  // 32 trips, every lane makes every one
    const int r = i / PL_TW, c = i - r * PL_TW;
    n += __popcll(__ballot(PL_IS(tb[(r + 1) * PL_LW + c + 1])));
  }
  if (lane == 0) wsum[wave] = n;
  __syncthreads();
  if (tid == 0) first = atomicAdd(counter, wsum[0] + wsum[1] + wsum[2] + wsum[3]);
  __syncthreads();
  int slot0 = first;
  for (int w = 0; w < wave; ++w) slot0 += wsum[w];
  for (int i = tid; i < PL_TH * PL_TW; i += 256) {
    const int r = i / PL_TW, c = i - r * PL_TW;
    const int gy = y0 + r, gx = x0 + c;
    const uint8_t* p = tb + (r + 1) * PL_LW + c + 1;
    const uint32_t t = p[0];
    const bool b = PL_IS(t);
    const unsigned long long m = __ballot(b);
    const int slot = slot0 + __popcll(m & ((1ull << lane) - 1ull));
    slot0 += __popcll(m);
    if (gy >= H || gx >= W) continue;
    const long g = base + (long)gy * W + gx;
    diag[g] = -1;
    if (!b || slot < 0 || slot >= cap) {                                            // a slot past the caller's P is never written
      rank[g] = -1;
      continue;
    }
    int nb[2] = {-1, -1};
    int deg = 0, info = 0;
    // the inner links: owned E, S, SE, SW, then the E / S / SE / SW link of the W / N / NW / NE neighbour
    const int dy[8] = {0, 1, 1, 1, 0, -1, -1, -1}, dx[8] = {1, 0, 1, -1, -1, 0, -1, 1};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t u = p[dy[k] * PL_LW + dx[k]];
      const uint32_t owner = k < 4 ? t : u;
      if (!((owner >> (4 + (k & 3))) & 1u) || !PL_IS(u)) continue;
      if (deg < 2) {
        nb[deg] = (gy + dy[k]) * W + gx + dx[k];
        info |= ((k & 3) >= 2 ? 1 : 0) << deg;
      }
      ++deg;
    }
    info |= (deg > 2 ? 4 : 0) | (deg <= 1 ? 8 : 0);
    ent[slot] = make_int4(gy * W + gx, (int)blockIdx.z | (info << 16), nb[0], nb[1]);
    rank[g] = slot;
  }
}

// ent: (pixel, plane | info << 16, neighbour pixel 0, neighbour pixel 1);  lnk: (neighbour slot 0, neighbour slot 1, root slot, info)
__global__ __launch_bounds__(256) void order_link_kernel(const int4* ent, const int* rank, const int* blabels, int hw, const int* counter, int cap,
                                                         int4* lnk, int* flags) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int n = min(cap, *counter);
  if (k >= n) return;
  const int4 e = ent[k];
  const long pb = (long)(e.y & 0xffff) * hw;
  int info = e.y >> 16;
  int ns[2] = {e.z >= 0 ? rank[pb + e.z] : -1, e.w >= 0 ? rank[pb + e.w] : -1};
  if ((unsigned)ns[0] >= (unsigned)n) ns[0] = -1;
  if ((unsigned)ns[1] >= (unsigned)n) ns[1] = -1;
  const int lab = blabels[pb + e.x];
  int root = lab >= 1 && lab <= hw ? rank[pb + lab - 1] : -1;
  if ((unsigned)root >= (unsigned)n) root = -1;
  const int f = ((info >> 2) & 1) | ((info >> 3) & 1) << 1;                         // 1: a pixel of degree > 2, 2: a terminal
  if (root >= 0 && f) atomicOr(flags + root, f);
  lnk[k] = make_int4(ns[0], ns[1], root, info);
}

__global__ __launch_bounds__(256) void order_init_kernel(const int4* lnk, const int* flags, const int* counter, int cap, int4* state) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int n = min(cap, *counter);
  if (k >= n) return;
  const int4 e = lnk[k];
  const int fl = e.z >= 0 ? flags[e.z] : 1;
  const bool chain = !(fl & 1), terminals = fl & 2;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int q = s ? e.y : e.x;
    int4 st = make_int4(k, 0, 0, PL_STOP);
    if (chain && q >= 0) {
      const int4 f = lnk[q];
      const int en = f.x == k ? 0 : 1;                                              // the side of q that leads back here
      const bool stop = ((f.w >> 3) & 1) || (!terminals && q == e.z) || (en ? f.y : f.x) != k || (en ? f.x : f.y) < 0;
      st = make_int4(q, 1, (e.w >> s) & 1, (stop ? PL_STOP : 1 - en) | en << 2);
    }
    state[2 * k + s] = st;
  }
}

__global__ __launch_bounds__(256) void order_jump_kernel(const int4* in, int4* out, const int* counter, int cap) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int n = min(cap, *counter);
  if (j >= 2 * n) return;
  int4 s = in[j];
  const int c = s.w & 3;
  if (c != PL_STOP) {
    const int4 t = in[2 * s.x + c];
    s = make_int4(t.x, s.y + t.y, s.z + t.z, t.w);
  }
  out[j] = s;
}

__global__ __launch_bounds__(256) void order_finish_kernel(const int4* ent, const int4* lnk, const int* flags, const int4* state, int hw,
                                                           const int* counter, int cap, int* rank, int* diag) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int n = min(cap, *counter);
  if (k >= n) return;
  const int4 e = ent[k], l = lnk[k];
  const int fl = l.z >= 0 ? flags[l.z] : 1;
  int r = -1, d = -1;
  if (!(fl & 1)) {
    const int4 a = state[2 * k], b = state[2 * k + 1];
    if (fl & 2) {                                                                   // a path: from the terminal with the smaller index
      const bool first = ent[a.x].x <= ent[b.x].x;
      r = first ? a.y : b.y;
      d = first ? a.z : b.z;
    } else if (k == l.z) {
      r = d = 0;
    } else {                                                                        // a cycle: the walk leaves the root through its smaller neighbour
      const int4 rt = lnk[l.z];
      if (rt.x >= 0 && rt.y >= 0) {
        const int side = ent[rt.x].x < ent[rt.y].x ? 0 : 1;
        const bool first = ((a.w >> 2) & 1) == side;
        r = first ? a.y : b.y;
        d = first ? a.z : b.z;
      }
    }
  }
  const long g = (long)(e.y & 0xffff) * hw + e.x;
  rank[g] = r;
  diag[g] = d;
}

__global__ __launch_bounds__(256) void branch_scatter_kernel(const int* blabels, const int* rank, const int* diag, const int* d2, const int* offsets,
                                                             int hw, int W, int rows, int4* points) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long base = (long)blockIdx.y * hw;
  const int r = rank[base + i];
  if (r < 0) return;
  const int lab = blabels[base + i];
  if (lab < 1 || lab > hw) return;
  const long row = (long)offsets[base + lab - 1] + r;
  if (row < 0 || row >= rows) return;
  points[row] = make_int4(i / W, i - i / W * W, diag[base + i], d2 ? d2[base + i] : 0);
}

static int pl_dims_ok(const char* what, int32_t N, int32_t H, int32_t W) {
  CSBSR_CHECK(N >= 1 && N <= 65535, "%s: 1 .. 65535 planes, got %d", what, N);
  CSBSR_CHECK(H >= 1 && W >= 1 && H <= PL_MAX_SIDE && W <= PL_MAX_SIDE, "%s: %d x %d is outside 1 .. %d per side (int32 indices)", what, H, W,
              PL_MAX_SIDE);
  return 0;
}

static inline int64_t pl_up(int64_t b) { return (b + 255) / 256 * 256; }

extern "C" int32_t csbsr_branch_order_rounds(int32_t P) {
  int r = 0;
  while (r < 31 && (1ll << r) < (long long)P) ++r;                                  // ceil(log2(P)), 0 for P <= 1
  return r;
}

extern "C" int64_t csbsr_branch_order_work_bytes(int32_t P) {
  if (P < 0 || P > PL_MAX_P) return 0;
  return PL_HEAD + pl_up(4ll * P) + 2 * pl_up(16ll * P) + pl_up(64ll * P);           // counter, flags, ent, lnk, two buffers of 2 P half-states
}

extern "C" int csbsr_branch_count(const uint8_t* topo, int32_t N, int32_t H, int32_t W, int64_t* count, csbsr_stream_t s) {
  CSBSR_CHECK(topo && count, "branch_count: null");
  if (pl_dims_ok("branch_count", N, H, W)) return 1;
  if (hipMemsetAsync(count, 0, 8, ST(s)) != hipSuccess) {
    csbsr_set_error("branch_count: memset failed");
    return 2;
  }
  const long total = (long)N * H * W;
  hipLaunchKernelGGL(branch_count_kernel, dim3((unsigned)((total + PL_TH * PL_TW - 1) / (PL_TH * PL_TW))), dim3(256), 0, ST(s), topo, total,
                     reinterpret_cast<unsigned long long*>(count));
  CSBSR_LAUNCH_CHECK("csbsr_branch_count");
  return 0;
}

extern "C" int csbsr_branch_order(const uint8_t* topo, const int32_t* blabels, int32_t N, int32_t H, int32_t W, int32_t P, void* work,
                                  int32_t* rank, int32_t* diag, csbsr_stream_t s) {
  CSBSR_CHECK(topo && blabels && work && rank && diag, "branch_order: null");
  CSBSR_CHECK(rank != diag && rank != blabels && diag != blabels && (const void*)rank != (const void*)topo && (const void*)diag != (const void*)topo &&
                  (void*)rank != work && (void*)diag != work && (const void*)topo != work && (const void*)blabels != work,
              "branch_order: topo, blabels, work, rank and diag are five arrays");
  if (pl_dims_ok("branch_order", N, H, W)) return 1;
  CSBSR_CHECK(P >= 0 && P <= PL_MAX_P, "branch_order: P = %d branch pixels is outside 0 .. %d", P, PL_MAX_P);
  CSBSR_CHECK((reinterpret_cast<uintptr_t>(work) & 15) == 0, "branch_order: work is 16-byte aligned");
  char* w = static_cast<char*>(work);
  int* counter = reinterpret_cast<int*>(w);
  int* flags = reinterpret_cast<int*>(w + PL_HEAD);
  int4* ent = reinterpret_cast<int4*>(w + PL_HEAD + pl_up(4ll * P));
  int4* lnk = reinterpret_cast<int4*>(reinterpret_cast<char*>(ent) + pl_up(16ll * P));
  int4* st[2];
  st[0] = reinterpret_cast<int4*>(reinterpret_cast<char*>(lnk) + pl_up(16ll * P));
  st[1] = st[0] + 2l * P;
  if (hipMemsetAsync(w, 0, PL_HEAD + pl_up(4ll * P), ST(s)) != hipSuccess) {         // the counter and the flags
    csbsr_set_error("branch_order: memset failed");
    return 2;
  }
  hipLaunchKernelGGL(order_local_kernel, dim3((W + PL_TW - 1) / PL_TW, (H + PL_TH - 1) / PL_TH, N), dim3(256), 0, ST(s), topo, H, W, rank, diag, counter,
                     ent, P);
  CSBSR_LAUNCH_CHECK("csbsr_branch_order (local)");
  if (P == 0) return 0;
  const int hw = H * W, gp = (P + 255) / 256, R = csbsr_branch_order_rounds(P);
  hipLaunchKernelGGL(order_link_kernel, dim3(gp), dim3(256), 0, ST(s), ent, rank, blabels, hw, counter, P, lnk, flags);
  CSBSR_LAUNCH_CHECK("csbsr_branch_order (link)");
  hipLaunchKernelGGL(order_init_kernel, dim3(gp), dim3(256), 0, ST(s), lnk, flags, counter, P, st[0]);
  CSBSR_LAUNCH_CHECK("csbsr_branch_order (init)");
  for (int r = 0; r < R; ++r) {                                                     // ceil(log2(P)) launches, whatever the branches' lengths
    hipLaunchKernelGGL(order_jump_kernel, dim3((2 * P + 255) / 256), dim3(256), 0, ST(s), st[r & 1], st[(r + 1) & 1], counter, P);
    CSBSR_LAUNCH_CHECK("csbsr_branch_order (jump)");
  }
  hipLaunchKernelGGL(order_finish_kernel, dim3(gp), dim3(256), 0, ST(s), ent, lnk, flags, st[R & 1], hw, counter, P, rank, diag);
  CSBSR_LAUNCH_CHECK("csbsr_branch_order (finish)");
  return 0;
}

extern "C" int csbsr_branch_scatter(const int32_t* blabels, const int32_t* rank, const int32_t* diag, const int32_t* d2, const int32_t* offsets,
                                    int32_t N, int32_t H, int32_t W, int32_t rows, int32_t* points, csbsr_stream_t s) {
  CSBSR_CHECK(blabels && rank && diag && offsets && points, "branch_scatter: null");
  CSBSR_CHECK(points != blabels && points != rank && points != diag && points != d2 && points != offsets,
              "branch_scatter: points is another array than its inputs");
  if (pl_dims_ok("branch_scatter", N, H, W)) return 1;
  CSBSR_CHECK(rows >= 0, "branch_scatter: %d rows", rows);
  CSBSR_CHECK((reinterpret_cast<uintptr_t>(points) & 15) == 0, "branch_scatter: points is 16-byte aligned");
  if (rows == 0) return 0;
  const int hw = H * W;
  hipLaunchKernelGGL(branch_scatter_kernel, dim3((hw + 255) / 256, N), dim3(256), 0, ST(s), blabels, rank, diag, d2, offsets, hw, W, rows,
                     reinterpret_cast<int4*>(points));
  CSBSR_LAUNCH_CHECK("csbsr_branch_scatter");
  return 0;
}
