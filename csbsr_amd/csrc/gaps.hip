// Crack gap bridging: for every end of the centerline the nearest centerline pixel of ANOTHER crack within a gap of G pixels, the cracks
// those gaps join, and the bridges drawn.  All integers.
//
// Inputs per plane: topo, the bytes of csbsr_skeleton_topology (class = topo & 7: 0 clear, 1 isolated, 2 end, 3 path, 4 junction), and
// labels, any int32 label map: two pixels belong to the same crack iff their labels are equal and non-zero.
//   source    : a pixel p of class 1 or 2 with labels[p] != 0.
//   candidate : a pixel q OF THE SAME PLANE with class != 0 (to_end: class 1 or 2), labels[q] != 0, labels[q] != labels[p] and
//               d2 = |q - p|^2 <= G^2.  Nothing outside the plane and nothing in another plane of the batch is a candidate.
//   the gap of p : the candidate with the smallest 64-bit key (d2 << 32) | q, q the linear index y W + x -- the nearest, and among equals
//               the first in raster order.
//
//   gap_search_kernel : a workgroup owns GP_TH x GP_TW pixels.
//     1. It compacts the tile's source pixels into an LDS list (ballot + one LDS atomic per wave; labels is read only where the class is 1
//        or 2) and writes gap_q = -1, gap_d2 = 0 at every other pixel of the tile.  A tile without a source -- nearly all of a crack map --
//        ends here, having read one byte and written two int32 per pixel.
//     2. It packs "class != 0" (to_end: "class is 1 or 2") of the tile plus a halo of G rows and hw = ceil(G / 32) words per side to bits
//        in LDS, straight from the topo bytes with wave ballots (four loads in flight per lane) -- of that window only the rows and words
//        within G of the sources' bounding box, which step 1 took with LDS atomics: for the one or two ends of a crack map's tile that is
//        less than half of it.  Positions outside the plane enter as CLEAR -- the opposite of width.hip, where the border must not count
//        as background: here a set bit is a candidate, and only pixels of the plane are.  So every set bit is a pixel of this plane, its
//        index q is inside the plane and labels[q] is a read inside the plane.
//     3. The search keeps lim = the best d2 so far, G^2 before there is one, and visits the rows dy = 0, -1, +1, -2, +2, ... while dy^2 <=
//        lim; at a set bit with d2 = dy^2 + dx^2 <= lim it reads labels[q] from global memory -- the skeleton is sparse: few reads, served
//        by L2 -- and keeps the minimum key.  "<=" and not "<": a pixel at the same distance with a smaller index still wins.  A pixel of
//        the source's own crack (the source itself included) is skipped and ends nothing: the own crack is always the nearest set bit.
//        Two routes, the same minimum:
//          a tile with more than GP_WAVE_SRC sources (a dense plane) gives a LANE to each.  In a row the lane visits the set bits with
//            |dx| <= m, m the largest whole number with dy^2 + m^2 <= lim (lim only falls and dy only grows, so m only falls: it is
//            stepped down, never recomputed -- no square root, no floating point);
//          a tile with up to GP_WAVE_SRC sources (a crack map: an end's own crack fills its neighbourhood, a hundred label reads that
//            one lane would make one after the other) gives a WAVE to each: 32 values of dy at a time, a lane per row, |dx| <= G, each
//            lane's best key reduced to the wave's with shuffles before the next 32 rows are looked at.
//     Bounds: lim <= G^2, so dy <= G and |dx| <= G.  The LDS rows are the tile's rows - G .. + G: a source of tile row ly reads the rows
//     (ly + G) +- dy, inside ly .. ly + 2 G and so inside min ly .. max ly + 2 G, the rows that were packed, and inside 0 .. GP_TH + 2 G - 1.
//     The LDS columns start 32 hw >= G pixels left of the tile: a source of tile column lx stands at bx = lx + 32 hw and reads the
//     columns bx - G .. bx + G at the most, inside min lx + 32 hw - G .. max lx + 32 hw + G, whose words were packed, and bx - G >= 32 hw
//     - G >= 0, bx + G <= 32 hw + GP_TW - 1 + G <= 32 (hw + GP_TWW + hw) - 1.  So every row and word touched lies inside the halo, at
//     most GP_ROWS x GP_WPR words, and was written in step 2.
//     Coherence: topo and labels are only read; each pixel's gap_q / gap_d2 is written by exactly one lane of the one workgroup that owns
//     it; no workgroup reads what another writes.
//
//   gap_groups : parent[n][i] = i; then a lane per pixel p with a gap joins the trees of labels[p] - 1 and labels[q] - 1 with cc_union at
//     agent scope -- the discipline of union_find.h unchanged: relaxed agent-scope loads and fetch_min only, a slot only decreases, no
//     flag, no spin, no workgroup waits for another --; then, in a launch of its own (the kernel boundary makes every slot's final value
//     visible), group_labels[p] = cc_find(labels[p] - 1) + 1.  A root is the smallest index of its tree: the result is a minimum over a
//     set and does not depend on scheduling.  Indices are checked against 0 .. H W - 1 before they are used: a label outside 1 .. H W
//     joins nothing and gets group label 0, a gap_q outside the plane is no gap.
//
//   gap_draw : bridge_map is cleared on the stream, then a lane per pixel with a gap draws the 8-connected Bresenham line from the end
//     with the smaller linear index to the other with byte stores of 1.  Both ends are inside the plane and the line stays inside their
//     bounding box, so every store is inside the plane; colliding stores write the same value.  The loop makes max(dx, dy) steps, and
//     is capped at that count.
#include "common.h"
#include "union_find.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define GP_TH 64                          // owned rows of a workgroup
#define GP_TWW 4                          // owned words per row
#define GP_TW (32 * GP_TWW)
#define GP_MAX_G 64
#define GP_MAX_HW ((GP_MAX_G + 31) / 32)  // halo words per side
#define GP_ROWS (GP_TH + 2 * GP_MAX_G)    // 192
#define GP_WPR (GP_TWW + 2 * GP_MAX_HW)   // 8
#define GP_MAX_SIDE 8192                  // 8192^2 = 2^26 pixels: every index fits an int32
#define GP_WAVE_SRC 32                    // up to this many sources in a tile: a wave per source, else a lane

__global__ __launch_bounds__(256) void gap_search_kernel(const uint8_t* topo, const int* labels, int H, int W, int G, int to_end, int* gap_q,
                                                         int* gap_d2) {
  __shared__ uint32_t bits[GP_ROWS * GP_WPR];                                       // 6 KB
  __shared__ uint16_t list[GP_TH * GP_TW];                                          // 16 KB: tile-local index of each source
  __shared__ int count;
  __shared__ int box[4];                                                            // the sources' min ly, max ly, min lx, max lx
  const int tid = threadIdx.x, lane = tid & 63;
  const int y0 = blockIdx.y * GP_TH, x0 = blockIdx.x * GP_TW;
  const long base = (long)blockIdx.z * H * W;
  if (tid == 0) {
    count = 0;
    box[0] = GP_TH;
    box[1] = -1;
    box[2] = GP_TW;
    box[3] = -1;
  }
  __syncthreads();
  for (int i = tid; i < GP_TH * GP_TW; i += 256) {                                  // every lane makes every trip: the ballots are whole
    const int ly = i / GP_TW, lx = i - ly * GP_TW;
    const int gy = y0 + ly, gx = x0 + lx;
    bool src = false;
    if (gy < H && gx < W) {
      const long o = base + (long)gy * W + gx;
      const int c = topo[o] & 7;
      src = (c == 1 || c == 2) && labels[o] != 0;
      if (!src) {
        gap_q[o] = -1;
        gap_d2[o] = 0;
      }
    }
    const unsigned long long m = __ballot(src);
    if (m) {                                                                        // wave-uniform
      int b = 0;
      if (lane == 0) b = atomicAdd(&count, __popcll(m));
      b = __shfl(b, 0);
      if (src) {
        list[b + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)i;
        atomicMin(&box[0], ly);
        atomicMax(&box[1], ly);
        atomicMin(&box[2], lx);
        atomicMax(&box[3], lx);
      }
    }
  }
  __syncthreads();
  const int n = count;
  if (n == 0) return;                                                               // the whole workgroup
  const int hw = (G + 31) >> 5, wpr = GP_TWW + 2 * hw;
  const int r0 = box[0], nrows = box[1] + 2 * G - r0 + 1;                            // halo rows min ly .. max ly + 2 G, inside 0 .. rows - 1
  const int w0 = (box[2] + 32 * hw - G) >> 5, nw = ((box[3] + 32 * hw + G) >> 5) - w0 + 1;      // and words, inside 0 .. wpr - 1
  const int rowpx = nw * 32, total = nrows * rowpx;                                 // a multiple of 32, <= 192 * 256
  const int gy0 = y0 - G + r0, gx0 = x0 - 32 * hw + 32 * w0;
  for (int i0 = tid; i0 < ((total + 1023) & ~1023); i0 += 1024) {                   // every lane makes every trip: the ballots are whole
    bool v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 256 * u;
      v[u] = false;                                                                 // outside the plane: clear, never a candidate
      if (i < total) {
        const int rr = i / rowpx, c = i - rr * rowpx;
        const int gy = gy0 + rr, gx = gx0 + c;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
          const int cl = topo[base + (long)gy * W + gx] & 7;
          v[u] = to_end ? (cl == 1 || cl == 2) : cl != 0;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 256 * u;
      const unsigned long long b = __ballot(v[u]);
      if ((tid & 31) == 0 && i < total) {
        const int rr = i / rowpx, c = i - rr * rowpx;
        bits[(r0 + rr) * wpr + w0 + (c >> 5)] = (uint32_t)(b >> (tid & 32));
      }
    }
  }
  __syncthreads();
  const int* lab = labels + base;
  if (n <= GP_WAVE_SRC) {                                                           // the whole workgroup: a wave per source
    for (int k = tid >> 6; k < n; k += 4) {
      const int p = list[k];
      const int ly = p / GP_TW, lx = p - ly * GP_TW;
      const int py = y0 + ly, px = x0 + lx;
      const int row = ly + G, bx = lx + 32 * hw;
      const int mine = lab[py * W + px];
      const int lo = bx - G, hi = bx + G;                                           // 0 <= lo, hi < 32 wpr
      int lim = G * G, bq = -1;                                                     // wave-uniform
      for (int d0 = 0; d0 <= G && d0 * d0 <= lim; d0 += 32) {
        const int dy = d0 + (lane >> 1), ry = (lane & 1) ? dy : -dy, dy2 = dy * dy;
        int llim = lim, lq = -1;                                                    // this lane's row
        if (dy <= G && dy2 <= lim && !(dy == 0 && (lane & 1))) {                    // dy <= G: the row is inside the halo
          const uint32_t* R = bits + (row + ry) * wpr;
          for (int w = lo >> 5; w <= (hi >> 5); ++w) {
            uint32_t word = R[w];
            if (w == (lo >> 5)) word &= 0xFFFFFFFFu << (lo & 31);
            if (w == (hi >> 5)) word &= 0xFFFFFFFFu >> (31 - (hi & 31));
            while (word) {
              const int c = 32 * w + __builtin_ctz(word);
              word &= word - 1;
              const int dx = c - bx;
              const int d = dy2 + dx * dx;
              if (d > llim || (d == llim && lq >= 0)) continue;                     // q grows along the row: an equal d2 later loses
              const int q = (py + ry) * W + px + dx;                                // a set bit: a pixel of the plane
              const int l = lab[q];
              if (l == 0 || l == mine) continue;
              llim = d;
              lq = q;
            }
          }
        }
        unsigned long long key = lq >= 0 ? ((unsigned long long)llim << 32) | (unsigned int)lq : ~0ull;
        for (int o = 32; o; o >>= 1) {
          const unsigned long long other = __shfl_xor(key, o);
          key = other < key ? other : key;
        }
        const unsigned long long cur = bq >= 0 ? ((unsigned long long)lim << 32) | (unsigned int)bq : ~0ull;
        if (key < cur) {
          lim = (int)(key >> 32);
          bq = (int)(key & 0xFFFFFFFFull);
        }
      }
      if (lane == 0) {
        const long o = base + (long)py * W + px;
        gap_q[o] = bq;
        gap_d2[o] = bq >= 0 ? lim : 0;
      }
    }
    return;
  }
  for (int k = tid; k < n; k += 256) {
    const int p = list[k];
    const int ly = p / GP_TW, lx = p - ly * GP_TW;
    const int py = y0 + ly, px = x0 + lx;
    const int row = ly + G, bx = lx + 32 * hw;
    const int mine = lab[py * W + px];
    int lim = G * G, bq = -1, m = G;                                                // lim: the best d2, G^2 while there is none
    for (int dy = 0; dy * dy <= lim; ++dy) {                                        // lim <= G^2: dy <= G, the row is inside the halo
      for (int s = 0; s < (dy ? 2 : 1); ++s) {
        const int dy2 = dy * dy;
        if (dy2 > lim) break;                                                       // the row above lowered lim below this distance
        while (dy2 + m * m > lim) --m;                                              // dy2 <= lim: ends at m >= 0
        const int ry = s ? dy : -dy;
        const uint32_t* R = bits + (row + ry) * wpr;
        const int lo = bx - m, hi = bx + m;                                         // 0 <= lo, hi < 32 wpr
        for (int w = lo >> 5; w <= (hi >> 5); ++w) {
          uint32_t word = R[w];
          if (w == (lo >> 5)) word &= 0xFFFFFFFFu << (lo & 31);
          if (w == (hi >> 5)) word &= 0xFFFFFFFFu >> (31 - (hi & 31));
          while (word) {
            const int c = 32 * w + __builtin_ctz(word);
            word &= word - 1;
            const int dx = c - bx;
            const int d = dy2 + dx * dx;
            if (d > lim) continue;
            const int q = (py + ry) * W + px + dx;                                  // a set bit: a pixel of the plane
            if (d == lim && bq >= 0 && q > bq) continue;
            const int l = lab[q];
            if (l == 0 || l == mine) continue;
            lim = d;
            bq = q;
          }
        }
      }
    }
    const long o = base + (long)py * W + px;
    gap_q[o] = bq;
    gap_d2[o] = bq >= 0 ? lim : 0;
  }
}

__global__ __launch_bounds__(256) void gap_parent_init_kernel(int hw, int* parent) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < hw) parent[(long)blockIdx.y * hw + i] = i;
}

__global__ __launch_bounds__(256) void gap_union_kernel(const int* labels, const int* gap_q, int hw, int* parent) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long n = blockIdx.y;
  const int q = gap_q[n * hw + i];
  if (q < 0 || q >= hw) return;
  const int a = labels[n * hw + i] - 1, b = labels[n * hw + q] - 1;
  if (a < 0 || a >= hw || b < 0 || b >= hw) return;                                 // no valid root index: nothing is indexed with it
  cc_union<CC_AGENT>(parent + n * hw, a, b);
}

__global__ __launch_bounds__(256) void gap_flatten_kernel(const int* labels, const int* parent, int hw, int* group_labels) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long n = blockIdx.y;
  const int a = labels[n * hw + i] - 1;
  group_labels[n * hw + i] = (a >= 0 && a < hw) ? cc_find<CC_AGENT>(parent + n * hw, a) + 1 : 0;
}

__global__ __launch_bounds__(256) void gap_draw_kernel(const int* gap_q, int W, int hw, uint8_t* bridge_map) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long n = blockIdx.y;
  const int q = gap_q[n * hw + i];
  if (q < 0 || q >= hw) return;
  const int a = min(i, q), b = max(i, q);                                           // from the smaller linear index: y1 >= y0
  int y = a / W, x = a - y * W;
  const int y1 = b / W, x1 = b - y1 * W;
  const int dx = abs(x1 - x), dy = y1 - y, sx = x1 > x ? 1 : (x1 < x ? -1 : 0);
  int err = dx - dy;
  uint8_t* out = bridge_map + n * hw;
  for (int step = max(dx, dy); step >= 0; --step) {                                 // max(dx, dy) + 1 pixels, all inside the ends' box
    out[y * W + x] = 1;
    if (y == y1 && x == x1) break;
    const int e2 = 2 * err;
    if (e2 > -dy) {
      err -= dy;
      x += sx;
    }
    if (e2 < dx) {
      err += dx;
      y += 1;
    }
  }
}

static int gp_dims_ok(const char* what, int32_t N, int32_t H, int32_t W) {
  CSBSR_CHECK(N >= 1 && N <= 65535, "%s: 1 .. 65535 planes, got %d", what, N);
  CSBSR_CHECK(H >= 1 && W >= 1 && H <= GP_MAX_SIDE && W <= GP_MAX_SIDE, "%s: %d x %d is outside 1 .. %d per side (int32 indices)", what, H, W,
              GP_MAX_SIDE);
  return 0;
}

extern "C" int32_t csbsr_gap_max_radius(void) { return GP_MAX_G; }

extern "C" int csbsr_endpoint_gaps(const uint8_t* topo, const int32_t* labels, int32_t N, int32_t H, int32_t W, int32_t G, int32_t to_end,
                                   int32_t* gap_q, int32_t* gap_d2, csbsr_stream_t s) {
  CSBSR_CHECK(topo && labels && gap_q && gap_d2, "endpoint_gaps: null");
  if (gp_dims_ok("endpoint_gaps", N, H, W)) return 1;
  CSBSR_CHECK(G >= 2 && G <= GP_MAX_G, "endpoint_gaps: the gap is 2 .. %d, got %d", GP_MAX_G, G);
  CSBSR_CHECK(to_end == 0 || to_end == 1, "endpoint_gaps: to_end is 0 or 1, got %d", to_end);
  CSBSR_CHECK(gap_q != gap_d2 && (const void*)gap_q != (const void*)labels && (const void*)gap_d2 != (const void*)labels,
              "endpoint_gaps: gap_q, gap_d2 and labels are three arrays");
  hipLaunchKernelGGL(gap_search_kernel, dim3((W + GP_TW - 1) / GP_TW, (H + GP_TH - 1) / GP_TH, N), dim3(256), 0, ST(s), topo, labels, H, W, G,
                     to_end, gap_q, gap_d2);
  CSBSR_LAUNCH_CHECK("csbsr_endpoint_gaps");
  return 0;
}

extern "C" int csbsr_gap_groups(const int32_t* labels, const int32_t* gap_q, int32_t N, int32_t H, int32_t W, int32_t* parent,
                                int32_t* group_labels, csbsr_stream_t s) {
  CSBSR_CHECK(labels && gap_q && parent && group_labels, "gap_groups: null");
  if (gp_dims_ok("gap_groups", N, H, W)) return 1;
  CSBSR_CHECK(parent != group_labels && (const void*)parent != (const void*)labels && (const void*)parent != (const void*)gap_q,
              "gap_groups: parent is scratch of its own");
  const int hw = H * W;
  const dim3 grid((hw + 255) / 256, N);
  hipLaunchKernelGGL(gap_parent_init_kernel, grid, dim3(256), 0, ST(s), hw, parent);
  CSBSR_LAUNCH_CHECK("csbsr_gap_groups (init)");
  hipLaunchKernelGGL(gap_union_kernel, grid, dim3(256), 0, ST(s), labels, gap_q, hw, parent);
  CSBSR_LAUNCH_CHECK("csbsr_gap_groups (union)");
  hipLaunchKernelGGL(gap_flatten_kernel, grid, dim3(256), 0, ST(s), labels, parent, hw, group_labels);
  CSBSR_LAUNCH_CHECK("csbsr_gap_groups (flatten)");
  return 0;
}

extern "C" int csbsr_gap_draw(const int32_t* gap_q, int32_t N, int32_t H, int32_t W, uint8_t* bridge_map, csbsr_stream_t s) {
  CSBSR_CHECK(gap_q && bridge_map, "gap_draw: null");
  if (gp_dims_ok("gap_draw", N, H, W)) return 1;
  CSBSR_CHECK((const void*)gap_q != (const void*)bridge_map, "gap_draw: bridge_map is another array than gap_q");
  const int hw = H * W;
  const hipError_t e = hipMemsetAsync(bridge_map, 0, (size_t)N * (size_t)hw, ST(s));
  CSBSR_CHECK(e == hipSuccess, "gap_draw: clearing the map failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(gap_draw_kernel, dim3((hw + 255) / 256, N), dim3(256), 0, ST(s), gap_q, W, hw, bridge_map);
  CSBSR_LAUNCH_CHECK("csbsr_gap_draw");
  return 0;
}
