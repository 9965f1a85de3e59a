// Input gradient AND weight gradient of the kernel predictor's full-resolution 1x1 layers (fe_SR.1, fe_cat.0: 49 -> 32 channels at
// 1792^2, kbpn.py:521-578) from ONE pass over the two maps both need.  The dgrad of such a layer reads its dPre (32 channels) and, as
// the activation-derivative mask of the layer below, the layer's own input (49 channels stored as 56); the wgrad reads exactly the
// same two maps: G[o][c] = sum_pix dPre[pix][o] * in[pix][c].  As two launches the pair moved the maps twice (conv_hr_kernel<4,taps=1,
// nct=2,mask=1> + conv_wgrad_kernel<32,128,1,4>); both are HBM-bound and the MFMA work of either is small next to the traffic.
//
//  * a persistent workgroup (four waves, one per SIMD) walks 8 x 32 pixel tiles in conv_hr's tile order; the dPre tile (80-byte pixel
//    pitch: five 16-byte slots, conflict-free for ds_read_b128 as in conv_hr.hip) and the input tile (112-byte pitch) go HBM -> LDS
//    with buffer_load ... lds into a ring of three tile buffers, one piece at a time between the MFMAs of the current tile;
//  * dIn = (dPre . W) x gate(in): conv_hr's product path -- the same fragment-ordered fp16 weights (csbsr_pack_weights_hr, kind 1) in
//    registers, the same MFMA and the same order of the two K slices, the same register epilogue -- so dIn is bit-identical to the
//    dgrad it replaces; the mask comes from the input tile in LDS instead of a second read of the map;
//  * G: pixels as K through the transposing LDS read (ds_read_b64_tr_b16) of both tiles, as in conv_wgrad_hr.hip; a wave owns one
//    32 x 32 block of G (input channels 0-31 or 32-63) for half of the tile's rows, the halves meet in LDS at the end;
//  * every workgroup writes one fp32 slab G[32][56] in csbsr_conv_wgrad's layout; csbsr_unpack_wgrad folds them in a fixed order.
#include "common.h"
#include "conv_wgrad.h"

#define PR_TH 8
#define PR_TW 32
#define PR_NBUF 3

struct PairK {
  const half_t* a; long a_sn, a_sy, a_sx;      // dPre [N, H, W, 32]
  const half_t* b; long b_sn, b_sy, b_sx;      // the layer's input [N, H, W, 56]: mask of the dgrad, B operand of the wgrad
  int N, H, W;
  const half_t* wt;                            // dgrad weights [2 cout tiles][2 K steps][64 lanes][8], conv_hr's fragment order
  half_t* out; long o_sn, o_sy, o_sx;          // dIn [N, H, W, 56]
  float aslope, mask_slope;                    // (aslope = 1: conv_hr's branch-free "no activation")
  float* g; long slab_stride;
  unsigned tiles_x, tiles_y;
};

constexpr int PR_PA = 80, PR_PB = 112;                                   // LDS bytes per pixel
constexpr int PR_NPA = PR_TH * PR_TW * PR_PA / 4096, PR_NPB = PR_TH * PR_TW * PR_PB / 4096, PR_NPW = PR_NPA + PR_NPB;      // DMA pieces per wave: 5 + 7
constexpr int PR_ABYTES = PR_NPA * 4096, PR_BUF = PR_NPW * 4096;
constexpr int PR_SMEM = PR_NBUF * PR_BUF + 256;                          // (+ the transposing reads of channels 56-63 run 16 bytes past the last pixel)
static_assert(PR_TH * PR_TW * PR_PA % 4096 == 0 && PR_TH * PR_TW * PR_PB % 4096 == 0, "whole pieces");
static_assert(PR_SMEM <= 160 * 1024, "LDS budget");

typedef int pr_v4i __attribute__((ext_vector_type(4)));
// One LDS-DMA piece: 64 lanes x 16 bytes from buffer offset voff (out of range: zeros) to LDS bytes [lds_addr, lds_addr + 1024); inline
// assembly for the reason given in conv_wgrad_hr.hip (the completion of the pieces is counted by hand: vmcnt + barrier per tile)
static __device__ __forceinline__ void pr_dma16(pr_v4i rs, int voff, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(rs), "s"(lds_addr));
}
static __device__ __forceinline__ pr_v4i pr_make_rs(const half_t* base) {
  const unsigned long a = reinterpret_cast<unsigned long>(base);
  pr_v4i r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
  r[1] = __builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xffffu));
  r[2] = 0x7fffffff;
  r[3] = 0x00020000;
  return r;
}

__global__ __launch_bounds__(256) void conv_pair1x1_kernel(const PairK p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int PA = PR_PA, PB = PR_PB, NPA = PR_NPA, NPW = PR_NPW, ABYTES = PR_ABYTES, BUF = PR_BUF, NBUF = PR_NBUF;
  constexpr int R = 4;                         // tile rows per wave, in both products
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pix = lane & 31, hi = lane >> 5;
  const int ctl = wid >> 1, row0 = (wid & 1) * R;                      // dgrad: 32-channel tile of dIn, first tile row
  const int bb = wid & 1, part = wid >> 1;                             // wgrad: 32-channel block of the input, row share
  const unsigned per_img = p.tiles_x * p.tiles_y, total = per_img * (unsigned)p.N, gsub = gridDim.x;

  h8 wf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) wf[ks] = *reinterpret_cast<const h8*>(p.wt + ((size_t)(ctl * 2 + ks) * 64 + lane) * 8);

  // ---- DMA roles, the same for every tile: piece i of a wave is wave instruction wid + 4 i of its region; its lane fills 16-byte slot
  // g = (wid + 4 i) * 64 + lane = (pixel, slot c) -- the fifth slot of a dPre pixel is zero-filled
  int voff[NPW], py0[NPW], px0[NPW];
#pragma unroll
  for (int i = 0; i < NPW; ++i) {
    const bool isa = i < NPA;
    const int g = (wid + 4 * (isa ? i : i - NPA)) * 64 + lane, slots = isa ? 5 : 7, px = g / slots, c = g - px * slots;
    const int ty = px / PR_TW, tx = px - ty * PR_TW;
    voff[i] = 2 * (int)(isa ? ty * p.a_sy + tx * p.a_sx + c * 8 : ty * p.b_sy + tx * p.b_sx + c * 8);
    py0[i] = (isa && c >= 4) ? 0x40000000 : ty;
    px0[i] = tx;
  }
  auto tile_at = [&](unsigned vb, int& n, int& y0, int& x0) {
    if (vb >= total) vb -= ((vb - total) / gsub + 1) * gsub;      // past the last tile: refetch the last one (uniform instruction counts)
    const unsigned lt = xcd_remap(vb, total);
    n = lt / per_img;
    const unsigned r_ = lt - n * per_img;
    y0 = (r_ / p.tiles_x) * PR_TH; x0 = (r_ % p.tiles_x) * PR_TW;
  };
  const unsigned lds0 = (unsigned)(unsigned long)((__attribute__((address_space(3))) char*)smem) + (unsigned)wid * 1024u;
  auto issue_piece = [&](pr_v4i rsa, pr_v4i rsb, int y0, int x0, int j, int buf) __attribute__((always_inline)) {
    const bool ok = (unsigned)(py0[j] + y0) < (unsigned)p.H && (unsigned)(px0[j] + x0) < (unsigned)p.W;
    if (j < NPA) pr_dma16(rsa, ok ? voff[j] : -1, lds0 + (unsigned)(buf * BUF + 4 * j * 1024));
    else pr_dma16(rsb, ok ? voff[j] : -1, lds0 + (unsigned)(buf * BUF + ABYTES + 4 * (j - NPA) * 1024));
  };
  auto src_a = [&](int n, int y0, int x0) { return p.a + n * p.a_sn + (long)y0 * p.a_sy + (long)x0 * p.a_sx; };
  auto src_b = [&](int n, int y0, int x0) { return p.b + n * p.b_sn + (long)y0 * p.b_sy + (long)x0 * p.b_sx; };

  // ---- wgrad fragment addressing (conv_wgrad_hr.hip): lane i of a 16-lane group supplies the address of pixel i / 4, channel quad
  // i % 4; afterwards the lane holds channel 16 (group & 1) + i of four pixels; lanes 32.. take pixels 8..15
  const int li = lane & 15;
  const int rsub = (lane >> 5) * 8 + (li >> 2);
  const int unit = (lane >> 4) & 1;
  const int aoff = rsub * PA + unit * 32 + (li & 3) * 8 + (part * R) * PR_TW * PA;
  const int boff = ABYTES + rsub * PB + (bb * 2 + unit) * 32 + (li & 3) * 8 + (part * R) * PR_TW * PB;
  auto tr8 = [&](const char* q, int rowbytes) __attribute__((always_inline)) {
    const fp16x4 r0 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)(q));
    const fp16x4 r1 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)(q + 4 * rowbytes));
    h8 v;
    v[0] = r0[0]; v[1] = r0[1]; v[2] = r0[2]; v[3] = r0[3]; v[4] = r1[0]; v[5] = r1[1]; v[6] = r1[2]; v[7] = r1[3];
    return v;
  };
  // ---- dgrad addressing (conv_hr.hip): lane = (pixel column, K half); fragment of K step ks = 16-byte chunk 2 ks + hi of the pixel
  const int doff = (row0 * PR_TW + pix) * PA + hi * 16;
  const int moff = ABYTES + (row0 * PR_TW + pix) * PB + (ctl * 32 + 8 * hi) * 2;

  f16v gacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) gacc[r] = 0.f;

  const unsigned j0 = blockIdx.x;
  if (j0 < total) {
#pragma unroll
    for (int k = 0; k < NBUF - 1; ++k) {
      int n, y0, x0;
      tile_at(j0 + k * gsub, n, y0, x0);
      const pr_v4i rsa = pr_make_rs(src_a(n, y0, x0)), rsb = pr_make_rs(src_b(n, y0, x0));
#pragma unroll
      for (int j = 0; j < NPW; ++j) issue_piece(rsa, rsb, y0, x0, j, k);
    }
    int buf = 0;
    for (unsigned vb = j0; vb < total; vb += gsub) {
      int n, y0, x0, nn, y0n, x0n;
      tile_at(vb, n, y0, x0);
      tile_at(vb + (NBUF - 1) * gsub, nn, y0n, x0n);
      const pr_v4i rsa = pr_make_rs(src_a(nn, y0n, x0n)), rsb = pr_make_rs(src_b(nn, y0n, x0n));
      const int bfill = buf == 0 ? NBUF - 1 : buf - 1;
      // this tile has landed everywhere (the tile after it may still be in flight) and every wave is done with the buffer of the
      // previous tile: the tile NBUF - 1 ahead goes there, piece by piece, below
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NBUF - 2) * NPW) : "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const char* tb = smem + buf * BUF;

      // ---- dIn: four rows = four independent accumulator chains, two K steps each
      f16v acc[R];
#pragma unroll
      for (int q = 0; q < R; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
      h8 bfr[R];
#pragma unroll
      for (int q = 0; q < R; ++q) bfr[q] = *reinterpret_cast<const h8*>(tb + doff + q * PR_TW * PA);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int q = 0; q < R; ++q) {
          acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[ks], bfr[q], acc[q], 0, 0, 0);
          if (ks == 0) bfr[q] = *reinterpret_cast<const h8*>(tb + doff + q * PR_TW * PA + 32);
          issue_piece(rsa, rsb, y0n, x0n, ks * R + q, bfill);
        }
      // ---- G: the wave's four rows, 16 pixels per MFMA
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const h8 af = tr8(tb + aoff + (r * PR_TW + h * 16) * PA, PA);
          const h8 bf = tr8(tb + boff + (r * PR_TW + h * 16) * PB, PB);
          gacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, gacc, 0, 0, 0);
          const int j = 2 * R + r * 2 + h;
          if (j < NPW) issue_piece(rsa, rsb, y0n, x0n, j, bfill);
        }
      // ---- dgrad epilogue (conv_hr.hip): acc[4q + j] = channel 8q + 4 hi + j of pixel `pix`; swap pairs -> 8 consecutive channels per lane
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int oy = y0 + row0 + q, ox = x0 + pix;
        const bool live = oy < p.H && ox < p.W;
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
          const h8 mk = *reinterpret_cast<const h8*>(tb + moff + q * PR_TW * PB + 32 * pair);
          float v[8];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const unsigned a = __float_as_uint(acc[q][8 * pair + j]), b = __float_as_uint(acc[q][8 * pair + 4 + j]);
            auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
            v[j] = __uint_as_float(r[0]);
            v[4 + j] = __uint_as_float(r[1]);
          }
          const int co = ctl * 32 + 16 * pair + 8 * hi;
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], v[e] * p.aslope);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] *= ((float)mk[e] > 0.f ? 1.f : p.mask_slope);
          if (live && co < 56) {
            h8 hv;
#pragma unroll
            for (int e = 0; e < 8; ++e) hv[e] = (half_t)v[e];
            *reinterpret_cast<h8*>(p.out + n * p.o_sn + oy * p.o_sy + ox * p.o_sx + co) = hv;
          }
        }
      }
      buf = buf + 1 == NBUF ? 0 : buf + 1;
    }
  }

  // ---- the two row shares of a block meet in LDS; share 0 adds them and writes the slab: every (a < 32, b < 56) exactly once
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the last refetch must not land on the sums)
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);
  if (part == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(bb * 16 + r) * 64 + lane] = gacc[r];
  }
  __syncthreads();
  if (part == 0) {
    float* slab = p.g + (size_t)blockIdx.x * p.slab_stride;
    const int b = bb * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = gacc[r] + red[(bb * 16 + r) * 64 + lane];
      const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (b < 56) slab[(size_t)row * 56 + b] = v;
    }
  }
#endif
}

static bool pair_geometry_ok(int64_t a_sy, int64_t b_sy, int64_t a_sx, int64_t b_sx, int64_t o_sx) {
  // 32-bit piece offsets over the eight rows of a tile; 16-byte chunks on every map
  return a_sy < (1l << 31) / 32 && b_sy < (1l << 31) / 32 && a_sx >= 32 && b_sx >= 56 && o_sx >= 56 && a_sx % 8 == 0 && b_sx % 8 == 0 && o_sx % 8 == 0;
}

static unsigned pair_grid(int32_t N, int32_t H, int32_t W, hipStream_t st) {
  const unsigned total = (unsigned)N * (unsigned)((H + PR_TH - 1) / PR_TH) * (unsigned)((W + PR_TW - 1) / PR_TW);
  unsigned g = (unsigned)csbsr_cu_budget(st);      // persistent: one workgroup per CU of the stream's partition, never more than there is work
  if (g > total) g = total;
  return (g + 7) / 8 * 8;                          // (a multiple of 8: xcd_remap hands every XCD one contiguous run of tiles)
}

extern "C" int32_t csbsr_conv_pair1x1_slabs(int32_t N, int32_t H, int32_t W, csbsr_stream_t s) {
  if (N < 1 || H < 1 || W < 1) return 0;
  return (int32_t)pair_grid(N, H, W, reinterpret_cast<hipStream_t>(s));
}

extern "C" int csbsr_conv_pair1x1_backward(const void* dpre, int64_t a_sn, int64_t a_sy, int64_t a_sx, const void* x, int64_t b_sn, int64_t b_sy,
                                           int64_t b_sx, const void* wt_packed, float mask_slope, int32_t N, int32_t H, int32_t W, void* din,
                                           int64_t o_sn, int64_t o_sy, int64_t o_sx, float* slabs, csbsr_stream_t s) {
  CSBSR_CHECK(dpre && x && wt_packed && din && slabs && N >= 1 && H >= 1 && W >= 1, "conv_pair1x1: bad args");
  CSBSR_CHECK(pair_geometry_ok(a_sy, b_sy, a_sx, b_sx, o_sx), "conv_pair1x1: strides (row stride too large for 32-bit piece offsets, or pixels not 16-byte chunks)");
  hipStream_t st = reinterpret_cast<hipStream_t>(s);
  PairK k;
  k.a = reinterpret_cast<const half_t*>(dpre); k.a_sn = a_sn; k.a_sy = a_sy; k.a_sx = a_sx;
  k.b = reinterpret_cast<const half_t*>(x); k.b_sn = b_sn; k.b_sy = b_sy; k.b_sx = b_sx;
  k.N = N; k.H = H; k.W = W;
  k.wt = reinterpret_cast<const half_t*>(wt_packed);
  k.out = reinterpret_cast<half_t*>(din); k.o_sn = o_sn; k.o_sy = o_sy; k.o_sx = o_sx;
  k.aslope = 1.f; k.mask_slope = mask_slope;
  k.g = slabs; k.slab_stride = 32l * 56;
  k.tiles_x = (unsigned)((W + PR_TW - 1) / PR_TW); k.tiles_y = (unsigned)((H + PR_TH - 1) / PR_TH);
  static LdsAttrOnce attr;
  if (int e = csbsr_lds_attr(attr, reinterpret_cast<const void*>(conv_pair1x1_kernel), PR_SMEM, "conv_pair1x1")) return e;
  hipLaunchKernelGGL(conv_pair1x1_kernel, dim3(pair_grid(N, H, W, st)), dim3(256), PR_SMEM, st, k);
  CSBSR_LAUNCH_CHECK("csbsr_conv_pair1x1_backward");
  return 0;
}
