// Batch selection out of an HBM-resident uint8 dataset (csbsr_amd/data/resident.py): index -> mirror -> crop -> /255 in one pass.
// The reference does this per sample on the host: PIL decode, RandomMirror / RandomVerticalFlip on the HWC array, ToTensor's HWC -> CHW,
// the crop, and `image / 255` (model/data/transforms/data_preprocess.py:17-28, model/data/crack_dataset.py:40-50).
//
// Streaming kernel, write-bound (1 source byte -> 4 output bytes).  A lane owns four consecutive output pixels of one crop row: it reads
// the 4 * C contiguous source bytes of that run (the run of a mirrored row is the same bytes walked backwards, so a wave's reads cover one
// contiguous span either way) and writes one 16-byte vector per output plane.  The window of a sel row is not trusted: y0 / x0 are
// clamped into the image before they become an address, so for a valid image index i no read leaves [offsets[i], offsets[i] + H * W * C).
// The image index itself cannot be checked here (the ABI carries no image count): it indexes dims / offsets as given, and keeping it
// inside the tables is the caller's responsibility alone.
#include "common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)

// C = 1 or 3 interleaved channels; VEC: w % 4 == 0, every lane stores whole 16-byte vectors
template <int C, bool VEC>
__global__ __launch_bounds__(256) void gather_crop_u8_kernel(const uint8_t* __restrict__ pool, const int64_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ dims, const int32_t* __restrict__ sel, int h, int w,
                                                             int wq, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= h * wq) return;
  const int y = idx / wq, x = (idx - y * wq) * 4;
  const int32_t* sb = sel + b * 5;                         // uniform per workgroup
  const int img = sb[0], y0 = sb[1], x0 = sb[2], mirror = sb[3], vflip = sb[4];
  const int H = dims[2 * img], W = dims[2 * img + 1];
  const uint8_t* src = pool + offsets[img];
  int ys = vflip ? H - 1 - (y0 + y) : y0 + y;
  ys = min(max(ys, 0), H - 1);
  const uint8_t* row = src + (int64_t)ys * W * C;
  const int n = VEC ? 4 : min(4, w - x);                   // pixels of this lane
  const int lo = mirror ? W - 1 - (x0 + x + 3) : x0 + x;   // leftmost source pixel of a full run
  uint8_t v[4 * C];                                        // v[j * C + c]: output pixel x + j
  if (n == 4 && lo >= 0 && lo <= W - 4) {
    uint32_t u[C];
    __builtin_memcpy(u, row + (int64_t)lo * C, 4 * C);     // 4 * C contiguous bytes, any alignment
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int kf = j * C + c, kr = (3 - j) * C + c;      // compile-time byte positions: the run forwards / backwards
        const uint32_t f = u[kf >> 2] >> (8 * (kf & 3)), r = u[kr >> 2] >> (8 * (kr & 3));
        v[j * C + c] = (uint8_t)(mirror ? r : f);
      }
    }
  } else {                                                 // a window that leaves the image (never from a validated table), or a row tail
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int xs = mirror ? W - 1 - (x0 + x + j) : x0 + x + j;
      xs = min(max(xs, 0), W - 1);
#pragma unroll
      for (int c = 0; c < C; ++c) v[j * C + c] = row[(int64_t)xs * C + c];
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float* o = out + (((int64_t)b * C + c) * h + y) * w + x;
    f4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = __fdiv_rn((float)v[j * C + c], 255.f);      // correctly rounded, = torch's image / 255
    if (VEC) {
      *reinterpret_cast<f4*>(o) = r;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n) o[j] = r[j];
    }
  }
}

extern "C" int csbsr_gather_crop_u8(const uint8_t* pool, const int64_t* offsets, const int32_t* dims, int32_t channels, const int32_t* sel,
                                    int32_t B, int32_t h, int32_t w, float* out, csbsr_stream_t s) {
  CSBSR_CHECK(pool && offsets && dims && sel && out, "gather_crop_u8: null pointer");
  CSBSR_CHECK(channels == 1 || channels == 3, "gather_crop_u8: channels must be 1 or 3 (got %d)", channels);
  CSBSR_CHECK(B > 0 && B <= 65535 && h > 0 && w > 0, "gather_crop_u8: bad batch / crop size");
  const int wq = (w + 3) / 4;
  CSBSR_CHECK((int64_t)h * wq < (1ll << 31) - 256, "gather_crop_u8: crop too large");
  const bool vec = (w & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const dim3 grid(cdiv((int64_t)h * wq, 256), B), block(256);
#define GATHER_LAUNCH(C_, V_) hipLaunchKernelGGL((gather_crop_u8_kernel<C_, V_>), grid, block, 0, ST(s), pool, offsets, dims, sel, h, w, wq, out)
  if (channels == 3) { if (vec) GATHER_LAUNCH(3, true); else GATHER_LAUNCH(3, false); }
  else               { if (vec) GATHER_LAUNCH(1, true); else GATHER_LAUNCH(1, false); }
#undef GATHER_LAUNCH
  CSBSR_LAUNCH_CHECK("csbsr_gather_crop_u8");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------- gather + resample
// csbsr_gather_resize_u8: the window (y0, x0, hs, ws) of a sel row, taken in the flipped image as above, resampled to h x w the way
// F.interpolate(mode="bilinear", align_corners=False, antialias=A) does on the CPU (the separable triangle filter of torch's
// _compute_indices_min_size_weights_aa: support and tap spacing stretched by the scale when it shrinks and A is set), then / 255: the
// reference's RandomResizedCrop (model/data/transforms/transforms.py:607-622) followed by data_preprocess.py:44.
//
// One workgroup owns RS_TH x RS_TW output pixels of one plane (sample, channel).  It (0) builds the tap tables of its RS_TW columns and
// RS_TH rows from the sample's sel row -- first source index, tap count, normalised fp32 weights -- in LDS, (1) runs the horizontal pass
// over the source rows its output rows touch, uint8 -> one fp32 row of RS_TW values per source row in LDS, and (2) runs the vertical pass
// out of LDS, one lane per four consecutive output pixels, and stores / 255.  No intermediate in HBM, no atomics, taps added in ascending
// order: two runs give the same bits.  A window of the output size has weights exactly {1, 0}, so its result is csbsr_gather_crop_u8's.
//
// LDS per workgroup (static): RS_ROWS * RS_TW fp32 rows 18,944 B + column table 64 * 17 * 4 = 4,352 B + row table 8 * 17 * 4 = 544 B
// + 4 * (64 + 64 + 8 + 8) = 576 B of starts and counts = 24,416 B, six workgroups of four waves per CU by LDS.  RS_ROWS: with
// hs <= 8 h the scale s <= 8 and the support <= 8, so RS_TH output rows touch fewer than s (RS_TH - 1) + 2 support + 1 = 73 source rows.
// Bank layout: pass (1) writes consecutive lanes to consecutive dwords; pass (2) reads 16-byte vectors from rows whose stride is 64
// dwords = one bank row, 16 lanes to a row, so each 16-lane group of a ds_read_b128 covers the 16 distinct slots whatever rows its lanes
// are on; the weight tables have the odd stride 17, so 32 lanes reading tap k of 32 columns hit 32 banks.
//
// Nothing of a sel row is trusted except the image index: hs / ws are raised to 1, tap counts are cut to RS_TAPS and the row span to
// RS_ROWS (a window over the 8x cap gives wrong pixels, not a wrong address), and every source coordinate is clamped into the image
// before it becomes an address, so a window that overhangs its image replicates the border.
#define RS_TH 8
#define RS_TW 64
#define RS_TAPS 17
#define RS_ROWS 74

// taps of output index o along an axis of n_in source and n_out output samples: first source index, count (<= RS_TAPS), normalised weights
__device__ __forceinline__ void resize_taps(int n_in, int n_out, int aa, int o, int& lo_out, int& n_out_taps, float* __restrict__ wt) {
#pragma clang fp contract(off)
  const float s = __fdiv_rn((float)n_in, (float)n_out);
  const bool shrink = aa && s >= 1.f;
  const float support = shrink ? s : 1.f, inv = shrink ? __fdiv_rn(1.f, s) : 1.f;
  const float c = s * ((float)o + 0.5f);
  const int lo = max(0, (int)(c - support + 0.5f));
  const int hi = min(n_in, (int)(c + support + 0.5f));
  const int n = min(max(hi - lo, 0), RS_TAPS);
  float total = 0.f;
  for (int k = 0; k < n; ++k) {
    const float wk = fmaxf(0.f, 1.f - fabsf(((float)(lo + k) - c + 0.5f) * inv));
    wt[k] = wk;
    total += wk;
  }
  for (int k = 0; k < n; ++k) wt[k] = __fdiv_rn(wt[k], total);
  lo_out = lo;
  n_out_taps = n;
}

// C = 1 or 3 interleaved channels, the channel of this workgroup in blockIdx.z; VEC: w % 4 == 0, every lane stores whole 16-byte vectors
template <int C, bool VEC>
__global__ __launch_bounds__(256) void gather_resize_u8_kernel(const uint8_t* __restrict__ pool, const int64_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ dims, const int32_t* __restrict__ sel, int h, int w,
                                                               int tiles_x, int aa, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float rows[RS_ROWS * RS_TW];
  __shared__ float wx[RS_TW * RS_TAPS], wy[RS_TH * RS_TAPS];
  __shared__ int xlo[RS_TW], xn[RS_TW], ylo[RS_TH], yn[RS_TH];
  const int tid = threadIdx.x, b = blockIdx.y, c = blockIdx.z;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int oy0 = ty * RS_TH, ox0 = tx * RS_TW;
  const int32_t* sb = sel + b * 7;                          // uniform per workgroup
  const int img = sb[0], y0 = sb[1], x0 = sb[2], mirror = sb[3], vflip = sb[4], hs = max(sb[5], 1), ws = max(sb[6], 1);
  const int H = dims[2 * img], W = dims[2 * img + 1];
  const uint8_t* src = pool + offsets[img] + c;

  // (0) tap tables: one lane per output column, then one per output row (a column / row past the output gets no taps)
  if (tid < RS_TW) {
    int lo = 0, n = 0;
    if (ox0 + tid < w) resize_taps(ws, w, aa, ox0 + tid, lo, n, wx + tid * RS_TAPS);
    xlo[tid] = lo;
    xn[tid] = n;
  } else if (tid < RS_TW + RS_TH) {
    const int t = tid - RS_TW;
    int lo = 0, n = 0;
    if (oy0 + t < h) resize_taps(hs, h, aa, oy0 + t, lo, n, wy + t * RS_TAPS);
    ylo[t] = lo;
    yn[t] = n;
  }
  __syncthreads();
  const int last = min(RS_TH, h - oy0) - 1;                // the tile's last output row inside the output (starts and ends ascend with o)
  const int row_lo = ylo[0];
  const int nrows = min(max(ylo[last] + yn[last] - row_lo, 0), RS_ROWS);

  // (1) horizontal pass: lane -> column of the tile, wave -> source row (4 rows in flight per workgroup).  A column's byte offsets and
  // weights do not change from row to row, so they are taken four taps at a time into registers and the rows run inside: four independent
  // byte loads per row and lane instead of one load waited for per tap.  A tap past the column's count repeats the last address with
  // weight 0 (acc + 0 * v is exact), later groups of four add to what the earlier ones left in LDS: ascending order either way.
  {
    const int t = tid & (RS_TW - 1);
    const int lo = xlo[t], n = xn[t];
    const float* wt = wx + t * RS_TAPS;
    for (int k0 = 0; k0 == 0 || k0 < n; k0 += 4) {
      int off[4];
      float wv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + j, kk = max(min(k, n - 1), 0);
        int xs = mirror ? W - 1 - (x0 + lo + kk) : x0 + lo + kk;
        xs = min(max(xs, 0), W - 1);
        off[j] = xs * C;
        wv[j] = k < n ? wt[k] : 0.f;
      }
      for (int r = tid / RS_TW; r < nrows; r += 256 / RS_TW) {
        int ys = vflip ? H - 1 - (y0 + row_lo + r) : y0 + row_lo + r;
        ys = min(max(ys, 0), H - 1);
        const uint8_t* row = src + (int64_t)ys * W * C;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)row[off[j]];
        float acc = k0 == 0 ? 0.f : rows[r * RS_TW + t];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += wv[j] * v[j];
        rows[r * RS_TW + t] = acc;
      }
    }
  }
  __syncthreads();

  // (2) vertical pass: a lane owns four consecutive output pixels of one row
  if (tid < RS_TH * (RS_TW / 4)) {
    const int t = tid / (RS_TW / 4), x = (tid - t * (RS_TW / 4)) * 4;
    const int oy = oy0 + t, ox = ox0 + x;
    if (oy < h && ox < w) {
      const int r0 = ylo[t] - row_lo;
      const int n = min(yn[t], RS_ROWS - r0);               // (never cuts a row of a validated table)
      const float* wt = wy + t * RS_TAPS;
      f4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < n; k0 += 4) {                   // four taps at a time, as above: the reads of a group are independent
        f4 v[4];
        float wk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = k0 + i;
          v[i] = *reinterpret_cast<const f4*>(rows + (r0 + min(k, n - 1)) * RS_TW + x);
          wk[i] = k < n ? wt[k] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] += wk[i] * v[i][j];
      }
      f4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = __fdiv_rn(acc[j], 255.f);
      float* o = out + (((int64_t)b * C + c) * h + oy) * w + ox;
      if (VEC) {
        *reinterpret_cast<f4*>(o) = r;
      } else {
        const int m = min(4, w - ox);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < m) o[j] = r[j];
      }
    }
  }
}

extern "C" int csbsr_gather_resize_u8(const uint8_t* pool, const int64_t* offsets, const int32_t* dims, int32_t channels, const int32_t* sel,
                                      int32_t B, int32_t h, int32_t w, int32_t antialias, float* out, csbsr_stream_t s) {
  CSBSR_CHECK(pool && offsets && dims && sel && out, "gather_resize_u8: null pointer");
  CSBSR_CHECK(channels == 1 || channels == 3, "gather_resize_u8: channels must be 1 or 3 (got %d)", channels);
  CSBSR_CHECK(B > 0 && B <= 65535 && h > 0 && w > 0, "gather_resize_u8: bad batch / output size");
  CSBSR_CHECK(antialias == 0 || antialias == 1, "gather_resize_u8: antialias must be 0 or 1 (got %d)", antialias);
  CSBSR_CHECK(h <= (1 << 24) / 8 && w <= (1 << 24) / 8, "gather_resize_u8: output too large for exact fp32 source coordinates");
  const int tiles_x = cdiv(w, RS_TW), tiles_y = cdiv(h, RS_TH);
  CSBSR_CHECK((int64_t)tiles_x * tiles_y < (1ll << 31), "gather_resize_u8: output too large");
  const bool vec = (w & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const dim3 grid(tiles_x * tiles_y, B, channels), block(256);
#define RESIZE_LAUNCH(C_, V_) \
  hipLaunchKernelGGL((gather_resize_u8_kernel<C_, V_>), grid, block, 0, ST(s), pool, offsets, dims, sel, h, w, tiles_x, antialias, out)
  if (channels == 3) { if (vec) RESIZE_LAUNCH(3, true); else RESIZE_LAUNCH(3, false); }
  else               { if (vec) RESIZE_LAUNCH(1, true); else RESIZE_LAUNCH(1, false); }
#undef RESIZE_LAUNCH
  CSBSR_LAUNCH_CHECK("csbsr_gather_resize_u8");
  return 0;
}
