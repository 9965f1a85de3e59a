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
