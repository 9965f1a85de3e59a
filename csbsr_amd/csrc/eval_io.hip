// The two outputs of the evaluation loop that leave the device (csbsr_amd/inference.py: evaluate_dataset): the mirror image of
// resident.hip -- fp32 in, bytes out.
//
//   csbsr_stitch_clip_u8        JointPatch (model/data/samplers/patch_sampler.py:30-51) + the two masked clip assignments of
//                               model/engine/inference.py:94-95 + ToPILImage's mul(255).byte() and its CHW -> HWC, in one pass over the
//                               model's patch batch: the stitched fp32 image for the metrics and / or the interleaved uint8 image for PIL.
//   csbsr_stitch_tiles_u8       the ragged counterpart for images of any size (csbsr_amd/inference.py: predict_dataset): every patch carries a
//                               table row that says which of its rectangles goes where in which image of an output pool.
//   csbsr_threshold_planes_u8   (pred - t_s > 0) * 255 for up to 16 thresholds (inference.py:111-118): one read of the map, S byte planes.
//
// All are streaming kernels without LDS or scratch.  A lane owns a run of consecutive output pixels of one row -- 4 in the stitch
// (a 16-byte load and store per fp32 plane, one 12-byte store of 4 RGB pixels or one dword of 4 grey ones), 16 in the threshold planes
// (four 16-byte loads, one 16-byte store per plane) -- and a run never crosses a patch's right edge because the vector kernels run only
// when pw % 4 == 0 (hw % 16 == 0) and every base is aligned; everything else takes the per-pixel kernels.  Every index is derived from
// the arguments: a lane past the last run returns before it forms an address.  (The ragged stitch decides load, fp32 store and byte store
// per lane at run time from the row's offsets, which are uniform per workgroup.)
#include "common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)

__device__ __forceinline__ float clip01_keep(float v) {          // sr[sr > 1] = 1; sr[sr < 0] = 0: NaN and -0.0 stay what they are
  return v > 1.f ? 1.f : (v < 0.f ? 0.f : v);
}

__device__ __forceinline__ uint32_t quant_u8(float v) {          // ToPILImage on the clipped image: mul(255).byte(); NaN -> 0
  const float c = v > 0.f ? (v < 1.f ? v : 1.f) : 0.f;
  return (uint32_t)__fmul_rn(c, 255.f);                          // c * 255 is in [0, 255]: the conversion truncates
}

// VEC: pw % 4 == 0 and aligned bases.  One lane = output pixels x .. x + 3 of row y of image blockIdx.y, all inside patch (y / ph, x / pw).
template <int C, bool VEC>
__global__ __launch_bounds__(256) void stitch_clip_u8_kernel(const float* __restrict__ patches, int nH, int nW, int ph, int pw, int wq,
                                                             int clip, float* __restrict__ out_f32, uint8_t* __restrict__ out_u8) {
  const int b = blockIdx.y;
  const int H = nH * ph, W = nW * pw;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= H * wq) return;
  const int y = idx / wq, x = (idx - y * wq) * 4;
  const int iy = y / ph, py = y - iy * ph;
  const int64_t plane = (int64_t)ph * pw;
  float v[C][4];
  int n = 4;
  if (VEC) {
    const int ix = x / pw, px = x - ix * pw;
    const float* src = patches + ((((int64_t)b * nH + iy) * nW + ix) * C) * plane + (int64_t)py * pw + px;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const f4 r = *reinterpret_cast<const f4*>(src + c * plane);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[c][j] = r[j];
    }
  } else {
    n = min(4, W - x);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xj = min(x + j, W - 1);                          // (a lane of the row tail re-reads the last pixel and does not store it)
      const int ix = xj / pw, px = xj - ix * pw;
      const float* src = patches + ((((int64_t)b * nH + iy) * nW + ix) * C) * plane + (int64_t)py * pw + px;
#pragma unroll
      for (int c = 0; c < C; ++c) v[c][j] = src[c * plane];
    }
  }
  if (out_f32) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float* o = out_f32 + (((int64_t)b * C + c) * H + y) * W + x;
      f4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = clip ? clip01_keep(v[c][j]) : v[c][j];
      if (VEC) {
        *reinterpret_cast<f4*>(o) = r;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < n) o[j] = r[j];
      }
    }
  }
  if (out_u8) {
    uint8_t* o = out_u8 + (((int64_t)b * H + y) * W + x) * C;
    if (VEC) {
      uint32_t u[C] = {};                                        // byte k = j * C + c of the run: pixel j, channel c
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int k = j * C + c;
          u[k >> 2] |= quant_u8(v[c][j]) << (8 * (k & 3));
        }
      }
      uint32_t* o32 = reinterpret_cast<uint32_t*>(o);            // (4 * C bytes at a multiple of 4 * C from a 4-byte-aligned base)
#pragma unroll
      for (int c = 0; c < C; ++c) o32[c] = u[c];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < n) {
#pragma unroll
          for (int c = 0; c < C; ++c) o[j * C + c] = (uint8_t)quant_u8(v[c][j]);
        }
      }
    }
  }
}

extern "C" int csbsr_stitch_clip_u8(const float* patches, int32_t B, int32_t C, int32_t nH, int32_t nW, int32_t ph, int32_t pw, int32_t clip,
                                    float* out_f32, uint8_t* out_u8, csbsr_stream_t s) {
  CSBSR_CHECK(patches && (out_f32 || out_u8), "stitch_clip_u8: null pointer (patches, or both outputs)");
  CSBSR_CHECK(C == 1 || C == 3, "stitch_clip_u8: C must be 1 or 3 (got %d)", C);
  CSBSR_CHECK(B > 0 && B <= 65535 && nH > 0 && nW > 0 && ph > 0 && pw > 0, "stitch_clip_u8: bad batch / patch grid / patch size");
  const int64_t H = (int64_t)nH * ph, W = (int64_t)nW * pw;
  CSBSR_CHECK(H < (1 << 24) && W < (1 << 24), "stitch_clip_u8: image too large");
  const int wq = (int)((W + 3) / 4);
  CSBSR_CHECK(H * wq < (1ll << 31) - 256, "stitch_clip_u8: image too large");
  const bool vec = (pw & 3) == 0 && (reinterpret_cast<uintptr_t>(patches) & 15) == 0 && (reinterpret_cast<uintptr_t>(out_f32) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out_u8) & 3) == 0;
  const dim3 grid(cdiv(H * wq, 256), B), block(256);
#define STITCH_LAUNCH(C_, V_) \
  hipLaunchKernelGGL((stitch_clip_u8_kernel<C_, V_>), grid, block, 0, ST(s), patches, nH, nW, ph, pw, wq, clip, out_f32, out_u8)
  if (C == 3) { if (vec) STITCH_LAUNCH(3, true); else STITCH_LAUNCH(3, false); }
  else        { if (vec) STITCH_LAUNCH(1, true); else STITCH_LAUNCH(1, false); }
#undef STITCH_LAUNCH
  CSBSR_LAUNCH_CHECK("csbsr_stitch_clip_u8");
  return 0;
}

// One workgroup row (blockIdx.y) per patch; a lane owns pixels x .. x + 3 of row y of the patch's owned rectangle.  The row of the table is
// not trusted: the rectangle is cut to what lies inside the patch AND inside the image before any address is formed, so no read leaves patch
// n and no write leaves the C * H * W elements of image `img`.  (img itself indexes dims / offsets as given, as in resident.hip.)
// al: bit 0 = patches 16-byte aligned and PW % 4 == 0, bit 1 = out_f32 16-byte aligned, bit 2 = out_u8 4-byte aligned.
template <int C>
__global__ __launch_bounds__(256) void stitch_tiles_u8_kernel(const float* __restrict__ patches, int PH, int PW, int wq,
                                                              const int32_t* __restrict__ tiles, const int64_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ dims, int clip, int al,
                                                              float* __restrict__ out_f32, uint8_t* __restrict__ out_u8) {
  const int n = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= PH * wq) return;
  const int y = idx / wq, x = (idx - y * wq) * 4;
  const int32_t* t = tiles + (int64_t)n * 8;                       // uniform per workgroup
  const int img = t[0];
  const int H = dims[2 * img], W = dims[2 * img + 1];
  if (H <= 0 || W <= 0) return;
  const int dy = min(max(t[1], 0), H), dx = min(max(t[2], 0), W);
  const int sy = min(max(t[3], 0), PH), sx = min(max(t[4], 0), PW);
  const int th = min(min(t[5], PH - sy), H - dy), tw = min(min(t[6], PW - sx), W - dx);      // <= 0: nothing of this tile survives
  if (y >= th || x >= tw) return;
  const int m = min(4, tw - x);                                    // pixels of this lane
  const int64_t plane = (int64_t)PH * PW, off = offsets[img], hw = (int64_t)H * W;
  const float* src = patches + (int64_t)n * C * plane + (int64_t)(sy + y) * PW + sx + x;
  float v[C][4];
  if (m == 4 && (al & 1) && (sx & 3) == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const f4 r = *reinterpret_cast<const f4*>(src + c * plane);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[c][j] = r[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xj = min(j, m - 1);                                // (a lane of the row tail re-reads its last pixel and does not store it)
#pragma unroll
      for (int c = 0; c < C; ++c) v[c][j] = src[c * plane + xj];
    }
  }
  const int64_t pix = (int64_t)(dy + y) * W + dx + x;              // first pixel of the run inside its image
  const bool run4 = m == 4 && ((W | dx) & 3) == 0 && (off & 3) == 0;      // pix % 4 == 0 and the image starts at a multiple of 4 elements
  if (out_f32) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float* o = out_f32 + off + c * hw + pix;
      f4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = clip ? clip01_keep(v[c][j]) : v[c][j];
      if (run4 && (al & 2)) {
        *reinterpret_cast<f4*>(o) = r;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < m) o[j] = r[j];
      }
    }
  }
  if (out_u8) {
    uint8_t* o = out_u8 + off + pix * C;
    if (run4 && (al & 4)) {
      uint32_t u[C] = {};                                          // byte k = j * C + c of the run: pixel j, channel c
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int k = j * C + c;
          u[k >> 2] |= quant_u8(v[c][j]) << (8 * (k & 3));
        }
      }
      uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
      for (int c = 0; c < C; ++c) o32[c] = u[c];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < m) {
#pragma unroll
          for (int c = 0; c < C; ++c) o[j * C + c] = (uint8_t)quant_u8(v[c][j]);
        }
      }
    }
  }
}

extern "C" int csbsr_stitch_tiles_u8(const float* patches, int32_t N, int32_t C, int32_t PH, int32_t PW, const int32_t* tiles,
                                     const int64_t* offsets, const int32_t* dims, int32_t clip, float* out_f32, uint8_t* out_u8,
                                     csbsr_stream_t s) {
  CSBSR_CHECK(patches && tiles && offsets && dims && (out_f32 || out_u8), "stitch_tiles_u8: null pointer (an input, or both outputs)");
  CSBSR_CHECK(C == 1 || C == 3, "stitch_tiles_u8: C must be 1 or 3 (got %d)", C);
  CSBSR_CHECK(N > 0 && PH > 0 && PW > 0, "stitch_tiles_u8: bad patch count / patch size");
  const int wq = (PW + 3) / 4;
  CSBSR_CHECK((int64_t)PH * wq < (1ll << 31) - 256, "stitch_tiles_u8: patch too large");
  const int al = (((PW & 3) == 0 && (reinterpret_cast<uintptr_t>(patches) & 15) == 0) ? 1 : 0) |
                 ((reinterpret_cast<uintptr_t>(out_f32) & 15) == 0 ? 2 : 0) | ((reinterpret_cast<uintptr_t>(out_u8) & 3) == 0 ? 4 : 0);
  const int64_t plane = (int64_t)PH * PW;
  for (int32_t n0 = 0; n0 < N; n0 += 65535) {                      // (grid.y carries the patch)
    const dim3 grid(cdiv((int64_t)PH * wq, 256), min(N - n0, 65535)), block(256);
    const float* p = patches + (int64_t)n0 * C * plane;            // (a multiple of 16 bytes whenever bit 0 of al is set)
    const int32_t* t = tiles + (int64_t)n0 * 8;
    if (C == 3) hipLaunchKernelGGL((stitch_tiles_u8_kernel<3>), grid, block, 0, ST(s), p, PH, PW, wq, t, offsets, dims, clip, al, out_f32, out_u8);
    else        hipLaunchKernelGGL((stitch_tiles_u8_kernel<1>), grid, block, 0, ST(s), p, PH, PW, wq, t, offsets, dims, clip, al, out_f32, out_u8);
  }
  CSBSR_LAUNCH_CHECK("csbsr_stitch_tiles_u8");
  return 0;
}

// VEC: hw % 16 == 0 and 16-byte-aligned bases.  One lane = pixels i .. i + 15 of map blockIdx.y, held in registers across the S planes.
template <bool VEC>
__global__ __launch_bounds__(256) void threshold_planes_u8_kernel(const float* __restrict__ pred, const float* __restrict__ thresholds,
                                                                  int64_t hw, int64_t runs, int S, uint8_t* __restrict__ out) {
  const int n = blockIdx.y;
  const int64_t run = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (run >= runs) return;
  const int64_t i = run * 16;
  const float* p = pred + (int64_t)n * hw + i;
  uint8_t* o = out + (int64_t)n * S * hw + i;
  float v[16];
  if (VEC) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f4 r = reinterpret_cast<const f4*>(p)[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[q * 4 + j] = r[j];
    }
    for (int s = 0; s < S; ++s) {
      const float t = thresholds[s];                             // uniform: a scalar load
      uint32_t u[4] = {};
#pragma unroll
      for (int j = 0; j < 16; ++j) u[j >> 2] |= (__fsub_rn(v[j], t) > 0.f ? 255u : 0u) << (8 * (j & 3));
      *reinterpret_cast<uint4*>(o + (int64_t)s * hw) = make_uint4(u[0], u[1], u[2], u[3]);
    }
  } else {
    const int m = (int)min((int64_t)16, hw - i);
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = p[min(j, m - 1)];
    for (int s = 0; s < S; ++s) {
      const float t = thresholds[s];
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j < m) o[(int64_t)s * hw + j] = __fsub_rn(v[j], t) > 0.f ? 255 : 0;
    }
  }
}

extern "C" int csbsr_threshold_planes_u8(const float* pred, const float* thresholds, int32_t N, int64_t hw, int32_t S, uint8_t* out,
                                         csbsr_stream_t s) {
  CSBSR_CHECK(pred && thresholds && out, "threshold_planes_u8: null pointer");
  CSBSR_CHECK(N > 0 && N <= 65535 && hw > 0, "threshold_planes_u8: bad map count / size");
  CSBSR_CHECK(S >= 1 && S <= 16, "threshold_planes_u8: 1 .. 16 thresholds per call (got %d)", S);
  const int64_t runs = (hw + 15) / 16;
  CSBSR_CHECK(runs < (1ll << 31) * 256 - 256, "threshold_planes_u8: map too large");
  const bool vec = (hw & 15) == 0 && (reinterpret_cast<uintptr_t>(pred) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const dim3 grid((unsigned)((runs + 255) / 256), N), block(256);
  if (vec) hipLaunchKernelGGL((threshold_planes_u8_kernel<true>), grid, block, 0, ST(s), pred, thresholds, hw, runs, S, out);
  else     hipLaunchKernelGGL((threshold_planes_u8_kernel<false>), grid, block, 0, ST(s), pred, thresholds, hw, runs, S, out);
  CSBSR_LAUNCH_CHECK("csbsr_threshold_planes_u8");
  return 0;
}
