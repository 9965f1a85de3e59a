// HBM-bound kernels on fp16 channels-last activations: epilogue backward, batch-norm, pooling, bilinear resize,
// layout converters.  Every thread moves 16 bytes (8 channels) per access; reductions go wave-shuffle ->
// LDS -> one partial row per workgroup -> csbsr_sum_partials (fixed order, no atomics: common.h).  Reference call sites are cited per entry point in include/csbsr_hip.h.
#include <cstdlib>
#include "common.h"

static inline int grid_for(long work, int block = 256, int cap = 8192) {
  long b = (work + block - 1) / block;
  if (b < 1) b = 1;
  return (int)(b > cap ? cap : b);
}
#define ST(s) reinterpret_cast<hipStream_t>(s)

// split-fp16 ("hi + lo") views of the detector precision mode: lo = element offset from the hi plane to the lo plane (0: plain fp16)
__device__ __forceinline__ void ld_split(const half_t* p, long lo, float (&v)[8]) {
  const h8 a = *reinterpret_cast<const h8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)a[e];
  if (lo) {
    const h8 b = *reinterpret_cast<const h8*>(p + lo);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += (float)b[e];
  }
}
__device__ __forceinline__ void st_split(half_t* p, long lo, const float (&v)[8]) {
  h8 a, b;
#pragma unroll
  for (int e = 0; e < 8; ++e) { a[e] = (half_t)v[e]; b[e] = (half_t)(v[e] - (float)a[e]); }
  *reinterpret_cast<h8*>(p) = a;
  if (lo) *reinterpret_cast<h8*>(p + lo) = b;
}
// eight consecutive fp32 values of a per-(sample, channel) row (dropout scales): two 16-byte loads.  Written as eight indexed reads of a
// pointer of unknown alignment the compiler issued eight 4-byte loads per channel octet: the x2 up-samplings of the detector's decoder
// ran at 1.7-2.2 TB/s with the scale row and 2.7-2.9 without (scripts/bench_bilinear.py).  (The row starts at a multiple of 8 floats.)
__device__ __forceinline__ void ld8f(const float* p, float (&v)[8]) {
  const f4 a = *reinterpret_cast<const f4*>(p), b = *reinterpret_cast<const f4*>(p + 4);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}

// ------------------------------------------------------------------------------------------- two-stage reductions
// One registration per DEVICE (keyed on the calling thread's current HIP device, which is also the device every launch below goes to):
// two models in one process -- a trainer and an evaluator, or replicas on several GPUs -- share their device's buffer instead of the
// last registration silently winning.  The host keeps each buffer alive for the life of the process (csbsr_amd/engine.py).
static float* g_red_buf[CSBSR_MAX_DEVICES] = {};
static long g_red_elems[CSBSR_MAX_DEVICES] = {};
extern "C" int csbsr_set_reduction_scratch(float* buf, int64_t elems) {
  int dev = 0;
  CSBSR_CHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < CSBSR_MAX_DEVICES, "set_reduction_scratch: no current device");
  g_red_buf[dev] = buf;
  g_red_elems[dev] = buf ? (long)elems : 0;
  return 0;
}
float* csbsr_red_scratch(long need_elems) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= CSBSR_MAX_DEVICES) { csbsr_set_error("reduction scratch: no current device"); return nullptr; }
  if (g_red_buf[dev] && need_elems + CSBSR_RED_TAIL <= g_red_elems[dev]) return g_red_buf[dev];
  // (every caller turns the nullptr into an error return; the text says which scratch was wanted)
  csbsr_set_error("reduction scratch missing or too small on device %d: %ld floats (+ %ld tail) needed, %ld registered (csbsr_set_reduction_scratch)",
                  dev, need_elems, (long)CSBSR_RED_TAIL, g_red_buf[dev] ? g_red_elems[dev] : 0l);
  return nullptr;
}
static float* red_tail() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= CSBSR_MAX_DEVICES || !g_red_buf[dev] || g_red_elems[dev] < CSBSR_RED_TAIL) return nullptr;
  return g_red_buf[dev] + (g_red_elems[dev] - CSBSR_RED_TAIL);
}
// Fixed-order fold of partial rows.  Block = 32 columns x 8 row slices; slice s adds rows s, s+8, ... of its chunk into four
// interleaved accumulators, the slices meet in LDS and are added in slice order: the tree depends on (rows, rows_per_chunk) only.
// grid = (column blocks, chunks, batch).  store: dst[...] = t (first level of a two-level fold), else dst[...] += t.
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* part, int rows, long ld, int count, float* dst, long part_bs, long dst_bs,
                                                           long dst_cs, int rpc, int store) {
  __shared__ float sm[8][33];
  const int col = blockIdx.x * 32 + (threadIdx.x & 31), sl = threadIdx.x >> 5;
  const int r0 = blockIdx.y * rpc, r1 = min(rows, r0 + rpc);
  part += (long)blockIdx.z * part_bs;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (col < count) {
    int b = r0 + sl;
    for (; b + 24 < r1; b += 32) {
      a0 += part[(long)b * ld + col]; a1 += part[(long)(b + 8) * ld + col];
      a2 += part[(long)(b + 16) * ld + col]; a3 += part[(long)(b + 24) * ld + col];
    }
    for (; b < r1; b += 8) a0 += part[(long)b * ld + col];
  }
  sm[sl][threadIdx.x & 31] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (sl == 0 && col < count) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) t += sm[q][threadIdx.x & 31];
    float* d = dst + (long)blockIdx.z * dst_bs + (long)blockIdx.y * dst_cs + col;
    *d = store ? t : *d + t;
  }
}
int csbsr_sum_partials_batched(const float* part, int rows, long ld, int count, float* dst, int batch, long dst_bs, hipStream_t st) {
  if (rows <= 0 || count <= 0 || batch <= 0) return 0;
  const int RPC = 1024;
  const int chunks = (rows + RPC - 1) / RPC;
  const dim3 blk(256);
  if (chunks == 1) {
    hipLaunchKernelGGL(sum_partials_kernel, dim3((count + 31) / 32, 1, batch), blk, 0, st, part, rows, ld, count, dst, (long)rows * ld, dst_bs, 0l, RPC, 0);
    return 0;
  }
  float* tmp = red_tail();
  CSBSR_CHECK(tmp && (long)batch * chunks * count <= CSBSR_RED_TAIL && chunks <= RPC, "sum_partials: %d x %d rows of %d columns exceed the scratch tail", batch, rows, count);
  hipLaunchKernelGGL(sum_partials_kernel, dim3((count + 31) / 32, chunks, batch), blk, 0, st, part, rows, ld, count, tmp, (long)rows * ld,
                     (long)chunks * count, (long)count, RPC, 1);
  hipLaunchKernelGGL(sum_partials_kernel, dim3((count + 31) / 32, 1, batch), blk, 0, st, (const float*)tmp, chunks, (long)count, count, dst,
                     (long)chunks * count, dst_bs, 0l, RPC, 0);
  return 0;
}

// ------------------------------------------------------------------------------------------- epilogue backward
struct EpiK {
  long npix; int c8, creal;
  const half_t* dout; long dout_ld;
  const half_t* out; long out_ld;
  const half_t* res; long res_ld;
  const half_t* res2; long res2_ld;
  int act; float slope; const float* prelu; int res_mode;
  half_t* dpre; long dpre_ld;
  half_t* dres; long dres_ld; int dres_acc;
  half_t* dres2; long dres2_ld; int dres2_acc;
  float* dbias; float* dprelu;
  float* part; long part_ld;        // per-workgroup partial rows [gridDim.x][part_ld]: bias sums in [0,c), PReLU-slope sum at c
};

// block = 256 threads = 32 pixel-lanes x 8? no: thread -> (pixel group, channel chunk): chunk = tid % c8 when c8 <= 256
__global__ __launch_bounds__(256) void epilogue_bwd_kernel(const EpiK p) {
  __shared__ float sRed[256 * 8];
  __shared__ float sPre[256];
  const int tid = threadIdx.x;
  const int cpb = p.c8 < 256 ? p.c8 : 256;           // chunks handled per block column sweep
  const int ppb = 256 / cpb;                         // pixels per block iteration (>=1)
  const int ch = tid % cpb, pl = tid / cpb;
  const float slope = p.act == CSBSR_ACT_PRELU ? *p.prelu : p.slope;
  float dpr = 0.f;
  for (int cbase = 0; cbase < p.c8; cbase += cpb) {
    const int c8i = cbase + ch;
    float db[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) db[e] = 0.f;
    if (c8i < p.c8 && pl < ppb) {
      const int c0 = c8i * 8;
      for (long px = (long)blockIdx.x * ppb + pl; px < p.npix; px += (long)gridDim.x * ppb) {
        const h8 go = *reinterpret_cast<const h8*>(p.dout + px * p.dout_ld + c0);
        h8 o = {0, 0, 0, 0, 0, 0, 0, 0}, r = {0, 0, 0, 0, 0, 0, 0, 0}, r2 = {0, 0, 0, 0, 0, 0, 0, 0};
        if (p.out) o = *reinterpret_cast<const h8*>(p.out + px * p.out_ld + c0);
        if (p.res) r = *reinterpret_cast<const h8*>(p.res + px * p.res_ld + c0);
        if (p.res2) r2 = *reinterpret_cast<const h8*>(p.res2 + px * p.res2_ld + c0);
        h8 dp, dr, dr2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float g = (float)go[e];
          float y, gy, gr = 0.f, gr2 = 0.f;   // y = act(pre): rebuilt from the saved output
          const float ov = (float)o[e], rv = (float)r[e], r2v = (float)r2[e];
          switch (p.res_mode) {
            case CSBSR_RES_ADD: y = ov - rv; gy = g; gr = g; break;
            case CSBSR_RES_SUB: y = ov + rv; gy = g; gr = -g; break;
            case CSBSR_RES_MUL: y = 0.f; gy = g * rv; gr = 0.f; break;   // y not recoverable: only act NONE allowed
            case 4 /*FMA: out = y + res*res2*/: y = ov - rv * r2v; gy = g; gr = g * r2v; gr2 = g * rv; break;
            default: y = ov; gy = g; break;
          }
          float d;
          switch (p.act) {
            case CSBSR_ACT_RELU: d = y > 0.f ? gy : 0.f; break;
            case CSBSR_ACT_LRELU: d = y > 0.f ? gy : gy * slope; break;
            case CSBSR_ACT_PRELU:
              d = y > 0.f ? gy : gy * slope;
              if (!(y > 0.f)) dpr += gy * (y / slope);          // pre-activation x = y / slope for x <= 0
              break;
            case CSBSR_ACT_SIGMOID: d = gy * y * (1.f - y); break;
            default: d = gy; break;
          }
          if (c0 + e >= p.creal) d = 0.f;
          dp[e] = (half_t)d; db[e] += d;
          dr[e] = (half_t)gr; dr2[e] = (half_t)gr2;
        }
        if (p.dpre) *reinterpret_cast<h8*>(p.dpre + px * p.dpre_ld + c0) = dp;
        if (p.dres) {
          half_t* q = p.dres + px * p.dres_ld + c0;
          if (p.dres_acc) { const h8 old = *reinterpret_cast<const h8*>(q);
#pragma unroll
            for (int e = 0; e < 8; ++e) dr[e] = (half_t)((float)dr[e] + (float)old[e]); }
          *reinterpret_cast<h8*>(q) = dr;
        }
        if (p.dres2) {
          half_t* q = p.dres2 + px * p.dres2_ld + c0;
          if (p.dres2_acc) { const h8 old = *reinterpret_cast<const h8*>(q);
#pragma unroll
            for (int e = 0; e < 8; ++e) dr2[e] = (half_t)((float)dr2[e] + (float)old[e]); }
          *reinterpret_cast<h8*>(q) = dr2;
        }
      }
    }
    if (p.dbias) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sRed[tid * 8 + e] = db[e];
      __syncthreads();
      if (tid < cpb && cbase + tid < p.c8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float s = 0.f;
          for (int q = 0; q < ppb; ++q) s += sRed[(q * cpb + tid) * 8 + e];
          p.part[(long)blockIdx.x * p.part_ld + (cbase + tid) * 8 + e] = s;
        }
      }
      __syncthreads();
    }
  }
  if (p.dprelu) {
    dpr = wave_sum(dpr);
    if ((tid & 63) == 0) sPre[tid >> 6] = dpr;
    __syncthreads();
    if (tid == 0) {
      p.part[(long)blockIdx.x * p.part_ld + p.c8 * 8] = sPre[0] + sPre[1] + sPre[2] + sPre[3];
    }
  }
}

extern "C" int csbsr_epilogue_backward(const csbsr_epi_bwd_desc_t* d, csbsr_stream_t s) {
  CSBSR_CHECK(d && d->dout, "epilogue_bwd: null dout");
  CSBSR_CHECK(d->c % 8 == 0, "epilogue_bwd: channels must be a multiple of 8");
  CSBSR_CHECK(d->act == CSBSR_ACT_NONE || d->out, "epilogue_bwd: activation backward needs the saved output");
  CSBSR_CHECK(!(d->res_mode == CSBSR_RES_MUL && d->act != CSBSR_ACT_NONE), "epilogue_bwd: MUL with activation unsupported");
  EpiK k;
  k.npix = d->npix; k.c8 = d->c / 8; k.creal = d->creal;
  k.dout = (const half_t*)d->dout; k.dout_ld = d->dout_ld;
  k.out = (const half_t*)d->out; k.out_ld = d->out_ld;
  k.res = (const half_t*)d->res; k.res_ld = d->res_ld;
  k.res2 = (const half_t*)d->res2; k.res2_ld = d->res2_ld;
  k.act = d->act; k.slope = d->act_slope; k.prelu = d->prelu; k.res_mode = d->res_mode;
  k.dpre = (half_t*)d->dpre; k.dpre_ld = d->dpre_ld;
  k.dres = (half_t*)d->dres; k.dres_ld = d->dres_ld; k.dres_acc = d->dres_accumulate;
  k.dres2 = (half_t*)d->dres2; k.dres2_ld = d->dres2_ld; k.dres2_acc = d->dres2_accumulate;
  k.dbias = d->dbias; k.dprelu = d->dprelu;
  const int cpb = k.c8 < 256 ? k.c8 : 256;
  const int ppb = 256 / cpb;
  int blocks = grid_for(d->npix, ppb * 8, 2048);
  k.part = nullptr; k.part_ld = d->c + 8;
  if (k.dbias || k.dprelu) {
    k.part = csbsr_red_scratch((long)blocks * k.part_ld);
    CSBSR_NEED_SCRATCH(k.part, "epilogue_bwd");
  }
  hipLaunchKernelGGL(epilogue_bwd_kernel, dim3(blocks), dim3(256), 0, ST(s), k);
  if (k.part) {
    if (k.dbias) csbsr_sum_partials(k.part, blocks, k.part_ld, d->creal, k.dbias, ST(s));
    if (k.dprelu) csbsr_sum_partials(k.part + d->c, blocks, k.part_ld, 1, k.dprelu, ST(s));
  }
  CSBSR_LAUNCH_CHECK("csbsr_epilogue_backward");
  return 0;
}

// ------------------------------------------------------------------------------------------- axpby / fill / casts
__global__ void axpby_kernel(long npix, int c8, const half_t* x, long x_ld, long x_lo, float a, const half_t* z, long z_ld, long z_lo,
                             float b, half_t* y, long y_ld, long y_lo) {
  const long total = npix * c8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long px = i / c8; const int c0 = (int)(i % c8) * 8;
    float xv[8], zv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, o[8];
    ld_split(x + px * x_ld + c0, x_lo, xv);
    if (z) ld_split(z + px * z_ld + c0, z_lo, zv);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = a * xv[e] + b * zv[e];
    if (y_lo) st_split(y + px * y_ld + c0, y_lo, o);
    else {
      h8 h;
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = (half_t)o[e];
      *reinterpret_cast<h8*>(y + px * y_ld + c0) = h;
    }
  }
}

extern "C" int csbsr_axpby_split(int64_t npix, int32_t c, const void* x, int64_t x_ld, int64_t x_lo, float a, const void* z, int64_t z_ld,
                                 int64_t z_lo, float b, void* y, int64_t y_ld, int64_t y_lo, csbsr_stream_t s) {
  CSBSR_CHECK(c % 8 == 0 && x && y, "axpby: bad args");
  hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(npix * (c / 8))), dim3(256), 0, ST(s), npix, c / 8, (const half_t*)x, x_ld, x_lo,
                     a, (const half_t*)z, z_ld, z_lo, b, (half_t*)y, y_ld, y_lo);
  CSBSR_LAUNCH_CHECK("csbsr_axpby");
  return 0;
}
extern "C" int csbsr_axpby(int64_t npix, int32_t c, const void* x, int64_t x_ld, float a, const void* z, int64_t z_ld,
                           float b, void* y, int64_t y_ld, csbsr_stream_t s) {
  return csbsr_axpby_split(npix, c, x, x_ld, 0, a, z, z_ld, 0, b, y, y_ld, 0, s);
}
// y = act(sum_{i<n} x_i): the n-ary fuse sum of an HRNet module (hrnet_backbone.py:276-296), one pass
struct SumK { const half_t* x[4]; long ld[4]; long lo[4]; int n; };
__global__ void sum_act_kernel(long npix, int c8, SumK k, half_t* y, long y_ld, long y_lo, int relu) {
  const long total = npix * c8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long px = i / c8; const int c0 = (int)(i % c8) * 8;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = 0; t < k.n; ++t) {
      float v[8];
      ld_split(k.x[t] + px * k.ld[t] + c0, k.lo[t], v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = (relu && acc[e] < 0.f) ? 0.f : acc[e];
    st_split(y + px * y_ld + c0, y_lo, acc);
  }
}
extern "C" int csbsr_sum_act_split(int64_t npix, int32_t c, int32_t n, const void* const* xs, const int64_t* x_lds, const int64_t* x_los,
                                   void* y, int64_t y_ld, int64_t y_lo, int32_t relu, csbsr_stream_t s) {
  CSBSR_CHECK(c % 8 == 0 && n >= 1 && n <= 4 && xs && x_lds && y, "sum_act: bad args");
  SumK k;
  k.n = n;
  for (int i = 0; i < 4; ++i) {
    k.x[i] = i < n ? (const half_t*)xs[i] : nullptr; k.ld[i] = i < n ? x_lds[i] : 0; k.lo[i] = (i < n && x_los) ? x_los[i] : 0;
  }
  hipLaunchKernelGGL(sum_act_kernel, dim3(grid_for(npix * (c / 8))), dim3(256), 0, ST(s), npix, c / 8, k, (half_t*)y, y_ld, y_lo, relu);
  CSBSR_LAUNCH_CHECK("csbsr_sum_act");
  return 0;
}
extern "C" int csbsr_sum_act(int64_t npix, int32_t c, int32_t n, const void* const* xs, const int64_t* x_lds, void* y, int64_t y_ld,
                             int32_t relu, csbsr_stream_t s) {
  return csbsr_sum_act_split(npix, c, n, xs, x_lds, nullptr, y, y_ld, 0, relu, s);
}

// Soft object-region pooling of the OCR head (SpatialGather_Module, spatial_ocr_block.py:58-66, one class):
//   out[n][c] = sum_p w[n][p] * x[n][p][c]                       (fp32 accumulation, out must be zeroed by the caller)
// and its adjoint:  dx[n][p][c] += w[n][p] * dout[n][c],   dw[n][p] = sum_c x[n][p][c] * dout[n][c].
// One workgroup = 256 pixels x all channels of one sample; a thread owns 8 channels and strides over pixels.
__global__ __launch_bounds__(256) void wpool_fwd_kernel(const half_t* x, long x_ld, const float* w, float* part, long hw, int c8, int chunks,
                                                        long x_lo) {
  __shared__ float sAcc[256][8];
  const int n = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const long p0 = (long)chunk * 1024, p1 = min(hw, p0 + 1024);
  const int lanes_c = c8, groups = 256 / lanes_c;           // c8 <= 256 (launcher splits wider maps)
  const int cg = threadIdx.x % lanes_c, pg = threadIdx.x / lanes_c;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (pg < groups)
  for (long p = p0 + pg; p < p1; p += groups) {
    const float wv = w[(long)n * hw + p];
    float v[8];
    ld_split(x + ((long)n * hw + p) * x_ld + cg * 8, x_lo, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += wv * v[e];
  }
  // the pixel groups of one channel octet meet in LDS and are added in group order; one partial row per (sample, chunk)
#pragma unroll
  for (int e = 0; e < 8; ++e) sAcc[threadIdx.x][e] = acc[e];
  __syncthreads();
  if (threadIdx.x < lanes_c) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = 0.f;
      for (int q = 0; q < groups; ++q) t += sAcc[q * lanes_c + threadIdx.x][e];
      part[(long)blockIdx.x * c8 * 8 + cg * 8 + e] = t;
    }
  }
}
extern "C" int csbsr_weighted_pool_fwd_split(const void* x, int64_t x_ld, int64_t x_lo, const float* w, float* out, int32_t N, int64_t hw,
                                             int32_t c, csbsr_stream_t s) {
  CSBSR_CHECK(x && w && out && c % 8 == 0 && c / 8 <= 256, "weighted_pool_fwd: bad args");
  const int chunks = (int)((hw + 1023) / 1024);
  float* part = csbsr_red_scratch((long)N * chunks * c);
  CSBSR_NEED_SCRATCH(part, "weighted_pool_fwd");
  hipLaunchKernelGGL(wpool_fwd_kernel, dim3(N * chunks), dim3(256), 0, ST(s), (const half_t*)x, x_ld, w, part, (long)hw, c / 8, chunks, x_lo);
  if (csbsr_sum_partials_batched(part, chunks, c, c, out, N, c, ST(s))) return 1;
  CSBSR_LAUNCH_CHECK("csbsr_weighted_pool_fwd");
  return 0;
}
extern "C" int csbsr_weighted_pool_fwd(const void* x, int64_t x_ld, const float* w, float* out, int32_t N, int64_t hw, int32_t c,
                                       csbsr_stream_t s) {
  return csbsr_weighted_pool_fwd_split(x, x_ld, 0, w, out, N, hw, c, s);
}
__global__ __launch_bounds__(256) void wpool_bwd_kernel(const half_t* x, long x_ld, const float* w, const float* dout, half_t* dx, long dx_ld,
                                                        float* dw, long hw, int c8) {
  // one wave per pixel: lanes stride over the channel octets, wave-reduce the dot product
  const int lane = threadIdx.x & 63, wv_id = threadIdx.x >> 6;
  const int n = blockIdx.y;
  for (long p = (long)blockIdx.x * 4 + wv_id; p < hw; p += (long)gridDim.x * 4) {
    const float wgt = w[(long)n * hw + p];
    float dot = 0.f;
    for (int cg = lane; cg < c8; cg += 64) {
      const long off = ((long)n * hw + p);
      const h8 v = *reinterpret_cast<const h8*>(x + off * x_ld + cg * 8);
      h8 d = *reinterpret_cast<const h8*>(dx + off * dx_ld + cg * 8);
      const float* g = dout + (long)n * c8 * 8 + cg * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) { dot += (float)v[e] * g[e]; d[e] = (half_t)((float)d[e] + wgt * g[e]); }
      *reinterpret_cast<h8*>(dx + off * dx_ld + cg * 8) = d;
    }
    dot = wave_sum(dot);
    if (lane == 0) dw[(long)n * hw + p] = dot;
  }
}
extern "C" int csbsr_weighted_pool_bwd(const void* x, int64_t x_ld, const float* w, const float* dout, void* dx, int64_t dx_ld, float* dw,
                                       int32_t N, int64_t hw, int32_t c, csbsr_stream_t s) {
  CSBSR_CHECK(x && w && dout && dx && dw && c % 8 == 0, "weighted_pool_bwd: bad args");
  const long blocks = (hw + 3) / 4;
  hipLaunchKernelGGL(wpool_bwd_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384), N), dim3(256), 0, ST(s), (const half_t*)x, x_ld, w,
                     dout, (half_t*)dx, dx_ld, dw, (long)hw, c / 8);
  CSBSR_LAUNCH_CHECK("csbsr_weighted_pool_bwd");
  return 0;
}

__global__ void fill16_kernel(half_t* p, long npix, int c8, long ld, float v) {
  const long total = npix * c8;
  h8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (half_t)v;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
    *reinterpret_cast<h8*>(p + (i / c8) * ld + (i % c8) * 8) = o;
}
extern "C" int csbsr_fill_f16(void* p, int64_t npix, int32_t c, int64_t ld, float v, csbsr_stream_t s) {
  CSBSR_CHECK(c % 8 == 0 && p, "fill: bad args");
  hipLaunchKernelGGL(fill16_kernel, dim3(grid_for(npix * (c / 8))), dim3(256), 0, ST(s), (half_t*)p, npix, c / 8, ld, v);
  CSBSR_LAUNCH_CHECK("csbsr_fill_f16");
  return 0;
}

// fp32 NCHW (optionally normalised per (n,c): (x-mean)*invstd) -> fp16 NHWC, channels padded with zeros
__global__ void nchw32_to_nhwc16_kernel(const float* src, half_t* dst, int N, int C, long hw, int cp, long d_ld,
                                        const float* mean, const float* invstd, long d_lo) {
  const int c8 = cp / 8;
  const long total = (long)N * hw * c8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % c8); const long px = i / c8;
    const long n = px / hw, r = px - n * hw;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = cc * 8 + e;
      float v = 0.f;
      if (c < C) {
        v = src[(n * C + c) * hw + r];
        if (mean) v = (v - mean[n * C + c]) * invstd[n * C + c];
      }
      o[e] = v;
    }
    st_split(dst + px * d_ld + cc * 8, d_lo, o);
  }
}
extern "C" int csbsr_nchw32_to_nhwc16_split(const float* src, void* dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t cp,
                                            int64_t dst_ld, int64_t dst_lo, const float* mean, const float* invstd, csbsr_stream_t s) {
  CSBSR_CHECK(src && dst && cp % 8 == 0 && cp >= C, "nchw32_to_nhwc16: bad args");
  const long hw = (long)H * W;
  hipLaunchKernelGGL(nchw32_to_nhwc16_kernel, dim3(grid_for((long)N * hw * (cp / 8))), dim3(256), 0, ST(s), src, (half_t*)dst, N,
                     C, hw, cp, dst_ld, mean, invstd, dst_lo);
  CSBSR_LAUNCH_CHECK("csbsr_nchw32_to_nhwc16");
  return 0;
}
extern "C" int csbsr_nchw32_to_nhwc16(const float* src, void* dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t cp,
                                      int64_t dst_ld, const float* mean, const float* invstd, csbsr_stream_t s) {
  return csbsr_nchw32_to_nhwc16_split(src, dst, N, C, H, W, cp, dst_ld, 0, mean, invstd, s);
}
// fp16 NHWC (first C channels) -> fp32 NCHW, dst = beta*dst + alpha*src
__global__ void nhwc16_to_nchw32_kernel(const half_t* src, long s_ld, float* dst, int N, int C, long hw, float alpha, float beta) {
  const long total = (long)N * hw;
  for (long px = (long)blockIdx.x * blockDim.x + threadIdx.x; px < total; px += (long)gridDim.x * blockDim.x) {
    const long n = px / hw, r = px - n * hw;
    const h8 v = *reinterpret_cast<const h8*>(src + px * s_ld);
    for (int c = 0; c < C && c < 8; ++c) {
      float* q = dst + (n * C + c) * hw + r;
      *q = (beta != 0.f ? beta * *q : 0.f) + alpha * (float)v[c];
    }
  }
}
extern "C" int csbsr_nhwc16_to_nchw32(const void* src, int64_t src_ld, float* dst, int32_t N, int32_t C, int32_t H, int32_t W,
                                      float alpha, float beta, csbsr_stream_t s) {
  CSBSR_CHECK(src && dst && C <= 8, "nhwc16_to_nchw32: supports up to 8 channels");
  const long hw = (long)H * W;
  hipLaunchKernelGGL(nhwc16_to_nchw32_kernel, dim3(grid_for((long)N * hw)), dim3(256), 0, ST(s), (const half_t*)src, src_ld, dst,
                     N, C, hw, alpha, beta);
  CSBSR_LAUNCH_CHECK("csbsr_nhwc16_to_nchw32");
  return 0;
}

// per-plane reductions of fp32 NCHW planes: out[plane][0] = sum a, [1] = sum a*a (b==NULL) or sum a*b
__global__ __launch_bounds__(256) void plane_reduce_kernel(const float* a, const float* b, long hw, float* out, int chunks) {
  __shared__ float s0[4], s1[4];
  const int plane = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const long per = (hw + chunks - 1) / chunks;
  const long beg = chunk * per, end = beg + per < hw ? beg + per : hw;
  const float* pa = a + (long)plane * hw;
  const float* pb = b ? b + (long)plane * hw : nullptr;
  float x0 = 0.f, x1 = 0.f;
  for (long i = beg + threadIdx.x; i < end; i += 256) {
    const float v = pa[i];
    x0 += v; x1 += pb ? v * pb[i] : v * v;
  }
  x0 = wave_sum(x0); x1 = wave_sum(x1);
  if ((threadIdx.x & 63) == 0) { s0[threadIdx.x >> 6] = x0; s1[threadIdx.x >> 6] = x1; }
  __syncthreads();
  if (threadIdx.x == 0) {      // partial row per (plane, chunk)
    out[(long)blockIdx.x * 2] = s0[0] + s0[1] + s0[2] + s0[3];
    out[(long)blockIdx.x * 2 + 1] = s1[0] + s1[1] + s1[2] + s1[3];
  }
}
extern "C" int csbsr_plane_reduce(const float* a, const float* b, int32_t planes, int64_t hw, float* out /*[planes][2] zeroed*/,
                                  csbsr_stream_t s) {
  CSBSR_CHECK(a && out, "plane_reduce: null");
  int chunks = (int)((hw + 65535) / 65536);
  if (chunks < 1) chunks = 1;
  float* part = csbsr_red_scratch((long)planes * chunks * 2);
  CSBSR_NEED_SCRATCH(part, "plane_reduce");
  hipLaunchKernelGGL(plane_reduce_kernel, dim3(planes * chunks), dim3(256), 0, ST(s), a, b, hw, part, chunks);
  if (csbsr_sum_partials_batched(part, chunks, 2, 2, out, planes, 2, ST(s))) return 1;
  CSBSR_LAUNCH_CHECK("csbsr_plane_reduce");
  return 0;
}

// Per-sample, per-channel mean of an fp16 NHWC map over a regular SUBSAMPLE of its pixels (every step-th row and column): the input
// statistic of the weight-rounding compensation (csbsr_amd/engine.py Conv._dc_bias) -- a correction term of relative size 2^-12, for
// which a 1 / step^2 sample of the pixels is plenty (>= 1e4 pixels per channel at the sizes that matter) and costs 1 / step^2 of a pass
// over the map.  grid = (slices, N); a workgroup walks its share of a sample's sampled pixels with ALL channel octets of a pixel on
// neighbouring lanes (256 / octets pixels per pass), so every cache line of a sampled pixel is fetched once, by one workgroup.  (Round 4
// gave every channel octet its own workgroup: the 16 octets of a 128-channel pixel -- two lines -- were fetched by 16 workgroups on 8
// XCDs, 0.42 GB per HR launch for 51 MB of sampled pixels, 4.5 GB per image-step.)  Each lane keeps the sums of its (pixel lane, octet);
// the pixel lanes of an octet are added in lane order through LDS; slices write partial rows that csbsr_sum_partials_batched folds in a
// fixed tree.  Bit-reproducible like every reduction here, and a function of the sample alone (KBPN stays free of batch-coupled
// operations).
#define CM_MAX_SLICES 64
__global__ __launch_bounds__(256) void channel_mean_sub_kernel(const half_t* x, long sn, long sy, long sx, int H, int W, int step,
                                                                float inv_count, float* part, int cp) {
  __shared__ float sm[256][8];
  const int slice = blockIdx.x, nsl = gridDim.x, n = blockIdx.y, tid = threadIdx.x;
  const int hs = (H + step - 1) / step, ws = (W + step - 1) / step;
  const int total = hs * ws, nocts = cp >> 3;
  for (int oct0 = 0; oct0 < nocts; oct0 += 256) {           // (more than 256 octets: 2048+ channels, not on today's path)
    const int no = nocts - oct0 < 256 ? nocts - oct0 : 256;
    const int P = 256 / no;                                  // pixels per pass
    const int pl = tid / no, oct = oct0 + tid % no;
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
    if (pl < P) {
#pragma unroll 4      // (independent loads: several in flight per thread -- the kernel is latency-bound)
      for (int i = slice * P + pl; i < total; i += nsl * P) {
        const int y = (i / ws) * step, xx = (i % ws) * step;
        const h8 v = *reinterpret_cast<const h8*>(x + n * sn + y * sy + xx * sx + oct * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += (float)v[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sm[tid][e] = a[e];
    __syncthreads();
    if (tid < no) {                                          // pixel lanes of this octet, in lane order
      float r[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = 0.f;
      for (int q = 0; q < P; ++q) {
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] += sm[q * no + tid][e];
      }
      float* dst = part + ((long)n * nsl + slice) * cp + (oct0 + tid) * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) dst[e] = r[e] * inv_count;
    }
    __syncthreads();
  }
}
extern "C" int csbsr_channel_mean_sub(const void* x, int64_t sn, int64_t sy, int64_t sx, int32_t N, int32_t H, int32_t W, int32_t cp,
                                      int32_t step, float* out /*[N][cp], overwritten*/, csbsr_stream_t s) {
  CSBSR_CHECK(x && out && cp > 0 && cp % 8 == 0 && step >= 1 && N > 0 && H > 0 && W > 0, "channel_mean_sub: bad args");
  const long count = (long)((H + step - 1) / step) * ((W + step - 1) / step);
  const int P = (cp >> 3) >= 256 ? 1 : 256 / (cp >> 3);
  long nsl = (count + (long)P * 16 - 1) / ((long)P * 16);      // >= 16 passes per workgroup
  if (nsl > CM_MAX_SLICES) nsl = CM_MAX_SLICES;
  if (nsl <= 1) {
    hipLaunchKernelGGL(channel_mean_sub_kernel, dim3(1, N), dim3(256), 0, ST(s), (const half_t*)x, (long)sn, (long)sy, (long)sx, H, W,
                       step, 1.f / (float)count, out, cp);
  } else {
    float* part = csbsr_red_scratch((long)N * nsl * cp);
    CSBSR_NEED_SCRATCH(part, "channel_mean_sub");
    CSBSR_CHECK(hipMemsetAsync(out, 0, (size_t)N * cp * sizeof(float), ST(s)) == hipSuccess, "channel_mean_sub: memset failed");
    hipLaunchKernelGGL(channel_mean_sub_kernel, dim3((unsigned)nsl, N), dim3(256), 0, ST(s), (const half_t*)x, (long)sn, (long)sy, (long)sx, H, W,
                       step, 1.f / (float)count, part, cp);
    if (csbsr_sum_partials_batched(part, (int)nsl, cp, cp, out, N, cp, ST(s))) return 1;
  }
  CSBSR_LAUNCH_CHECK("csbsr_channel_mean_sub");
  return 0;
}

// Weight rounding for the plain-fp16 (KBPN) layers and the two small contractions of its compensation (engine.Conv._wq / _dc_bias):
//   round_weights: wq = the fp16 value each weight is multiplied as (held as fp32), S[o][c] = sum over taps of (w - wq)[o][c][tap]
//                  (once per layer and optimiser step).  mode 0: round to nearest.  mode >= 1: TAP-SUM-PRESERVING -- after rounding to nearest,
//                  per (o, c) and tap group the taps that sat closest to a rounding midpoint move to their other fp16 neighbour until the
//                  group's summed residual is below half an ulp, so the rounding error of a filter has (almost) no response to an input that
//                  is constant over its footprint.  Group = all taps (mode 1: Conv2d, any stride) or the taps (ky % mode, kx % mode) one
//                  output PHASE of a stride-``mode`` transposed convolution sees.  What is left of the response to the input's mean goes
//                  back through the bias (S, dc_bias).  CPU study: tests/study_kbpn_precision.py (segmentation map of the contractive
//                  fixture, W + X plan: 1.61e-3 nearest, 1.38e-3 nearest + bias, 1.15e-3 tap-sum + bias).
//   dc_bias:       out[n][o] = (bias ? bias[o] : 0) + sum_c S[o][c] * mean[n][c]    (once per layer and forward; the means of up to two
//                  input segments, c0 / c1 real channels each).  One wave per (sample, output channel): lanes stride the channels, fixed
//                  xor-shuffle tree -- order-fixed.
__device__ __forceinline__ float f16_spacing(float q, float dir) {      // distance from the fp16 value q to its neighbour in direction dir (+-1)
  const float a = fabsf(q);
  if (a <= 6.103515625e-05f) return 5.9604644775390625e-08f;     // subnormals and the smallest normal: 2^-24 either way
  int e;
  const float m = frexpf(a, &e);                                 // a = m 2^e, m in [0.5, 1)
  const bool inward = q * dir < 0.f;                             // towards zero: below a power of two the grid is twice as fine
  return ldexpf(1.f, e - ((inward && m == 0.5f) ? 12 : 11));
}
// one thread per (d0, d1) filter.  Generic form: taps re-read from memory in every scan (any KH x KW; latency-bound: 160 us per 8x8 layer)
__global__ void round_weights_kernel(const float* w, float* wq, float* S, long rows, int KH, int KW, int mode) {
  const int T = KH * KW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (long)gridDim.x * blockDim.x) {
    const float* src = w + i * T;
    float* q = wq + i * T;
    for (int t = 0; t < T; ++t) q[t] = (float)(half_t)src[t];
    if (mode >= 1 && T > 1) {
      const int ng = mode * mode;
      for (int g = 0; g < ng; ++g) {
        const int gy = g / mode, gx = g % mode;
        for (int it = 0; it < T; ++it) {
          float r = 0.f;
          for (int ky = gy; ky < KH; ky += mode)
            for (int kx = gx; kx < KW; kx += mode) r += src[ky * KW + kx] - q[ky * KW + kx];
          if (r == 0.f) break;
          const float sg = r > 0.f ? 1.f : -1.f;
          int best = -1;
          float bs = 0.f, bu = 0.f;
          for (int ky = gy; ky < KH; ky += mode)
            for (int kx = gx; kx < KW; kx += mode) {
              const int t = ky * KW + kx;
              const float d = src[t] - q[t];
              if (d * sg <= 0.f) continue;
              const float u = f16_spacing(q[t], sg);
              if (fabsf(r) - fabsf(r - sg * u) <= 0.f) continue;       // moving this tap would not shrink the group's residual
              const float sc = fabsf(d) / u;                            // closest to its rounding midpoint first: least extra error
              if (sc > bs) { bs = sc; best = t; bu = u; }
            }
          if (best < 0) break;
          q[best] = (float)(half_t)(q[best] + sg * bu);
        }
      }
    }
    if (S) {
      float a = 0.f;
      for (int t = 0; t < T; ++t) a += src[t] - q[t];
      S[i] = a;
    }
  }
}
// the same rule with the filter in registers (compile-time tap count and grouping, every loop unrolled, the moved tap written by a
// predicated sweep instead of a dynamic index): the layers of the x4 network -- 3x3, 8x8 Conv2d (one group of 64 taps), 8x8 stride-4
// ConvTranspose2d (16 phases of 4 taps).  Same summation order as the generic form: bit-identical results.
template <int KH, int KW, int MODE>
__global__ __launch_bounds__(64) void round_weights_reg_kernel(const float* w, float* wq, float* S, long rows) {
  constexpr int T = KH * KW;
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= rows) return;
  float src[T], q[T];
#pragma unroll
  for (int t = 0; t < T; ++t) { src[t] = w[i * T + t]; q[t] = (float)(half_t)src[t]; }
  // hipcc (ROCm 7.2) MISCOMPILES this nest when the group loop is unrolled and the iteration loop is left through lane-divergent
  // breaks: rows whose neighbours in the wave finished earlier lose moves (found by the test against the CPU form; a stand-alone
  // reproduction behaves the same).  So the multi-group instances run a FIXED number of iterations per group with a ``done`` predicate
  // -- a group of n taps settles within n moves, 2 n + 2 is generous -- and only the single-group instances keep their breaks.
  constexpr int GT = (KH / MODE) * (KW / MODE);
  constexpr int NIT = MODE > 1 ? 2 * GT + 2 : T;
#pragma unroll
  for (int g = 0; g < MODE * MODE; ++g) {
    const int gy = g / MODE, gx = g % MODE;
    for (int it = 0; it < NIT; ++it) {
      float r = 0.f;
#pragma unroll
      for (int ky = 0; ky < KH; ++ky)
#pragma unroll
        for (int kx = 0; kx < KW; ++kx)
          if (ky % MODE == gy && kx % MODE == gx) r += src[ky * KW + kx] - q[ky * KW + kx];
      const bool done = r == 0.f;
      if constexpr (MODE == 1) { if (done) break; }
      const float sg = r > 0.f ? 1.f : -1.f;
      int best = -1;
      float bs = 0.f, bu = 0.f;
#pragma unroll
      for (int ky = 0; ky < KH; ++ky)
#pragma unroll
        for (int kx = 0; kx < KW; ++kx)
          if (ky % MODE == gy && kx % MODE == gx) {
            const int t = ky * KW + kx;
            const float d = src[t] - q[t];
            const float u = f16_spacing(q[t], sg);
            const float sc = fabsf(d) / u;
            const bool cand = !done && d * sg > 0.f && fabsf(r) - fabsf(r - sg * u) > 0.f && sc > bs;
            if (cand) { bs = sc; best = t; bu = u; }
          }
      if constexpr (MODE == 1) { if (best < 0) break; }
#pragma unroll
      for (int t = 0; t < T; ++t)
        if (t == best) q[t] = (float)(half_t)(q[t] + sg * bu);      // (best = -1: nothing moves)
    }
  }
  float a = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) { wq[i * T + t] = q[t]; a += src[t] - q[t]; }
  if (S) S[i] = a;
}
// The large filters, LPF lanes per filter with TPL taps each (a filter's taps are one coalesced read of its lanes):
//   MODE > 1 (ConvTranspose2d of that stride): LPF = MODE^2, lane = output phase (ky % MODE, kx % MODE), its <= TPL taps ARE the phase's
//   group -- no communication but the final tap sum;   MODE 1 (Conv2d): lane = TPL consecutive taps of the one group -- residual and best
//   candidate by fixed LPF-lane xor trees (ties -> the lower tap index, like the serial scan).
// The thread-per-filter forms above took 170-240 us per 128 x 128 x 8 x 8 layer (one wave per CU, 64 strided loads each: 25 launches, 5.3 ms
// per step of config 2) and milliseconds on the 12 x 12 filters of the x8 network.  Wave-uniform exit only (see the miscompile note above):
// a filter that has settled idles under its ``done`` flag.
template <int KH, int KW, int MODE, int LPF, int TPL>
__global__ __launch_bounds__(256) void round_weights_lanes_kernel(const float* w, float* wq, float* S, long rows) {
  constexpr int T = KH * KW;
  constexpr int NB = (KW + MODE - 1) / MODE;
  static_assert(MODE == 1 ? LPF * TPL >= T : (LPF == MODE * MODE && TPL == ((KH + MODE - 1) / MODE) * NB), "lane layout");
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = gid / LPF;
  const int sub = (int)(gid % LPF);
  const bool live = row < rows;
  int tix[TPL];
  bool ok[TPL];
#pragma unroll
  for (int j = 0; j < TPL; ++j) {
    if (MODE == 1) { tix[j] = sub * TPL + j; ok[j] = tix[j] < T; }
    else {
      const int ky = sub / MODE + MODE * (j / NB), kx = sub % MODE + MODE * (j % NB);
      tix[j] = ky * KW + kx; ok[j] = ky < KH && kx < KW;
    }
    ok[j] = ok[j] && live;
  }
  float src[TPL], q[TPL];
#pragma unroll
  for (int j = 0; j < TPL; ++j) { src[j] = ok[j] ? w[row * T + tix[j]] : 0.f; q[j] = (float)(half_t)src[j]; }
  bool done = !live;
  for (int it = 0; it < 2 * T + 2; ++it) {
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < TPL; ++j) r += src[j] - q[j];
    if (MODE == 1) {
#pragma unroll
      for (int o = 1; o < LPF; o <<= 1) r += __shfl_xor(r, o, 64);
    }
    done = done || r == 0.f;
    const float sg = r > 0.f ? 1.f : -1.f;
    int best = -1;
    float bs = 0.f, bu = 0.f;
#pragma unroll
    for (int j = 0; j < TPL; ++j) {
      const float d = src[j] - q[j];
      const float u = f16_spacing(q[j], sg);
      const float sc = fabsf(d) / u;
      const bool cand = !done && d * sg > 0.f && fabsf(r) - fabsf(r - sg * u) > 0.f && sc > bs;
      if (cand) { bs = sc; best = j; bu = u; }
    }
    int bt = T;                          // tap index of this lane's candidate
#pragma unroll
    for (int j = 0; j < TPL; ++j)
      if (j == best) bt = tix[j];
    bool mine = best >= 0;
    if (MODE == 1) {       // the lanes of a filter agree on ONE move: highest score, then lowest tap index
      float ws = bs;
      int wt = bt;
#pragma unroll
      for (int o = 1; o < LPF; o <<= 1) {
        const float os = __shfl_xor(ws, o, 64);
        const int ot = __shfl_xor(wt, o, 64);
        if (os > ws || (os == ws && ot < wt)) { ws = os; wt = ot; }
      }
      mine = best >= 0 && wt == bt;
      done = done || wt == T;
    } else {
      done = done || best < 0;
    }
#pragma unroll
    for (int j = 0; j < TPL; ++j)
      if (mine && j == best) q[j] = (float)(half_t)(q[j] + sg * bu);
    if (__all(done)) break;        // wave-uniform
  }
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < TPL; ++j) { if (ok[j]) wq[row * T + tix[j]] = q[j]; a += src[j] - q[j]; }
#pragma unroll
  for (int o = 1; o < LPF; o <<= 1) a += __shfl_xor(a, o, 64);
  if (S && live && sub == 0) S[row] = a;
}
template <int KH, int KW, int MODE, int LPF, int TPL>
static void launch_round_lanes(const float* w, float* wq, float* S, long rows, hipStream_t st) {
  hipLaunchKernelGGL((round_weights_lanes_kernel<KH, KW, MODE, LPF, TPL>), dim3((unsigned)((rows * LPF + 255) / 256)), dim3(256), 0, st, w, wq, S, rows);
}
extern "C" int csbsr_round_weights(const float* w, float* wq, float* S, int32_t D0, int32_t D1, int32_t KH, int32_t KW, int32_t mode,
                                   csbsr_stream_t s) {
  CSBSR_CHECK(w && wq && D0 > 0 && D1 > 0 && KH > 0 && KW > 0 && mode >= 0 && mode <= KH && mode <= KW, "round_weights: bad args");
  const long rows = (long)D0 * D1;
  const unsigned nb = (unsigned)((rows + 63) / 64);
  if (KH == 3 && KW == 3 && mode == 1) hipLaunchKernelGGL((round_weights_reg_kernel<3, 3, 1>), dim3(nb), dim3(64), 0, ST(s), w, wq, S, rows);
  else if (KH == 8 && KW == 8 && mode == 1) launch_round_lanes<8, 8, 1, 16, 4>(w, wq, S, rows, ST(s));
  else if (KH == 8 && KW == 8 && mode == 4) launch_round_lanes<8, 8, 4, 16, 4>(w, wq, S, rows, ST(s));
  else if (KH == 12 && KW == 12 && mode == 1) launch_round_lanes<12, 12, 1, 16, 9>(w, wq, S, rows, ST(s));
  else if (KH == 12 && KW == 12 && mode == 8) launch_round_lanes<12, 12, 8, 64, 4>(w, wq, S, rows, ST(s));
  else {
    const int blocks = (int)(nb > 4096 ? 4096 : nb);
    hipLaunchKernelGGL(round_weights_kernel, dim3(blocks), dim3(64), 0, ST(s), w, wq, S, rows, KH, KW, mode);
  }
  CSBSR_LAUNCH_CHECK("csbsr_round_weights");
  return 0;
}
__global__ __launch_bounds__(256) void dc_bias_kernel(const float* S, int cin, const float* m0, long m0_ld, int c0, const float* m1, long m1_ld, int c1,
                                                       const float* bias, float* out, int cout) {
  const int n = blockIdx.y, o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (o >= cout) return;
  const float* row = S + (long)o * cin;
  float a = 0.f;
  for (int c = lane; c < c0; c += 64) a += row[c] * m0[n * m0_ld + c];
  for (int c = lane; c < c1; c += 64) a += row[c0 + c] * m1[n * m1_ld + c];
  a = wave_sum(a);
  if (lane == 0) out[(long)n * cout + o] = a + (bias ? bias[o] : 0.f);
}
extern "C" int csbsr_dc_bias(const float* S, int32_t cout, int32_t cin, const float* m0, int64_t m0_ld, int32_t c0, const float* m1, int64_t m1_ld,
                             int32_t c1, const float* bias, int32_t N, float* out, csbsr_stream_t s) {
  CSBSR_CHECK(S && m0 && out && cout > 0 && c0 > 0 && c1 >= 0 && c0 + c1 <= cin && N > 0 && (c1 == 0 || m1), "dc_bias: bad args");
  hipLaunchKernelGGL(dc_bias_kernel, dim3((cout + 3) / 4, N), dim3(256), 0, ST(s), S, cin, m0, (long)m0_ld, c0, m1, (long)m1_ld, c1, bias, out, cout);
  CSBSR_LAUNCH_CHECK("csbsr_dc_bias");
  return 0;
}

// InstanceNorm2d backward on planes: dx (+)= invstd*(dy - mean(dy) - xhat*mean(dy*xhat)), dy given as fp16 NHWC8
__global__ void instnorm_bwd_reduce_kernel(const half_t* dy, long dy_ld, const float* x, const float* mean, const float* invstd,
                                           int C, long hw, float* red /*[N*C][2]*/, int chunks) {
  __shared__ float sm[4][8][2];
  const int n = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const long per = (hw + chunks - 1) / chunks;
  const long beg = chunk * per, end = beg + per < hw ? beg + per : hw;
  float a0[8], a1[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) a0[c] = a1[c] = 0.f;
  for (long i = beg + threadIdx.x; i < end; i += 256) {
    const h8 g = *reinterpret_cast<const h8*>(dy + ((long)n * hw + i) * dy_ld);
    for (int c = 0; c < C; ++c) {
      const float xh = (x[((long)n * C + c) * hw + i] - mean[n * C + c]) * invstd[n * C + c];
      a0[c] += (float)g[c]; a1[c] += (float)g[c] * xh;
    }
  }
  for (int c = 0; c < C; ++c) {
    const float v0 = wave_sum(a0[c]), v1 = wave_sum(a1[c]);
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][c][0] = v0; sm[threadIdx.x >> 6][c][1] = v1; }
  }
  __syncthreads();
  if (threadIdx.x < C) {      // partial row per (sample, chunk): [C][2]
    const int c = threadIdx.x;
    red[((long)blockIdx.x * C + c) * 2] = sm[0][c][0] + sm[1][c][0] + sm[2][c][0] + sm[3][c][0];
    red[((long)blockIdx.x * C + c) * 2 + 1] = sm[0][c][1] + sm[1][c][1] + sm[2][c][1] + sm[3][c][1];
  }
}
__global__ void instnorm_bwd_apply_kernel(const half_t* dy, long dy_ld, const float* x, const float* mean, const float* invstd,
                                          const float* red, int N, int C, long hw, float* dx, int accumulate) {
  const long total = (long)N * hw;
  for (long px = (long)blockIdx.x * blockDim.x + threadIdx.x; px < total; px += (long)gridDim.x * blockDim.x) {
    const long n = px / hw, r = px - n * hw;
    const h8 g = *reinterpret_cast<const h8*>(dy + px * dy_ld);
    for (int c = 0; c < C; ++c) {
      const long pi = n * C + c;
      const float is = invstd[pi];
      const float xh = (x[pi * hw + r] - mean[pi]) * is;
      const float v = is * ((float)g[c] - red[pi * 2] / hw - xh * red[pi * 2 + 1] / hw);
      float* q = dx + pi * hw + r;
      *q = accumulate ? *q + v : v;
    }
  }
}
extern "C" int csbsr_instnorm_bwd(const void* dy, int64_t dy_ld, const float* x, const float* mean, const float* invstd,
                                  float* dx, int32_t accumulate, int32_t N, int32_t C, int64_t hw, float* red /*[N*C][2] zeroed*/,
                                  csbsr_stream_t s) {
  CSBSR_CHECK(dy && x && dx && red && C <= 8, "instnorm_bwd: bad args");
  int chunks = (int)((hw + 65535) / 65536);
  if (chunks < 1) chunks = 1;
  float* part = csbsr_red_scratch((long)N * chunks * C * 2);
  CSBSR_NEED_SCRATCH(part, "instnorm_bwd");
  hipLaunchKernelGGL(instnorm_bwd_reduce_kernel, dim3(N * chunks), dim3(256), 0, ST(s), (const half_t*)dy, dy_ld, x, mean, invstd, C,
                     hw, part, chunks);
  if (csbsr_sum_partials_batched(part, chunks, 2 * C, 2 * C, red, N, 2 * C, ST(s))) return 1;
  hipLaunchKernelGGL(instnorm_bwd_apply_kernel, dim3(grid_for((long)N * hw)), dim3(256), 0, ST(s), (const half_t*)dy, dy_ld, x, mean,
                     invstd, red, N, C, hw, dx, accumulate);
  CSBSR_LAUNCH_CHECK("csbsr_instnorm_bwd");
  return 0;
}

// ------------------------------------------------------------------------------------------- batch norm (train)
__global__ void bn_finalize_kernel(const float* stat, long count, int c, int cstride, float eps, float momentum, float* mean,
                                   float* invstd, float* rmean, float* rvar) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c) return;
  const double m = (double)stat[i] / count;
  double var = (double)stat[cstride + i] / count - m * m;
  if (var < 0) var = 0;
  mean[i] = (float)m;
  invstd[i] = (float)(1.0 / sqrt(var + eps));
  if (rmean) {
    const double unb = count > 1 ? var * count / (count - 1) : var;
    rmean[i] = (1.f - momentum) * rmean[i] + momentum * (float)m;
    rvar[i] = (1.f - momentum) * rvar[i] + momentum * (float)unb;
  }
}
extern "C" int csbsr_bn_finalize(const float* stat, int64_t count, int32_t c, int32_t cstride, float eps, float momentum,
                                 float* mean, float* invstd, float* running_mean, float* running_var, csbsr_stream_t s) {
  CSBSR_CHECK(stat && mean && invstd, "bn_finalize: null");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((c + 255) / 256), dim3(256), 0, ST(s), stat, (long)count, c, cstride, eps, momentum, mean,
                     invstd, running_mean, running_var);
  CSBSR_LAUNCH_CHECK("csbsr_bn_finalize");
  return 0;
}

struct BnK {
  long npix, hw; int c8;
  const half_t* x; long x_ld;
  const float *mean, *invstd, *gamma, *beta;
  const half_t* res; long res_ld;
  int act; const float* prelu; const float* drop;
  half_t* y; long y_ld;
  long x_lo, res_lo, y_lo;          // split-fp16 planes (0: plain fp16)
  // backward
  const half_t* dy; long dy_ld;
  float* red; float* dprelu;
  half_t* dx; long dx_ld;
  half_t* dres; long dres_ld; int dres_acc;
  float *dgamma, *dbeta;
  int cp;
  float* part; long part_ld;        // bn_bwd_reduce partial rows: [2*cp] sums, PReLU-slope sum at 2*cp
};

// Elementwise BN kernels: the launch has a multiple of c8 threads in total, so a thread keeps ONE channel octet for its whole
// grid-stride loop -- per-channel parameters live in registers and the loop has no integer division (the first version spent
// most of its time in two 64-bit divisions and 40 parameter loads per 48 bytes of traffic: ~1 TB/s).
static inline int grid_for_c8(long work, int c8) {
  int g = grid_for(work), a = 256, b = c8;
  while (b) { const int t = a % b; a = b; b = t; }       // a = gcd(256, c8)
  const int m = c8 / a;                                  // grid must be a multiple of m
  g = (g + m - 1) / m * m;
  return g;
}

__global__ void bn_apply_kernel(const BnK p) {
  const long T = (long)gridDim.x * blockDim.x;
  const long gt = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c0 = (int)(gt % p.c8) * 8;
  const long pstep = T / p.c8;
  const float slope = p.act == CSBSR_ACT_PRELU ? *p.prelu : 0.f;
  float mean[8], sc[8], be[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { mean[e] = p.mean[c0 + e]; sc[e] = p.invstd[c0 + e] * p.gamma[c0 + e]; be[e] = p.beta[c0 + e]; }
  for (long px = gt / p.c8; px < p.npix; px += pstep) {
    float xv[8], rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, o[8];
    ld_split(p.x + px * p.x_ld + c0, p.x_lo, xv);
    if (p.res) ld_split(p.res + px * p.res_ld + c0, p.res_lo, rv);
    float dr[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    if (p.drop) ld8f(p.drop + (long)((unsigned)px / (unsigned)p.hw) * p.cp + c0, dr);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = (xv[e] - mean[e]) * sc[e] + be[e] + rv[e];
      v = apply_act(v, p.act, slope);
      v *= dr[e];
      o[e] = v;
    }
    st_split(p.y + px * p.y_ld + c0, p.y_lo, o);
  }
}

// z = gamma*xhat + beta + res ; y = drop * act(z).  dz = dy * drop * act'(z)
__device__ __forceinline__ float bn_dz(const BnK& p, float dy, float xh, float r, int c, long n, float slope, float& dslope) {
  const float z = xh * p.gamma[c] + p.beta[c] + r;
  float g = dy;
  if (p.drop) g *= p.drop[n * p.cp + c];
  switch (p.act) {
    case CSBSR_ACT_RELU: return z > 0.f ? g : 0.f;
    case CSBSR_ACT_PRELU:
      if (!(z > 0.f)) { dslope += g * z; return g * slope; }
      return g;
    default: return g;
  }
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const BnK p) {
  __shared__ float sRed[256 * 16];
  __shared__ float sPre[4];
  const int tid = threadIdx.x;
  const int cpb = p.c8 < 256 ? p.c8 : 256;
  const int ppb = 256 / cpb;
  const int ch = tid % cpb, pl = tid / cpb;
  const float slope = p.act == CSBSR_ACT_PRELU ? *p.prelu : 0.f;
  float dsl = 0.f;
  for (int cbase = 0; cbase < p.c8; cbase += cpb) {
    float s0[8], s1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s0[e] = s1[e] = 0.f;
    const int c8i = cbase + ch;
    if (c8i < p.c8 && pl < ppb) {
      const int c0 = c8i * 8;
      float mean[8], istd[8], ga[8], be[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { mean[e] = p.mean[c0 + e]; istd[e] = p.invstd[c0 + e]; ga[e] = p.gamma[c0 + e]; be[e] = p.beta[c0 + e]; }
      for (long px = (long)blockIdx.x * ppb + pl; px < p.npix; px += (long)gridDim.x * ppb) {
        const h8 g = *reinterpret_cast<const h8*>(p.dy + px * p.dy_ld + c0);
        float xv[8], rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        ld_split(p.x + px * p.x_ld + c0, p.x_lo, xv);
        if (p.res) ld_split(p.res + px * p.res_ld + c0, p.res_lo, rv);
        float dr[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    if (p.drop) ld8f(p.drop + (long)((unsigned)px / (unsigned)p.hw) * p.cp + c0, dr);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xh = (xv[e] - mean[e]) * istd[e];
          const float z = xh * ga[e] + be[e] + rv[e];
          float gg = (float)g[e];
          gg *= dr[e];
          float dz = gg;
          if (p.act == CSBSR_ACT_RELU) dz = z > 0.f ? gg : 0.f;
          else if (p.act == CSBSR_ACT_PRELU && !(z > 0.f)) { dsl += gg * z; dz = gg * slope; }
          s0[e] += dz; s1[e] += dz * xh;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { sRed[tid * 16 + e] = s0[e]; sRed[tid * 16 + 8 + e] = s1[e]; }
    __syncthreads();
    if (tid < cpb && cbase + tid < p.c8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float a = 0.f, b = 0.f;
        for (int q = 0; q < ppb; ++q) { a += sRed[(q * cpb + tid) * 16 + e]; b += sRed[(q * cpb + tid) * 16 + 8 + e]; }
        p.part[(long)blockIdx.x * p.part_ld + (cbase + tid) * 8 + e] = a;
        p.part[(long)blockIdx.x * p.part_ld + p.cp + (cbase + tid) * 8 + e] = b;
      }
    }
    __syncthreads();
  }
  if (p.dprelu) {
    dsl = wave_sum(dsl);
    if ((tid & 63) == 0) sPre[tid >> 6] = dsl;
    __syncthreads();
    if (tid == 0) {
      p.part[(long)blockIdx.x * p.part_ld + 2 * p.cp] = sPre[0] + sPre[1] + sPre[2] + sPre[3];
    }
  }
}

__global__ void bn_bwd_apply_kernel(const BnK p) {
  const long T = (long)gridDim.x * blockDim.x;
  const long gt = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c0 = (int)(gt % p.c8) * 8;
  const long pstep = T / p.c8;
  const float slope = p.act == CSBSR_ACT_PRELU ? *p.prelu : 0.f;
  const float inv_cnt = 1.f / (float)p.npix;
  float mean[8], istd[8], ga[8], be[8], k1[8], k2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = c0 + e;
    mean[e] = p.mean[c]; istd[e] = p.invstd[c]; ga[e] = p.gamma[c]; be[e] = p.beta[c];
    k1[e] = p.red[c] * inv_cnt; k2[e] = p.red[p.cp + c] * inv_cnt;
  }
  for (long px = gt / p.c8; px < p.npix; px += pstep) {
    const h8 g = *reinterpret_cast<const h8*>(p.dy + px * p.dy_ld + c0);
    float xv[8], rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    ld_split(p.x + px * p.x_ld + c0, p.x_lo, xv);
    if (p.res) ld_split(p.res + px * p.res_ld + c0, p.res_lo, rv);
    float dr[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    if (p.drop) ld8f(p.drop + (long)((unsigned)px / (unsigned)p.hw) * p.cp + c0, dr);
    h8 old = {0, 0, 0, 0, 0, 0, 0, 0};
    if (p.dres && p.dres_acc) old = *reinterpret_cast<const h8*>(p.dres + px * p.dres_ld + c0);
    h8 o, drs;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = (xv[e] - mean[e]) * istd[e];
      const float z = xh * ga[e] + be[e] + rv[e];
      float gg = (float)g[e];
      gg *= dr[e];
      float dz = gg;
      if (p.act == CSBSR_ACT_RELU) dz = z > 0.f ? gg : 0.f;
      else if (p.act == CSBSR_ACT_PRELU) dz = z > 0.f ? gg : gg * slope;
      o[e] = (half_t)(ga[e] * istd[e] * (dz - k1[e] - xh * k2[e]));
      drs[e] = (half_t)(dz + (float)old[e]);
    }
    *reinterpret_cast<h8*>(p.dx + px * p.dx_ld + c0) = o;
    if (p.dres) *reinterpret_cast<h8*>(p.dres + px * p.dres_ld + c0) = drs;
  }
}
__global__ void bn_param_grad_kernel(const float* red, int c, int cp, float* dgamma, float* dbeta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c) return;
  dbeta[i] += red[i];
  dgamma[i] += red[cp + i];
}

static void fill_bnk(BnK& k, const csbsr_bn_desc_t* d) {
  k.npix = d->npix; k.hw = d->hw; k.c8 = d->c / 8; k.cp = d->c;
  k.x = (const half_t*)d->x; k.x_ld = d->x_ld;
  k.mean = d->mean; k.invstd = d->invstd; k.gamma = d->gamma; k.beta = d->beta;
  k.res = (const half_t*)d->res; k.res_ld = d->res_ld;
  k.act = d->act; k.prelu = d->prelu; k.drop = d->drop;
  k.y = (half_t*)d->y; k.y_ld = d->y_ld;
  k.x_lo = d->x_lo; k.res_lo = d->res_lo; k.y_lo = d->y_lo;
  k.dy = (const half_t*)d->dy; k.dy_ld = d->dy_ld;
  k.red = d->red; k.dprelu = d->dprelu;
  k.dx = (half_t*)d->dx; k.dx_ld = d->dx_ld;
  k.dres = (half_t*)d->dres; k.dres_ld = d->dres_ld; k.dres_acc = d->dres_accumulate;
  k.dgamma = d->dgamma; k.dbeta = d->dbeta;
}
extern "C" int csbsr_bn_apply(const csbsr_bn_desc_t* d, csbsr_stream_t s) {
  CSBSR_CHECK(d && d->x && d->y && d->c % 8 == 0, "bn_apply: bad args");
  BnK k; fill_bnk(k, d);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for_c8(k.npix * k.c8, k.c8)), dim3(256), 0, ST(s), k);
  CSBSR_LAUNCH_CHECK("csbsr_bn_apply");
  return 0;
}
extern "C" int csbsr_bn_backward(const csbsr_bn_desc_t* d, csbsr_stream_t s) {
  CSBSR_CHECK(d && d->x && d->dy && d->dx && d->red && d->c % 8 == 0, "bn_backward: bad args");
  BnK k; fill_bnk(k, d);
  const int cpb = k.c8 < 256 ? k.c8 : 256;
  const int ppb = 256 / cpb;
  const int rblocks = grid_for(k.npix, ppb * 8, 1024);
  k.part = nullptr; k.part_ld = 2 * k.cp + 8;
  k.part = csbsr_red_scratch((long)rblocks * k.part_ld);
  CSBSR_NEED_SCRATCH(k.part, "bn_backward");
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(rblocks), dim3(256), 0, ST(s), k);
  if (k.part) {
    csbsr_sum_partials(k.part, rblocks, k.part_ld, 2 * k.cp, k.red, ST(s));
    if (k.dprelu) csbsr_sum_partials(k.part + 2 * k.cp, rblocks, k.part_ld, 1, k.dprelu, ST(s));
  }
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for_c8(k.npix * k.c8, k.c8)), dim3(256), 0, ST(s), k);
  if (d->dgamma)
    hipLaunchKernelGGL(bn_param_grad_kernel, dim3((d->creal + 255) / 256), dim3(256), 0, ST(s), d->red, d->creal, d->c, d->dgamma, d->dbeta);
  CSBSR_LAUNCH_CHECK("csbsr_bn_backward");
  return 0;
}

// ------------------------------------------------------------------------------------------- max pool 3x3 s2 p1
__global__ void maxpool_fwd_kernel(const half_t* x, half_t* y, int N, int H, int W, int c8, int OH, int OW, long x_ld, long x_lo,
                                   long y_ld, long y_lo) {
  const long total = (long)N * OH * OW * c8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % c8); long t = i / c8;
    const int ox = (int)(t % OW); t /= OW;
    const int oy = (int)(t % OH); const int n = (int)(t / OH);
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = -65504.f;
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * 2 - 1 + ky; if ((unsigned)iy >= (unsigned)H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * 2 - 1 + kx; if ((unsigned)ix >= (unsigned)W) continue;
        float v[8];
        ld_split(x + (((long)n * H + iy) * W + ix) * x_ld + cc * 8, x_lo, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], v[e]);
      }
    }
    st_split(y + (i / c8) * y_ld + cc * 8, y_lo, m);
  }
}
// Backward, block-stationary gather: a thread owns a 2 x 2 block of input pixels (rows 2a, 2a+1; columns 2b, 2b+1) of one channel octet.
// Only the four windows (oy, ox) in {a, a+1} x {b, b+1} can touch the block; each is rescanned from x -- first maximum in scan order,
// torch's argmax rule (strict >) -- with nine 16-byte loads (L1 / L2 hits: a pixel is read by nine windows), its gradient goes to the
// block pixel that holds the argmax.  No saved output needed, no scalar loads, every dx pixel written once.  (The per-pixel version
// tested "am I the first maximum" with up to 8 scalar loads per element and window: 6.1 ms for the 64-channel 896^2 map at B = 8.)
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const half_t* x, const half_t* dy, half_t* dx, int N, int H, int W, int c8, int OH,
                                                          int OW, long x_ld, long x_lo) {
  const int HB = (H + 1) / 2, WB = (W + 1) / 2;
  const long total = (long)N * HB * WB * c8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % c8); long t = i / c8;
    const int b = (int)(t % WB); t /= WB;
    const int a = (int)(t % HB); const int n = (int)(t / HB);
    float acc[2][2][8];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[q >> 1][q & 1][e] = 0.f;
#pragma unroll
    for (int wy = 0; wy < 2; ++wy) {
      const int oy = a + wy;
      if (oy >= OH) continue;
#pragma unroll
      for (int wx = 0; wx < 2; ++wx) {
        const int ox = b + wx;
        if (ox >= OW) continue;
        float m[8];
        int idx[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { m[e] = -INFINITY; idx[e] = -1; }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int jy = 2 * oy - 1 + ky;
          if ((unsigned)jy >= (unsigned)H) continue;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int jx = 2 * ox - 1 + kx;
            if ((unsigned)jx >= (unsigned)W) continue;
            float v[8];
            ld_split(x + (((long)n * H + jy) * W + jx) * x_ld + cc * 8, x_lo, v);
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (v[e] > m[e]) { m[e] = v[e]; idx[e] = ky * 3 + kx; }
          }
        }
        const h8 g = *reinterpret_cast<const h8*>(dy + ((((long)n * OH + oy) * OW + ox) * c8 + cc) * 8);
        // block pixel (py, px) sits at window position (py + 1 - 2 wy, px + 1 - 2 wx)
#pragma unroll
        for (int py = 0; py < 2; ++py) {
          const int ky = py + 1 - 2 * wy;
          if (ky < 0) continue;
#pragma unroll
          for (int px = 0; px < 2; ++px) {
            const int kx = px + 1 - 2 * wx;
            if (kx < 0) continue;
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (idx[e] == ky * 3 + kx) acc[py][px][e] += (float)g[e];
          }
        }
      }
    }
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        const int iy = 2 * a + py, ix = 2 * b + px;
        if (iy >= H || ix >= W) continue;
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)acc[py][px][e];
        *reinterpret_cast<h8*>(dx + ((((long)n * H + iy) * W + ix) * c8 + cc) * 8) = o;
      }
  }
}
extern "C" int csbsr_maxpool3x3s2_fwd_split(const void* x, int64_t x_ld, int64_t x_lo, void* y, int64_t y_ld, int64_t y_lo, int32_t N,
                                            int32_t H, int32_t W, int32_t c, csbsr_stream_t s) {
  CSBSR_CHECK(x && y && c % 8 == 0, "maxpool: bad args");
  const int OH = (H + 2 - 3) / 2 + 1, OW = (W + 2 - 3) / 2 + 1;
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(grid_for((long)N * OH * OW * (c / 8))), dim3(256), 0, ST(s), (const half_t*)x, (half_t*)y, N,
                     H, W, c / 8, OH, OW, x_ld, x_lo, y_ld, y_lo);
  CSBSR_LAUNCH_CHECK("csbsr_maxpool3x3s2_fwd");
  return 0;
}
extern "C" int csbsr_maxpool3x3s2_fwd(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t c, csbsr_stream_t s) {
  return csbsr_maxpool3x3s2_fwd_split(x, c, 0, y, c, 0, N, H, W, c, s);
}
extern "C" int csbsr_maxpool3x3s2_bwd_split(const void* x, int64_t x_ld, int64_t x_lo, const void* y, int64_t y_ld, int64_t y_lo,
                                            const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t c, csbsr_stream_t s) {
  CSBSR_CHECK(x && y && dy && dx && c % 8 == 0, "maxpool_bwd: bad args");
  const int OH = (H + 2 - 3) / 2 + 1, OW = (W + 2 - 3) / 2 + 1;
  (void)y; (void)y_ld; (void)y_lo;        // (the saved output is not needed: the windows are rescanned)
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid_for((long)N * ((H + 1) / 2) * ((W + 1) / 2) * (c / 8))), dim3(256), 0, ST(s), (const half_t*)x,
                     (const half_t*)dy, (half_t*)dx, N, H, W, c / 8, OH, OW, x_ld, x_lo);
  CSBSR_LAUNCH_CHECK("csbsr_maxpool3x3s2_bwd");
  return 0;
}
extern "C" int csbsr_maxpool3x3s2_bwd(const void* x, const void* y, const void* dy, void* dx, int32_t N, int32_t H, int32_t W,
                                      int32_t c, csbsr_stream_t s) {
  return csbsr_maxpool3x3s2_bwd_split(x, c, 0, y, c, 0, dy, dx, N, H, W, c, s);
}

// ------------------------------------------------------------------------------------------- adaptive avg pool
__global__ void aap_fwd_kernel(const half_t* x, long x_ld, half_t* y, int N, int H, int W, int c8, int OH, int OW, long x_lo, long y_ld,
                               long y_lo) {
  const long total = (long)N * OH * OW * c8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % c8); long t = i / c8;
    const int ox = (int)(t % OW); t /= OW;
    const int oy = (int)(t % OH); const int n = (int)(t / OH);
    const int y0 = (oy * H) / OH, y1 = ((oy + 1) * H + OH - 1) / OH;
    const int x0 = (ox * W) / OW, x1 = ((ox + 1) * W + OW - 1) / OW;
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
    for (int iy = y0; iy < y1; ++iy)
      for (int ix = x0; ix < x1; ++ix) {
        float v[8];
        ld_split(x + (((long)n * H + iy) * W + ix) * x_ld + cc * 8, x_lo, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += v[e];
      }
    const float inv = 1.f / ((y1 - y0) * (x1 - x0));
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] *= inv;
    st_split(y + (i / c8) * y_ld + cc * 8, y_lo, a);
  }
}
__global__ void aap_bwd_kernel(const half_t* dy, half_t* dx, long dx_ld, int accumulate, int N, int H, int W, int c8, int OH, int OW) {
  const long total = (long)N * H * W * c8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % c8); long t = i / c8;
    const int ix = (int)(t % W); t /= W;
    const int iy = (int)(t % H); const int n = (int)(t / H);
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
    for (int oy = 0; oy < OH; ++oy) {
      const int y0 = (oy * H) / OH, y1 = ((oy + 1) * H + OH - 1) / OH;
      if (iy < y0 || iy >= y1) continue;
      for (int ox = 0; ox < OW; ++ox) {
        const int x0 = (ox * W) / OW, x1 = ((ox + 1) * W + OW - 1) / OW;
        if (ix < x0 || ix >= x1) continue;
        const h8 g = *reinterpret_cast<const h8*>(dy + ((((long)n * OH + oy) * OW + ox) * c8 + cc) * 8);
        const float inv = 1.f / ((y1 - y0) * (x1 - x0));
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += (float)g[e] * inv;
      }
    }
    half_t* q = dx + (((long)n * H + iy) * W + ix) * dx_ld + cc * 8;
    h8 o;
    if (accumulate) { const h8 old = *reinterpret_cast<const h8*>(q);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += (float)old[e]; }
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)a[e];
    *reinterpret_cast<h8*>(q) = o;
  }
}
// large bins (PSP priors 1,2,3,6 over a 224^2 map): one workgroup per (sample, bin, 64-channel group);
// 8 channel-chunk lanes x 32 pixel lanes, LDS tree over the pixel lanes
__global__ __launch_bounds__(256) void aap_fwd_block_kernel(const half_t* x, long x_ld, half_t* y, int N, int H, int W, int c8, int OH, int OW,
                                                            long x_lo, long y_ld, long y_lo) {
  __shared__ float sred[32][8][8];
  const int groups = (c8 + 7) / 8;
  int b = blockIdx.x;
  const int g = b % groups; b /= groups;
  const int ox = b % OW; b /= OW;
  const int oy = b % OH; const int n = b / OH;
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int cc = g * 8 + cl;
  const int y0 = (oy * H) / OH, y1 = ((oy + 1) * H + OH - 1) / OH;
  const int x0 = (ox * W) / OW, x1 = ((ox + 1) * W + OW - 1) / OW;
  const int bw = x1 - x0, cnt = (y1 - y0) * bw;
  float a[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = 0.f;
  if (cc < c8)
    for (int i = pl; i < cnt; i += 32) {
      const int iy = y0 + i / bw, ix = x0 + i % bw;
      float v[8];
      ld_split(x + (((long)n * H + iy) * W + ix) * x_ld + cc * 8, x_lo, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += v[e];
    }
#pragma unroll
  for (int e = 0; e < 8; ++e) sred[pl][cl][e] = a[e];
  __syncthreads();
  if (pl == 0 && cc < c8) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float s_ = 0.f;
      for (int q = 0; q < 32; ++q) s_ += sred[q][cl][e];
      o[e] = s_ / cnt;
    }
    st_split(y + (((long)n * OH + oy) * OW + ox) * y_ld + cc * 8, y_lo, o);
  }
}
extern "C" int csbsr_adaptive_avgpool_fwd_split(const void* x, int64_t x_ld, int64_t x_lo, void* y, int64_t y_ld, int64_t y_lo, int32_t N,
                                                int32_t H, int32_t W, int32_t c, int32_t OH, int32_t OW, csbsr_stream_t s) {
  CSBSR_CHECK(x && y && c % 8 == 0, "aap_fwd: bad args");
  if ((long)(H / OH) * (W / OW) >= 64) {
    const int groups = (c / 8 + 7) / 8;
    hipLaunchKernelGGL(aap_fwd_block_kernel, dim3(N * OH * OW * groups), dim3(256), 0, ST(s), (const half_t*)x, x_ld, (half_t*)y, N, H, W,
                       c / 8, OH, OW, x_lo, y_ld, y_lo);
  } else {
    hipLaunchKernelGGL(aap_fwd_kernel, dim3(grid_for((long)N * OH * OW * (c / 8))), dim3(256), 0, ST(s), (const half_t*)x, x_ld, (half_t*)y,
                       N, H, W, c / 8, OH, OW, x_lo, y_ld, y_lo);
  }
  CSBSR_LAUNCH_CHECK("csbsr_adaptive_avgpool_fwd");
  return 0;
}
extern "C" int csbsr_adaptive_avgpool_fwd(const void* x, int64_t x_ld, void* y, int32_t N, int32_t H, int32_t W, int32_t c,
                                          int32_t OH, int32_t OW, csbsr_stream_t s) {
  return csbsr_adaptive_avgpool_fwd_split(x, x_ld, 0, y, c, 0, N, H, W, c, OH, OW, s);
}
extern "C" int csbsr_adaptive_avgpool_bwd(const void* dy, void* dx, int64_t dx_ld, int32_t accumulate, int32_t N, int32_t H,
                                          int32_t W, int32_t c, int32_t OH, int32_t OW, csbsr_stream_t s) {
  CSBSR_CHECK(dy && dx && c % 8 == 0, "aap_bwd: bad args");
  hipLaunchKernelGGL(aap_bwd_kernel, dim3(grid_for((long)N * H * W * (c / 8))), dim3(256), 0, ST(s), (const half_t*)dy, (half_t*)dx,
                     dx_ld, accumulate, N, H, W, c / 8, OH, OW);
  CSBSR_LAUNCH_CHECK("csbsr_adaptive_avgpool_bwd");
  return 0;
}

// ------------------------------------------------------------------------------------------- bilinear resize
__device__ __forceinline__ void bil_src(int o, int in, int out, int align, int& i0, int& i1, float& w1) {
  float src;
  if (align) src = out > 1 ? o * (float)(in - 1) / (float)(out - 1) : 0.f;
  else { src = (o + 0.5f) * ((float)in / (float)out) - 0.5f; if (src < 0.f) src = 0.f; }
  i0 = (int)src; if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + 1 < in ? i0 + 1 : in - 1;
  w1 = src - i0;
}
// grid = (chunks of one output row's (pixel, channel octet) pairs, N * OH): the row index and its source rows are workgroup-uniform and
// the in-row index needs one 32-bit division -- the flat version spent three 64-bit divisions per octet (3.8 ms for the 64-channel
// full-resolution map at B = 8, 1.1 TB/s).
__global__ void bilinear_fwd_kernel(const half_t* x, long x_ld, half_t* y, long y_ld, int N, int H, int W, int c8, int OH, int OW,
                                    int align, const float* drop, int cp, long x_lo, long y_lo) {
  for (unsigned row = blockIdx.y; row < (unsigned)N * (unsigned)OH; row += gridDim.y) {
  const int n = (int)(row / (unsigned)OH), oy = (int)(row - (unsigned)n * (unsigned)OH);
  int y0, y1; float wy;
  bil_src(oy, H, OH, align, y0, y1, wy);
  const half_t* b0 = x + ((long)n * H + y0) * W * x_ld;
  const half_t* b1 = x + ((long)n * H + y1) * W * x_ld;
  half_t* yr = y + ((long)n * OH + oy) * OW * y_ld;
  const unsigned per_row = (unsigned)OW * (unsigned)c8;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < per_row; i += gridDim.x * blockDim.x) {
    const int ox = (int)(i / (unsigned)c8), cc = (int)(i - (unsigned)ox * (unsigned)c8);
    int x0, x1; float wx;
    bil_src(ox, W, OW, align, x0, x1, wx);
    float v00[8], v01[8], v10[8], v11[8], o[8], dr[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    if (drop) ld8f(drop + n * cp + cc * 8, dr);
    ld_split(b0 + (long)x0 * x_ld + cc * 8, x_lo, v00);
    ld_split(b0 + (long)x1 * x_ld + cc * 8, x_lo, v01);
    ld_split(b1 + (long)x0 * x_ld + cc * 8, x_lo, v10);
    ld_split(b1 + (long)x1 * x_ld + cc * 8, x_lo, v11);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = (1.f - wy) * ((1.f - wx) * v00[e] + wx * v01[e]) + wy * ((1.f - wx) * v10[e] + wx * v11[e]);
      if (drop) v *= dr[e];
      o[e] = v;
    }
    st_split(yr + (long)ox * y_ld + cc * 8, y_lo, o);
  }
  }
}
// (round 5) the same arithmetic with the loops swapped: a thread OWNS one (output column, channel octet) and walks a strip of BIL_RS output
// rows, so the column's source positions, weight and addresses -- one 32-bit division and one float division per octet in the kernel above,
// ~250 VALU instructions per octet next to ~100 of conversions and lerps: the pass was VALU-bound at 1.65 ms per 3.3 GB of output whatever the
// input size (2.0 TB/s written; torch's fill writes 6.9 on the same buffer) -- are computed once per thread; the strip's row sources come from LDS.
#define BIL_RS 16
__global__ __launch_bounds__(256) void bilinear_fwd_cols_kernel(const half_t* x, long x_ld, half_t* y, long y_ld, int N, int H, int W, int c8, int OH,
                                                                 int OW, int align, const float* drop, int cp, long x_lo, long y_lo) {
  __shared__ int sy0[BIL_RS], sy1[BIL_RS];
  __shared__ float swy[BIL_RS];
  const unsigned strips = (unsigned)(OH + BIL_RS - 1) / BIL_RS;
  const int n = (int)(blockIdx.y / strips), r0 = (int)(blockIdx.y % strips) * BIL_RS;
  if (threadIdx.x < BIL_RS) {
    int a0 = 0, a1 = 0; float wq = 0.f;
    if (r0 + (int)threadIdx.x < OH) bil_src(r0 + (int)threadIdx.x, H, OH, align, a0, a1, wq);
    sy0[threadIdx.x] = a0; sy1[threadIdx.x] = a1; swy[threadIdx.x] = wq;
  }
  __syncthreads();
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)OW * (unsigned)c8) return;
  const int ox = (int)(i / (unsigned)c8), cc = (int)(i - (unsigned)ox * (unsigned)c8);
  int x0, x1; float wx;
  bil_src(ox, W, OW, align, x0, x1, wx);
  float dr[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
  if (drop) ld8f(drop + n * cp + cc * 8, dr);
  const half_t* c0 = x + (long)n * H * W * x_ld + (long)x0 * x_ld + cc * 8;
  const half_t* c1 = x + (long)n * H * W * x_ld + (long)x1 * x_ld + cc * 8;
  half_t* yc = y + ((long)n * OH * OW + ox) * y_ld + cc * 8;
  const long rs_in = (long)W * x_ld, rs_out = (long)OW * y_ld;
  const int rows = OH - r0 < BIL_RS ? OH - r0 : BIL_RS;
#pragma unroll 4
  for (int r = 0; r < rows; ++r) {
    const long o0 = sy0[r] * rs_in, o1 = sy1[r] * rs_in;
    const float wy = swy[r];
    float v00[8], v01[8], v10[8], v11[8], o[8];
    ld_split(c0 + o0, x_lo, v00);
    ld_split(c1 + o0, x_lo, v01);
    ld_split(c0 + o1, x_lo, v10);
    ld_split(c1 + o1, x_lo, v11);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = (1.f - wy) * ((1.f - wx) * v00[e] + wx * v01[e]) + wy * ((1.f - wx) * v10[e] + wx * v11[e]);
      if (drop) v *= dr[e];
      o[e] = v;
    }
    st_split(yc + (long)(r0 + r) * rs_out, y_lo, o);
  }
}
// gather-form adjoint: each input pixel sums the output pixels that reference it (scan of a bounded output window)
__global__ void bilinear_bwd_kernel(const half_t* dy, long dy_ld, half_t* dx, long dx_ld, int accumulate, int N, int H, int W, int c8,
                                    int OH, int OW, int align, const float* drop, int cp) {
  const long total = (long)N * H * W * c8;
  // output-per-input ratio of the source mapping (align_corners: (out-1)/(in-1))
  const float ry = (align && H > 1) ? (float)(OH - 1) / (H - 1) : (float)OH / H, rx = (align && W > 1) ? (float)(OW - 1) / (W - 1) : (float)OW / W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % c8); long t = i / c8;
    const int ix = (int)(t % W); t /= W;
    const int iy = (int)(t % H); const int n = (int)(t / H);
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
    int oy_lo = (int)floorf((iy - 1.5f) * ry) - 2, oy_hi = (int)ceilf((iy + 1.5f) * ry) + 2;
    int ox_lo = (int)floorf((ix - 1.5f) * rx) - 2, ox_hi = (int)ceilf((ix + 1.5f) * rx) + 2;
    if (iy == 0) oy_lo = 0;
    if (ix == 0) ox_lo = 0;
    if (iy == H - 1) oy_hi = OH - 1;
    if (ix == W - 1) ox_hi = OW - 1;
    oy_lo = oy_lo < 0 ? 0 : oy_lo; ox_lo = ox_lo < 0 ? 0 : ox_lo;
    oy_hi = oy_hi > OH - 1 ? OH - 1 : oy_hi; ox_hi = ox_hi > OW - 1 ? OW - 1 : ox_hi;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      int y0, y1; float wy; bil_src(oy, H, OH, align, y0, y1, wy);
      float cy = 0.f;
      if (y0 == iy) cy += 1.f - wy;
      if (y1 == iy) cy += wy;
      if (cy == 0.f) continue;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        int x0, x1; float wx; bil_src(ox, W, OW, align, x0, x1, wx);
        float cx = 0.f;
        if (x0 == ix) cx += 1.f - wx;
        if (x1 == ix) cx += wx;
        if (cx == 0.f) continue;
        const h8 g = *reinterpret_cast<const h8*>(dy + (((long)n * OH + oy) * OW + ox) * dy_ld + cc * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += cy * cx * (float)g[e];
      }
    }
    if (drop) {
      float dr[8];
      ld8f(drop + n * cp + cc * 8, dr);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] *= dr[e];
    }
    half_t* q = dx + (((long)n * H + iy) * W + ix) * dx_ld + cc * 8;
    if (accumulate) { const h8 old = *reinterpret_cast<const h8*>(q);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += (float)old[e]; }
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)a[e];
    *reinterpret_cast<h8*>(q) = o;
  }
}
extern "C" int csbsr_bilinear_fwd_split(const void* x, int64_t x_ld, int64_t x_lo, void* y, int64_t y_ld, int64_t y_lo, int32_t N, int32_t H,
                                        int32_t W, int32_t c, int32_t OH, int32_t OW, int32_t align_corners, const float* drop,
                                        csbsr_stream_t s) {
  CSBSR_CHECK(x && y && c % 8 == 0, "bilinear_fwd: bad args");
  CSBSR_CHECK((long)N * OH < (1l << 31) && (long)OW * (c / 8) < (1l << 31), "bilinear_fwd: size");
  const long per_row = (long)OW * (c / 8), rows = (long)N * OH;
  static int cols = -1;
  if (cols < 0) { const char* e = getenv("CSBSR_BIL_COLS"); cols = e ? atoi(e) : 1; }      // (A/B hook: 0 = the row-major kernel)
  const long strips = (long)N * ((OH + BIL_RS - 1) / BIL_RS);
  if (cols && OH >= BIL_RS && strips <= 65535 && (per_row + 255) / 256 * strips >= 64) {
    hipLaunchKernelGGL(bilinear_fwd_cols_kernel, dim3((unsigned)((per_row + 255) / 256), (unsigned)strips), dim3(256), 0, ST(s), (const half_t*)x, x_ld,
                       (half_t*)y, y_ld, N, H, W, c / 8, OH, OW, align_corners, drop, c, x_lo, y_lo);
    CSBSR_LAUNCH_CHECK("csbsr_bilinear_fwd");
    return 0;
  }
  const int bx = (int)((per_row + 255) / 256 > 64 ? 64 : (per_row + 255) / 256);
  hipLaunchKernelGGL(bilinear_fwd_kernel, dim3(bx, (unsigned)(rows > 65535 ? 65535 : rows)), dim3(256), 0, ST(s), (const half_t*)x, x_ld,
                     (half_t*)y, y_ld, N, H, W, c / 8, OH, OW, align_corners, drop, c, x_lo, y_lo);
  CSBSR_LAUNCH_CHECK("csbsr_bilinear_fwd");
  return 0;
}
extern "C" int csbsr_bilinear_fwd(const void* x, int64_t x_ld, void* y, int64_t y_ld, int32_t N, int32_t H, int32_t W, int32_t c,
                                  int32_t OH, int32_t OW, int32_t align_corners, const float* drop, csbsr_stream_t s) {
  return csbsr_bilinear_fwd_split(x, x_ld, 0, y, y_ld, 0, N, H, W, c, OH, OW, align_corners, drop, s);
}
// large up-sampling ratios (PSP priors): the adjoint window of one input pixel spans thousands of outputs --
// one workgroup per (sample, input pixel, 64-channel group), 32 window lanes, LDS tree
__global__ __launch_bounds__(256) void bilinear_bwd_block_kernel(const half_t* dy, long dy_ld, half_t* dx, long dx_ld, int accumulate, int N,
                                                                 int H, int W, int c8, int OH, int OW, int align, const float* drop, int cp) {
  __shared__ float sred[32][8][8];
  const int groups = (c8 + 7) / 8;
  int b = blockIdx.x;
  const int g = b % groups; b /= groups;
  const int ix = b % W; b /= W;
  const int iy = b % H; const int n = b / H;
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int cc = g * 8 + cl;
  const float ry = (align && H > 1) ? (float)(OH - 1) / (H - 1) : (float)OH / H, rx = (align && W > 1) ? (float)(OW - 1) / (W - 1) : (float)OW / W;
  int oy_lo = (int)floorf((iy - 1.5f) * ry) - 2, oy_hi = (int)ceilf((iy + 1.5f) * ry) + 2;
  int ox_lo = (int)floorf((ix - 1.5f) * rx) - 2, ox_hi = (int)ceilf((ix + 1.5f) * rx) + 2;
  if (iy == 0) oy_lo = 0;
  if (ix == 0) ox_lo = 0;
  if (iy == H - 1) oy_hi = OH - 1;
  if (ix == W - 1) ox_hi = OW - 1;
  oy_lo = oy_lo < 0 ? 0 : oy_lo; ox_lo = ox_lo < 0 ? 0 : ox_lo;
  oy_hi = oy_hi > OH - 1 ? OH - 1 : oy_hi; ox_hi = ox_hi > OW - 1 ? OW - 1 : ox_hi;
  const int ww = ox_hi - ox_lo + 1, cnt = (oy_hi - oy_lo + 1) * ww;
  float a[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = 0.f;
  if (cc < c8)
    for (int i = pl; i < cnt; i += 32) {
      const int oy = oy_lo + i / ww, ox = ox_lo + i % ww;
      int y0, y1, x0, x1; float wy, wx;
      bil_src(oy, H, OH, align, y0, y1, wy); bil_src(ox, W, OW, align, x0, x1, wx);
      float cy = 0.f, cx = 0.f;
      if (y0 == iy) cy += 1.f - wy;
      if (y1 == iy) cy += wy;
      if (x0 == ix) cx += 1.f - wx;
      if (x1 == ix) cx += wx;
      const float w_ = cy * cx;
      if (w_ == 0.f) continue;
      const h8 gv = *reinterpret_cast<const h8*>(dy + (((long)n * OH + oy) * OW + ox) * dy_ld + cc * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += w_ * (float)gv[e];
    }
#pragma unroll
  for (int e = 0; e < 8; ++e) sred[pl][cl][e] = a[e];
  __syncthreads();
  if (pl == 0 && cc < c8) {
    half_t* q = dx + (((long)n * H + iy) * W + ix) * dx_ld + cc * 8;
    h8 old = {0, 0, 0, 0, 0, 0, 0, 0};
    if (accumulate) old = *reinterpret_cast<const h8*>(q);
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float s_ = 0.f;
      for (int k = 0; k < 32; ++k) s_ += sred[k][cl][e];
      if (drop) s_ *= drop[n * cp + cc * 8 + e];      // (one thread per pixel and octet here: not a stream)
      o[e] = (half_t)(s_ + (float)old[e]);
    }
    *reinterpret_cast<h8*>(q) = o;
  }
}
// (round 5) small ratios with the adjoint's window TABULATED: per input coordinate i the outputs o that reference it are a short run
// [lo, lo + cnt) with weights w[k] (the scan of the kernel above, done once per axis by bil_tab_kernel -- on the device, with bil_src's own
// float arithmetic, so the tables are the forward's index map exactly), and a thread owns one (input column, channel octet) and walks a
// strip of input rows: no bil_src, no division, no window scan per octet (the scan was ~1000 VALU instructions per octet: 2.07 ms for the
// decoder's 256-channel x2 gradient at B = 8).  Same sums in the same order (rows outer, columns inner, (cy cx) g), so the results are the
// old kernel's bit for bit except where it skipped an exactly-zero weight in the middle of a run (now adds +0).
#define BIL_KMAX 6
struct BilTab { int lo, cnt; float w[BIL_KMAX]; };
__global__ void bil_tab_kernel(BilTab* tab, int in, int out, int align) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= in) return;
  const float r = (align && in > 1) ? (float)(out - 1) / (in - 1) : (float)out / in;
  int lo = (int)floorf((i - 1.5f) * r) - 2, hi = (int)ceilf((i + 1.5f) * r) + 2;
  if (i == 0) lo = 0;
  if (i == in - 1) hi = out - 1;
  lo = lo < 0 ? 0 : lo; hi = hi > out - 1 ? out - 1 : hi;
  BilTab t; t.lo = 0; t.cnt = 0;
  for (int k = 0; k < BIL_KMAX; ++k) t.w[k] = 0.f;
  int first = -1, last = -2;
  for (int o = lo; o <= hi; ++o) {
    int i0, i1; float w1; bil_src(o, in, out, align, i0, i1, w1);
    float c = 0.f;
    if (i0 == i) c += 1.f - w1;
    if (i1 == i) c += w1;
    if (c != 0.f) { if (first < 0) first = o; last = o; }
  }
  if (first >= 0) {
    t.lo = first; t.cnt = last - first + 1;
    for (int o = first; o <= last && o - first < BIL_KMAX; ++o) {
      int i0, i1; float w1; bil_src(o, in, out, align, i0, i1, w1);
      float c = 0.f;
      if (i0 == i) c += 1.f - w1;
      if (i1 == i) c += w1;
      t.w[o - first] = c;
    }
  }
  tab[i] = t;          // (cnt > BIL_KMAX cannot happen for the ratios this path takes: out / in < 2.5)
}
#define BILB_RS 8
__global__ __launch_bounds__(256) void bilinear_bwd_cols_kernel(const half_t* dy, long dy_ld, half_t* dx, long dx_ld, int accumulate, int N, int H,
                                                                 int W, int c8, int OH, int OW, const float* drop, int cp, const BilTab* tabx,
                                                                 const BilTab* taby) {
  __shared__ BilTab sy[BILB_RS];
  const unsigned strips = (unsigned)(H + BILB_RS - 1) / BILB_RS;
  const int n = (int)(blockIdx.y / strips), r0 = (int)(blockIdx.y % strips) * BILB_RS;
  if (threadIdx.x < BILB_RS && r0 + (int)threadIdx.x < H) sy[threadIdx.x] = taby[r0 + threadIdx.x];
  __syncthreads();
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)W * (unsigned)c8) return;
  const int ix = (int)(i / (unsigned)c8), cc = (int)(i - (unsigned)ix * (unsigned)c8);
  const BilTab tx = tabx[ix];
  float dr[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
  if (drop) ld8f(drop + n * cp + cc * 8, dr);
  const half_t* g0 = dy + ((long)n * OH * OW + tx.lo) * dy_ld + cc * 8;
  half_t* q0 = dx + ((long)n * H * W + ix) * dx_ld + cc * 8;
  const int rows = H - r0 < BILB_RS ? H - r0 : BILB_RS;
  for (int r = 0; r < rows; ++r) {
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
    const BilTab ty = sy[r];
    for (int ky = 0; ky < ty.cnt; ++ky) {
      const float cy = ty.w[ky];
      if (cy == 0.f) continue;
      const half_t* gr = g0 + (long)(ty.lo + ky) * OW * dy_ld;
#pragma unroll
      for (int kx = 0; kx < BIL_KMAX; ++kx) {
        if (kx < tx.cnt && tx.w[kx] != 0.f) {
          const h8 g = *reinterpret_cast<const h8*>(gr + (long)kx * dy_ld);
          const float wv = cy * tx.w[kx];
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] += wv * (float)g[e];
        }
      }
    }
    if (drop) {
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] *= dr[e];
    }
    half_t* q = q0 + (long)(r0 + r) * W * dx_ld;
    if (accumulate) { const h8 old = *reinterpret_cast<const h8*>(q);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += (float)old[e]; }
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)a[e];
    *reinterpret_cast<h8*>(q) = o;
  }
}
extern "C" int csbsr_bilinear_bwd(const void* dy, int64_t dy_ld, void* dx, int64_t dx_ld, int32_t accumulate, int32_t N, int32_t H,
                                  int32_t W, int32_t c, int32_t OH, int32_t OW, int32_t align_corners, const float* drop,
                                  csbsr_stream_t s) {
  CSBSR_CHECK(dy && dx && c % 8 == 0, "bilinear_bwd: bad args");
  if ((long)(OH / H) * (OW / W) >= 64) {
    const int groups = (c / 8 + 7) / 8;
    hipLaunchKernelGGL(bilinear_bwd_block_kernel, dim3(N * H * W * groups), dim3(256), 0, ST(s), (const half_t*)dy, dy_ld, (half_t*)dx, dx_ld,
                       accumulate, N, H, W, c / 8, OH, OW, align_corners, drop, c);
  } else {
    static int cols = -1;
    if (cols < 0) { const char* e = getenv("CSBSR_BIL_COLS"); cols = e ? atoi(e) : 1; }      // (A/B hook: 0 = the scanning kernel)
    const long per_row = (long)W * (c / 8), strips = (long)N * ((H + BILB_RS - 1) / BILB_RS);
    BilTab* tab = (cols && OH >= H && OW >= W && 2 * OH <= 5 * H && 2 * OW <= 5 * W && strips <= 65535 && (per_row + 255) / 256 * strips >= 64)
                      ? reinterpret_cast<BilTab*>(csbsr_red_scratch(((long)W + H) * (long)(sizeof(BilTab) / 4))) : nullptr;
    if (tab) {
      hipLaunchKernelGGL(bil_tab_kernel, dim3((W + 255) / 256), dim3(256), 0, ST(s), tab, W, OW, align_corners);
      hipLaunchKernelGGL(bil_tab_kernel, dim3((H + 255) / 256), dim3(256), 0, ST(s), tab + W, H, OH, align_corners);
      hipLaunchKernelGGL(bilinear_bwd_cols_kernel, dim3((unsigned)((per_row + 255) / 256), (unsigned)strips), dim3(256), 0, ST(s), (const half_t*)dy, dy_ld,
                         (half_t*)dx, dx_ld, accumulate, N, H, W, c / 8, OH, OW, drop, c, tab, tab + W);
    } else {
      hipLaunchKernelGGL(bilinear_bwd_kernel, dim3(grid_for((long)N * H * W * (c / 8))), dim3(256), 0, ST(s), (const half_t*)dy, dy_ld,
                         (half_t*)dx, dx_ld, accumulate, N, H, W, c / 8, OH, OW, align_corners, drop, c);
    }
  }
  CSBSR_LAUNCH_CHECK("csbsr_bilinear_bwd");
  return 0;
}

// ------------------------------------------------------------------------------------------- constant-operand folding
// A zero-padded 3x3 convolution of a spatially constant map (kbpn.py:565-567: fe_kernel.0 applied to GAP(kernel).expand(HR))
// takes only 16 distinct values per (sample, channel): one per border class (first/last row) x (first/last column).
// class id = (y==0)*8 + (y==H-1)*4 + (x==0)*2 + (x==W-1).  fill: out[n,y,x,:] = V[n][class][:]
// (optional mask: out *= mask > 0 ? 1 : mslope -- the activation derivative of the layer whose saved output `mask` is, for the dgrad form)
__global__ void border_class_fill_kernel(const float* V, half_t* out, long ld, int N, int H, int W, int c8, const half_t* mask, long mld, float mslope) {
  const long total = (long)N * H * W * c8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % c8); long t = i / c8;
    const int x = (int)(t % W); t /= W;
    const int y = (int)(t % H); const int n = (int)(t / H);
    const int cls = (y == 0) * 8 + (y == H - 1) * 4 + (x == 0) * 2 + (x == W - 1);
    const float* v = V + ((long)n * 16 + cls) * c8 * 8 + cc * 8;
    h8 o;
    if (mask) {
      const h8 m = *reinterpret_cast<const h8*>(mask + (((long)n * H + y) * W + x) * mld + cc * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (half_t)(v[e] * ((float)m[e] > 0.f ? 1.f : mslope));
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (half_t)v[e];
    }
    *reinterpret_cast<h8*>(out + (((long)n * H + y) * W + x) * ld + cc * 8) = o;
  }
}
// adjoint: sums[n][class][:] += sum over the pixels of that class of x[n,y,x,:] (both paths ACCUMULATE: the caller zeroes sums before the
// first call).  Degenerate / tiny maps: ONE workgroup per sample,
// a thread owns a channel octet and walks the pixels in raster order (fixed order, no atomics).
__global__ __launch_bounds__(256) void border_class_sums_small_kernel(const half_t* x, long ld, float* sums, int H, int W, int c8) {
  const int n = blockIdx.x;
  for (int cc = threadIdx.x; cc < c8; cc += 256) {
    float a[16][8];
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) a[k][e] = 0.f;
    for (int y = 0; y < H; ++y)
      for (int xx = 0; xx < W; ++xx) {
        const h8 v = *reinterpret_cast<const h8*>(x + (((long)n * H + y) * W + xx) * ld + cc * 8);
        const int cls = (y == 0) * 8 + (y == H - 1) * 4 + (xx == 0) * 2 + (xx == W - 1);
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (k == cls) {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[k][e] += (float)v[e];
          }
      }
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) sums[((long)n * 16 + k) * c8 * 8 + cc * 8 + e] += a[k][e];
  }
}
extern "C" int csbsr_border_class_fill(const float* V, void* out, int64_t ld, int32_t N, int32_t H, int32_t W, int32_t c, csbsr_stream_t s) {
  CSBSR_CHECK(V && out && c % 8 == 0, "border_class_fill: bad args");
  hipLaunchKernelGGL(border_class_fill_kernel, dim3(grid_for((long)N * H * W * (c / 8))), dim3(256), 0, ST(s), V, (half_t*)out, (long)ld, N, H, W, c / 8,
                     (const half_t*)nullptr, 0l, 0.f);
  CSBSR_LAUNCH_CHECK("csbsr_border_class_fill");
  return 0;
}
extern "C" int csbsr_border_class_fill_masked(const float* V, void* out, int64_t ld, const void* mask, int64_t mask_ld, float mask_slope, int32_t N,
                                              int32_t H, int32_t W, int32_t c, csbsr_stream_t s) {
  CSBSR_CHECK(V && out && mask && c % 8 == 0, "border_class_fill_masked: bad args");
  hipLaunchKernelGGL(border_class_fill_kernel, dim3(grid_for((long)N * H * W * (c / 8))), dim3(256), 0, ST(s), V, (half_t*)out, (long)ld, N, H, W, c / 8,
                     (const half_t*)mask, (long)mask_ld, mask_slope);
  CSBSR_LAUNCH_CHECK("csbsr_border_class_fill_masked");
  return 0;
}
// fast path for real image sizes: (1) plain total over all pixels, (2) the O(perimeter) border pixels binned per class in LDS by one
// workgroup per (sample, edge), (3) interior = total - sum of the border classes.  No contended global atomics.
// T: also the per-channel sums of x * t over the pixels with t <= 0 (t = a second map of the same geometry) into part2 -- the PReLU-slope
// gradient of a layer whose saved output is t and whose dPre is x (csbsr_border_class_sums_prelu)
template <bool T>
__global__ __launch_bounds__(256) void bcs_total_kernel(const half_t* x, long ld, float* sums, long hw, int c8, int chunks, float* part,
                                                        const half_t* t = nullptr, long t_ld = 0, float* part2 = nullptr) {
  __shared__ float sred[256][T ? 16 : 8];
  const int n = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const int cpb = c8 < 256 ? c8 : 256, ppb = 256 / cpb;
  const int ch = threadIdx.x % cpb, pl = threadIdx.x / cpb;
  const long per = (hw + chunks - 1) / chunks;
  const long beg = chunk * per, end = beg + per < hw ? beg + per : hw;
  for (int cbase = 0; cbase < c8; cbase += cpb) {
    const int cc = cbase + ch;
    float a[8], b[T ? 8 : 1];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
#pragma unroll
    for (int e = 0; e < (T ? 8 : 1); ++e) b[e] = 0.f;
    if (cc < c8 && pl < ppb)
      for (long px = beg + pl; px < end; px += ppb) {
        const h8 v = *reinterpret_cast<const h8*>(x + ((long)n * hw + px) * ld + cc * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += (float)v[e];
        if constexpr (T) {
          const h8 tv = *reinterpret_cast<const h8*>(t + ((long)n * hw + px) * t_ld + cc * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) b[e] += (float)tv[e] > 0.f ? 0.f : (float)v[e] * (float)tv[e];
        }
      }
#pragma unroll
    for (int e = 0; e < 8; ++e) sred[threadIdx.x][e] = a[e];
    if constexpr (T) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sred[threadIdx.x][8 + e] = b[e];
    }
    __syncthreads();
    if (threadIdx.x < cpb && cbase + threadIdx.x < c8) {
#pragma unroll
      for (int e = 0; e < (T ? 16 : 8); ++e) {
        float s_ = 0.f;
        for (int q = 0; q < ppb; ++q) s_ += sred[q * cpb + threadIdx.x][e];
        if (e < 8) part[(long)blockIdx.x * c8 * 8 + (cbase + threadIdx.x) * 8 + e] = s_;      // row per (sample, chunk): folded by csbsr_sum_partials
        else part2[(long)blockIdx.x * c8 * 8 + (cbase + threadIdx.x) * 8 + (e - 8)] = s_;
      }
    }
    __syncthreads();
  }
}
// grid = N * 4 edges * groups of 32 channel chunks * SEG segments; block: 32 chunk lanes x 8 pixel lanes.  The 8 pixel lanes meet in
// LDS and are added in lane order; every block writes its (edge class, two corner classes) sums as one partial row
// part[((n * 4 + edge) * SEG + seg)][3][c], folded per class in segment order by bcs_edges_finish_kernel.
constexpr int BCS_SEG = 8;
__global__ __launch_bounds__(256) void bcs_edges_kernel(const half_t* x, long ld, float* part, int H, int W, int c8) {
  __shared__ float sbin[8][3][32][8];
  const int groups = (c8 + 31) / 32;
  int b = blockIdx.x;
  const int seg = b % BCS_SEG; b /= BCS_SEG;
  const int g = b % groups; b /= groups;
  const int edge = b % 4; const int n = b / 4;
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int cc = g * 32 + cl;
  // edges: 0 top row, 1 bottom row (full rows incl. corners), 2 left col, 3 right col (rows 1..H-2 only: corners belong to the rows)
  const int len = edge < 2 ? W : H - 2;
  float a[3][8];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) a[k][e] = 0.f;
  const int i0 = (int)((long)len * seg / BCS_SEG), i1 = (int)((long)len * (seg + 1) / BCS_SEG);
  if (cc < c8)
    for (int i = i0 + pl; i < i1; i += 8) {
      int y, xx;
      if (edge == 0) { y = 0; xx = i; } else if (edge == 1) { y = H - 1; xx = i; } else if (edge == 2) { y = i + 1; xx = 0; } else { y = i + 1; xx = W - 1; }
      const h8 v = *reinterpret_cast<const h8*>(x + (((long)n * H + y) * W + xx) * ld + cc * 8);
      const int k = (edge < 2) ? (xx == 0 ? 1 : (xx == W - 1 ? 2 : 0)) : 0;
#pragma unroll
      for (int kk = 0; kk < 3; ++kk)
        if (kk == k) {
#pragma unroll
          for (int e = 0; e < 8; ++e) a[kk][e] += (float)v[e];
        }
    }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) sbin[pl][k][cl][e] = a[k][e];
  __syncthreads();
  if (pl == 0 && cc < c8) {
    float* row = part + (((long)n * 4 + edge) * BCS_SEG + seg) * 3 * c8 * 8;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += sbin[q][k][cl][e];
        row[(long)k * c8 * 8 + cc * 8 + e] = t;
      }
  }
}
// border class of bin k (0 the edge proper, 1 its x == 0 corner, 2 its x == W - 1 corner) of edge 0 .. 3 (top, bottom, left, right): the one
// map both kernels below use
__device__ __forceinline__ int bcs_cls(int edge, int k) {
  const int base_cls = edge == 0 ? 8 : (edge == 1 ? 4 : (edge == 2 ? 2 : 1));
  return base_cls + (k == 1 ? 2 : (k == 2 ? 1 : 0));
}
// sums[n][cls][ch] += the edge / corner sums of the segments, in segment order (cls = border-class index of conv_epilogue_row).  The folded
// sum also goes back into the row of segment 0 (read by this thread alone), where bcs_fixup_kernel finds THIS call's border sums.
__global__ void bcs_edges_finish_kernel(float* part, float* sums, int N, int c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * 4 * 3 * c) return;
  const int ch = i % c; int r = i / c;
  const int k = r % 3; r /= 3;
  const int edge = r % 4; const int n = r / 4;
  if (edge >= 2 && k > 0) return;
  float t = 0.f;
  for (int seg = 0; seg < BCS_SEG; ++seg) t += part[((((long)n * 4 + edge) * BCS_SEG + seg) * 3 + k) * c + ch];
  sums[((long)n * 16 + bcs_cls(edge, k)) * c + ch] += t;
  part[(((long)n * 4 + edge) * BCS_SEG * 3 + k) * c + ch] = t;
}
// class 0 holds (what it held before +) the total: take this call's border sums off it, in ascending class order 1, 2, 4, 5, 6, 8, 9, 10
// (the host takes this path only for H, W >= 3, where no pixel falls into another class) -- not the content of sums[1 .. 15], which
// includes whatever the caller had accumulated there
__global__ void bcs_fixup_kernel(const float* part, float* sums, int N, int c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * c) return;
  const int n = i / c, ch = i % c;
  float border = 0.f;
  for (int cls = 1; cls <= 10; ++cls)
    for (int edge = 0; edge < 4; ++edge)
      for (int k = 0; k < (edge < 2 ? 3 : 1); ++k)
        if (bcs_cls(edge, k) == cls) border += part[(((long)n * 4 + edge) * BCS_SEG * 3 + k) * c + ch];
  sums[(long)n * 16 * c + ch] -= border;
}
// stages (2) and (3) of the fast path below: the border pixels binned per class, then interior = total - border (the totals are in class 0)
static void bcs_border_classes(const void* x, int64_t ld, float* sums, int32_t N, int32_t H, int32_t W, int32_t c, float* epart, csbsr_stream_t s) {
  hipLaunchKernelGGL(bcs_edges_kernel, dim3(N * 4 * ((c / 8 + 31) / 32) * BCS_SEG), dim3(256), 0, ST(s), (const half_t*)x, (long)ld, epart, H, W, c / 8);
  hipLaunchKernelGGL(bcs_edges_finish_kernel, dim3((N * 12 * c + 255) / 256), dim3(256), 0, ST(s), epart, sums, N, c);
  hipLaunchKernelGGL(bcs_fixup_kernel, dim3((N * c + 255) / 256), dim3(256), 0, ST(s), (const float*)epart, sums, N, c);
}
static int border_class_sums_impl(const void* x, int64_t ld, float* sums, int32_t N, int32_t H, int32_t W, int32_t c, const void* t, int64_t t_ld,
                                  float* negdot, csbsr_stream_t s) {
  CSBSR_CHECK(x && sums && c % 8 == 0, "border_class_sums: bad args");
  CSBSR_CHECK(!t || (negdot && H >= 3 && W >= 3 && (long)H * W >= 1024), "border_class_sums_prelu: maps of >= 1024 pixels, negdot required");
  if (H >= 3 && W >= 3 && (long)H * W >= 1024) {
    // (1) plain total over all pixels, (2) the O(perimeter) border pixels binned per class by one workgroup per (sample, edge, segment),
    // (3) interior = total - sum of the border classes.  Every stage is a fixed-order fold of partial rows.
    const long hw = (long)H * W;
    int chunks = (int)((hw + 511) / 512);     // >= 392 workgroups at LR 448^2: the 4096-pixel chunks left 4/5 of the CUs idle
    if (chunks > 2048) chunks = 2048;
    const long n_tot = (long)N * chunks * c, n_edge = (long)N * 4 * BCS_SEG * 3 * c;
    float* part = csbsr_red_scratch(n_tot + n_edge + (t ? n_tot : 0));
    CSBSR_NEED_SCRATCH(part, "border_class_sums");
    if (t) {
      float* part2 = part + n_tot + n_edge;
      hipLaunchKernelGGL(bcs_total_kernel<true>, dim3(N * chunks), dim3(256), 0, ST(s), (const half_t*)x, (long)ld, sums, hw, c / 8, chunks, part,
                         (const half_t*)t, (long)t_ld, part2);
      if (csbsr_sum_partials_batched(part2, chunks, c, c, negdot, N, (long)c, ST(s))) return 1;
    } else {
      hipLaunchKernelGGL(bcs_total_kernel<false>, dim3(N * chunks), dim3(256), 0, ST(s), (const half_t*)x, (long)ld, sums, hw, c / 8, chunks, part,
                         (const half_t*)nullptr, 0l, (float*)nullptr);
    }
    if (csbsr_sum_partials_batched(part, chunks, c, c, sums, N, 16l * c, ST(s))) return 1;
    bcs_border_classes(x, ld, sums, N, H, W, c, part + n_tot, s);
    CSBSR_LAUNCH_CHECK("csbsr_border_class_sums");
    return 0;
  }
  hipLaunchKernelGGL(border_class_sums_small_kernel, dim3(N), dim3(256), 0, ST(s), (const half_t*)x, (long)ld, sums, H, W, c / 8);
  CSBSR_LAUNCH_CHECK("csbsr_border_class_sums");
  return 0;
}
extern "C" int csbsr_border_class_sums(const void* x, int64_t ld, float* sums, int32_t N, int32_t H, int32_t W, int32_t c, csbsr_stream_t s) {
  return border_class_sums_impl(x, ld, sums, N, H, W, c, nullptr, 0, nullptr, s);
}

// csbsr_border_class_fill_masked and csbsr_border_class_sums OF THE MASK MAP in one pass: the fill streams the mask anyway, so its plain
// totals ride along -- bcs_total_kernel's walk (same chunks, same lane order, same partial rows: the sums are bit-identical to the
// stand-alone pass) with the fill's store for every pixel it visits.  The weight gradient of a 3x3 layer behind a global average pool
// (dPre spatially constant) needs exactly these sums of the layer's input (csbsr_amd/modeling/kp_bwd.py, fold_const_wgrad).
__global__ __launch_bounds__(256) void bcs_fill_total_kernel(const float* V, half_t* out, long ld, const half_t* mask, long mld, float mslope, int H, int W,
                                                             int c8, int chunks, float* part) {
  __shared__ float sred[256][8];
  const long hw = (long)H * W;
  const int n = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const int cpb = c8 < 256 ? c8 : 256, ppb = 256 / cpb;
  const int ch = threadIdx.x % cpb, pl = threadIdx.x / cpb;
  const long per = (hw + chunks - 1) / chunks;
  const long beg = chunk * per, end = beg + per < hw ? beg + per : hw;
  for (int cbase = 0; cbase < c8; cbase += cpb) {
    const int cc = cbase + ch;
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
    if (cc < c8 && pl < ppb)
      for (long px = beg + pl; px < end; px += ppb) {
        const h8 m = *reinterpret_cast<const h8*>(mask + ((long)n * hw + px) * mld + cc * 8);
        const int y = (int)(px / W), x = (int)(px - (long)y * W);
        const int cls = (y == 0) * 8 + (y == H - 1) * 4 + (x == 0) * 2 + (x == W - 1);
        const float* v = V + ((long)n * 16 + cls) * c8 * 8 + cc * 8;
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          a[e] += (float)m[e];
          o[e] = (half_t)(v[e] * ((float)m[e] > 0.f ? 1.f : mslope));
        }
        *reinterpret_cast<h8*>(out + ((long)n * hw + px) * ld + cc * 8) = o;
      }
#pragma unroll
    for (int e = 0; e < 8; ++e) sred[threadIdx.x][e] = a[e];
    __syncthreads();
    if (threadIdx.x < cpb && cbase + threadIdx.x < c8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float s_ = 0.f;
        for (int q = 0; q < ppb; ++q) s_ += sred[q * cpb + threadIdx.x][e];
        part[(long)blockIdx.x * c8 * 8 + (cbase + threadIdx.x) * 8 + e] = s_;      // row per (sample, chunk): folded by csbsr_sum_partials
      }
    }
    __syncthreads();
  }
}
extern "C" int csbsr_border_class_fill_masked_sums(const float* V, void* out, int64_t ld, const void* mask, int64_t mask_ld, float mask_slope, float* sums,
                                                   int32_t N, int32_t H, int32_t W, int32_t c, csbsr_stream_t s) {
  CSBSR_CHECK(V && out && mask && sums && c % 8 == 0, "border_class_fill_masked_sums: bad args");
  if (!(H >= 3 && W >= 3 && (long)H * W >= 1024)) {      // tiny maps: the two stand-alone launches
    if (int e = csbsr_border_class_fill_masked(V, out, ld, mask, mask_ld, mask_slope, N, H, W, c, s)) return e;
    return csbsr_border_class_sums(mask, mask_ld, sums, N, H, W, c, s);
  }
  const long hw = (long)H * W;
  int chunks = (int)((hw + 511) / 512);      // (the chunking of border_class_sums_impl)
  if (chunks > 2048) chunks = 2048;
  const long n_tot = (long)N * chunks * c, n_edge = (long)N * 4 * BCS_SEG * 3 * c;
  float* part = csbsr_red_scratch(n_tot + n_edge);
  CSBSR_NEED_SCRATCH(part, "border_class_fill_masked_sums");
  hipLaunchKernelGGL(bcs_fill_total_kernel, dim3(N * chunks), dim3(256), 0, ST(s), V, (half_t*)out, (long)ld, (const half_t*)mask, (long)mask_ld, mask_slope,
                     H, W, c / 8, chunks, part);
  if (csbsr_sum_partials_batched(part, chunks, c, c, sums, N, 16l * c, ST(s))) return 1;
  bcs_border_classes(mask, mask_ld, sums, N, H, W, c, part + n_tot, s);
  CSBSR_LAUNCH_CHECK("csbsr_border_class_fill_masked_sums");
  return 0;
}
extern "C" int csbsr_border_class_sums_prelu(const void* x, int64_t ld, const void* t, int64_t t_ld, float* sums, float* negdot, int32_t N, int32_t H,
                                             int32_t W, int32_t c, csbsr_stream_t s) {
  CSBSR_CHECK(t && negdot, "border_class_sums_prelu: null pointer");
  return border_class_sums_impl(x, ld, sums, N, H, W, c, t, t_ld, negdot, s);
}

// ---- two-ring classes (csbsr_ring_class_sums): class = ty * 5 + tx, t = 0, 1, 2, 3, 4 for coordinate 0, 1, interior, size-2, size-1.
// Lines: the four special rows (full width, binned by column type) and the four special columns restricted to the interior rows
// (one class each).  grid = N * 8 lines * channel groups * BCS_SEG segments; partial rows part[((n * 8 + line) * SEG + seg)][5][c].
__global__ __launch_bounds__(256) void rcs_lines_kernel(const half_t* x, long ld, float* part, int H, int W, int c8) {
  __shared__ float sbin[8][5][32][8];
  const int groups = (c8 + 31) / 32;
  int b = blockIdx.x;
  const int seg = b % BCS_SEG; b /= BCS_SEG;
  const int g = b % groups; b /= groups;
  const int line = b % 8; const int n = b / 8;
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int cc = g * 32 + cl;
  const bool is_row = line < 4;
  const int coord = (line & 3) < 2 ? (line & 3) : ((is_row ? H : W) - 4 + (line & 3));      // 0, 1, size-2, size-1
  const int lo = is_row ? 0 : 2, hi = is_row ? W : H - 2;                                    // columns: interior rows only
  float a[5][8];
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) a[k][e] = 0.f;
  const int len = hi - lo;
  const int i0 = lo + (int)((long)len * seg / BCS_SEG), i1 = lo + (int)((long)len * (seg + 1) / BCS_SEG);
  if (cc < c8)
    for (int i = i0 + pl; i < i1; i += 8) {
      const int y = is_row ? coord : i, xx = is_row ? i : coord;
      const h8 v = *reinterpret_cast<const h8*>(x + (((long)n * H + y) * W + xx) * ld + cc * 8);
      const int k = is_row ? (xx < 2 ? xx : (xx >= W - 2 ? xx - W + 5 : 2)) : 2;
#pragma unroll
      for (int kk = 0; kk < 5; ++kk)
        if (kk == k) {
#pragma unroll
          for (int e = 0; e < 8; ++e) a[kk][e] += (float)v[e];
        }
    }
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) sbin[pl][k][cl][e] = a[k][e];
  __syncthreads();
  if (pl == 0 && cc < c8) {
    float* row = part + (((long)n * 8 + line) * BCS_SEG + seg) * 5 * c8 * 8;
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += sbin[q][k][cl][e];
        row[(long)k * c8 * 8 + cc * 8 + e] = t;
      }
  }
}
// sums[n][ty*5+tx][ch] += ...: special rows from their lines, special columns (interior rows) from theirs, the interior class =
// total (already in class 12 from the fold of bcs_total_kernel's rows) minus the 24 others -- every sum in a fixed order
__global__ void rcs_finish_kernel(const float* part, float* sums, int N, int c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * c) return;
  const int n = i / c, ch = i % c;
  float* S = sums + (long)n * 25 * c + ch;
  float others = 0.f;
  for (int line = 0; line < 8; ++line) {
    const int t = (line & 3) < 2 ? (line & 3) : (line & 3) + 1;      // 0, 1, 3, 4
    for (int k = 0; k < 5; ++k) {
      if (line >= 4 && k != 2) continue;
      float v = 0.f;
      for (int seg = 0; seg < BCS_SEG; ++seg) v += part[((((long)n * 8 + line) * BCS_SEG + seg) * 5 + k) * c + ch];
      const int cls = line < 4 ? t * 5 + k : 2 * 5 + t;
      S[(long)cls * c] += v;
      others += v;
    }
  }
  S[12l * c] -= others;
}
extern "C" int csbsr_ring_class_sums(const void* x, int64_t ld, float* sums, int32_t N, int32_t H, int32_t W, int32_t c, csbsr_stream_t s) {
  CSBSR_CHECK(x && sums && c % 8 == 0 && H >= 5 && W >= 5, "ring_class_sums: bad args (H, W >= 5, c % 8 == 0)");
  const long hw = (long)H * W;
  int chunks = (int)((hw + 511) / 512);
  if (chunks > 2048) chunks = 2048;
  const long n_tot = (long)N * chunks * c, n_line = (long)N * 8 * BCS_SEG * 5 * c;
  float* part = csbsr_red_scratch(n_tot + n_line);
  CSBSR_NEED_SCRATCH(part, "ring_class_sums");
  hipLaunchKernelGGL(bcs_total_kernel<false>, dim3(N * chunks), dim3(256), 0, ST(s), (const half_t*)x, (long)ld, sums, hw, c / 8, chunks, part,
                     (const half_t*)nullptr, 0l, (float*)nullptr);
  if (csbsr_sum_partials_batched(part, chunks, c, c, sums + 12l * c, N, 25l * c, ST(s))) return 1;      // the total lands in the interior class
  float* lpart = part + n_tot;
  hipLaunchKernelGGL(rcs_lines_kernel, dim3(N * 8 * ((c / 8 + 31) / 32) * BCS_SEG), dim3(256), 0, ST(s), (const half_t*)x, (long)ld, lpart, H, W, c / 8);
  hipLaunchKernelGGL(rcs_finish_kernel, dim3((N * c + 255) / 256), dim3(256), 0, ST(s), (const float*)lpart, sums, N, c);
  CSBSR_LAUNCH_CHECK("csbsr_ring_class_sums");
  return 0;
}
