// Multi-tensor kernels: ONE launch over a list of tensors.  The host (csbsr_amd/multi_tensor.py) uploads a table with one row per tensor
// and a chunk map: workgroup b handles chunk block_chunk[b] (CSBSR_MT_CHUNK elements) of tensor block_tensor[b].  The two optimiser steps
// and the replica fingerprint; entry points in include/csbsr_hip.h.
#include "common.h"

#define CSBSR_MT_CHUNK 8192
// (tensor length, chunk index) -> first element ``base`` and element count of the chunk (0 for a chunk past the end)
__device__ __forceinline__ int mt_chunk(long n, int chunk, long& base) {
  base = (long)chunk * CSBSR_MT_CHUNK;
  const long rem = n - base;
  return rem < CSBSR_MT_CHUNK ? (rem > 0 ? (int)rem : 0) : CSBSR_MT_CHUNK;
}

// ---- multi-tensor Adam (csbsr_hip.h): one workgroup per chunk of one tensor, 16-byte accesses (torch allocations are 256-byte
// aligned and the chunk size keeps every chunk start aligned), a scalar tail.  The arithmetic follows torch's own kernels operation by
// operation (lerp as m + w (g - m), addcmul, sqrt / bias-correction + eps, addcdiv) so that the two optimisers agree to fp32 rounding.
__global__ __launch_bounds__(256) void adam_step_kernel(const csbsr_adam_tensor_t* __restrict__ tt, const int* __restrict__ bt,
                                                        const int* __restrict__ bc, float w1, float beta2, float w2, float eps) {
  const csbsr_adam_tensor_t t = tt[bt[blockIdx.x]];
  long base;
  const int cnt = mt_chunk(t.n, bc[blockIdx.x], base);
  auto upd = [&](float& p, float g, float& m, float& v) {
    m = m + w1 * (g - m);
    v = v * beta2 + w2 * g * g;
    const float denom = sqrtf(v) / t.bc2_sqrt + eps;
    p = p - t.step_size * (m / denom);
  };
  const int nv = cnt >> 2;
  float4* p4 = reinterpret_cast<float4*>(t.p + base);
  const float4* g4 = reinterpret_cast<const float4*>(t.g + base);
  float4* m4 = reinterpret_cast<float4*>(t.m + base);
  float4* v4 = reinterpret_cast<float4*>(t.v + base);
  for (int i = threadIdx.x; i < nv; i += 256) {
    float4 p = p4[i], m = m4[i], v = v4[i];
    const float4 g = g4[i];
    upd(p.x, g.x, m.x, v.x); upd(p.y, g.y, m.y, v.y); upd(p.z, g.z, m.z, v.z); upd(p.w, g.w, m.w, v.w);
    p4[i] = p; m4[i] = m; v4[i] = v;
  }
  for (int i = 4 * nv + threadIdx.x; i < cnt; i += 256) {
    float p = t.p[base + i], m = t.m[base + i], v = t.v[base + i];
    upd(p, t.g[base + i], m, v);
    t.p[base + i] = p; t.m[base + i] = m; t.v[base + i] = v;
  }
}
extern "C" int csbsr_adam_step(const csbsr_adam_tensor_t* tensors, const int32_t* block_tensor, const int32_t* block_chunk, int32_t nblocks,
                               double beta1_d, double beta2_d, float eps, csbsr_stream_t s) {
  CSBSR_CHECK(tensors && block_tensor && block_chunk && nblocks >= 0, "adam_step: bad arguments");
  if (nblocks == 0) return 0;
  // (1 - beta in DOUBLE, then rounded: torch passes the Python float 1 - beta2 = 0.001, where 1.f - 0.999f is 0.99998713e-3)
  hipLaunchKernelGGL(adam_step_kernel, dim3(nblocks), dim3(256), 0, reinterpret_cast<hipStream_t>(s), tensors, block_tensor, block_chunk,
                     (float)(1.0 - (double)beta1_d), (float)beta2_d, (float)(1.0 - beta2_d), eps);
  CSBSR_LAUNCH_CHECK("csbsr_adam_step");
  return 0;
}
// ---- multi-tensor SGD (csbsr_hip.h): the chunk map and access pattern of the Adam kernel above; torch's foreach sequence per element
// (d = g + wd p; buf = momentum buf + d; p -= lr buf).  A tensor whose p / g / buf is not 16-byte aligned (``vec`` = 0: a view that starts
// inside an allocation) takes the scalar loop for the whole chunk.
template <bool MOMENTUM, bool DECAY>
__global__ __launch_bounds__(256) void sgd_step_kernel(const csbsr_sgd_tensor_t* __restrict__ tt, const int* __restrict__ bt,
                                                       const int* __restrict__ bc, float lr, float momentum, float wd) {
  const csbsr_sgd_tensor_t t = tt[bt[blockIdx.x]];
  long base;
  const int cnt = mt_chunk(t.n, bc[blockIdx.x], base);
  auto upd = [&](float& p, float g, float& b) {
    float d = g;
    if (DECAY) d = g + wd * p;
    if (MOMENTUM) { b = momentum * b + d; d = b; }
    p = p - lr * d;
  };
  const int nv = t.vec ? cnt >> 2 : 0;
  float4* p4 = reinterpret_cast<float4*>(t.p + base);
  const float4* g4 = reinterpret_cast<const float4*>(t.g + base);
  float4* b4 = reinterpret_cast<float4*>(t.buf + base);      // (never dereferenced without MOMENTUM: buf may be NULL then)
  for (int i = threadIdx.x; i < nv; i += 256) {
    float4 p = p4[i], b = {0.f, 0.f, 0.f, 0.f};
    const float4 g = g4[i];
    if (MOMENTUM) b = b4[i];
    upd(p.x, g.x, b.x); upd(p.y, g.y, b.y); upd(p.z, g.z, b.z); upd(p.w, g.w, b.w);
    p4[i] = p;
    if (MOMENTUM) b4[i] = b;
  }
  for (int i = 4 * nv + threadIdx.x; i < cnt; i += 256) {
    float p = t.p[base + i], b = 0.f;
    if (MOMENTUM) b = t.buf[base + i];
    upd(p, t.g[base + i], b);
    t.p[base + i] = p;
    if (MOMENTUM) t.buf[base + i] = b;
  }
}
extern "C" int csbsr_sgd_step(const csbsr_sgd_tensor_t* tensors, const int32_t* block_tensor, const int32_t* block_chunk, int32_t nblocks,
                              double lr, double momentum, double weight_decay, csbsr_stream_t s) {
  CSBSR_CHECK(tensors && block_tensor && block_chunk && nblocks >= 0, "sgd_step: bad arguments");
  CSBSR_CHECK(momentum >= 0.0 && weight_decay >= 0.0, "sgd_step: momentum and weight_decay must not be negative");
  if (nblocks == 0) return 0;
  const bool mom = momentum != 0.0, dec = weight_decay != 0.0;
  auto k = mom ? (dec ? sgd_step_kernel<true, true> : sgd_step_kernel<true, false>)
               : (dec ? sgd_step_kernel<false, true> : sgd_step_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(nblocks), dim3(256), 0, reinterpret_cast<hipStream_t>(s), tensors, block_tensor, block_chunk, (float)lr,
                     (float)momentum, (float)weight_decay);
  CSBSR_LAUNCH_CHECK("csbsr_sgd_step");
  return 0;
}
// ---- multi-tensor fingerprint (csbsr_hip.h): the chunk map of the two optimiser kernels above, read-only.  Per workgroup the two sums of
// its <= 8192 words (64-bit integers, wrapping), folded wave shuffle -> LDS -> ONE pair of 64-bit integer atomic adds per workgroup onto
// the tensor's zeroed row.  Addition modulo 2^64 is associative and commutative, so neither the chunk size, nor the block size, nor the
// order in which workgroups retire can change a bit of the result (unlike a floating-point atomic sum).  No floating point anywhere.
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}
__global__ __launch_bounds__(256) void fingerprint_kernel(const csbsr_fp_tensor_t* __restrict__ tt, const int* __restrict__ bt,
                                                          const int* __restrict__ bc, unsigned long long* __restrict__ out) {
  typedef unsigned long long u64;
  const int ti = bt[blockIdx.x];
  const csbsr_fp_tensor_t t = tt[ti];
  long base;
  const int cnt = mt_chunk(t.n, bc[blockIdx.x], base);
  u64 s0 = 0, s1 = 0;
  const int nv = t.vec ? cnt >> 2 : 0;
  const uint4* w4 = reinterpret_cast<const uint4*>(t.w + base);
  for (int i = threadIdx.x; i < nv; i += 256) {
    const uint4 w = w4[i];
    const u64 j1 = (u64)(base + 4 * i) + 1;          // (index of w.x) + 1
    s0 += (u64)w.x + (u64)w.y + (u64)w.z + (u64)w.w;
    s1 += (u64)w.x * j1 + (u64)w.y * (j1 + 1) + (u64)w.z * (j1 + 2) + (u64)w.w * (j1 + 3);
  }
  for (int i = 4 * nv + threadIdx.x; i < cnt; i += 256) {
    const u64 w = t.w[base + i];
    s0 += w;
    s1 += w * ((u64)(base + i) + 1);
  }
  s0 = wave_sum_u64(s0);
  s1 = wave_sum_u64(s1);
  __shared__ u64 part[4][2];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[wave][0] = s0; part[wave][1] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(out + 2 * (long)ti, part[0][0] + part[1][0] + part[2][0] + part[3][0]);
    atomicAdd(out + 2 * (long)ti + 1, part[0][1] + part[1][1] + part[2][1] + part[3][1]);
  }
}
extern "C" int csbsr_fingerprint(const csbsr_fp_tensor_t* tensors, const int32_t* block_tensor, const int32_t* block_chunk, int32_t nblocks,
                                 uint64_t* out, csbsr_stream_t s) {
  CSBSR_CHECK(tensors && block_tensor && block_chunk && out && nblocks >= 0, "fingerprint: bad arguments");
  if (nblocks == 0) return 0;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit atomics");
  hipLaunchKernelGGL(fingerprint_kernel, dim3(nblocks), dim3(256), 0, reinterpret_cast<hipStream_t>(s), tensors, block_tensor, block_chunk,
                     reinterpret_cast<unsigned long long*>(out));
  CSBSR_LAUNCH_CHECK("csbsr_fingerprint");
  return 0;
}
