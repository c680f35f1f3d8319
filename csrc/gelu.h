// bias + GELU device math, shared by the elementwise kernels
// (elementwise.hip) and the FFN GEMM epilogues (gemm_nt.hip) so that both
// compile the same expressions.
#pragma once

#include "common.h"

// ---------------------------------------------------------------------
// bias + GELU, tanh form — the approximation google-research BERT (and
// hence the reference's bert_base package) actually computes:
//   y = 0.5 u (1 + tanh(0.7978845608 (u + 0.044715 u^3)))
// tanh via exp2: tanh(a) = 1 - 2/(exp2(2a*log2e)+1) — one fast exp2.
// ---------------------------------------------------------------------
#define GELU_C0 0.7978845608028654f
#define GELU_C1 0.044715f
__device__ __forceinline__ float fast_tanh_f(float a) {
  const float e = exp2f(a * 2.885390081777927f);  // exp(2a)
  return 1.f - 2.f / (e + 1.f);
}
__device__ __forceinline__ float gelu_f(float u) {
  return 0.5f * u * (1.f + fast_tanh_f(GELU_C0 * u * (1.f + GELU_C1 * u * u)));
}
__device__ __forceinline__ float dgelu_f(float u) {
  const float a = GELU_C0 * u * (1.f + GELU_C1 * u * u);
  const float t = fast_tanh_f(a);
  const float da = GELU_C0 * (1.f + 3.f * GELU_C1 * u * u);
  return 0.5f * (1.f + t) + 0.5f * u * (1.f - t * t) * da;
}

// 8 consecutive bias values as fp32, from the bias in its stored dtype
// (a bf16 parameter is read in place, no per-call cast kernel)
__device__ __forceinline__ void load_bias8(const float* bias, int col0,
                                           float* be) {
  const f32x4 lo = *reinterpret_cast<const f32x4*>(bias + col0);
  const f32x4 hi = *reinterpret_cast<const f32x4*>(bias + col0 + 4);
#pragma unroll
  for (int e = 0; e < 8; ++e) be[e] = e < 4 ? lo[e] : hi[e - 4];
}
__device__ __forceinline__ void load_bias8(const bf16* bias, int col0,
                                           float* be) {
  const s16x8 raw = *reinterpret_cast<const s16x8*>(bias + col0);
#pragma unroll
  for (int e = 0; e < 8; ++e)
    be[e] = to_f32(reinterpret_cast<const bf16*>(&raw)[e]);
}

// 4 consecutive bias values (a GEMM epilogue lane owns 4 columns)
__device__ __forceinline__ void load_bias4(const float* bias, long col0,
                                           float* be) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(bias + col0);
#pragma unroll
  for (int e = 0; e < 4; ++e) be[e] = v[e];
}
__device__ __forceinline__ void load_bias4(const bf16* bias, long col0,
                                           float* be) {
  const s16x4 raw = *reinterpret_cast<const s16x4*>(bias + col0);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    be[e] = to_f32(reinterpret_cast<const bf16*>(&raw)[e]);
}
