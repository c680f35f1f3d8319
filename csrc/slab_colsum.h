// Fixed-order column sum of an fp32 partial slab: the finisher shared by
// the LN backward, bias_gelu backward (elementwise.hip) and the attention
// backward's QKV bias gradient (attention.hip).
#pragma once

#include "common.h"

// Column sums of an fp32 partial slab [R][C] in a fixed order (rows
// strided over 8 slices per column, then the slices in order): columns
// [0, CA) go to outA, the rest to outB, each in its own dtype. Finishes
// the LN backward and bias_gelu backward reductions.
#define SCS_COLS 32
#define SCS_SLICES 8
template <typename TA, typename TB>
__global__ __launch_bounds__(SCS_COLS * SCS_SLICES) void slab_colsum_kernel(
    const float* __restrict__ slab, int R, int C, TA* __restrict__ outA,
    int CA, TB* __restrict__ outB) {
  __shared__ float red[SCS_SLICES][SCS_COLS];
  const int tx = threadIdx.x % SCS_COLS;
  const int ty = threadIdx.x / SCS_COLS;
  const int col = blockIdx.x * SCS_COLS + tx;
  float acc = 0.f;
  if (col < C) {
#pragma unroll 8
    for (int r = ty; r < R; r += SCS_SLICES) acc += slab[(long)r * C + col];
  }
  red[ty][tx] = acc;
  __syncthreads();
  if (ty == 0 && col < C) {
    float a = red[0][tx];
#pragma unroll
    for (int v = 1; v < SCS_SLICES; ++v) a += red[v][tx];
    if (col < CA)
      from_f32(a, &outA[col]);
    else
      from_f32(a, &outB[col - CA]);
  }
}

template <typename TA, typename TB>
static void launch_slab_colsum(const at::Tensor& slab, void* outA, int CA,
                               void* outB, hipStream_t stream) {
  const int R = slab.size(0);
  const int C = slab.size(1);
  hipLaunchKernelGGL((slab_colsum_kernel<TA, TB>),
                     dim3((C + SCS_COLS - 1) / SCS_COLS),
                     dim3(SCS_COLS * SCS_SLICES), 0, stream,
                     slab.data_ptr<float>(), R, C, (TA*)outA, CA, (TB*)outB);
}
