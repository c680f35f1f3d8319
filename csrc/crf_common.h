// Pieces shared by the wave-per-sequence CRF kernels (crf_wide.hip,
// crf_posterior.hip): the supported range, the padded LDS image of the
// transition matrix, the per-lane register copies of its column / row and
// the broadcast read of a staged message vector.
#pragma once

#include "common.h"

#define NEG (-1e30f)

constexpr int CRFW_MAX_T = 64;
constexpr int CRFW_MAX_L = 512;

inline __host__ __device__ int round4(int x) { return (x + 3) & ~3; }

// Transition image in LDS: [W][W+1] floats, pad cells = NEG. tr[i][lane] is
// contiguous across lanes and tr[lane][jj] lands on bank (lane+jj)%32, so
// both reads are conflict-free inside a 32-lane group.
template <int W> struct CrfTransImage {
  static constexpr int TRS = W + 1;                    // padded row stride
  static constexpr int TR_FLOATS = (W * TRS + 3) & ~3; // multiple of 16 B
};

template <int W>
__device__ __forceinline__ void stage_trans(float* tr_s,
                                            const float* __restrict__ trans,
                                            int T) {
  constexpr int TRS = CrfTransImage<W>::TRS;
  for (int idx = threadIdx.x; idx < W * TRS; idx += blockDim.x) {
    const int i = idx / TRS, j = idx - i * TRS;
    tr_s[idx] = (i < T && j < T) ? trans[i * T + j] : NEG;
  }
}

// trc[i] = trans[i][jc]: this lane's column, for scans that run over the
// predecessors of tag jc
// (N <= W entries: a kernel that knows T <= N keeps only those)
template <int W, int N>
__device__ __forceinline__ void load_trans_col(const float* tr_s, int jc,
                                               float (&trc)[N]) {
  constexpr int TRS = CrfTransImage<W>::TRS;
#pragma unroll
  for (int i = 0; i < N; ++i) trc[i] = tr_s[i * TRS + jc];
}

// trr[q] = trans[jc][q]: this lane's row, for scans over the successors
template <int W, int N>
__device__ __forceinline__ void load_trans_row(const float* tr_s, int jc,
                                               float (&trr)[N]) {
  constexpr int TRS = CrfTransImage<W>::TRS;
#pragma unroll
  for (int q = 0; q < N; ++q) trr[q] = tr_s[jc * TRS + q];
}

// cells [4q, 4q+4) of a 16 B-aligned LDS vector; every lane passes the same
// address, so the read is one broadcast
__device__ __forceinline__ f32x4 lds_bcast4(const float* vec, int q) {
  return reinterpret_cast<const f32x4*>(vec)[q];
}

inline void check_wide_range(int L, int T) {
  TORCH_CHECK(T >= 1 && T <= CRFW_MAX_T && L >= 1 && L <= CRFW_MAX_L,
              "CRF: label_size ", T, " / seq_len ", L,
              " outside the supported range (1 <= label_size <= ", CRFW_MAX_T,
              ", 1 <= seq_len <= ", CRFW_MAX_L, ")");
}
