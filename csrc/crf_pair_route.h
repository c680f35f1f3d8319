// LDS carve and route of the CRF loss kernel (crf_pair.hip), shared by the
// kernel, its launcher and crf_fwd's dispatch in crf.hip.
#pragma once

#include "crf_common.h"

constexpr size_t CRFPAIR_LDS_BYTES = 160 * 1024;
constexpr int CRFPAIR_MAX_SEQS = 2;  // sequences per block: 2 waves each

// Offsets in floats, every region a multiple of 4 floats (16 B).
template <int W, int TC> struct CrfPairCarve {
  static constexpr int TRS = CrfTransImage<W>::TRS;
  static constexpr int TR_FLOATS = CrfTransImage<W>::TR_FLOATS;
  // per sequence: logZ (one double, padded to 16 B), cur [W], then Z [LP]
  // fp64, k_b [LP], tags [LP], alpha_hat [L][TC], beta_hat [L][TC]
  static constexpr int HEAD = 4 + W;
  static __host__ __device__ int seq_floats(int L) {
    return HEAD + 4 * round4(L) + 2 * L * TC;
  }
  static __host__ __device__ size_t bytes(int seqs, int L) {
    return sizeof(float) *
           ((size_t)TR_FLOATS + (size_t)seqs * seq_floats(L));
  }
};

// crf_fwd's range: crf_wide.hip's, and beyond seq_len 512 the shapes the
// former narrow kernels accepted (label_size <= 20) as far as they fit here.
constexpr int CRFPAIR_LONG_ROW_MAX_T = 20;

inline void check_pair_range(int L, int T) {
  if (L > CRFW_MAX_L && T >= 1 && T <= CRFPAIR_LONG_ROW_MAX_T) return;
  check_wide_range(L, T);
}

// Label sizes above this stay on crf_wide.hip: at 64 scanned tags the pair
// sums (one exp per (t, i, j), none shared with the scan's) cost more than
// the concurrent scans save, 745 us against 535 us at (64, 128, 64)
// (profiles/crf_pair_r16.md).
constexpr int CRFPAIR_MAX_T = 48;

// (W, TC) of a label size <= CRFPAIR_MAX_T: the scanned width is the least
// of 12, 24, 32 | 48 that holds T
#define CRFPAIR_DISPATCH(T, X) \
  do {                         \
    if ((T) <= 12)             \
      X(32, 12);               \
    else if ((T) <= 24)        \
      X(32, 24);               \
    else if ((T) <= 32)        \
      X(32, 32);               \
    else                       \
      X(64, 48);               \
  } while (0)

// The one place that routes crf_fwd: the pair kernel for label sizes up to
// CRFPAIR_MAX_T wherever one sequence's two tables fit LDS next to the
// transition image, crf_wide.hip everywhere else.
// Sequences per block: one. Two (four waves) halve the blocks and share the
// image, but at the flagship batch the grid is far smaller than the device,
// and a block's combine runs over its sequences one after the other;
// profiles/crf_pair_r16.md has the comparison.
struct CrfFwdRoute {
  bool pair = false;
  int seqs = 0;
  size_t smem = 0;
  CrfFwdRoute(int L, int T) {
    if (T > CRFPAIR_MAX_T) return;
#define CRFPAIR_FITS(W, TC)                                 \
  do {                                                      \
    const size_t need = CrfPairCarve<W, TC>::bytes(1, L);   \
    if (need <= CRFPAIR_LDS_BYTES) {                        \
      pair = true;                                          \
      seqs = 1;                                             \
      smem = need;                                          \
    }                                                       \
  } while (0)
    CRFPAIR_DISPATCH(T, CRFPAIR_FITS);
#undef CRFPAIR_FITS
  }
};
