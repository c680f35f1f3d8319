// Device helpers shared by the attention kernels (attention.hip: full-LDS,
// attention_tiled.hip: K/V-tiled online softmax). Fragment conventions are
// documented at the top of attention.hip.
#pragma once

#include "common.h"

using bfrag = mfma_bf16x8;
using cfrag = mfma_f32x4;

__device__ __forceinline__ bfrag lds_frag(const bf16* base, int i0, int ld,
                                          int k0) {
  const int l = threadIdx.x & (WAVE - 1);
  return *reinterpret_cast<const bfrag*>(base + (long)(i0 + (l & 15)) * ld +
                                         k0 + ((l >> 4) << 3));
}

// 16x16x32 operand read TRANSPOSED from a row-major [K][N] LDS image with
// two ds_read_b64_tr_b16: element j of lane (g = l>>4, i = l&15) is
// base[k0 + 8g + j][column i of the group's 16 columns]. Lane 4q+p of a
// group addresses row q of a 4-row block, 4 contiguous columns starting at
// `col` -- the caller picks `col` per lane (n0 + 4p for 16 natural columns;
// any other 4-column chunk per p permutes the operand's row/column index).
// Needs EXEC all ones, 8-byte aligned addresses (ld % 4 == 0, col % 4 == 0)
// and every lane's address inside the padded tile.
__device__ __forceinline__ bfrag lds_frag_tr(const bf16* base, int k0, int ld,
                                             int col) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const int l = threadIdx.x & (WAVE - 1);
  const bf16* a = base + (long)(k0 + ((l >> 4) << 3) + ((l & 15) >> 2)) * ld +
                  col;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a);
  const s16x4 hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + 4 * ld));
  const s16x8 f = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bfrag, f);
}

__device__ __forceinline__ cfrag mfma16(bfrag a, bfrag b, cfrag c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// counter-based dropout RNG (same construction as elementwise.hip):
// splitmix64 hash of (seed, element) -> uniform [0,1)
__device__ __forceinline__ float attn_hash_uniform(unsigned long long ctr,
                                                   unsigned long long idx) {
  unsigned long long z = ctr * 0x9E3779B97F4A7C15ull ^ idx;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (float)(z >> 40) * (1.f / 16777216.f);
}

// stage a [rows x D] global tile (row stride rs) into LDS [rpad x ld]
// (ld > D pads the row stride so MFMA operand reads are bank-conflict
// free: ld*2B/4B/4 odd <=> ld % 16 == 8 for the strides used here)
__device__ __forceinline__ void stage_tile(const bf16* g, long rs, bf16* s,
                                           int rows, int rpad, int D,
                                           int ld) {
  const int nv = rpad * D / 8;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const int r = (i * 8) / D;
    const int c = (i * 8) % D;
    s16x8 val{};
    if (r < rows)
      val = *reinterpret_cast<const s16x8*>(g + (long)r * rs + c);
    *reinterpret_cast<s16x8*>(s + (long)r * ld + c) = val;
  }
}

// stage transposed: global [rows x D] (row stride rs) -> LDS [D x ld]
__device__ __forceinline__ void stage_tile_T(const bf16* g, long rs, bf16* s,
                                             int rows, int rpad, int D,
                                             int ld) {
  for (int i = threadIdx.x; i < rpad * D / 8; i += blockDim.x) {
    const int r = (i * 8) / D;
    const int c0 = (i * 8) % D;
    s16x8 val{};
    if (r < rows)
      val = *reinterpret_cast<const s16x8*>(g + (long)r * rs + c0);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      s[(long)(c0 + e) * ld + r] = reinterpret_cast<const bf16*>(&val)[e];
  }
}
