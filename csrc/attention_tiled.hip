// Tiled (flash-style) fused attention fwd/bwd for 1 <= L <= 512 on gfx950:
// online softmax over 64-key K/V tiles, MFMA 16x16x32 bf16, same strided
// I/O, masking, lse and counter-hash dropout as the full-LDS kernels in
// attention.hip (fragment conventions documented there). Nothing of size
// L x L ever leaves the chip.
//
// forward   workgroup = (batch*head, 64-query block), 4 waves x 16 rows;
//           loops over key tiles below lens[b] with running (m, l, O).
//           The row max is updated on every tile (no rescale threshold,
//           so no data-dependent branch). Dropout multiplies the
//           un-normalised tile probabilities that feed P.V; l sums the
//           undropped ones; 1/(l*keep) is applied once at the end.
// backward  two sweeps, no atomics, fixed summation order:
//           dK/dV: workgroup = (batch*head, 64-key block), 4 waves x 16
//             keys, S^T and dP^T computed with the key on the MFMA row so
//             the accumulators are [key][query]; dK/dV stay in registers
//             over the query-tile loop.
//           dQ: workgroup = (batch*head, 64-query block), loops over the
//             key tiles below lens[b].
//           P is recomputed from lse; delta = rowsum(dO.O) per query tile.
//
// LDS (D=64): fwd 36 KiB, dQ and dK/dV 54.5 KiB each -> >= 2 workgroups
// per CU. All row strides satisfy ld % 16 == 8.
#include "attn_common.h"

#define TQ 64          // query rows per tile
#define TK 64          // keys per tile
#define TLS (TK + 8)   // LDS stride of [*][64]-wide tiles
#define TILED_LMAX 512

// order a wave-private LDS write before the same wave's fragment reads
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// delta[r] = dot(dO[r], O[r]) for the TQ rows of one query tile, 4 threads
// per row (blockDim.x == 256); lse tile alongside. Rows >= rows get 0.
template <int D>
__device__ __forceinline__ void stage_row_stats(const bf16* dout_t,
                                                const bf16* o_t, long rs,
                                                const float* lse_t, int rows,
                                                float* delta_s, float* lse_s) {
  const int r = threadIdx.x >> 2;
  const int part = threadIdx.x & 3;
  float acc = 0.f;
  if (r < rows) {
#pragma unroll
    for (int c = part * (D / 4); c < (part + 1) * (D / 4); c += 8) {
      const s16x8 vdo =
          *reinterpret_cast<const s16x8*>(dout_t + (long)r * rs + c);
      const s16x8 vo = *reinterpret_cast<const s16x8*>(o_t + (long)r * rs + c);
      const bf16* pd = reinterpret_cast<const bf16*>(&vdo);
      const bf16* po = reinterpret_cast<const bf16*>(&vo);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc += to_f32(pd[e]) * to_f32(po[e]);
    }
  }
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  if (part == 0) {
    delta_s[r] = acc;
    lse_s[r] = (r < rows) ? lse_t[r] : 0.f;
  }
}

// ---------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attn_tiled_fwd_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const int* __restrict__ lens,
    bf16* __restrict__ out, float* __restrict__ lse, int H, int L,
    float scale, long q_bs, long q_hs, long q_rs, long o_bs, long o_hs,
    long o_rs, float keep, const unsigned long long* __restrict__ seed) {
  constexpr int DS = D + 8;
  constexpr int NKK = D / 32;
  constexpr int NFD = D / 16;
  __shared__ __attribute__((aligned(16))) bf16 q_s[TQ * DS];
  __shared__ __attribute__((aligned(16))) bf16 k_s[TK * DS];
  __shared__ __attribute__((aligned(16))) bf16 vt_s[D * TLS];
  __shared__ __attribute__((aligned(16))) bf16 p_s[4 * 16 * TLS];

  const int bh = blockIdx.x;
  const int b = bh / H;
  const int h = bh - b * H;
  const int q0 = blockIdx.y * TQ;
  const long qb = (long)b * q_bs + (long)h * q_hs;
  const long ob = (long)b * o_bs + (long)h * o_hs;
  const int kend = min(lens[b], L);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int lr0 = (lane >> 4) << 2;   // first of this lane's 4 C rows
  const int lc = lane & 15;           // this lane's C column
  const unsigned long long sv = (keep < 1.f) ? *seed : 0ull;
  bf16* pw = p_s + wid * 16 * TLS;

  stage_tile(q + qb + (long)q0 * q_rs, q_rs, q_s, min(TQ, L - q0), TQ, D, DS);
  __syncthreads();
  bfrag aq[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) aq[kk] = lds_frag(q_s, wid * 16, DS, kk * 32);

  float m_run[4], l_run[4];
  cfrag oacc[NFD];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = -1e30f;
    l_run[r] = 0.f;
  }
#pragma unroll
  for (int nd = 0; nd < NFD; ++nd) oacc[nd] = cfrag{0.f, 0.f, 0.f, 0.f};

  // tiles wholly at or beyond lens[b] are skipped (workgroup-uniform), so
  // every processed tile holds at least one unmasked key per row
  for (int k0 = 0; k0 < kend; k0 += TK) {
    __syncthreads();
    const int krows = min(TK, L - k0);
    stage_tile(k + qb + (long)k0 * q_rs, q_rs, k_s, krows, TK, D, DS);
    stage_tile_T(v + qb + (long)k0 * q_rs, q_rs, vt_s, krows, TK, D, TLS);
    __syncthreads();

    cfrag acc[4];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      acc[nf] = cfrag{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk)
        acc[nf] = mfma16(aq[kk], lds_frag(k_s, nf * 16, DS, kk * 32), acc[nf]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = -1e30f;
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        const int col = k0 + nf * 16 + lc;
        const float s = (col < kend) ? acc[nf][r] * scale : -1e30f;
        acc[nf][r] = s;
        mx = fmaxf(mx, s);
      }
      mx = group16_reduce_max(mx);
      const float m_new = fmaxf(m_run[r], mx);
      const float alpha = __expf(m_run[r] - m_new);
      float sum = 0.f;
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        const int col = k0 + nf * 16 + lc;
        // masked keys are exactly 0, never exp(-1e30 - (-1e30))
        const float p = (col < kend) ? __expf(acc[nf][r] - m_new) : 0.f;
        acc[nf][r] = p;
        sum += p;
      }
      sum = group16_reduce_sum(sum);
      l_run[r] = l_run[r] * alpha + sum;
      m_run[r] = m_new;
#pragma unroll
      for (int nd = 0; nd < NFD; ++nd) oacc[nd][r] *= alpha;
    }
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = acc[nf][r];
        if (keep < 1.f) {
          const long idx = ((long)bh * L + (q0 + wid * 16 + lr0 + r)) * L +
                           k0 + nf * 16 + lc;
          p = attn_hash_uniform(sv, (unsigned long long)idx) < keep ? p : 0.f;
        }
        pw[(lr0 + r) * TLS + nf * 16 + lc] = __float2bfloat16(p);
      }
    }
    wave_lds_sync();
    // O += P V
#pragma unroll
    for (int kk = 0; kk < TK / 32; ++kk) {
      const bfrag ap = lds_frag(pw, 0, TLS, kk * 32);
#pragma unroll
      for (int nd = 0; nd < NFD; ++nd)
        oacc[nd] = mfma16(ap, lds_frag(vt_s, nd * 16, TLS, kk * 32), oacc[nd]);
    }
  }

  const float inv_keep = 1.f / keep;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = q0 + wid * 16 + lr0 + r;
    if (row < L) {
      const float inv = __frcp_rn(l_run[r]) * inv_keep;
#pragma unroll
      for (int nd = 0; nd < NFD; ++nd)
        out[ob + (long)row * o_rs + nd * 16 + lc] =
            __float2bfloat16(oacc[nd][r] * inv);
      if (lc == 0) lse[(long)bh * L + row] = m_run[r] + __logf(l_run[r]);
    }
  }
}

// ---------------------------------------------------------------------
// backward sweep 1: dK, dV of one 64-key block
// ---------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attn_tiled_bwd_dkdv_kernel(
    const bf16* __restrict__ dout, const bf16* __restrict__ q,
    const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ o, const float* __restrict__ lse,
    const int* __restrict__ lens, bf16* __restrict__ dk,
    bf16* __restrict__ dv, int H, int L, float scale, long q_bs, long q_hs,
    long q_rs, long o_bs, long o_hs, long o_rs, float keep,
    const unsigned long long* __restrict__ seed) {
  constexpr int DS = D + 8;
  constexpr int NKK = D / 32;
  constexpr int NFD = D / 16;
  __shared__ __attribute__((aligned(16))) bf16 q_s[TQ * DS];
  __shared__ __attribute__((aligned(16))) bf16 do_s[TQ * DS];
  __shared__ __attribute__((aligned(16))) bf16 qt_s[D * TLS];    // Q^T
  __shared__ __attribute__((aligned(16))) bf16 dot_s[D * TLS];   // dO^T
  __shared__ __attribute__((aligned(16))) bf16 p_s[4 * 16 * TLS];   // P'^T
  __shared__ __attribute__((aligned(16))) bf16 ds_s[4 * 16 * TLS];  // dS^T
  __shared__ float delta_s[TQ];
  __shared__ float lse_s[TQ];
  // K and V are only read once, into this wave's A fragments, before the
  // first P'^T / dS^T tile is written: they borrow those buffers
  static_assert(TK * DS <= 4 * 16 * TLS, "K/V tile must fit the P buffer");
  bf16* k_s = p_s;
  bf16* v_s = ds_s;

  const int bh = blockIdx.x;
  const int b = bh / H;
  const int h = bh - b * H;
  const int k0 = blockIdx.y * TK;
  const long qb = (long)b * q_bs + (long)h * q_hs;
  const long ob = (long)b * o_bs + (long)h * o_hs;
  const int kend = min(lens[b], L);
  const int krows = min(TK, L - k0);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int lr0 = (lane >> 4) << 2;
  const int lc = lane & 15;

  if (k0 >= kend) {
    // wholly masked key block: its dK/dV rows are exactly zero
    for (int i = threadIdx.x; i < krows * (D / 8); i += blockDim.x) {
      const int r = i / (D / 8);
      const int c = (i % (D / 8)) * 8;
      const long off = qb + (long)(k0 + r) * q_rs + c;
      *reinterpret_cast<s16x8*>(dk + off) = s16x8{};
      *reinterpret_cast<s16x8*>(dv + off) = s16x8{};
    }
    return;
  }

  const unsigned long long sv = (keep < 1.f) ? *seed : 0ull;
  const float inv_keep = 1.f / keep;
  bf16* pw = p_s + wid * 16 * TLS;
  bf16* dw = ds_s + wid * 16 * TLS;

  stage_tile(k + qb + (long)k0 * q_rs, q_rs, k_s, krows, TK, D, DS);
  stage_tile(v + qb + (long)k0 * q_rs, q_rs, v_s, krows, TK, D, DS);
  __syncthreads();
  bfrag ak[NKK], av[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) {
    ak[kk] = lds_frag(k_s, wid * 16, DS, kk * 32);
    av[kk] = lds_frag(v_s, wid * 16, DS, kk * 32);
  }
  cfrag dkacc[NFD], dvacc[NFD];
#pragma unroll
  for (int nd = 0; nd < NFD; ++nd) {
    dkacc[nd] = cfrag{0.f, 0.f, 0.f, 0.f};
    dvacc[nd] = cfrag{0.f, 0.f, 0.f, 0.f};
  }

  for (int q0 = 0; q0 < L; q0 += TQ) {
    const int qrows = min(TQ, L - q0);
    __syncthreads();
    stage_tile(q + qb + (long)q0 * q_rs, q_rs, q_s, qrows, TQ, D, DS);
    stage_tile(dout + ob + (long)q0 * o_rs, o_rs, do_s, qrows, TQ, D, DS);
    stage_tile_T(q + qb + (long)q0 * q_rs, q_rs, qt_s, qrows, TQ, D, TLS);
    stage_tile_T(dout + ob + (long)q0 * o_rs, o_rs, dot_s, qrows, TQ, D, TLS);
    stage_row_stats<D>(dout + ob + (long)q0 * o_rs, o + ob + (long)q0 * o_rs,
                       o_rs, lse + (long)bh * L + q0, qrows, delta_s, lse_s);
    __syncthreads();

    // S^T = K Q^T and dP^T = V dO^T: [this wave's 16 keys][64 queries]
    cfrag st[4], dpt[4];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      st[nf] = cfrag{0.f, 0.f, 0.f, 0.f};
      dpt[nf] = cfrag{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        st[nf] = mfma16(ak[kk], lds_frag(q_s, nf * 16, DS, kk * 32), st[nf]);
        dpt[nf] = mfma16(av[kk], lds_frag(do_s, nf * 16, DS, kk * 32),
                         dpt[nf]);
      }
    }
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      const int ql = nf * 16 + lc;
      const int query = q0 + ql;
      const float row_lse = lse_s[ql];
      const float row_delta = delta_s[ql];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + wid * 16 + lr0 + r;
        float p = 0.f;
        if (key < kend && query < L)
          p = __expf(st[nf][r] * scale - row_lse);
        float pd = p;
        float dpr = dpt[nf][r];
        if (keep < 1.f) {
          const long idx = ((long)bh * L + query) * L + key;
          const bool kept =
              attn_hash_uniform(sv, (unsigned long long)idx) < keep;
          pd = kept ? p * inv_keep : 0.f;
          dpr = kept ? dpr * inv_keep : 0.f;
        }
        const float dsv = p * (dpr - row_delta) * scale;
        pw[(lr0 + r) * TLS + ql] = __float2bfloat16(pd);
        dw[(lr0 + r) * TLS + ql] = __float2bfloat16(dsv);
      }
    }
    wave_lds_sync();
    // dV += P'^T dO ; dK += dS^T Q
#pragma unroll
    for (int kk = 0; kk < TQ / 32; ++kk) {
      const bfrag ap = lds_frag(pw, 0, TLS, kk * 32);
      const bfrag ad = lds_frag(dw, 0, TLS, kk * 32);
#pragma unroll
      for (int nd = 0; nd < NFD; ++nd) {
        dvacc[nd] =
            mfma16(ap, lds_frag(dot_s, nd * 16, TLS, kk * 32), dvacc[nd]);
        dkacc[nd] =
            mfma16(ad, lds_frag(qt_s, nd * 16, TLS, kk * 32), dkacc[nd]);
      }
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = k0 + wid * 16 + lr0 + r;
    if (key < L) {
#pragma unroll
      for (int nd = 0; nd < NFD; ++nd) {
        const long off = qb + (long)key * q_rs + nd * 16 + lc;
        dk[off] = __float2bfloat16(dkacc[nd][r]);
        dv[off] = __float2bfloat16(dvacc[nd][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------
// backward sweep 2: dQ of one 64-query block
// ---------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attn_tiled_bwd_dq_kernel(
    const bf16* __restrict__ dout, const bf16* __restrict__ q,
    const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ o, const float* __restrict__ lse,
    const int* __restrict__ lens, bf16* __restrict__ dq, int H, int L,
    float scale, long q_bs, long q_hs, long q_rs, long o_bs, long o_hs,
    long o_rs, float keep, const unsigned long long* __restrict__ seed) {
  constexpr int DS = D + 8;
  constexpr int NKK = D / 32;
  constexpr int NFD = D / 16;
  __shared__ __attribute__((aligned(16))) bf16 q_s[TQ * DS];
  __shared__ __attribute__((aligned(16))) bf16 do_s[TQ * DS];
  __shared__ __attribute__((aligned(16))) bf16 k_s[TK * DS];
  __shared__ __attribute__((aligned(16))) bf16 v_s[TK * DS];
  __shared__ __attribute__((aligned(16))) bf16 kt_s[D * TLS];      // K^T
  __shared__ __attribute__((aligned(16))) bf16 ds_s[4 * 16 * TLS];  // dS
  __shared__ float delta_s[TQ];
  __shared__ float lse_s[TQ];

  const int bh = blockIdx.x;
  const int b = bh / H;
  const int h = bh - b * H;
  const int q0 = blockIdx.y * TQ;
  const long qb = (long)b * q_bs + (long)h * q_hs;
  const long ob = (long)b * o_bs + (long)h * o_hs;
  const int kend = min(lens[b], L);
  const int qrows = min(TQ, L - q0);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int lr0 = (lane >> 4) << 2;
  const int lc = lane & 15;
  const unsigned long long sv = (keep < 1.f) ? *seed : 0ull;
  const float inv_keep = 1.f / keep;
  bf16* dw = ds_s + wid * 16 * TLS;

  stage_tile(q + qb + (long)q0 * q_rs, q_rs, q_s, qrows, TQ, D, DS);
  stage_tile(dout + ob + (long)q0 * o_rs, o_rs, do_s, qrows, TQ, D, DS);
  stage_row_stats<D>(dout + ob + (long)q0 * o_rs, o + ob + (long)q0 * o_rs,
                     o_rs, lse + (long)bh * L + q0, qrows, delta_s, lse_s);
  __syncthreads();
  bfrag aq[NKK], ado[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) {
    aq[kk] = lds_frag(q_s, wid * 16, DS, kk * 32);
    ado[kk] = lds_frag(do_s, wid * 16, DS, kk * 32);
  }
  float row_lse[4], row_delta[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    row_lse[r] = lse_s[wid * 16 + lr0 + r];
    row_delta[r] = delta_s[wid * 16 + lr0 + r];
  }
  cfrag dqacc[NFD];
#pragma unroll
  for (int nd = 0; nd < NFD; ++nd) dqacc[nd] = cfrag{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < kend; k0 += TK) {
    const int krows = min(TK, L - k0);
    __syncthreads();
    stage_tile(k + qb + (long)k0 * q_rs, q_rs, k_s, krows, TK, D, DS);
    stage_tile(v + qb + (long)k0 * q_rs, q_rs, v_s, krows, TK, D, DS);
    stage_tile_T(k + qb + (long)k0 * q_rs, q_rs, kt_s, krows, TK, D, TLS);
    __syncthreads();

    cfrag s[4], dp[4];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      s[nf] = cfrag{0.f, 0.f, 0.f, 0.f};
      dp[nf] = cfrag{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        s[nf] = mfma16(aq[kk], lds_frag(k_s, nf * 16, DS, kk * 32), s[nf]);
        dp[nf] = mfma16(ado[kk], lds_frag(v_s, nf * 16, DS, kk * 32), dp[nf]);
      }
    }
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      const int key = k0 + nf * 16 + lc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int query = q0 + wid * 16 + lr0 + r;
        float p = 0.f;
        if (key < kend && query < L)
          p = __expf(s[nf][r] * scale - row_lse[r]);
        float dpr = dp[nf][r];
        if (keep < 1.f) {
          const long idx = ((long)bh * L + query) * L + key;
          dpr = attn_hash_uniform(sv, (unsigned long long)idx) < keep
                    ? dpr * inv_keep
                    : 0.f;
        }
        const float dsv = p * (dpr - row_delta[r]) * scale;
        dw[(lr0 + r) * TLS + nf * 16 + lc] = __float2bfloat16(dsv);
      }
    }
    wave_lds_sync();
    // dQ += dS K
#pragma unroll
    for (int kk = 0; kk < TK / 32; ++kk) {
      const bfrag ad = lds_frag(dw, 0, TLS, kk * 32);
#pragma unroll
      for (int nd = 0; nd < NFD; ++nd)
        dqacc[nd] =
            mfma16(ad, lds_frag(kt_s, nd * 16, TLS, kk * 32), dqacc[nd]);
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = q0 + wid * 16 + lr0 + r;
    if (row < L) {
#pragma unroll
      for (int nd = 0; nd < NFD; ++nd)
        dq[qb + (long)row * q_rs + nd * 16 + lc] =
            __float2bfloat16(dqacc[nd][r]);
    }
  }
}

// ===================================================================== host
namespace {

struct TiledStrides {
  long q_bs, q_hs, q_rs, o_bs, o_hs, o_rs;
};

void tiled_check_shape(long B, long H, long L, long D) {
  TORCH_CHECK(D == 32 || D == 64, "attn_tiled: head dim must be 32 or 64 "
              "(pad in the wrapper), got ", D);
  TORCH_CHECK(L >= 1 && L <= TILED_LMAX, "attn_tiled: seq len must be in "
              "[1, 512], got ", L);
  TORCH_CHECK(B >= 1 && H >= 1, "attn_tiled: empty batch or heads");
}

void tiled_check_common(const at::Tensor& ref, const at::Tensor& lens, long B,
                        double keep, const c10::optional<at::Tensor>& seed) {
  TORCH_CHECK(lens.is_cuda() && lens.is_contiguous() &&
                  lens.scalar_type() == at::kInt && lens.dim() == 1 &&
                  lens.size(0) == B && lens.get_device() == ref.get_device(),
              "attn_tiled: lens must be a contiguous int32 [B] GPU tensor");
  TORCH_CHECK(keep > 0.0 && keep <= 1.0, "attn_tiled: keep must be in (0, 1]");
  if (keep < 1.0) {
    TORCH_CHECK(seed.has_value() && seed->is_cuda() && seed->numel() >= 1 &&
                    seed->element_size() == 8,
                "attn_tiled: keep < 1 needs a 64-bit device seed");
  }
}

void tiled_check_bf16(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), "attn_tiled: ", name,
              " must be a contiguous GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, "attn_tiled: ", name,
              " must be bf16");
}

const unsigned long long* seed_ptr(const c10::optional<at::Tensor>& seed) {
  return seed ? (const unsigned long long*)seed->data_ptr() : nullptr;
}

void launch_fwd(hipStream_t st, const bf16* q, const bf16* k, const bf16* v,
                const int* lens, bf16* out, float* lse, int B, int H, int L,
                int D, float scale, const TiledStrides& s, float keep,
                const unsigned long long* seed) {
  const dim3 grid(B * H, (L + TQ - 1) / TQ);
  if (D == 64)
    hipLaunchKernelGGL(attn_tiled_fwd_kernel<64>, grid, dim3(256), 0, st, q, k,
                       v, lens, out, lse, H, L, scale, s.q_bs, s.q_hs, s.q_rs,
                       s.o_bs, s.o_hs, s.o_rs, keep, seed);
  else
    hipLaunchKernelGGL(attn_tiled_fwd_kernel<32>, grid, dim3(256), 0, st, q, k,
                       v, lens, out, lse, H, L, scale, s.q_bs, s.q_hs, s.q_rs,
                       s.o_bs, s.o_hs, s.o_rs, keep, seed);
  HIP_CHECK_LAST();
}

void launch_bwd(hipStream_t st, const bf16* dout, const bf16* q, const bf16* k,
                const bf16* v, const bf16* o, const float* lse,
                const int* lens, bf16* dq, bf16* dk, bf16* dv, int B, int H,
                int L, int D, float scale, const TiledStrides& s, float keep,
                const unsigned long long* seed) {
  const dim3 kgrid(B * H, (L + TK - 1) / TK);
  const dim3 qgrid(B * H, (L + TQ - 1) / TQ);
  if (D == 64) {
    hipLaunchKernelGGL(attn_tiled_bwd_dkdv_kernel<64>, kgrid, dim3(256), 0, st,
                       dout, q, k, v, o, lse, lens, dk, dv, H, L, scale,
                       s.q_bs, s.q_hs, s.q_rs, s.o_bs, s.o_hs, s.o_rs, keep,
                       seed);
    HIP_CHECK_LAST();
    hipLaunchKernelGGL(attn_tiled_bwd_dq_kernel<64>, qgrid, dim3(256), 0, st,
                       dout, q, k, v, o, lse, lens, dq, H, L, scale, s.q_bs,
                       s.q_hs, s.q_rs, s.o_bs, s.o_hs, s.o_rs, keep, seed);
  } else {
    hipLaunchKernelGGL(attn_tiled_bwd_dkdv_kernel<32>, kgrid, dim3(256), 0, st,
                       dout, q, k, v, o, lse, lens, dk, dv, H, L, scale,
                       s.q_bs, s.q_hs, s.q_rs, s.o_bs, s.o_hs, s.o_rs, keep,
                       seed);
    HIP_CHECK_LAST();
    hipLaunchKernelGGL(attn_tiled_bwd_dq_kernel<32>, qgrid, dim3(256), 0, st,
                       dout, q, k, v, o, lse, lens, dq, H, L, scale, s.q_bs,
                       s.q_hs, s.q_rs, s.o_bs, s.o_hs, s.o_rs, keep, seed);
  }
  HIP_CHECK_LAST();
}

}  // namespace

// [B,H,L,D] layout API
std::vector<at::Tensor> attn_tiled_fwd(const at::Tensor& q,
                                       const at::Tensor& k,
                                       const at::Tensor& v,
                                       const at::Tensor& lens, double scale,
                                       double keep,
                                       c10::optional<at::Tensor> seed) {
  tiled_check_bf16(q, "q");
  tiled_check_bf16(k, "k");
  tiled_check_bf16(v, "v");
  TORCH_CHECK(q.dim() == 4 && k.sizes() == q.sizes() && v.sizes() == q.sizes(),
              "attn_tiled: q, k, v must be [B,H,L,D] of one shape");
  const long B = q.size(0), H = q.size(1), L = q.size(2), D = q.size(3);
  tiled_check_shape(B, H, L, D);
  tiled_check_common(q, lens, B, keep, seed);
  auto out = at::empty_like(q);
  auto lse = at::empty({B, H, L}, q.options().dtype(at::kFloat));
  const TiledStrides s{H * L * D, L * D, D, H * L * D, L * D, D};
  launch_fwd(cur_stream(q), (const bf16*)q.data_ptr(),
             (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
             lens.data_ptr<int>(), (bf16*)out.data_ptr(),
             lse.data_ptr<float>(), B, H, L, D, (float)scale, s, (float)keep,
             seed_ptr(seed));
  return {out, lse};
}

std::vector<at::Tensor> attn_tiled_bwd(const at::Tensor& dout,
                                       const at::Tensor& q,
                                       const at::Tensor& k,
                                       const at::Tensor& v,
                                       const at::Tensor& o,
                                       const at::Tensor& lse,
                                       const at::Tensor& lens, double scale,
                                       double keep,
                                       c10::optional<at::Tensor> seed) {
  tiled_check_bf16(dout, "dout");
  tiled_check_bf16(q, "q");
  tiled_check_bf16(k, "k");
  tiled_check_bf16(v, "v");
  tiled_check_bf16(o, "o");
  TORCH_CHECK(q.dim() == 4 && k.sizes() == q.sizes() &&
                  v.sizes() == q.sizes() && o.sizes() == q.sizes() &&
                  dout.sizes() == q.sizes(),
              "attn_tiled: dout, q, k, v, o must be [B,H,L,D] of one shape");
  const long B = q.size(0), H = q.size(1), L = q.size(2), D = q.size(3);
  tiled_check_shape(B, H, L, D);
  tiled_check_common(q, lens, B, keep, seed);
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == at::kFloat && lse.numel() == B * H * L,
              "attn_tiled: lse must be a contiguous fp32 [B,H,L] GPU tensor");
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  const TiledStrides s{H * L * D, L * D, D, H * L * D, L * D, D};
  launch_bwd(cur_stream(q), (const bf16*)dout.data_ptr(),
             (const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(),
             (const bf16*)v.data_ptr(), (const bf16*)o.data_ptr(),
             lse.data_ptr<float>(), lens.data_ptr<int>(), (bf16*)dq.data_ptr(),
             (bf16*)dk.data_ptr(), (bf16*)dv.data_ptr(), B, H, L, D,
             (float)scale, s, (float)keep, seed_ptr(seed));
  return {dq, dk, dv};
}

// packed layout API: qkv [B,L,3,H,D] -> out [B,L,H,D] (no copies)
std::vector<at::Tensor> attn_tiled_fwd_qkv(const at::Tensor& qkv,
                                           const at::Tensor& lens,
                                           double scale, double keep,
                                           c10::optional<at::Tensor> seed) {
  tiled_check_bf16(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "qkv must be [B,L,3,H,D]");
  const long B = qkv.size(0), L = qkv.size(1), H = qkv.size(3),
             D = qkv.size(4);
  tiled_check_shape(B, H, L, D);
  tiled_check_common(qkv, lens, B, keep, seed);
  auto out = at::empty({B, L, H, D}, qkv.options());
  auto lse = at::empty({B, H, L}, qkv.options().dtype(at::kFloat));
  const long HD = H * D;
  const TiledStrides s{L * 3 * HD, D, 3 * HD, L * HD, D, HD};
  const bf16* base = (const bf16*)qkv.data_ptr();
  launch_fwd(cur_stream(qkv), base, base + HD, base + 2 * HD,
             lens.data_ptr<int>(), (bf16*)out.data_ptr(),
             lse.data_ptr<float>(), B, H, L, D, (float)scale, s, (float)keep,
             seed_ptr(seed));
  return {out, lse};
}

std::vector<at::Tensor> attn_tiled_bwd_qkv(const at::Tensor& dout,
                                           const at::Tensor& qkv,
                                           const at::Tensor& o,
                                           const at::Tensor& lse,
                                           const at::Tensor& lens,
                                           double scale, double keep,
                                           c10::optional<at::Tensor> seed) {
  tiled_check_bf16(dout, "dout");
  tiled_check_bf16(qkv, "qkv");
  tiled_check_bf16(o, "o");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "qkv must be [B,L,3,H,D]");
  const long B = qkv.size(0), L = qkv.size(1), H = qkv.size(3),
             D = qkv.size(4);
  tiled_check_shape(B, H, L, D);
  tiled_check_common(qkv, lens, B, keep, seed);
  TORCH_CHECK(dout.dim() == 4 && dout.size(0) == B && dout.size(1) == L &&
                  dout.size(2) == H && dout.size(3) == D &&
                  o.sizes() == dout.sizes(),
              "attn_tiled: dout and o must be [B,L,H,D]");
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == at::kFloat && lse.numel() == B * H * L,
              "attn_tiled: lse must be a contiguous fp32 [B,H,L] GPU tensor");
  auto dqkv = at::empty_like(qkv);
  const long HD = H * D;
  const TiledStrides s{L * 3 * HD, D, 3 * HD, L * HD, D, HD};
  const bf16* base = (const bf16*)qkv.data_ptr();
  bf16* dbase = (bf16*)dqkv.data_ptr();
  launch_bwd(cur_stream(qkv), (const bf16*)dout.data_ptr(), base, base + HD,
             base + 2 * HD, (const bf16*)o.data_ptr(), lse.data_ptr<float>(),
             lens.data_ptr<int>(), dbase, dbase + HD, dbase + 2 * HD, B, H, L,
             D, (float)scale, s, (float)keep, seed_ptr(seed));
  return {dqkv};
}
