// Fused attention fwd/bwd for BERT + vanilla MHA,
// hand-written for gfx950: MFMA 16x16x32 bf16, all tiles LDS-resident
// (reference seq lens are <= 170 -> K/V/P fit whole in the 160 KiB LDS;
// no online softmax needed; L_pad <= 176).
//
// Layout notes (guide cdna_hip_programming.md par.3):
//  * A-frag  lane l -> A[(l&15)][kk*32 + (l>>4)*8 + e], e = 0..7
//  * B-frag  lane l -> B[kk*32 + (l>>4)*8 + e][(l&15)] -- read from an
//    [N][K]-stored (transposed) buffer with the same indexing as A.
//  * C/D     lane l, reg r -> D[(l>>4)*4 + r][nf*16 + (l&15)]
// Forward: K and V^T are staged so every MFMA operand read is one 16-byte
// contiguous LDS read. Backward: row-major images only; operands that run
// down a column come from ds_read_b64_tr_b16 (lds_frag_tr), see the
// phase/layout comment above attn_bwd_kernel.
//
// Strided I/O: the kernels take (batch, head, row) strides so the hot
// path consumes the fused-QKV projection output [B,L,3,H,D] directly and
// writes O as [B,L,H,D] -- zero transpose/copy around the kernel
// (torch-side reshape of the GEMM output is free).
#include "attn_common.h"
#include "slab_colsum.h"

#define MAXNF 11  // N-tiles of 16: L_pad <= 176
#define LPAD_MAX 176

// ---------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_fwd_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const int* __restrict__ lens,
    bf16* __restrict__ out, float* __restrict__ lse, int B, int H, int L,
    int D, int Lpad, float scale, long q_bs, long q_hs, long q_rs, long o_bs,
    long o_hs, long o_rs, int ds, int ls, float keep,
    const unsigned long long* __restrict__ seed) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  bf16* q_s = reinterpret_cast<bf16*>(smem_raw);    // [Lpad][ds]
  bf16* k_s = q_s + Lpad * ds;                      // [Lpad][ds]
  bf16* vt_s = k_s + Lpad * ds;                     // [D][ls]
  bf16* p_s = vt_s + D * ls;                        // [4 waves][16][ls]

  const int bh = blockIdx.x;
  const int b = bh / H;
  const int h = bh - b * H;
  const long qb = (long)b * q_bs + (long)h * q_hs;
  const long ob = (long)b * o_bs + (long)h * o_hs;
  const int len = lens[b];
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);

  stage_tile(q + qb, q_rs, q_s, L, Lpad, D, ds);
  stage_tile(k + qb, q_rs, k_s, L, Lpad, D, ds);
  stage_tile_T(v + qb, q_rs, vt_s, L, Lpad, D, ls);
  __syncthreads();

  const int NF = Lpad / 16;
  const int NKK = D / 32;
  const int NFD = D / 16;
  bf16* pw = p_s + wid * 16 * ls;

  for (int m0 = wid * 16; m0 < L; m0 += 4 * 16) {
    cfrag acc[MAXNF];
#pragma unroll
    for (int nf = 0; nf < MAXNF; ++nf) acc[nf] = cfrag{0.f, 0.f, 0.f, 0.f};
    bfrag aq[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      if (kk < NKK) aq[kk] = lds_frag(q_s, m0, ds, kk * 32);
#pragma unroll
    for (int nf = 0; nf < MAXNF; ++nf) {
      if (nf < NF) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          if (kk < NKK)
            acc[nf] = mfma16(aq[kk], lds_frag(k_s, nf * 16, ds, kk * 32),
                             acc[nf]);
      }
    }
    // softmax over rows (C layout: reg r = row, lane&15 = col)
    float row_lse[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = -1e30f;
#pragma unroll
      for (int nf = 0; nf < MAXNF; ++nf) {
        if (nf < NF) {
          const int col = nf * 16 + (lane & 15);
          const float s = (col < len) ? acc[nf][r] * scale : -1e30f;
          acc[nf][r] = s;
          mx = fmaxf(mx, s);
        }
      }
      mx = group16_reduce_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int nf = 0; nf < MAXNF; ++nf) {
        if (nf < NF) {
          const float p = __expf(acc[nf][r] - mx);
          acc[nf][r] = p;
          sum += p;
        }
      }
      sum = group16_reduce_sum(sum);
      const float inv = __frcp_rn(sum);
#pragma unroll
      for (int nf = 0; nf < MAXNF; ++nf)
        if (nf < NF) acc[nf][r] *= inv;
      row_lse[r] = mx + __logf(sum);
    }
    const unsigned long long sv = (keep < 1.f) ? *seed : 0ull;
#pragma unroll
    for (int nf = 0; nf < MAXNF; ++nf) {
      if (nf < NF) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int lr = ((lane >> 4) << 2) + r;
          float p = acc[nf][r];
          if (keep < 1.f) {
            // attention-prob dropout (BERT attention_probs_dropout_prob):
            // mask regenerated in backward from the same (seed, index)
            const long idx = ((long)bh * L + (m0 + lr)) * L + nf * 16 +
                             (lane & 15);
            p = attn_hash_uniform(sv, (unsigned long long)idx) < keep
                    ? p / keep
                    : 0.f;
          }
          pw[lr * ls + nf * 16 + (lane & 15)] = __float2bfloat16(p);
        }
      }
    }
    if ((lane & 15) == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + ((lane >> 4) << 2) + r;
        if (row < L) lse[(long)bh * L + row] = row_lse[r];
      }
    }
    // O = P V
    cfrag oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[i] = cfrag{0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < Lpad / 32; ++kk) {
      const bfrag ap = lds_frag(pw, 0, ls, kk * 32);
#pragma unroll
      for (int nd = 0; nd < 4; ++nd)
        if (nd < NFD)
          oacc[nd] = mfma16(ap, lds_frag(vt_s, nd * 16, ls, kk * 32),
                            oacc[nd]);
    }
#pragma unroll
    for (int nd = 0; nd < 4; ++nd) {
      if (nd < NFD) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + ((lane >> 4) << 2) + r;
          if (row < L)
            out[ob + (long)row * o_rs + nd * 16 + (lane & 15)] =
                __float2bfloat16(oacc[nd][r]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------
// backward: P recomputed from lse; dV = P'^T dO ; dS = P*(D.dP/keep -
// delta); dK = dS^T Q ; dQ = dS K. P^T is overwritten by dS^T in place.
//
// LDS images (all bf16, row-major): Q, K, V, dO as [Lpad][ds] and
// P^T / dS^T as [key][query] = [Lpad][ls]. One image per tile serves both
// kinds of operand read: rows by ds_read_b128 (lds_frag) for S = Q K^T and
// dP = dO V^T, columns by ds_read_b64_tr_b16 (lds_frag_tr) for the three
// output products. Those are computed TRANSPOSED (dV^T = dO^T P', dK^T =
// Q^T dS, dQ^T = K^T dS^T) with the image's d columns permuted over the
// MFMA rows so that a lane ends up with D/4 consecutive d of one output
// row: every dq/dk/dv store is 16 bytes per lane.
//
// Phases (block-wide barrier after 0, 1, 2, 3):
//  0  issue all global loads of the block; stage Q, K, lse
//  1  P = exp(S*scale - lse) -> P^T, 4 queries packed per 8-byte store;
//     the dropout decision (one hash per cell) rides in the bf16 sign bit
//     (P >= 0): set = dropped. Then stage V, dO (their loads were in
//     flight behind this phase) and delta[r] = dot(dO[r], O[r])
//  2  dV^T: B operand = P^T rows, sign bit -> 0, else * 1/keep
//  3  dP; dS = P (keep-bit ? dP/keep : 0  - delta) scale -> dS^T in place
//  4  dK^T: B = dS^T rows          5  dQ^T: B = dS^T transposed read
// Optional QKV bias gradient: each wave sums the bf16-rounded values it
// stores over its rows, a fixed-order reduction over the 8 waves follows,
// and the block writes its 3*D fp32 partials to dbias_slab[b][3*H*D].
// ---------------------------------------------------------------------
#define BWD_WAVES 8
// staging passes of 512 x 16 bytes per tile: LPAD_MAX * 64 / 8 / 512
#define BWD_STAGE_IT 3

// P^T fragment -> dropped-and-rescaled P'^T fragment (sign bit = dropped)
__device__ __forceinline__ bfrag ptfrag_apply_drop(bfrag f, float inv_keep) {
  const s16x8 in = __builtin_bit_cast(s16x8, f);
  s16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const unsigned bits = (unsigned short)in[e];
    const float p = __uint_as_float((bits & 0x7fffu) << 16);
    reinterpret_cast<bf16*>(&o)[e] =
        __float2bfloat16((bits & 0x8000u) ? 0.f : p * inv_keep);
  }
  return __builtin_bit_cast(bfrag, o);
}

// One output product, transposed: out[n][d] = sum_k img[k][d] * X[k][n]
// for this wave's 16-wide strips of n. X[k][n] = pt_s[n][k] (B_TR false:
// row read) or pt_s[k][n] (B_TR true: transposed read). MFMA row m of d-tile
// tau (< D/16) is d = (D/4) (m >> 2) + 4 tau + (m & 3), so lane
// (G = lane >> 4) holds the D/4 consecutive d from (D/4) G of row
// n0 + (lane & 15): whole 16-byte stores. (At D = 64 this spreading of
// a lane group's four 8-byte chunks 32 bytes apart is also what keeps the
// transposed read of the [Lpad][72] images 2-way; see attn_strides.)
template <bool B_TR, bool DROP>
__device__ __forceinline__ void bwd_out_phase(
    const bf16* img_s, int ds, const bf16* pt_s, int ls, int L, int Lpad,
    int D, float inv_keep, bf16* __restrict__ out, long rs, float* bpart) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int G = lane >> 4;
  const int NT = D / 16;
  const int pcol = (D >> 2) * (lane & 3);
  const int d0 = (D >> 2) * G;
  float bs[4][4];
#pragma unroll
  for (int tau = 0; tau < 4; ++tau)
#pragma unroll
    for (int r = 0; r < 4; ++r) bs[tau][r] = 0.f;

  for (int n0 = wid * 16; n0 < L; n0 += BWD_WAVES * 16) {
    cfrag acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = cfrag{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Lpad; k0 += 32) {
      // Lpad % 32 == 16 leaves half a k-chunk at the end: lanes whose 8 k
      // lie past Lpad re-read the chunk's first half (in bounds, finite)
      // and contribute a zero A operand. Selects only: EXEC stays full.
      const bool past = k0 + (G << 3) >= Lpad;
      const int kb = past ? k0 - 16 : k0;
      bfrag b = B_TR ? lds_frag_tr(pt_s, kb, ls, n0 + ((lane & 3) << 2))
                     : lds_frag(pt_s, n0, ls, kb);
      if (DROP) b = ptfrag_apply_drop(b, inv_keep);
#pragma unroll
      for (int tau = 0; tau < 4; ++tau) {
        if (tau < NT) {
          bfrag a = lds_frag_tr(img_s, kb, ds, pcol + 4 * tau);
          if (past) a = bfrag{};
          acc[tau] = mfma16(a, b, acc[tau]);
        }
      }
    }
    const int row = n0 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (2 * j < NT) {
        s16x8 o;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bf16 x = __float2bfloat16(acc[2 * j + t][r]);
            reinterpret_cast<bf16*>(&o)[t * 4 + r] = x;
            if (row < L) bs[2 * j + t][r] += to_f32(x);
          }
        }
        if (row < L)
          *reinterpret_cast<s16x8*>(out + (long)row * rs + d0 + 8 * j) = o;
      }
    }
  }
  if (bpart != nullptr) {
#pragma unroll
    for (int tau = 0; tau < 4; ++tau) {
      if (tau < NT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = group16_reduce_sum(bs[tau][r]);
          if ((lane & 15) == 0) bpart[d0 + 4 * tau + r] = v;
        }
      }
    }
  }
}

__global__ __launch_bounds__(BWD_WAVES * WAVE) void attn_bwd_kernel(
    const bf16* __restrict__ dout, const bf16* __restrict__ q,
    const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ o, const float* __restrict__ lse,
    const int* __restrict__ lens, bf16* __restrict__ dq,
    bf16* __restrict__ dk, bf16* __restrict__ dv, int B, int H, int L, int D,
    int Lpad, float scale, long q_bs, long q_hs, long q_rs, long o_bs,
    long o_hs, long o_rs, int ds, int ls, float keep,
    const unsigned long long* __restrict__ seed,
    float* __restrict__ dbias_slab) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  bf16* q_s = reinterpret_cast<bf16*>(smem_raw);   // [Lpad][ds]
  bf16* k_s = q_s + Lpad * ds;                     // [Lpad][ds]
  bf16* v_s = k_s + Lpad * ds;                     // [Lpad][ds]
  bf16* do_s = v_s + Lpad * ds;                    // [Lpad][ds]
  bf16* pt_s = do_s + Lpad * ds;                   // [Lpad][ls] P^T / dS^T
  float* delta_s = reinterpret_cast<float*>(pt_s + (long)Lpad * ls);
  float* lse_s = delta_s + Lpad;
  float* bpart_s = lse_s + Lpad;                   // [BWD_WAVES][3][D]

  const int bh = blockIdx.x;
  const int b = bh / H;
  const int h = bh - b * H;
  const long qb = (long)b * q_bs + (long)h * q_hs;
  const long ob = (long)b * o_bs + (long)h * o_hs;
  const int len = lens[b];
  const bool drop = keep < 1.f;
  const unsigned long long sv = drop ? *seed : 0ull;
  const float inv_keep = 1.f / keep;
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int G = lane >> 4;
  const int NF = Lpad / 16;
  const int NKK = D / 32;

  // phase 0: issue every global load of the block at once (Q and K first;
  // loads return in order), stage Q, K and lse, and leave V, dO and O in
  // flight behind phase 1. Lpad * D / 8 is a multiple of 64, so a wave
  // takes each `i < nv` branch with all lanes or not at all.
  const int nv = Lpad * D / 8;
  s16x8 vq[BWD_STAGE_IT], vk[BWD_STAGE_IT], vv[BWD_STAGE_IT],
      vdo[BWD_STAGE_IT], vo[BWD_STAGE_IT];
#pragma unroll
  for (int it = 0; it < BWD_STAGE_IT; ++it) {
    const int i = threadIdx.x + it * BWD_WAVES * WAVE;
    const int r = (i * 8) / D;
    const int c = (i * 8) % D;
    vq[it] = s16x8{};
    vk[it] = s16x8{};
    if (i < nv && r < L) {
      const long go = qb + (long)r * q_rs + c;
      vq[it] = *reinterpret_cast<const s16x8*>(q + go);
      vk[it] = *reinterpret_cast<const s16x8*>(k + go);
    }
  }
  for (int r = threadIdx.x; r < Lpad; r += blockDim.x)
    lse_s[r] = (r < L) ? lse[(long)bh * L + r] : 0.f;
#pragma unroll
  for (int it = 0; it < BWD_STAGE_IT; ++it) {
    const int i = threadIdx.x + it * BWD_WAVES * WAVE;
    const int r = (i * 8) / D;
    const int c = (i * 8) % D;
    vv[it] = s16x8{};
    vdo[it] = s16x8{};
    vo[it] = s16x8{};
    if (i < nv && r < L) {
      const long go = qb + (long)r * q_rs + c;
      const long oo = ob + (long)r * o_rs + c;
      vv[it] = *reinterpret_cast<const s16x8*>(v + go);
      vdo[it] = *reinterpret_cast<const s16x8*>(dout + oo);
      vo[it] = *reinterpret_cast<const s16x8*>(o + oo);
    }
  }
#pragma unroll
  for (int it = 0; it < BWD_STAGE_IT; ++it) {
    const int i = threadIdx.x + it * BWD_WAVES * WAVE;
    if (i < nv) {
      const long so = (long)((i * 8) / D) * ds + (i * 8) % D;
      *reinterpret_cast<s16x8*>(q_s + so) = vq[it];
      *reinterpret_cast<s16x8*>(k_s + so) = vk[it];
    }
  }
  __syncthreads();

  // phase 1: recompute P -> P^T (+ dropout decision in the sign bit)
  for (int m0 = wid * 16; m0 < Lpad; m0 += BWD_WAVES * 16) {
    cfrag acc[MAXNF];
#pragma unroll
    for (int nf = 0; nf < MAXNF; ++nf) acc[nf] = cfrag{0.f, 0.f, 0.f, 0.f};
    bfrag aq[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      if (kk < NKK) aq[kk] = lds_frag(q_s, m0, ds, kk * 32);
#pragma unroll
    for (int nf = 0; nf < MAXNF; ++nf) {
      if (nf < NF) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          if (kk < NKK)
            acc[nf] = mfma16(aq[kk], lds_frag(k_s, nf * 16, ds, kk * 32),
                             acc[nf]);
      }
    }
#pragma unroll
    for (int nf = 0; nf < MAXNF; ++nf) {
      if (nf < NF) {
        const int col = nf * 16 + (lane & 15);
        s16x4 pk;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + (G << 2) + r;
          float p = 0.f;
          bool dropped = false;
          if (row < L && col < len) {
            p = __expf(acc[nf][r] * scale - lse_s[row]);
            if (drop) {
              const long idx = ((long)bh * L + row) * L + col;
              dropped =
                  !(attn_hash_uniform(sv, (unsigned long long)idx) < keep);
            }
          }
          const bf16 pb = __float2bfloat16(p);
          short bits = *reinterpret_cast<const short*>(&pb);
          if (dropped) bits |= (short)0x8000;
          pk[r] = bits;
        }
        *reinterpret_cast<s16x4*>(pt_s + (long)col * ls + m0 + (G << 2)) = pk;
      }
    }
  }
  // stage V and dO; delta[r] = dot(dO[r], O[r]) over the row's D/8
  // consecutive lanes
#pragma unroll
  for (int it = 0; it < BWD_STAGE_IT; ++it) {
    const int i = threadIdx.x + it * BWD_WAVES * WAVE;
    if (i < nv) {
      const int r = (i * 8) / D;
      const int c = (i * 8) % D;
      const long so = (long)r * ds + c;
      *reinterpret_cast<s16x8*>(v_s + so) = vv[it];
      *reinterpret_cast<s16x8*>(do_s + so) = vdo[it];
      const bf16* pd = reinterpret_cast<const bf16*>(&vdo[it]);
      const bf16* po = reinterpret_cast<const bf16*>(&vo[it]);
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc += to_f32(pd[e]) * to_f32(po[e]);
      for (int off = D / 16; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
      if (c == 0) delta_s[r] = acc;
    }
  }
  __syncthreads();

  // phase 2: dV^T = dO^T P'
  float* bp = dbias_slab ? bpart_s + (long)wid * 3 * D : nullptr;
  if (drop)
    bwd_out_phase<false, true>(do_s, ds, pt_s, ls, L, Lpad, D, inv_keep,
                               dv + qb, q_rs, bp ? bp + 2 * D : nullptr);
  else
    bwd_out_phase<false, false>(do_s, ds, pt_s, ls, L, Lpad, D, inv_keep,
                                dv + qb, q_rs, bp ? bp + 2 * D : nullptr);
  __syncthreads();

  // phase 3: dP = dO V^T ; dS = P (dP' - delta) * scale -> overwrite P^T
  for (int m0 = wid * 16; m0 < L; m0 += BWD_WAVES * 16) {
    cfrag acc[MAXNF];
#pragma unroll
    for (int nf = 0; nf < MAXNF; ++nf) acc[nf] = cfrag{0.f, 0.f, 0.f, 0.f};
    bfrag ado[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      if (kk < NKK) ado[kk] = lds_frag(do_s, m0, ds, kk * 32);
#pragma unroll
    for (int nf = 0; nf < MAXNF; ++nf) {
      if (nf < NF) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          if (kk < NKK)
            acc[nf] = mfma16(ado[kk], lds_frag(v_s, nf * 16, ds, kk * 32),
                             acc[nf]);
      }
    }
    float dl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) dl[r] = delta_s[m0 + (G << 2) + r];
#pragma unroll
    for (int nf = 0; nf < MAXNF; ++nf) {
      if (nf < NF) {
        const int col = nf * 16 + (lane & 15);
        s16x4* cell =
            reinterpret_cast<s16x4*>(pt_s + (long)col * ls + m0 + (G << 2));
        const s16x4 pk = *cell;
        s16x4 dsk;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned bits = (unsigned short)pk[r];
          const float p = __uint_as_float((bits & 0x7fffu) << 16);
          float dpr = acc[nf][r];
          if (drop) dpr = (bits & 0x8000u) ? 0.f : dpr * inv_keep;
          const float dsv = p * (dpr - dl[r]) * scale;
          reinterpret_cast<bf16*>(&dsk)[r] = __float2bfloat16(dsv);
        }
        *cell = dsk;
      }
    }
  }
  __syncthreads();

  // phase 4: dK^T = Q^T dS ; phase 5: dQ^T = K^T dS^T
  bwd_out_phase<false, false>(q_s, ds, pt_s, ls, L, Lpad, D, 1.f, dk + qb,
                              q_rs, bp ? bp + D : nullptr);
  bwd_out_phase<true, false>(k_s, ds, pt_s, ls, L, Lpad, D, 1.f, dq + qb,
                             q_rs, bp);

  if (dbias_slab != nullptr) {
    __syncthreads();
    // fixed order over the waves; slab row b is [3][H][D]
    for (int i = threadIdx.x; i < 3 * D; i += blockDim.x) {
      float a = bpart_s[i];
#pragma unroll
      for (int w = 1; w < BWD_WAVES; ++w) a += bpart_s[(long)w * 3 * D + i];
      const int which = i / D;
      const int d = i - which * D;
      dbias_slab[((long)b * 3 + which) * H * D + (long)h * D + d] = a;
    }
  }
}

// ===================================================================== host
struct AttnShape {
  int B, H, L, D, Lpad;
};

// The forward pads L to a multiple of 32 (L <= 160). The backward also
// takes 161 <= L <= 176 with L padded to 16 only (half a k-chunk at the
// end, see bwd_out_phase): Lpad = 176 is its LDS limit at D = 64.
static AttnShape attn_shape(int B, int H, int L, int D, bool bwd = false) {
  TORCH_CHECK(D == 32 || D == 64, "attention: head dim must be 32 or 64 "
              "(pad in the wrapper), got ", D);
  TORCH_CHECK(L >= 1, "attention: empty sequence");
  int Lpad = ((L + 31) / 32) * 32;
  if (bwd && Lpad > LPAD_MAX) Lpad = ((L + 15) / 16) * 16;
  TORCH_CHECK(Lpad <= LPAD_MAX,
              "attention: seq len > 176 unsupported by the full-LDS kernel");
  return {B, H, L, D, Lpad};
}


// LDS strides: pad so stride_bytes/16 is odd (ld % 16 == 8 for bf16);
// fall back to unpadded when over 160 KiB. Banking at these strides (bank
// = (addr/4) % 64 for b64/b128/tr reads, % 32 for writes; counted per
// 32-lane half):
//  * ds_read_b128 row reads (lds_frag): conflict-free.
//  * backward, ds_read_b64_tr_b16 of the [Lpad][D+8] images with the
//    permuted columns of bwd_out_phase: 2-way at D = 64 (stride 72), 3-way
//    at D = 32 (stride 40); of the P^T image (natural columns): 2-way.
//  * backward, 8-byte packed P^T / dS^T stores: 2-way.
//  No plain stride that keeps rows 16-byte aligned does better for the
//  transposed read: 8 rows of 8 dwords cannot tile 64 banks when the row
//  stride is a multiple of 4 dwords. With the images unpadded (Lpad = 176,
//  D = 64 only) the transposed reads are 4-way and the row reads conflict
//  too; that case only has to fit.
static void attn_strides(int D, int Lpad, bool bwd, int& ds, int& ls,
                         size_t& smem) {
  ds = D + 8;
  ls = Lpad + 8;
  auto sz = [&](int ds_, int ls_) -> size_t {
    if (bwd)
      return (size_t)(4 * Lpad * ds_ + (long)Lpad * ls_) * sizeof(bf16)
             + (2 * Lpad + BWD_WAVES * 3 * D) * sizeof(float);
    return (size_t)(2 * Lpad * ds_ + D * ls_ + 4 * 16 * ls_) * sizeof(bf16);
  };
  smem = sz(ds, ls);
  if (smem > 160 * 1024) {  // rare (bwd at Lpad = 176, D = 64): unpad the
    ds = D;                 // four [Lpad][D] images, keep P^T padded
    smem = sz(ds, ls);
  }
  if (smem > 160 * 1024) {
    ls = Lpad;
    smem = sz(ds, ls);
  }
}

// old layout API: q,k,v,out all [B,H,L,D]
std::vector<at::Tensor> attn_fwd(const at::Tensor& q, const at::Tensor& k,
                                 const at::Tensor& v, const at::Tensor& lens,
                                 double scale, double keep,
                                 c10::optional<at::Tensor> seed) {
  CHECK_CUDA_CONTIG(q);
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "attention: bf16 only");
  auto s = attn_shape(q.size(0), q.size(1), q.size(2), q.size(3));
  auto out = at::empty_like(q);
  auto lse = at::empty({s.B, s.H, s.L}, q.options().dtype(at::kFloat));
  int ds, ls;
  size_t smem;
  attn_strides(s.D, s.Lpad, false, ds, ls, smem);
  TORCH_CHECK(smem <= 160 * 1024, "attn fwd LDS overflow");
  const long bs = (long)s.H * s.L * s.D, hs = (long)s.L * s.D, rs = s.D;
  hipLaunchKernelGGL(attn_fwd_kernel, dim3(s.B * s.H), dim3(256), smem,
                     cur_stream(q), (const bf16*)q.data_ptr(),
                     (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
                     lens.data_ptr<int>(), (bf16*)out.data_ptr(),
                     lse.data_ptr<float>(), s.B, s.H, s.L, s.D, s.Lpad,
                     (float)scale, bs, hs, rs, bs, hs, rs, ds, ls,
                     (float)keep,
                     seed ? (const unsigned long long*)seed->data_ptr()
                          : nullptr);
  HIP_CHECK_LAST();
  return {out, lse};
}

std::vector<at::Tensor> attn_bwd(const at::Tensor& dout, const at::Tensor& q,
                                 const at::Tensor& k, const at::Tensor& v,
                                 const at::Tensor& o, const at::Tensor& lse,
                                 const at::Tensor& lens, double scale,
                                 double keep, c10::optional<at::Tensor> seed) {
  auto s = attn_shape(q.size(0), q.size(1), q.size(2), q.size(3), true);
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  int ds, ls;
  size_t smem;
  attn_strides(s.D, s.Lpad, true, ds, ls, smem);
  TORCH_CHECK(smem <= 160 * 1024, "attn bwd LDS overflow");
  const long bs = (long)s.H * s.L * s.D, hs = (long)s.L * s.D, rs = s.D;
  hipLaunchKernelGGL(attn_bwd_kernel, dim3(s.B * s.H),
                     dim3(BWD_WAVES * WAVE), smem,
                     cur_stream(q), (const bf16*)dout.data_ptr(),
                     (const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(),
                     (const bf16*)v.data_ptr(), (const bf16*)o.data_ptr(),
                     lse.data_ptr<float>(), lens.data_ptr<int>(),
                     (bf16*)dq.data_ptr(), (bf16*)dk.data_ptr(),
                     (bf16*)dv.data_ptr(), s.B, s.H, s.L, s.D, s.Lpad,
                     (float)scale, bs, hs, rs, bs, hs, rs, ds, ls,
                     (float)keep,
                     seed ? (const unsigned long long*)seed->data_ptr()
                          : nullptr,
                     (float*)nullptr);
  HIP_CHECK_LAST();
  return {dq, dk, dv};
}

// packed layout API: qkv [B,L,3,H,D] -> out [B,L,H,D] (no copies)
std::vector<at::Tensor> attn_fwd_qkv(const at::Tensor& qkv,
                                     const at::Tensor& lens, double scale,
                                     double keep,
                                     c10::optional<at::Tensor> seed) {
  CHECK_CUDA_CONTIG(qkv);
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, "attention: bf16 only");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "qkv must be [B,L,3,H,D]");
  auto s = attn_shape(qkv.size(0), qkv.size(3), qkv.size(1), qkv.size(4));
  auto out = at::empty({s.B, s.L, s.H, s.D}, qkv.options());
  auto lse = at::empty({s.B, s.H, s.L}, qkv.options().dtype(at::kFloat));
  int ds, ls;
  size_t smem;
  attn_strides(s.D, s.Lpad, false, ds, ls, smem);
  TORCH_CHECK(smem <= 160 * 1024, "attn fwd LDS overflow");
  const long HD = (long)s.H * s.D;
  const long q_bs = (long)s.L * 3 * HD, q_hs = s.D, q_rs = 3 * HD;
  const long o_bs = (long)s.L * HD, o_hs = s.D, o_rs = HD;
  const bf16* base = (const bf16*)qkv.data_ptr();
  hipLaunchKernelGGL(attn_fwd_kernel, dim3(s.B * s.H), dim3(256), smem,
                     cur_stream(qkv), base, base + HD, base + 2 * HD,
                     lens.data_ptr<int>(), (bf16*)out.data_ptr(),
                     lse.data_ptr<float>(), s.B, s.H, s.L, s.D, s.Lpad,
                     (float)scale, q_bs, q_hs, q_rs, o_bs, o_hs, o_rs, ds, ls,
                     (float)keep,
                     seed ? (const unsigned long long*)seed->data_ptr()
                          : nullptr);
  HIP_CHECK_LAST();
  return {out, lse};
}

// packed backward; slab (optional) receives the per-batch QKV bias-grad
// partials [B][3*H*D]
static at::Tensor attn_bwd_qkv_launch(const at::Tensor& dout,
                                      const at::Tensor& qkv,
                                      const at::Tensor& o,
                                      const at::Tensor& lse,
                                      const at::Tensor& lens, double scale,
                                      double keep,
                                      const c10::optional<at::Tensor>& seed,
                                      float* slab) {
  CHECK_CUDA_CONTIG(dout);
  auto s = attn_shape(qkv.size(0), qkv.size(3), qkv.size(1), qkv.size(4),
                      true);
  auto dqkv = at::empty_like(qkv);
  int ds, ls;
  size_t smem;
  attn_strides(s.D, s.Lpad, true, ds, ls, smem);
  TORCH_CHECK(smem <= 160 * 1024, "attn bwd LDS overflow");
  const long HD = (long)s.H * s.D;
  const long q_bs = (long)s.L * 3 * HD, q_hs = s.D, q_rs = 3 * HD;
  const long o_bs = (long)s.L * HD, o_hs = s.D, o_rs = HD;
  const bf16* base = (const bf16*)qkv.data_ptr();
  bf16* dbase = (bf16*)dqkv.data_ptr();
  hipLaunchKernelGGL(attn_bwd_kernel, dim3(s.B * s.H),
                     dim3(BWD_WAVES * WAVE), smem,
                     cur_stream(qkv), (const bf16*)dout.data_ptr(), base,
                     base + HD, base + 2 * HD, (const bf16*)o.data_ptr(),
                     lse.data_ptr<float>(), lens.data_ptr<int>(), dbase,
                     dbase + HD, dbase + 2 * HD, s.B, s.H, s.L, s.D, s.Lpad,
                     (float)scale, q_bs, q_hs, q_rs, o_bs, o_hs, o_rs, ds, ls,
                     (float)keep,
                     seed ? (const unsigned long long*)seed->data_ptr()
                          : nullptr,
                     slab);
  HIP_CHECK_LAST();
  return dqkv;
}

std::vector<at::Tensor> attn_bwd_qkv(const at::Tensor& dout,
                                     const at::Tensor& qkv,
                                     const at::Tensor& o, const at::Tensor& lse,
                                     const at::Tensor& lens, double scale,
                                     double keep,
                                     c10::optional<at::Tensor> seed) {
  return {attn_bwd_qkv_launch(dout, qkv, o, lse, lens, scale, keep, seed,
                              nullptr)};
}

// as attn_bwd_qkv, plus the QKV bias gradient: dbias [3*H*D] in `bias`'s
// dtype (bf16 or fp32) equals the column sum of the returned dqkv viewed
// as [B*L, 3*H*D], summed in fp32 in a fixed order (rows of one batch item
// inside the kernel, then over B by slab_colsum_kernel). No atomics.
std::vector<at::Tensor> attn_bwd_qkv_dbias(
    const at::Tensor& dout, const at::Tensor& qkv, const at::Tensor& o,
    const at::Tensor& lse, const at::Tensor& lens, double scale, double keep,
    c10::optional<at::Tensor> seed, const at::Tensor& bias) {
  const long C = 3 * qkv.size(3) * qkv.size(4);
  TORCH_CHECK(bias.is_cuda() && bias.numel() == C,
              "attn_bwd_qkv_dbias: bias must be a GPU tensor of 3*H*D");
  TORCH_CHECK(bias.scalar_type() == at::kBFloat16 ||
                  bias.scalar_type() == at::kFloat,
              "attn_bwd_qkv_dbias: bias must be bf16 or fp32");
  auto slab = at::empty({qkv.size(0), C}, qkv.options().dtype(at::kFloat));
  auto dqkv = attn_bwd_qkv_launch(dout, qkv, o, lse, lens, scale, keep, seed,
                                  slab.data_ptr<float>());
  auto dbias = at::empty({C}, bias.options());
  if (bias.scalar_type() == at::kBFloat16)
    launch_slab_colsum<bf16, bf16>(slab, dbias.data_ptr(), (int)C, nullptr,
                                   cur_stream(qkv));
  else
    launch_slab_colsum<float, float>(slab, dbias.data_ptr(), (int)C, nullptr,
                                     cur_stream(qkv));
  HIP_CHECK_LAST();
  return {dqkv, dbias};
}
