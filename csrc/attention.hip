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
// K and V^T are staged so every MFMA operand read is one 16-byte
// contiguous LDS read.
//
// Strided I/O: the kernels take (batch, head, row) strides so the hot
// path consumes the fused-QKV projection output [B,L,3,H,D] directly and
// writes O as [B,L,H,D] -- zero transpose/copy around the kernel
// (torch-side reshape of the GEMM output is free).
#include "attn_common.h"

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

// masked P'^T fragment for the dV matmul: pt_s stores UNMASKED P
// (phase 3 needs it); the dropout mask is regenerated per element
__device__ __forceinline__ bfrag ptfrag_dropped(const bf16* pt_s, int k0,
                                                int ls, int kq0, long bh,
                                                int L, float keep,
                                                unsigned long long sv) {
  const int l = threadIdx.x & (WAVE - 1);
  const int key = k0 + (l & 15);
  const float inv_keep = 1.f / keep;
  bfrag f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int query = kq0 + ((l >> 4) << 3) + e;
    float p = to_f32(pt_s[(long)key * ls + query]);
    const long idx = (bh * L + query) * (long)L + key;
    p = attn_hash_uniform(sv, (unsigned long long)idx) < keep ? p * inv_keep
                                                              : 0.f;
    reinterpret_cast<bf16*>(&f)[e] = __float2bfloat16(p);
  }
  return f;
}

// ---------------------------------------------------------------------
// backward: P recomputed from lse; dV = P'^T dO ; dS = P*(D.dP/keep -
// delta); dK = dS^T Q ; dQ = dS K. P^T is overwritten by dS^T in place.
// ---------------------------------------------------------------------
__global__ __launch_bounds__(512) void attn_bwd_kernel(
    const bf16* __restrict__ dout, const bf16* __restrict__ q,
    const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ o, const float* __restrict__ lse,
    const int* __restrict__ lens, bf16* __restrict__ dq,
    bf16* __restrict__ dk, bf16* __restrict__ dv, int B, int H, int L, int D,
    int Lpad, float scale, long q_bs, long q_hs, long q_rs, long o_bs,
    long o_hs, long o_rs, int ds, int ls, float keep,
    const unsigned long long* __restrict__ seed) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  bf16* q_s = reinterpret_cast<bf16*>(smem_raw);   // [Lpad][ds]
  bf16* k_s = q_s + Lpad * ds;                     // [Lpad][ds]
  bf16* v_s = k_s + Lpad * ds;                     // [Lpad][ds] row major
  bf16* do_s = v_s + Lpad * ds;                    // [Lpad][ds]
  bf16* pt_s = do_s + Lpad * ds;                   // [Lpad][ls] P^T / dS^T
  float* delta_s = reinterpret_cast<float*>(pt_s + (long)Lpad * ls);
  float* lse_s = delta_s + Lpad;

  const int bh = blockIdx.x;
  const int b = bh / H;
  const int h = bh - b * H;
  const long qb = (long)b * q_bs + (long)h * q_hs;
  const long ob = (long)b * o_bs + (long)h * o_hs;
  const int len = lens[b];
  const unsigned long long sv = (keep < 1.f) ? *seed : 0ull;
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int NF = Lpad / 16;
  const int NKK = D / 32;
  const int NFD = D / 16;

  stage_tile(q + qb, q_rs, q_s, L, Lpad, D, ds);
  stage_tile(k + qb, q_rs, k_s, L, Lpad, D, ds);
  stage_tile(v + qb, q_rs, v_s, L, Lpad, D, ds);
  stage_tile(dout + ob, o_rs, do_s, L, Lpad, D, ds);
  // delta[r] = dot(dO[r], O[r]) — one wave per row, 8-wide vector loads
  for (int r = wid; r < Lpad; r += blockDim.x / WAVE) {
    float acc = 0.f;
    if (r < L) {
      for (int d = lane * 8; d < D; d += WAVE * 8) {
        const s16x8 vdo =
            *reinterpret_cast<const s16x8*>(dout + ob + (long)r * o_rs + d);
        const s16x8 vo =
            *reinterpret_cast<const s16x8*>(o + ob + (long)r * o_rs + d);
        const bf16* pd = reinterpret_cast<const bf16*>(&vdo);
        const bf16* po = reinterpret_cast<const bf16*>(&vo);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += to_f32(pd[e]) * to_f32(po[e]);
      }
      for (int off = WAVE / 2; off > 0; off >>= 1)
        acc += __shfl_down(acc, off, WAVE);
      acc = __shfl(acc, 0, WAVE);
      if (lane == 0) lse_s[r] = lse[(long)bh * L + r];
    } else if (lane == 0) {
      lse_s[r] = 0.f;
    }
    if (lane == 0) delta_s[r] = acc;
  }
  __syncthreads();

  // phase 1: recompute P -> P^T
  for (int m0 = wid * 16; m0 < Lpad; m0 += (blockDim.x >> 6) << 4) {
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
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + ((lane >> 4) << 2) + r;
          const int col = nf * 16 + (lane & 15);
          float p = 0.f;
          if (row < L && col < len)
            p = __expf(acc[nf][r] * scale - lse_s[row]);
          pt_s[(long)col * ls + row] = __float2bfloat16(p);
        }
      }
    }
  }
  __syncthreads();

  // phase 2: dV[keys] = P^T dO
  for (int k0 = wid * 16; k0 < L; k0 += (blockDim.x >> 6) << 4) {
    cfrag acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = cfrag{0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < Lpad / 32; ++kk) {
      const bfrag ap =
          (keep < 1.f)
              ? ptfrag_dropped(pt_s, k0, ls, kk * 32, bh, L, keep, sv)
              : lds_frag(pt_s, k0, ls, kk * 32);
#pragma unroll
      for (int nd = 0; nd < 4; ++nd)
        if (nd < NFD)
          acc[nd] = mfma16(ap, lds_fragB_rowmajor(do_s, kk * 32, ds, nd * 16),
                           acc[nd]);
    }
#pragma unroll
    for (int nd = 0; nd < 4; ++nd) {
      if (nd < NFD) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int krow = k0 + ((lane >> 4) << 2) + r;
          if (krow < L)
            dv[qb + (long)krow * q_rs + nd * 16 + (lane & 15)] =
                __float2bfloat16(acc[nd][r]);
        }
      }
    }
  }
  __syncthreads();

  // phase 3: dP = dO V^T ; dS = P (dP - delta) * scale -> overwrite P^T
  for (int m0 = wid * 16; m0 < L; m0 += (blockDim.x >> 6) << 4) {
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
#pragma unroll
    for (int nf = 0; nf < MAXNF; ++nf) {
      if (nf < NF) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + ((lane >> 4) << 2) + r;
          const int col = nf * 16 + (lane & 15);
          const float p = to_f32(pt_s[(long)col * ls + row]);
          float dpr = acc[nf][r];
          if (keep < 1.f) {
            const long idx = ((long)bh * L + row) * L + col;
            dpr = attn_hash_uniform(sv, (unsigned long long)idx) < keep
                      ? dpr / keep
                      : 0.f;
          }
          const float dsv = p * (dpr - delta_s[row]) * scale;
          pt_s[(long)col * ls + row] = __float2bfloat16(dsv);
        }
      }
    }
  }
  __syncthreads();

  // phase 4: dK[keys] = dS^T Q
  for (int k0 = wid * 16; k0 < L; k0 += (blockDim.x >> 6) << 4) {
    cfrag acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = cfrag{0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < Lpad / 32; ++kk) {
      const bfrag ads = lds_frag(pt_s, k0, ls, kk * 32);
#pragma unroll
      for (int nd = 0; nd < 4; ++nd)
        if (nd < NFD)
          acc[nd] = mfma16(ads, lds_fragB_rowmajor(q_s, kk * 32, ds, nd * 16),
                           acc[nd]);
    }
#pragma unroll
    for (int nd = 0; nd < 4; ++nd) {
      if (nd < NFD) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int krow = k0 + ((lane >> 4) << 2) + r;
          if (krow < L)
            dk[qb + (long)krow * q_rs + nd * 16 + (lane & 15)] =
                __float2bfloat16(acc[nd][r]);
        }
      }
    }
  }

  // phase 5: dQ = dS K (A strided from dS^T, B row-major K)
  for (int m0 = wid * 16; m0 < L; m0 += (blockDim.x >> 6) << 4) {
    cfrag acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = cfrag{0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < Lpad / 32; ++kk) {
      bfrag ads;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        reinterpret_cast<bf16*>(&ads)[e] =
            pt_s[(long)(kk * 32 + ((lane >> 4) << 3) + e) * ls + m0 +
                 (lane & 15)];
#pragma unroll
      for (int nd = 0; nd < 4; ++nd)
        if (nd < NFD)
          acc[nd] = mfma16(ads, lds_fragB_rowmajor(k_s, kk * 32, ds, nd * 16),
                           acc[nd]);
    }
#pragma unroll
    for (int nd = 0; nd < 4; ++nd) {
      if (nd < NFD) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + ((lane >> 4) << 2) + r;
          if (row < L)
            dq[qb + (long)row * q_rs + nd * 16 + (lane & 15)] =
                __float2bfloat16(acc[nd][r]);
        }
      }
    }
  }
}

// ===================================================================== host
struct AttnShape {
  int B, H, L, D, Lpad;
};

static AttnShape attn_shape(int B, int H, int L, int D) {
  TORCH_CHECK(D == 32 || D == 64, "attention: head dim must be 32 or 64 "
              "(pad in the wrapper), got ", D);
  const int Lpad = ((L + 31) / 32) * 32;
  TORCH_CHECK(Lpad <= LPAD_MAX,
              "attention: seq len > 176 unsupported by the full-LDS kernel");
  return {B, H, L, D, Lpad};
}


// bank-conflict-free LDS strides: pad so stride_bytes/16 is odd
// (ld % 16 == 8 for bf16); fall back to unpadded when over 160 KiB.
static void attn_strides(int D, int Lpad, bool bwd, int& ds, int& ls,
                         size_t& smem) {
  ds = D + 8;
  ls = Lpad + 8;
  auto sz = [&](int ds_, int ls_) -> size_t {
    if (bwd)
      return (size_t)(4 * Lpad * ds_ + (long)Lpad * ls_) * sizeof(bf16)
             + 2 * Lpad * sizeof(float);
    return (size_t)(2 * Lpad * ds_ + D * ls_ + 4 * 16 * ls_) * sizeof(bf16);
  };
  smem = sz(ds, ls);
  if (smem > 160 * 1024) {  // drop padding (rare: bwd at Lpad > ~168)
    ds = D;
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
  auto s = attn_shape(q.size(0), q.size(1), q.size(2), q.size(3));
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  int ds, ls;
  size_t smem;
  attn_strides(s.D, s.Lpad, true, ds, ls, smem);
  TORCH_CHECK(smem <= 160 * 1024, "attn bwd LDS overflow");
  const long bs = (long)s.H * s.L * s.D, hs = (long)s.L * s.D, rs = s.D;
  hipLaunchKernelGGL(attn_bwd_kernel, dim3(s.B * s.H), dim3(512), smem,
                     cur_stream(q), (const bf16*)dout.data_ptr(),
                     (const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(),
                     (const bf16*)v.data_ptr(), (const bf16*)o.data_ptr(),
                     lse.data_ptr<float>(), lens.data_ptr<int>(),
                     (bf16*)dq.data_ptr(), (bf16*)dk.data_ptr(),
                     (bf16*)dv.data_ptr(), s.B, s.H, s.L, s.D, s.Lpad,
                     (float)scale, bs, hs, rs, bs, hs, rs, ds, ls,
                     (float)keep,
                     seed ? (const unsigned long long*)seed->data_ptr()
                          : nullptr);
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

std::vector<at::Tensor> attn_bwd_qkv(const at::Tensor& dout,
                                     const at::Tensor& qkv,
                                     const at::Tensor& o, const at::Tensor& lse,
                                     const at::Tensor& lens, double scale,
                                     double keep,
                                     c10::optional<at::Tensor> seed) {
  CHECK_CUDA_CONTIG(dout);
  auto s = attn_shape(qkv.size(0), qkv.size(3), qkv.size(1), qkv.size(4));
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
  hipLaunchKernelGGL(attn_bwd_kernel, dim3(s.B * s.H), dim3(512), smem,
                     cur_stream(qkv), (const bf16*)dout.data_ptr(), base,
                     base + HD, base + 2 * HD, (const bf16*)o.data_ptr(),
                     lse.data_ptr<float>(), lens.data_ptr<int>(), dbase,
                     dbase + HD, dbase + 2 * HD, s.B, s.H, s.L, s.D, s.Lpad,
                     (float)scale, q_bs, q_hs, q_rs, o_bs, o_hs, o_rs, ds, ls,
                     (float)keep,
                     seed ? (const unsigned long long*)seed->data_ptr()
                          : nullptr);
  HIP_CHECK_LAST();
  return {dqkv};
}
