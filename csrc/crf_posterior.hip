// Linear-chain CRF path posterior for 1 <= T <= 64 tags, 1 <= L <= 512:
// for a given tag path p (normally the Viterbi path) emit two [B,L] fp64
// arrays so that, for every 0 <= s <= e < len,
//
//   log P(y_s..y_e = p_s..p_e | x) = span_a[s] + span_b[e]
//
// with  span_a[t] = alpha_t(p_t) - C_t            (>= 0)
//       span_b[t] = beta_t(p_t) + C_t - logZ      (<= 0)
// and C_t the score of the path prefix 0..t. Cells at t >= len, and rows
// with len == 0, hold 0.
//
// Layout: two waves per sequence, lane = tag, tag width W (32 or 64) a
// compile-time constant as in crf_wide.hip, whose transition image and
// register copies are reused (crf_common.h). A second constant TC <= W
// (12, 24, 32 | 48, 64; T <= TC) is the number of tags a step sums over:
// with it the step has no branch on T, so its LDS reads issue back to back
// under one wait; behind a runtime `4q < T` test every read waits out its
// own latency. Cells in [T, TC) hold NEG and add exp(-huge) = 0. The even wave runs the forward
// scan, the odd wave the backward scan, concurrently: given the path they
// do not depend on each other, and at serving batch sizes the serial chain
// is the whole cost. Because the path is known neither scan keeps a table:
// each holds only its current message vector (W floats in LDS for the
// broadcast read) and at step t the lane that owns p_t files one scalar.
//
// Numerics: each scan keeps its messages relative to its own running offset
// (k_f[t] = max_i alpha_hat[t-1][i], k_b[t] = max_j (x[t+1][j] +
// beta_hat[t+1][j]); every lane holds the whole vector, so neither costs a
// cross-lane op). The scans are fp32; the offsets, the path increments and
// logZ are summed in fp64 by the finishing pass, which is also what keeps
// the large, nearly cancelling terms of span_a[s] + span_b[e] exact.
#include "crf_common.h"

namespace {

constexpr int CRFP_SEQS = 2;  // sequences per block: 2 waves each

// ---- LDS carve, shared by host and device. Offsets in floats, every
// region a multiple of 4 floats (16 B).
template <int W> struct CrfPostCarve {
  static constexpr int TRS = CrfTransImage<W>::TRS;
  static constexpr int TR_FLOATS = CrfTransImage<W>::TR_FLOATS;
  // per sequence: logZ (one double, padded to 16 B), cur_f [W], cur_b [W],
  // then path, a_p, b_p, k_f, k_b, x_p: [LP] each
  static constexpr int HEAD = 4 + 2 * W;
  static __host__ __device__ int seq_floats(int L) {
    return HEAD + 6 * round4(L);
  }
  static size_t bytes(int L) {
    return sizeof(float) * ((size_t)TR_FLOATS +
                            (size_t)CRFP_SEQS * seq_floats(L));
  }
};

// inclusive prefix sum across the wave
__device__ __forceinline__ double wave_scan_f64(double v, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const double o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

// One forward step: alpha_hat[t][j] from alpha_hat[t-1] (a, one value per
// lane) and x[t][j]; k = max_i alpha_hat[t-1][i] is the offset taken out.
template <int W, int TC>
__device__ __forceinline__ float fwd_step(float* cur_s,
                                          const float (&trc)[TC], float a,
                                          float et, bool act, int lane,
                                          float& k) {
  __builtin_amdgcn_wave_barrier();
  if (lane < W) cur_s[lane] = a;
  __builtin_amdgcn_wave_barrier();
  float v[TC];
  f32x4 m4 = {NEG, NEG, NEG, NEG}, k4 = {NEG, NEG, NEG, NEG};
#pragma unroll
  for (int q = 0; q < TC / 4; ++q) {
    const f32x4 a4 = lds_bcast4(cur_s, q);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[q * 4 + c] = a4[c] + trc[q * 4 + c];
      m4[c] = fmaxf(m4[c], v[q * 4 + c]);
      k4[c] = fmaxf(k4[c], a4[c]);
    }
  }
  const float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
  k = fmaxf(fmaxf(k4[0], k4[1]), fmaxf(k4[2], k4[3]));
  f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < TC / 4; ++q) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s4[c] += __expf(v[q * 4 + c] - m);
  }
  const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
  return act ? (m - k) + __logf(s) + et : NEG;
}

// One backward step: beta_hat[t][i] from cur[jj] = x[t+1][jj] +
// beta_hat[t+1][jj]; k = max_jj cur[jj] is the offset taken out.
template <int W, int TC>
__device__ __forceinline__ float bwd_step(float* cur_s,
                                          const float (&trr)[TC], float beta,
                                          float eu, bool act, int lane,
                                          float& k) {
  const float mine = act ? eu + beta : NEG;
  __builtin_amdgcn_wave_barrier();
  if (lane < W) cur_s[lane] = mine;
  __builtin_amdgcn_wave_barrier();
  float rw[TC];  // trans[i=lane][jj] + cur[jj]
  f32x4 m4 = {NEG, NEG, NEG, NEG}, k4 = {NEG, NEG, NEG, NEG};
#pragma unroll
  for (int q = 0; q < TC / 4; ++q) {
    const f32x4 c4 = lds_bcast4(cur_s, q);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      rw[q * 4 + c] = trr[q * 4 + c] + c4[c];
      m4[c] = fmaxf(m4[c], rw[q * 4 + c]);
      k4[c] = fmaxf(k4[c], c4[c]);
    }
  }
  const float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
  k = fmaxf(fmaxf(k4[0], k4[1]), fmaxf(k4[2], k4[3]));
  f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < TC / 4; ++q) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s4[c] += __expf(rw[q * 4 + c] - m);
  }
  const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
  return act ? (m - k) + __logf(s) : NEG;
}

template <int W, int TC>
__global__ __launch_bounds__(CRFP_SEQS * 2 * WAVE) void crf_posterior_kernel(
    const float* __restrict__ emis,   // [B,L,T]
    const int* __restrict__ lens,     // [B]
    const float* __restrict__ trans,  // [T,T]
    const int* __restrict__ path,     // [B,L]
    double* __restrict__ span_a,      // [B,L]
    double* __restrict__ span_b,      // [B,L]
    int B, int L, int T) {
  using Carve = CrfPostCarve<W>;
  constexpr int TRS = Carve::TRS;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tr_s = reinterpret_cast<float*>(smem_raw);  // [W][TRS]
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int sq = wid >> 1;       // sequence slot in the block
  const bool bwd = wid & 1;      // odd wave: backward scan, span_b
  const int LP = round4(L);
  float* base = tr_s + Carve::TR_FLOATS + (size_t)sq * Carve::seq_floats(L);
  double* logz_s = reinterpret_cast<double*>(base);
  float* curf_s = base + 4;                                // [W]
  float* curb_s = curf_s + W;                              // [W]
  int* p_s = reinterpret_cast<int*>(curb_s + W);           // [LP]
  float* ap_s = reinterpret_cast<float*>(p_s) + LP;        // alpha_hat_t(p_t)
  float* bp_s = ap_s + LP;                                 // beta_hat_t(p_t)
  float* kf_s = bp_s + LP;                                 // forward offsets
  float* kb_s = kf_s + LP;                                 // backward offsets
  float* xp_s = kb_s + LP;                                 // x_t(p_t)

  const int b = blockIdx.x * CRFP_SEQS + sq;
  const bool row = b < B;
  const int n = row ? min(max(lens[b], 0), L) : 0;
  const float* e = emis + (long)(row ? b : 0) * L * T;
  {  // both waves of the pair stage the clamped path
    const int* pg = path + (long)(row ? b : 0) * L;
    for (int t = threadIdx.x & (2 * WAVE - 1); t < n; t += 2 * WAVE)
      p_s[t] = min(max(pg[t], 0), T - 1);
  }
  stage_trans<W>(tr_s, trans, T);
  __syncthreads();

  const int j = lane;  // tag owned by this lane
  const bool act = j < T;
  const int jc = lane & (W - 1);  // in-bounds LDS index for idle lanes
  double ksum = 0.0;              // sum of this wave's offsets

  if (n > 0 && !bwd) {
    // ---- forward scan ----
    float trc[TC];
    load_trans_col<W>(tr_s, jc, trc);
    float a = act ? e[j] : NEG;  // alpha_hat[0] = x_0
    if (lane == p_s[0]) {
      ap_s[0] = a;
      xp_s[0] = a;
    }
    if (lane == 0) kf_s[0] = 0.f;
    // emissions are prefetched one step ahead; a deeper ring (4 steps,
    // unrolled) measured 5-10% slower at every benchmarked shape
    float e_nxt = (act && n > 1) ? e[T + j] : 0.f;
    for (int t = 1; t < n; ++t) {
      const float et = e_nxt;
      if (act && t + 1 < n) e_nxt = e[(t + 1) * T + j];
      float k;
      a = fwd_step<W>(curf_s, trc, a, et, act, lane, k);
      if (lane == p_s[t]) {  // p_t < T: an active lane
        ap_s[t] = a;
        xp_s[t] = et;
      }
      if (lane == 0) kf_s[t] = k;
      ksum += (double)k;
    }
    // logZ = ksum + lse_j alpha_hat[n-1][j]
    const float mz = wave_reduce_max(a);
    const float sz = wave_reduce_sum(act ? __expf(a - mz) : 0.f);
    const float lse_hat = mz + __logf(sz);
    if (lane == 0) *logz_s = ksum + (double)lse_hat;
  } else if (n > 0) {
    // ---- backward scan ----
    float trr[TC];
    load_trans_row<W>(tr_s, jc, trr);
    float beta = act ? 0.f : NEG;  // beta_hat[n-1]
    if (lane == p_s[n - 1]) bp_s[n - 1] = 0.f;
    if (lane == 0) kb_s[n - 1] = 0.f;
    float e_nxt = act ? e[(n - 1) * T + j] : 0.f;
    for (int t = n - 2; t >= 0; --t) {
      const float eu = e_nxt;  // x[t+1][j]
      if (act && t > 0) e_nxt = e[t * T + j];
      float k;
      beta = bwd_step<W>(curb_s, trr, beta, eu, act, lane, k);
      if (lane == p_s[t]) bp_s[t] = beta;
      if (lane == 0) kb_s[t] = k;
      ksum += (double)k;
    }
  }
  // every wave of the block arrives here, rows past B and empty rows too
  __syncthreads();
  if (!row) return;

  // ---- finishing pass: fp64 prefix sums over t, 64 steps per round. The
  // forward wave writes span_a, the backward wave span_b; both rebuild C_t.
  double* out = (bwd ? span_b : span_a) + (long)b * L;
  const float* hat_s = bwd ? bp_s : ap_s;
  const float* k_s = bwd ? kb_s : kf_s;
  // span_b's constant: sum of all backward offsets - logZ
  const double cst = bwd ? ksum - (n > 0 ? *logz_s : 0.0) : 0.0;
  double carry_k = 0.0, carry_c = 0.0;
  for (int t0 = 0; t0 < L; t0 += WAVE) {
    const int t = t0 + lane;
    double val = 0.0;
    if (t0 < n) {  // wave-uniform
      const bool in = t < n;
      double kv = 0.0, cv = 0.0;
      if (in) {
        kv = (double)k_s[t];
        cv = (double)xp_s[t];
        if (t > 0) cv += (double)tr_s[p_s[t - 1] * TRS + p_s[t]];
      }
      const double ki = wave_scan_f64(kv, lane) + carry_k;  // sum_{u<=t} k[u]
      const double ci = wave_scan_f64(cv, lane) + carry_c;  // C_t
      carry_k = __shfl(ki, WAVE - 1);
      carry_c = __shfl(ci, WAVE - 1);
      if (in) {
        // forward:  alpha_t = alpha_hat_t + sum_{u<=t} k_f[u]
        // backward: beta_t  = beta_hat_t + sum_{u>=t} k_b[u]
        const double off = bwd ? (cst - (ki - kv)) + ci : ki - ci;
        val = (double)hat_s[t] + off;
      }
    }
    if (t < L) out[t] = val;
  }
}

template <int W, int TC>
void launch_posterior(const at::Tensor& emissions, const at::Tensor& lens,
                      const at::Tensor& trans, const at::Tensor& path,
                      at::Tensor& span_a, at::Tensor& span_b, int B, int L,
                      int T) {
  hipLaunchKernelGGL((crf_posterior_kernel<W, TC>),
                     dim3((B + CRFP_SEQS - 1) / CRFP_SEQS),
                     dim3(CRFP_SEQS * 2 * WAVE), CrfPostCarve<W>::bytes(L),
                     cur_stream(emissions), emissions.data_ptr<float>(),
                     lens.data_ptr<int>(), trans.data_ptr<float>(),
                     path.data_ptr<int>(), span_a.data_ptr<double>(),
                     span_b.data_ptr<double>(), B, L, T);
  HIP_CHECK_LAST();
}

}  // namespace

// ===================================================================== host
std::vector<at::Tensor> crf_path_posterior(const at::Tensor& emissions,
                                           const at::Tensor& lens,
                                           const at::Tensor& trans,
                                           const at::Tensor& path) {
  CHECK_CUDA_CONTIG(emissions);
  CHECK_CUDA_CONTIG(lens);
  CHECK_CUDA_CONTIG(trans);
  CHECK_CUDA_CONTIG(path);
  TORCH_CHECK(emissions.dim() == 3, "CRF: emissions must be [B,L,T]");
  TORCH_CHECK(emissions.scalar_type() == at::kFloat &&
                  trans.scalar_type() == at::kFloat &&
                  lens.scalar_type() == at::kInt &&
                  path.scalar_type() == at::kInt,
              "CRF: emissions/transitions must be float32, lens/path int32");
  const int B = emissions.size(0), L = emissions.size(1), T = emissions.size(2);
  check_wide_range(L, T);
  TORCH_CHECK(path.numel() == (int64_t)B * L && lens.numel() == B &&
                  trans.numel() == (int64_t)T * T,
              "CRF: path/lens/transitions do not match emissions");
  // the kernel writes every cell, so no memset node ahead of it
  auto span_a = at::empty({B, L}, emissions.options().dtype(at::kDouble));
  auto span_b = at::empty({B, L}, emissions.options().dtype(at::kDouble));
  if (B == 0) return {span_a, span_b};
#define CRFP_LAUNCH(W, TC) \
  launch_posterior<W, TC>(emissions, lens, trans, path, span_a, span_b, B, L, T)
  if (T <= 12)
    CRFP_LAUNCH(32, 12);
  else if (T <= 24)
    CRFP_LAUNCH(32, 24);
  else if (T <= 32)
    CRFP_LAUNCH(32, 32);
  else if (T <= 48)
    CRFP_LAUNCH(64, 48);
  else
    CRFP_LAUNCH(64, 64);
#undef CRFP_LAUNCH
  return {span_a, span_b};
}
