// Wide-tagset linear-chain CRF: forward-backward (loss + analytic grads)
// and Viterbi decode for 1 <= T <= 64 tags and 1 <= L <= 512 tokens.
// crf.hip routes here every shape its own kernels cannot launch (T > 20,
// or T <= 20 whose alpha does not fit LDS at four waves per block).
//
// Layout: one wave per sequence, lane = tag, tag width W (32 or 64) is a
// compile-time constant so the per-lane row[] / exp_row[] arrays unroll
// into registers. The transition matrix is staged once per block in LDS
// at a row stride of W+1 floats (pad cells = NEG): tr[i][lane] is
// contiguous across lanes and tr[lane][jj] lands on bank (lane+jj)%32,
// so both reads are conflict-free inside a 32-lane group. Each wave then
// keeps its own column and row of it in registers for the whole scan.
//
// Numerics: alpha and beta are stored relative to a running offset
// k[t] = max_i alpha_hat[t-1][i] (every lane already holds that whole row,
// so k costs no cross-lane op). The same k[t] is subtracted from beta, so
// the offsets cancel term by term in the marginals and never appear in
// them; only logZ adds them up, in fp64. Without this alpha reaches ~2.7e3
// at L=512, T=64 and its fp32 ulp (2.4e-4 per step) shows in the grads.
#include "crf_common.h"

namespace {

constexpr size_t CRFW_LDS_BYTES = 160 * 1024;

// ---- LDS carve, shared by host and device so the byte count lives in
// one place. All offsets are multiples of 4 floats (16 B).
template <int W> struct CrfWideCarve {
  static constexpr int TRS = CrfTransImage<W>::TRS;
  static constexpr int TR_FLOATS = CrfTransImage<W>::TR_FLOATS;
  // fwd, per wave: alpha [L][TP] (reused as the [T][TRS] dtrans tile once
  // the backward scan is done), cur [W], k [LP], tags [LP]
  static __host__ __device__ int alpha_floats(int L, int T) {
    const int a = L * round4(T), g = TR_FLOATS;
    return a > g ? a : g;
  }
  static __host__ __device__ int fwd_wave_floats(int L, int T) {
    return alpha_floats(L, T) + W + 2 * round4(L);
  }
  static size_t fwd_bytes(int nw, int L, int T) {
    return sizeof(float) * ((size_t)TR_FLOATS +
                            (size_t)nw * fwd_wave_floats(L, T));
  }
  // viterbi, per wave: delta [W] floats, backpointers [L][W] bytes
  static __host__ __device__ int vit_wave_bytes(int L) {
    return W * (int)sizeof(float) + ((L * W + 15) & ~15);
  }
  static size_t vit_bytes(int nw, int L) {
    return sizeof(float) * (size_t)TR_FLOATS + (size_t)nw * vit_wave_bytes(L);
  }
};

// ------------------------------------------------------------------ fwd
template <int W>
__global__ __launch_bounds__(256) void crf_wide_fwd_kernel(
    const float* __restrict__ emis,   // [B,L,T]
    const int* __restrict__ tags,     // [B,L]
    const int* __restrict__ lens,     // [B]
    const float* __restrict__ trans,  // [T,T]
    float* __restrict__ ll,           // [B] zeroed
    float* __restrict__ demis,        // [B,L,T] zeroed
    float* __restrict__ dtrans,       // [B,T,T] zeroed
    int B, int L, int T) {
  using Carve = CrfWideCarve<W>;
  constexpr int TRS = Carve::TRS;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tr_s = reinterpret_cast<float*>(smem_raw);  // [W][TRS]
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int nw = blockDim.x / WAVE;
  const int TP = round4(T), LP = round4(L);
  float* alpha = tr_s + Carve::TR_FLOATS +
                 (size_t)wid * Carve::fwd_wave_floats(L, T);  // [L][TP]
  float* cur_s = alpha + Carve::alpha_floats(L, T);           // [W]
  float* k_s = cur_s + W;                                     // [LP]
  int* tg_s = reinterpret_cast<int*>(k_s + LP);               // [LP]
  stage_trans<W>(tr_s, trans, T);
  __syncthreads();

  const int b = blockIdx.x * nw + wid;
  if (b >= B) return;
  const int n = min(lens[b], L);
  if (n <= 0) return;
  const float* e = emis + (long)b * L * T;
  const int* tg = tags + (long)b * L;
  const int j = lane;  // tag owned by this lane
  const bool act = j < T;
  const int jc = lane & (W - 1);  // in-bounds LDS index for idle lanes

  // this lane's column of the transitions, held for the forward scan
  float trc[W];
  load_trans_col<W>(tr_s, jc, trc);
  for (int t = lane; t < n; t += WAVE) tg_s[t] = min(max(tg[t], 0), T - 1);

  // ---- forward scan: alpha_hat[t][:] in LDS, pad cells [T,TP) = NEG ----
  float a = act ? e[j] : NEG;
  if (lane < TP) alpha[lane] = a;
  float e_nxt = (act && n > 1) ? e[T + j] : 0.f;
  double ksum = 0.0;  // sum of the offsets taken out of alpha
  for (int t = 1; t < n; ++t) {
    const float et = e_nxt;
    if (act && t + 1 < n) e_nxt = e[(t + 1) * T + j];
    __builtin_amdgcn_wave_barrier();
    const float* ap = alpha + (t - 1) * TP;
    float v[W];
    f32x4 m4 = {NEG, NEG, NEG, NEG}, k4 = {NEG, NEG, NEG, NEG};
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
      if (q * 4 < T) {
        const f32x4 a4 = lds_bcast4(ap, q);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          v[q * 4 + c] = a4[c] + trc[q * 4 + c];
          m4[c] = fmaxf(m4[c], v[q * 4 + c]);
          k4[c] = fmaxf(k4[c], a4[c]);
        }
      }
    }
    const float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    const float k = fmaxf(fmaxf(k4[0], k4[1]), fmaxf(k4[2], k4[3]));
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
      if (q * 4 < T) {
#pragma unroll
        for (int c = 0; c < 4; ++c) s4[c] += __expf(v[q * 4 + c] - m);
      }
    }
    const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    a = act ? (m - k) + __logf(s) + et : NEG;
    if (lane < TP) alpha[t * TP + lane] = a;
    if (lane == 0) k_s[t] = k;
    ksum += (double)k;
  }
  // logZ = ksum + lse_j alpha_hat[n-1][j]
  const float mz = wave_reduce_max(a);
  const float sz = wave_reduce_sum(act ? __expf(a - mz) : 0.f);
  const float lse_hat = mz + __logf(sz);

  // ---- gold score, strided over the lanes ----
  __builtin_amdgcn_wave_barrier();
  float sc = 0.f;
  for (int t = lane; t < n; t += WAVE) {
    const int c = tg_s[t];
    float x = e[t * T + c];
    if (t > 0) x += tr_s[tg_s[t - 1] * TRS + c];
    sc += x;
  }
  sc = wave_reduce_sum(sc);
  if (lane == 0) ll[b] = (float)((double)sc - (ksum + (double)lse_hat));

  // ---- backward scan + grads ----
  float* de = demis + (long)b * L * T;
  float beta = 0.f;  // beta_hat[n-1][j]
  if (act) {
    const float marg = __expf(a - lse_hat);
    de[(n - 1) * T + j] = ((j == tg_s[n - 1]) ? 1.f : 0.f) - marg;
  }
  float trr[W];      // this lane's row of the transitions
  float exp_row[W];  // lane i: sum_t P(y_t=i, y_{t+1}=jj)
  load_trans_row<W>(tr_s, jc, trr);
#pragma unroll
  for (int q = 0; q < W; ++q) exp_row[q] = 0.f;
  e_nxt = act ? e[(n - 1) * T + j] : 0.f;
  for (int t = n - 2; t >= 0; --t) {
    // cur[jj] = e[t+1][jj] + beta_hat[t+1][jj], staged for a broadcast read
    const float mine = act ? e_nxt + beta : NEG;
    if (act && t > 0) e_nxt = e[t * T + j];
    __builtin_amdgcn_wave_barrier();
    if (lane < W) cur_s[lane] = mine;
    __builtin_amdgcn_wave_barrier();
    const float k = k_s[t + 1];
    const float a_ti = alpha[t * TP + jc];  // lane = i here
    float row[W];  // trans[i=lane][jj] + cur[jj], then exp(. - m)
    f32x4 m4 = {NEG, NEG, NEG, NEG};
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
      if (q * 4 < T) {
        const f32x4 c4 = lds_bcast4(cur_s, q);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          row[q * 4 + c] = trr[q * 4 + c] + c4[c];
          m4[c] = fmaxf(m4[c], row[q * 4 + c]);
        }
      }
    }
    const float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
      if (q * 4 < T) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          row[q * 4 + c] = __expf(row[q * 4 + c] - m);
          s4[c] += row[q * 4 + c];
        }
      }
    }
    const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    const float beta_t = act ? (m - k) + __logf(s) : NEG;  // beta_hat[t][i]
    // P(y_t=i, y_{t+1}=jj) = exp(alpha_hat[t][i] + m - k - lse_hat) * row[jj]
    const float cf = act ? __expf(a_ti + (m - k) - lse_hat) : 0.f;
#pragma unroll
    for (int q = 0; q < W; ++q) {
      if ((q & ~3) < T) exp_row[q] += cf * row[q];
    }
    if (act) {
      const float marg = __expf(a_ti + beta_t - lse_hat);
      de[t * T + j] = ((j == tg_s[t]) ? 1.f : 0.f) - marg;
    }
    beta = beta_t;
  }

  // ---- dtrans[b] = gold pair counts - expected, through an LDS tile in
  // the (now dead) alpha region so the global store is coalesced ----
  __builtin_amdgcn_wave_barrier();
  float* g_s = alpha;  // [T][TRS]
  if (act) {
#pragma unroll
    for (int q = 0; q < W; ++q) {
      if (q < T) g_s[j * TRS + q] = -exp_row[q];
    }
  }
  __builtin_amdgcn_wave_barrier();
  for (int t = 1; t < n; ++t) {  // row tg[t-1] belongs to lane tg[t-1]
    const int pi = tg_s[t - 1];
    if (lane == pi) g_s[pi * TRS + tg_s[t]] += 1.f;
  }
  __builtin_amdgcn_wave_barrier();
  float* dt = dtrans + (long)b * T * T;
  if (act) {
    for (int r = 0; r < T; ++r) dt[r * T + j] = g_s[r * TRS + j];
  }
}

// -------------------------------------------------------------- viterbi
template <int W>
__global__ __launch_bounds__(256) void crf_wide_viterbi_kernel(
    const float* __restrict__ emis, const int* __restrict__ lens,
    const float* __restrict__ trans,
    int* __restrict__ pred,  // [B,L] zeroed
    int B, int L, int T) {
  using Carve = CrfWideCarve<W>;
  constexpr int TRS = Carve::TRS;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tr_s = reinterpret_cast<float*>(smem_raw);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int nw = blockDim.x / WAVE;
  char* wbase = smem_raw + Carve::TR_FLOATS * sizeof(float) +
                (size_t)wid * Carve::vit_wave_bytes(L);
  float* dl_s = reinterpret_cast<float*>(wbase);                     // [W]
  unsigned char* bp = reinterpret_cast<unsigned char*>(dl_s + W);  // [L][W]
  stage_trans<W>(tr_s, trans, T);
  __syncthreads();

  const int b = blockIdx.x * nw + wid;
  if (b >= B) return;
  const int n = min(lens[b], L);
  if (n <= 0) return;
  const float* e = emis + (long)b * L * T;
  const int j = lane;
  const bool act = j < T;
  const int jc = lane & (W - 1);
  float trc[W];
  load_trans_col<W>(tr_s, jc, trc);

  float delta = act ? e[j] : NEG;  // delta[0][j]
  float e_nxt = (act && n > 1) ? e[T + j] : 0.f;
  for (int t = 1; t < n; ++t) {
    const float et = e_nxt;
    if (act && t + 1 < n) e_nxt = e[(t + 1) * T + j];
    __builtin_amdgcn_wave_barrier();
    if (lane < W) dl_s[lane] = delta;
    __builtin_amdgcn_wave_barrier();
    // four contiguous index blocks scanned independently, then merged in
    // index order with a strict '>' so the first maximum wins
    float best[4];
    int arg[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      best[h] = NEG;
      arg[h] = h * (W / 4);
#pragma unroll
      for (int q = h * (W / 16); q < (h + 1) * (W / 16); ++q) {
        if (q * 4 < T) {
          const f32x4 d4 = lds_bcast4(dl_s, q);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float v = d4[c] + trc[q * 4 + c];
            if (v > best[h]) {
              best[h] = v;
              arg[h] = q * 4 + c;
            }
          }
        }
      }
    }
    float bst = best[0];
    int ag = arg[0];
#pragma unroll
    for (int h = 1; h < 4; ++h) {
      if (best[h] > bst) {
        bst = best[h];
        ag = arg[h];
      }
    }
    delta = act ? bst + et : NEG;
    if (act) bp[t * W + j] = (unsigned char)ag;
  }
  // argmax over lanes
  float bv = delta;
  int barg = act ? j : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int oa = __shfl_xor(barg, off);
    if (ov > bv) {
      bv = ov;
      barg = oa;
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) {
    int* pr = pred + (long)b * L;
    // clamp: non-finite emissions must not turn into out-of-bounds
    // backtraces
    int cur = min(max(barg, 0), T - 1);
    pr[n - 1] = cur;
    for (int t = n - 2; t >= 0; --t) {
      cur = min(max((int)bp[(t + 1) * W + cur], 0), T - 1);
      pr[t] = cur;
    }
  }
}

// waves per block: the most of 4, 2, 1 whose LDS fits
template <typename BytesFn> int pick_waves(BytesFn bytes, size_t* smem) {
  for (int nw = 4; nw >= 1; nw >>= 1) {
    *smem = bytes(nw);
    if (*smem <= CRFW_LDS_BYTES) return nw;
  }
  TORCH_CHECK(false, "CRF wide: LDS overflow (", *smem, " bytes at one wave)");
  return 0;
}

template <int W>
void launch_fwd(const at::Tensor& emissions, const at::Tensor& tags,
                const at::Tensor& lens, const at::Tensor& trans,
                at::Tensor& ll, at::Tensor& demis, at::Tensor& dtrans, int B,
                int L, int T) {
  size_t smem = 0;
  const int nw = pick_waves(
      [&](int w) { return CrfWideCarve<W>::fwd_bytes(w, L, T); }, &smem);
  hipLaunchKernelGGL(crf_wide_fwd_kernel<W>, dim3((B + nw - 1) / nw),
                     dim3(nw * WAVE), smem, cur_stream(emissions),
                     emissions.data_ptr<float>(), tags.data_ptr<int>(),
                     lens.data_ptr<int>(), trans.data_ptr<float>(),
                     ll.data_ptr<float>(), demis.data_ptr<float>(),
                     dtrans.data_ptr<float>(), B, L, T);
  HIP_CHECK_LAST();
}

template <int W>
void launch_viterbi(const at::Tensor& emissions, const at::Tensor& lens,
                    const at::Tensor& trans, at::Tensor& pred, int B, int L,
                    int T) {
  size_t smem = 0;
  const int nw = pick_waves(
      [&](int w) { return CrfWideCarve<W>::vit_bytes(w, L); }, &smem);
  hipLaunchKernelGGL(crf_wide_viterbi_kernel<W>, dim3((B + nw - 1) / nw),
                     dim3(nw * WAVE), smem, cur_stream(emissions),
                     emissions.data_ptr<float>(), lens.data_ptr<int>(),
                     trans.data_ptr<float>(), pred.data_ptr<int>(), B, L, T);
  HIP_CHECK_LAST();
}

}  // namespace

// ===================================================================== host
std::vector<at::Tensor> crf_wide_fwd(const at::Tensor& emissions,
                                     const at::Tensor& tags,
                                     const at::Tensor& lens,
                                     const at::Tensor& trans) {
  CHECK_CUDA_CONTIG(emissions);
  CHECK_CUDA_CONTIG(tags);
  CHECK_CUDA_CONTIG(lens);
  CHECK_CUDA_CONTIG(trans);
  TORCH_CHECK(emissions.dim() == 3, "CRF: emissions must be [B,L,T]");
  const int B = emissions.size(0), L = emissions.size(1), T = emissions.size(2);
  check_wide_range(L, T);
  TORCH_CHECK(tags.numel() == (int64_t)B * L && lens.numel() == B &&
                  trans.numel() == (int64_t)T * T,
              "CRF: tags/lens/transitions do not match emissions");
  auto ll = at::zeros({B}, emissions.options());
  auto demis = at::zeros_like(emissions);
  auto dtrans = at::zeros({B, T, T}, emissions.options());
  if (B == 0) return {ll, demis, dtrans};
  if (T <= 32)
    launch_fwd<32>(emissions, tags, lens, trans, ll, demis, dtrans, B, L, T);
  else
    launch_fwd<64>(emissions, tags, lens, trans, ll, demis, dtrans, B, L, T);
  return {ll, demis, dtrans};
}

at::Tensor crf_wide_viterbi(const at::Tensor& emissions, const at::Tensor& lens,
                            const at::Tensor& trans) {
  CHECK_CUDA_CONTIG(emissions);
  CHECK_CUDA_CONTIG(lens);
  CHECK_CUDA_CONTIG(trans);
  TORCH_CHECK(emissions.dim() == 3, "CRF: emissions must be [B,L,T]");
  const int B = emissions.size(0), L = emissions.size(1), T = emissions.size(2);
  check_wide_range(L, T);
  TORCH_CHECK(lens.numel() == B && trans.numel() == (int64_t)T * T,
              "CRF: lens/transitions do not match emissions");
  auto pred = at::zeros({B, L}, emissions.options().dtype(at::kInt));
  if (B == 0) return pred;
  if (T <= 32)
    launch_viterbi<32>(emissions, lens, trans, pred, B, L, T);
  else
    launch_viterbi<64>(emissions, lens, trans, pred, B, L, T);
  return pred;
}
