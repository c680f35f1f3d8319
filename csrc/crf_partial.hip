// Partial-annotation (constrained) linear-chain CRF for 1 <= T <= 64 tags
// and 1 <= L <= 512 tokens: every position carries a set of allowed tags as
// one 64-bit word, and
//
//   ll[b] = log Z_allowed - log Z            (<= 0)
//   demis = P_S(y_t = j) - P(y_t = j)
//   dtrans[b] = E_S[pairs] - E[pairs]
//
// with Z_allowed / P_S taken over the paths that stay inside the sets. Bits
// at or above T are ignored; a word with no bit below T set stands for all
// T tags. Empty rows give 0 everywhere, cells at t >= len are 0.
//
// Layout: crf_wide.hip's forward-backward scan (one wave per scan, lane =
// tag, W = 32 / 64 at compile time, alpha and beta relative to the running
// offset k[t], the offsets summed in fp64), with crf_posterior.hip's second
// constant TC (12, 24, 32 | 48, 64; T <= TC): a step sums over exactly TC
// tags and has no branch on T. The alpha rows therefore have stride TC and
// their cells in [T, TC) hold NEG.
//
// Masking is a select: a lane whose bit is clear gets alpha = NEG (forward)
// or an e + beta term of NEG (backward), assigned, never added to. The free
// scan is the same code with an all-ones word, so on a row whose words are
// all open both scans execute the same arithmetic and their difference is
// exactly 0.
//
// A scan parks its marginal row t in the alpha row it has just consumed
// (row t is dead after backward step t), and its expected pair counts in a
// [T][TRS] tile over the alpha region once the marginals have been read.
//
// Two routes (CrfPartialRoute):
//   pair   one launch; waves 2s and 2s+1 of a block scan one sequence, free
//          and constrained, each in its own alpha region. After a block
//          barrier both write demis = P_S - P from LDS, every cell once and
//          coalesced; dtrans and ll likewise, the two logZ subtracted in
//          fp64.
//   split  (a pair's two alpha regions do not fit LDS: W = 64 at long L) the
//          kernel in single-scan mode, launched twice on the stream: pass 0
//          writes the free scan's -P, -E[pairs] and its fp64 logZ, pass 1
//          adds the constrained scan's terms with plain loads and stores.
// No atomics; every output cell is written, so the outputs are not zeroed.
//
// Transitions that leave an allowed set without a finite-score path
// (-1e4-style hard constraints) give a finite but meaningless result.
#include "crf_common.h"

namespace {

constexpr size_t CRFC_LDS_BYTES = 160 * 1024;
constexpr int CRFC_THREADS = 256;

// ---- LDS carve, shared by host and device. Offsets in floats, every region
// a multiple of 4 floats (16 B).
template <int W, int TC> struct CrfPartialCarve {
  static constexpr int TRS = CrfTransImage<W>::TRS;
  static constexpr int TR_FLOATS = CrfTransImage<W>::TR_FLOATS;
  // per wave: logZ (one double, padded to 16 B), cur [W], k [LP], then
  // alpha [L][TC], reused for the marginals and then the [T][TRS] pair tile
  static constexpr int HEAD = 4 + W;
  static __host__ __device__ int alpha_floats(int L) {
    const int a = L * TC, g = TR_FLOATS;
    return a > g ? a : g;
  }
  static __host__ __device__ int wave_floats(int L) {
    return HEAD + round4(L) + alpha_floats(L);
  }
  static size_t bytes(int nw, int L) {
    return sizeof(float) * ((size_t)TR_FLOATS + (size_t)nw * wave_floats(L));
  }
};

// The one place that picks the route: the pair route at the most of 2, 1
// pairs per block that fit; where not even one pair fits, single scans at
// one wave per block (two waves would need the bytes of a pair).
template <int W, int TC> struct CrfPartialRoute {
  bool pair = false;
  int nw = 1;
  size_t smem = 0;
  explicit CrfPartialRoute(int L) {
    using Carve = CrfPartialCarve<W, TC>;
    for (int w = CRFC_THREADS / WAVE; w >= 2 && !pair; w >>= 1) {
      if (Carve::bytes(w, L) <= CRFC_LDS_BYTES) {
        pair = true;
        nw = w;
      }
    }
    smem = Carve::bytes(nw, L);
    TORCH_CHECK(smem <= CRFC_LDS_BYTES, "CRF partial: LDS overflow (", smem,
                " bytes at one wave)");
  }
};

// Is this lane's tag in the allowed set of position t? A lane tests its own
// bit; the free scan (con == false) reads no word at all.
__device__ __forceinline__ bool tag_open(const unsigned long long* wd, int t,
                                         bool con, unsigned long long tmask,
                                         int lane) {
  unsigned long long w = ~0ull;
  if (con) {
    w = wd[t] & tmask;
    if (w == 0ull) w = ~0ull;  // nothing known: all tags
  }
  return (w >> lane) & 1ull;
}

template <int W, int TC, bool PAIR>
__global__ __launch_bounds__(CRFC_THREADS) void crf_partial_kernel(
    const float* __restrict__ emis,                 // [B,L,T]
    const unsigned long long* __restrict__ allowed,  // [B,L]
    const int* __restrict__ lens,                   // [B]
    const float* __restrict__ trans,                // [T,T]
    float* __restrict__ ll,                         // [B]
    float* __restrict__ demis,                      // [B,L,T]
    float* __restrict__ dtrans,                     // [B,T,T]
    double* __restrict__ logz_g,  // [B] free logZ between the split passes
    int pass,                     // split route: 0 free scan, 1 constrained
    int B, int L, int T) {
  using Carve = CrfPartialCarve<W, TC>;
  constexpr int TRS = Carve::TRS;
  constexpr int G = PAIR ? 2 : 1;  // waves per sequence
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tr_s = reinterpret_cast<float*>(smem_raw);  // [W][TRS]
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int nw = blockDim.x / WAVE;
  const int LP = round4(L);
  const int wf = Carve::wave_floats(L);
  float* base = tr_s + Carve::TR_FLOATS + (size_t)wid * wf;
  double* logz_s = reinterpret_cast<double*>(base);
  float* cur_s = base + 4;       // [W]
  float* k_s = cur_s + W;        // [LP]
  float* alpha = k_s + LP;       // [L][TC]
  const bool con = PAIR ? (wid & 1) : (pass != 0);  // constrained scan?

  const int b = blockIdx.x * (nw / G) + wid / G;
  const bool row = b < B;
  const int n = row ? min(max(lens[b], 0), L) : 0;
  const float* e = emis + (long)(row ? b : 0) * L * T;
  const unsigned long long* wd = allowed + (long)(row ? b : 0) * L;
  const unsigned long long tmask = T >= 64 ? ~0ull : ((1ull << T) - 1ull);
  stage_trans<W>(tr_s, trans, T);
  __syncthreads();

  const int j = lane;  // tag owned by this lane
  const bool act = j < T;
  const int jc = lane & (W - 1);  // in-bounds LDS index for idle lanes
  float exp_row[TC];  // lane i: sum_t P(y_t=i, y_{t+1}=jj) of this scan
#pragma unroll
  for (int q = 0; q < TC; ++q) exp_row[q] = 0.f;
  double logz = 0.0;

  if (n > 0) {
    // ---- forward scan: alpha_hat[t][:] in LDS, closed tags and the pad
    // cells [T,TC) = NEG ----
    bool ok = act && tag_open(wd, 0, con, tmask, lane);
    float a = ok ? e[j] : NEG;
    if (lane < TC) alpha[lane] = a;
    float e_nxt = 0.f;
    bool ok_nxt = false;
    if (n > 1) {
      ok_nxt = act && tag_open(wd, 1, con, tmask, lane);
      if (act) e_nxt = e[T + j];
    }
    double ksum = 0.0;  // sum of the offsets taken out of alpha
    {
      float trc[TC];  // this lane's column of the transitions
      load_trans_col<W>(tr_s, jc, trc);
      for (int t = 1; t < n; ++t) {
        const float et = e_nxt;
        ok = ok_nxt;
        if (t + 1 < n) {
          ok_nxt = act && tag_open(wd, t + 1, con, tmask, lane);
          if (act) e_nxt = e[(t + 1) * T + j];
        }
        __builtin_amdgcn_wave_barrier();
        const float* ap = alpha + (t - 1) * TC;
        float v[TC];
        f32x4 m4 = {NEG, NEG, NEG, NEG}, k4 = {NEG, NEG, NEG, NEG};
#pragma unroll
        for (int q = 0; q < TC / 4; ++q) {
          const f32x4 a4 = lds_bcast4(ap, q);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            v[q * 4 + c] = a4[c] + trc[q * 4 + c];
            m4[c] = fmaxf(m4[c], v[q * 4 + c]);
            k4[c] = fmaxf(k4[c], a4[c]);
          }
        }
        const float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
        const float k = fmaxf(fmaxf(k4[0], k4[1]), fmaxf(k4[2], k4[3]));
        f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < TC / 4; ++q) {
#pragma unroll
          for (int c = 0; c < 4; ++c) s4[c] += __expf(v[q * 4 + c] - m);
        }
        const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        a = ok ? (m - k) + __logf(s) + et : NEG;
        if (lane < TC) alpha[t * TC + lane] = a;
        if (lane == 0) k_s[t] = k;
        ksum += (double)k;
      }
    }
    // logZ = ksum + lse_j alpha_hat[n-1][j]
    const float mz = wave_reduce_max(a);
    const float sz = wave_reduce_sum(act ? __expf(a - mz) : 0.f);
    const float lse_hat = mz + __logf(sz);
    logz = ksum + (double)lse_hat;

    // ---- backward scan; marginal row t parked in alpha row t ----
    __builtin_amdgcn_wave_barrier();
    if (act) alpha[(n - 1) * TC + j] = __expf(a - lse_hat);
    float beta = 0.f;  // beta_hat[n-1][j]
    float trr[TC];     // this lane's row of the transitions
    load_trans_row<W>(tr_s, jc, trr);
    bool ok_u = ok;  // tag j open at t+1?
    e_nxt = act ? e[(n - 1) * T + j] : 0.f;
    for (int t = n - 2; t >= 0; --t) {
      // cur[jj] = e[t+1][jj] + beta_hat[t+1][jj], staged for a broadcast
      // read; NEG where jj is closed at t+1
      const float mine = ok_u ? e_nxt + beta : NEG;
      if (t > 0) {
        ok_u = act && tag_open(wd, t, con, tmask, lane);
        if (act) e_nxt = e[t * T + j];
      }
      __builtin_amdgcn_wave_barrier();
      if (lane < W) cur_s[lane] = mine;
      __builtin_amdgcn_wave_barrier();
      const float k = k_s[t + 1];
      // lane = i here; lanes past the row read nothing
      const float a_ti = lane < TC ? alpha[t * TC + lane] : NEG;
      float rw[TC];  // trans[i=lane][jj] + cur[jj], then exp(. - m)
      f32x4 m4 = {NEG, NEG, NEG, NEG};
#pragma unroll
      for (int q = 0; q < TC / 4; ++q) {
        const f32x4 c4 = lds_bcast4(cur_s, q);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          rw[q * 4 + c] = trr[q * 4 + c] + c4[c];
          m4[c] = fmaxf(m4[c], rw[q * 4 + c]);
        }
      }
      const float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < TC / 4; ++q) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          rw[q * 4 + c] = __expf(rw[q * 4 + c] - m);
          s4[c] += rw[q * 4 + c];
        }
      }
      const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      const float beta_t = act ? (m - k) + __logf(s) : NEG;  // beta_hat[t][i]
      // P(y_t=i, y_{t+1}=jj) = exp(alpha_hat[t][i] + m - k - lse_hat) * rw[jj]
      // (alpha_hat = NEG where i is closed at t: exp gives 0)
      const float cf = act ? __expf(a_ti + (m - k) - lse_hat) : 0.f;
#pragma unroll
      for (int q = 0; q < TC; ++q) exp_row[q] += cf * rw[q];
      if (act) alpha[t * TC + j] = __expf(a_ti + beta_t - lse_hat);
      beta = beta_t;
    }
  }
  if (PAIR && lane == 0) *logz_s = logz;
  // every wave of the block reaches the three barriers below, rows past B
  // and empty rows too
  __syncthreads();

  // the even wave's regions of this sequence (pair route: the free scan)
  float* base_f = PAIR ? base - (size_t)(wid & 1) * wf : base;
  const float* mg_f = base_f + Carve::HEAD + LP;  // free marginals / tile
  const float* mg_s = mg_f + wf;                  // constrained ones (PAIR)
  const int pl = PAIR ? (wid & 1) * WAVE + lane : lane;  // thread of the group
  if (row) {
    float* de = demis + (long)b * L * T;
    const int cells = L * T, live = n * T;
    for (int c = pl; c < cells; c += G * WAVE) {
      if (PAIR) {
        float v = 0.f;
        if (c < live) {
          const int t = c / T, jj = c - t * T;
          v = mg_s[t * TC + jj] - mg_f[t * TC + jj];
        }
        de[c] = v;
      } else if (c < live) {
        const int t = c / T, jj = c - t * T;
        const float p = alpha[t * TC + jj];
        de[c] = pass ? de[c] + p : -p;
      } else if (!pass) {
        de[c] = 0.f;
      }
    }
  }
  __syncthreads();
  // ---- expected pair counts through an LDS tile in the (now dead) alpha
  // region, so the global store is coalesced ----
  if (n > 0 && act) {
#pragma unroll
    for (int q = 0; q < TC; ++q) {
      if (q < T) alpha[j * TRS + q] = exp_row[q];
    }
  }
  __syncthreads();
  if (row) {
    float* dt = dtrans + (long)b * T * T;
    const int cells = T * T;
    for (int c = pl; c < cells; c += G * WAVE) {
      const int r = c / T, jj = c - r * T;
      if (PAIR) {
        dt[c] = n > 0 ? mg_s[r * TRS + jj] - mg_f[r * TRS + jj] : 0.f;
      } else if (n > 0) {
        const float g = alpha[r * TRS + jj];
        dt[c] = pass ? dt[c] + g : -g;
      } else if (!pass) {
        dt[c] = 0.f;
      }
    }
    if (pl == 0) {
      if (PAIR) {
        const double zf = *reinterpret_cast<const double*>(base_f);
        const double zs = *reinterpret_cast<const double*>(base_f + wf);
        ll[b] = (float)(zs - zf);  // empty row: 0 - 0
      } else if (pass) {
        ll[b] = (float)(logz - logz_g[b]);
      } else {
        logz_g[b] = logz;
      }
    }
  }
}

template <int W, int TC>
void launch_partial(const at::Tensor& emissions, const at::Tensor& allowed,
                    const at::Tensor& lens, const at::Tensor& trans,
                    at::Tensor& ll, at::Tensor& demis, at::Tensor& dtrans,
                    int B, int L, int T) {
  const CrfPartialRoute<W, TC> rt(L);
  const auto* wd =
      reinterpret_cast<const unsigned long long*>(allowed.data_ptr<int64_t>());
  if (rt.pair) {
    const int seqs = rt.nw / 2;
    hipLaunchKernelGGL((crf_partial_kernel<W, TC, true>),
                       dim3((B + seqs - 1) / seqs), dim3(rt.nw * WAVE),
                       rt.smem, cur_stream(emissions),
                       emissions.data_ptr<float>(), wd, lens.data_ptr<int>(),
                       trans.data_ptr<float>(), ll.data_ptr<float>(),
                       demis.data_ptr<float>(), dtrans.data_ptr<float>(),
                       (double*)nullptr, 0, B, L, T);
    HIP_CHECK_LAST();
    return;
  }
  // stream order is the only synchronisation between the two passes
  auto logz = at::empty({B}, emissions.options().dtype(at::kDouble));
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL((crf_partial_kernel<W, TC, false>),
                       dim3((B + rt.nw - 1) / rt.nw), dim3(rt.nw * WAVE),
                       rt.smem, cur_stream(emissions),
                       emissions.data_ptr<float>(), wd, lens.data_ptr<int>(),
                       trans.data_ptr<float>(), ll.data_ptr<float>(),
                       demis.data_ptr<float>(), dtrans.data_ptr<float>(),
                       logz.data_ptr<double>(), pass, B, L, T);
    HIP_CHECK_LAST();
  }
}

// (W, TC) of a label size: the scanned width is the least of 12, 24, 32 |
// 48, 64 that holds T
#define CRFC_DISPATCH(T, X) \
  do {                      \
    if ((T) <= 12)          \
      X(32, 12);            \
    else if ((T) <= 24)     \
      X(32, 24);            \
    else if ((T) <= 32)     \
      X(32, 32);            \
    else if ((T) <= 48)     \
      X(64, 48);            \
    else                    \
      X(64, 64);            \
  } while (0)

}  // namespace

// ===================================================================== host
std::vector<at::Tensor> crf_partial_fwd(const at::Tensor& emissions,
                                        const at::Tensor& allowed,
                                        const at::Tensor& lens,
                                        const at::Tensor& trans) {
  CHECK_CUDA_CONTIG(emissions);
  CHECK_CUDA_CONTIG(allowed);
  CHECK_CUDA_CONTIG(lens);
  CHECK_CUDA_CONTIG(trans);
  TORCH_CHECK(emissions.dim() == 3, "CRF: emissions must be [B,L,T]");
  TORCH_CHECK(emissions.scalar_type() == at::kFloat &&
                  trans.scalar_type() == at::kFloat &&
                  lens.scalar_type() == at::kInt &&
                  allowed.scalar_type() == at::kLong,
              "CRF: emissions/transitions must be float32, lens int32, "
              "allowed int64");
  const int B = emissions.size(0), L = emissions.size(1), T = emissions.size(2);
  check_wide_range(L, T);
  TORCH_CHECK(allowed.numel() == (int64_t)B * L && lens.numel() == B &&
                  trans.numel() == (int64_t)T * T,
              "CRF: allowed/lens/transitions do not match emissions");
  // the kernel writes every cell, so no memset node ahead of it
  auto ll = at::empty({B}, emissions.options());
  auto demis = at::empty_like(emissions);
  auto dtrans = at::empty({B, T, T}, emissions.options());
  if (B == 0) return {ll, demis, dtrans};
#define CRFC_LAUNCH(W, TC) \
  launch_partial<W, TC>(emissions, allowed, lens, trans, ll, demis, dtrans, \
                        B, L, T)
  CRFC_DISPATCH(T, CRFC_LAUNCH);
#undef CRFC_LAUNCH
  return {ll, demis, dtrans};
}

// {pair route (1) or split (0), waves per block, LDS bytes} of that launch
std::vector<int64_t> crf_partial_route(int64_t L, int64_t T) {
  check_wide_range((int)L, (int)T);
  std::vector<int64_t> out;
#define CRFC_ROUTE(W, TC)                                \
  do {                                                   \
    const CrfPartialRoute<W, TC> rt((int)L);             \
    out = {rt.pair ? 1 : 0, rt.nw, (int64_t)rt.smem};    \
  } while (0)
  CRFC_DISPATCH(T, CRFC_ROUTE);
#undef CRFC_ROUTE
  return out;
}
