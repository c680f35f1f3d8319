// Linear-chain CRF loss and gradients for 1 <= T <= 48 tags wherever both
// scan tables of one sequence fit LDS (crf_fwd routes here; every other
// shape goes to crf_wide.hip), and the one-launch chain rule of its
// backward (crf_grad_scale).
//
//   ll[b]     = score(tags) - logZ
//   demis     = onehot(tag) - P(y_t = j)
//   dtrans[b] = gold pair counts - sum_t P(y_t = i, y_{t+1} = j)
//
// Empty rows give 0 everywhere, cells at t >= len are 0. Every output cell
// is written exactly once, so the outputs are not zeroed.
//
// Layout: crf_posterior.hip's. Two waves per sequence, lane = tag, tag
// width W (32 | 64) and scanned width TC (12, 24, 32 | 48; T <= TC) at
// compile time, so a step has no branch on T; cells in [T, TC) hold NEG.
// The even wave runs the forward scan and files alpha_hat rows in LDS as
// [L][TC]; the odd wave runs the backward scan at the same time and files
// beta_hat rows likewise. Neither depends on the other, so the serial chain
// is one scan long, not two. Each scan loads the next step's emission one
// step ahead, from a clamped address.
//
// After one block barrier every wave of the block works on the combine,
// whose depth does not depend on L but for the per-cell sum over t:
//   rows    thread = t: Z_t = lse_j(alpha_hat[t][j] + beta_hat[t][j]) in fp64
//   barrier
//   demis   flat over L*T, coalesced: exp(alpha_hat + beta_hat - Z_t)
//   dtrans  flat over T*T, thread = (i, j), summed over t in index order:
//           exp(alpha_hat[t][i] + trans[i][j] + cur[t+1][j] - Z_t - k_b[t])
//           with cur[t+1][j] = x[t+1][j] + beta_hat[t+1][j] and k_b[t] its
//           maximum over j, both exactly what the backward step saw.
//
// Numerics: each scan keeps its row relative to its own running offset,
// taken out *before* the transition is added (k = max of the incoming row;
// v = (row - k) + trans). The offsets matter only to logZ, which sums them
// in fp64. A marginal is normalised by its own row's Z_t, so neither scan's
// offsets nor logZ enter it and no error accumulates along the row; the
// pair term uses the identity sum_ij exp(alpha_hat[t][i] + trans[i][j] +
// cur[t+1][j]) = exp(Z_t + k_b[t]). Exponents are put together in fp64 from
// the stored fp32 cells and rounded once. With one tag every step is exact
// (v = trans, s = 1), every exponent is exactly 0, so marginals are exactly
// 1 and pair sums exact integers.
//
// No atomics, no scratch; bitwise reproducible.
#include "crf_common.h"

#include "crf_pair_route.h"

namespace {

template <int W, int TC>
__global__ __launch_bounds__(CRFPAIR_MAX_SEQS * 2 * WAVE) void crf_pair_kernel(
    const float* __restrict__ emis,   // [B,L,T]
    const int* __restrict__ tags,     // [B,L]
    const int* __restrict__ lens,     // [B]
    const float* __restrict__ trans,  // [T,T]
    float* __restrict__ ll,           // [B]
    float* __restrict__ demis,        // [B,L,T]
    float* __restrict__ dtrans,       // [B,T,T]
    int B, int L, int T) {
  using Carve = CrfPairCarve<W, TC>;
  constexpr int TRS = Carve::TRS;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tr_s = reinterpret_cast<float*>(smem_raw);  // [W][TRS]
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int seqs = blockDim.x / (2 * WAVE);  // sequences of this block
  const int sq = wid >> 1;                   // this wave's sequence slot
  const bool bwd = wid & 1;                  // odd wave: backward scan
  const int LP = round4(L);
  const int sf = Carve::seq_floats(L);
  float* seq0 = tr_s + Carve::TR_FLOATS;

  // regions of sequence slot s
  auto logz_of = [&](int s) { return reinterpret_cast<double*>(seq0 + (size_t)s * sf); };
  auto cur_of = [&](int s) { return seq0 + (size_t)s * sf + 4; };          // [W]
  auto z_of = [&](int s) {                                                 // [LP] fp64
    return reinterpret_cast<double*>(seq0 + (size_t)s * sf + Carve::HEAD);
  };
  auto kb_of = [&](int s) { return seq0 + (size_t)s * sf + Carve::HEAD + 2 * LP; };
  auto tg_of = [&](int s) { return reinterpret_cast<int*>(kb_of(s) + LP); };
  auto al_of = [&](int s) { return kb_of(s) + 2 * LP; };                    // [L][TC]
  auto be_of = [&](int s) { return al_of(s) + (size_t)L * TC; };           // [L][TC]

  const int b = blockIdx.x * seqs + sq;
  const bool row = b < B;
  const int n = row ? min(max(lens[b], 0), L) : 0;
  const float* e = emis + (long)(row ? b : 0) * L * T;
  {  // both waves of the pair stage the clamped tags
    const int* tg = tags + (long)(row ? b : 0) * L;
    int* tg_s = tg_of(sq);
    for (int t = threadIdx.x & (2 * WAVE - 1); t < n; t += 2 * WAVE)
      tg_s[t] = min(max(tg[t], 0), T - 1);
  }
  stage_trans<W>(tr_s, trans, T);
  __syncthreads();

  const bool act = lane < T;
  const int jc = lane & (W - 1);   // in-bounds LDS index for idle lanes
  const int jx = min(lane, T - 1);  // in-bounds emission column

  if (n > 0 && !bwd) {
    // ---- forward scan: alpha_hat[t][:] ----
    float* al = al_of(sq);
    float trc[TC];
    load_trans_col<W>(tr_s, jc, trc);
    float a = act ? e[jx] : NEG;  // alpha_hat[0] = x_0
    if (lane < TC) al[lane] = a;
    float e_nxt = e[min(1, n - 1) * T + jx];
    double ksum = 0.0;  // sum of the offsets taken out of alpha
    for (int t = 1; t < n; ++t) {
      const float et = e_nxt;
      e_nxt = e[min(t + 1, n - 1) * T + jx];
      __builtin_amdgcn_wave_barrier();
      const float* ap = al + (t - 1) * TC;
      f32x4 a4[TC / 4];
      f32x4 k4 = {NEG, NEG, NEG, NEG};
#pragma unroll
      for (int q = 0; q < TC / 4; ++q) {
        a4[q] = lds_bcast4(ap, q);
#pragma unroll
        for (int c = 0; c < 4; ++c) k4[c] = fmaxf(k4[c], a4[q][c]);
      }
      const float k = fmaxf(fmaxf(k4[0], k4[1]), fmaxf(k4[2], k4[3]));
      f32x4 m4 = {NEG, NEG, NEG, NEG};
#pragma unroll
      for (int q = 0; q < TC / 4; ++q) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          a4[q][c] = (a4[q][c] - k) + trc[q * 4 + c];
          m4[c] = fmaxf(m4[c], a4[q][c]);
        }
      }
      const float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < TC / 4; ++q) {
#pragma unroll
        for (int c = 0; c < 4; ++c) s4[c] += __expf(a4[q][c] - m);
      }
      const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      a = act ? m + __logf(s) + et : NEG;
      if (lane < TC) al[t * TC + lane] = a;
      ksum += (double)k;
    }
    // logZ = ksum + lse_j alpha_hat[n-1][j]
    const float mz = wave_reduce_max(a);
    const float sz = wave_reduce_sum(act ? __expf(a - mz) : 0.f);
    if (lane == 0) *logz_of(sq) = ksum + (double)(mz + __logf(sz));
  } else if (n > 0) {
    // ---- backward scan: beta_hat[t][:], and k_b[t] = max_j cur[t+1][j] ----
    float* be = be_of(sq);
    float* cur_s = cur_of(sq);
    float* kb_s = kb_of(sq);
    float trr[TC];
    load_trans_row<W>(tr_s, jc, trr);
    float beta = act ? 0.f : NEG;  // beta_hat[n-1]
    if (lane < TC) be[(n - 1) * TC + lane] = beta;
    if (lane == 0) kb_s[n - 1] = 0.f;
    float e_nxt = e[(n - 1) * T + jx];
    for (int t = n - 2; t >= 0; --t) {
      // cur[jj] = x[t+1][jj] + beta_hat[t+1][jj], staged for a broadcast read
      const float mine = act ? e_nxt + beta : NEG;
      e_nxt = e[t * T + jx];
      __builtin_amdgcn_wave_barrier();
      if (lane < W) cur_s[lane] = mine;
      __builtin_amdgcn_wave_barrier();
      f32x4 c4[TC / 4];
      f32x4 k4 = {NEG, NEG, NEG, NEG};
#pragma unroll
      for (int q = 0; q < TC / 4; ++q) {
        c4[q] = lds_bcast4(cur_s, q);
#pragma unroll
        for (int c = 0; c < 4; ++c) k4[c] = fmaxf(k4[c], c4[q][c]);
      }
      const float k = fmaxf(fmaxf(k4[0], k4[1]), fmaxf(k4[2], k4[3]));
      f32x4 m4 = {NEG, NEG, NEG, NEG};
#pragma unroll
      for (int q = 0; q < TC / 4; ++q) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          c4[q][c] = trr[q * 4 + c] + (c4[q][c] - k);
          m4[c] = fmaxf(m4[c], c4[q][c]);
        }
      }
      const float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < TC / 4; ++q) {
#pragma unroll
        for (int c = 0; c < 4; ++c) s4[c] += __expf(c4[q][c] - m);
      }
      const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      beta = act ? m + __logf(s) : NEG;
      if (lane < TC) be[t * TC + lane] = beta;
      if (lane == 0) kb_s[t] = k;
    }
  } else if (!bwd && lane == 0) {
    *logz_of(sq) = 0.0;  // empty row, or no row: ll = 0 - 0
  }
  // every wave of the block arrives here and at the barrier below, rows
  // past B and empty rows too
  __syncthreads();

  // ---- combine, all threads of the block on one sequence slot after the
  // other ----
  const int nthr = blockDim.x;
  for (int s = 0; s < seqs; ++s) {
    const int bs = blockIdx.x * seqs + s;
    if (bs >= B) break;  // block-uniform
    const int ns = min(max(lens[bs], 0), L);
    const float* al = al_of(s);
    const float* be = be_of(s);
    double* z_s = z_of(s);
    // Z_t: thread = t. A lane starts its walk over j at its own offset, so
    // that the lanes of a wave (row stride TC) spread over the LDS banks.
    for (int t = threadIdx.x; t < ns; t += nthr) {
      const float* ar = al + t * TC;
      const float* br = be + t * TC;
      int j = lane % T;
      const int j0 = j;
      double smax = (double)NEG;
      for (int q = 0; q < T; ++q) {
        smax = fmax(smax, (double)ar[j] + (double)br[j]);
        j = j + 1 == T ? 0 : j + 1;
      }
      j = j0;
      float sum = 0.f;
      for (int q = 0; q < T; ++q) {
        sum += __expf((float)(((double)ar[j] + (double)br[j]) - smax));
        j = j + 1 == T ? 0 : j + 1;
      }
      z_s[t] = smax + (double)__logf(sum);
    }
    // ll: the slot's backward wave sums the gold score over its lanes
    if (wid == 2 * s + 1) {
      const float* es = emis + (long)bs * L * T;
      const int* tg_s = tg_of(s);
      double sc = 0.0;
      for (int t = lane; t < ns; t += WAVE) {
        const int c = tg_s[t];
        sc += (double)es[t * T + c];
        if (t > 0) sc += (double)tr_s[tg_s[t - 1] * TRS + c];
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) sc += __shfl_xor(sc, off);
      if (lane == 0) ll[bs] = (float)(sc - *logz_of(s));
    }
  }
  __syncthreads();

  for (int s = 0; s < seqs; ++s) {
    const int bs = blockIdx.x * seqs + s;
    if (bs >= B) break;
    const int ns = min(max(lens[bs], 0), L);
    const float* es = emis + (long)bs * L * T;
    const float* al = al_of(s);
    const float* be = be_of(s);
    const double* z_s = z_of(s);
    const float* kb_s = kb_of(s);
    const int* tg_s = tg_of(s);
    // demis, flat and coalesced; zeros at t >= len
    float* de = demis + (long)bs * L * T;
    const int cells = L * T, live = ns * T;
    for (int c = threadIdx.x; c < cells; c += nthr) {
      float v = 0.f;
      if (c < live) {
        const int t = c / T, j = c - t * T;
        const double x =
            ((double)al[t * TC + j] + (double)be[t * TC + j]) - z_s[t];
        v = (j == tg_s[t] ? 1.f : 0.f) - __expf((float)x);
      }
      de[c] = v;
    }
    // dtrans[b]: thread = (i, j), t in index order
    float* dt = dtrans + (long)bs * T * T;
    for (int c = threadIdx.x; c < T * T; c += nthr) {
      const int i = c / T, j = c - i * T;
      const double tij = (double)tr_s[i * TRS + j];
      float acc = 0.f, gold = 0.f;
      for (int t = 0; t + 1 < ns; ++t) {
        const float cur = es[(t + 1) * T + j] + be[(t + 1) * TC + j];
        const double x = (((double)al[t * TC + i] - z_s[t]) + tij) +
                         ((double)cur - (double)kb_s[t]);
        acc += __expf((float)x);
        gold += (tg_s[t] == i && tg_s[t + 1] == j) ? 1.f : 0.f;
      }
      dt[c] = gold - acc;
    }
  }
}

template <int W, int TC>
void launch_pair(const at::Tensor& emissions, const at::Tensor& tags,
                 const at::Tensor& lens, const at::Tensor& trans,
                 at::Tensor& ll, at::Tensor& demis, at::Tensor& dtrans, int B,
                 int L, int T, int seqs) {
  const size_t smem = CrfPairCarve<W, TC>::bytes(seqs, L);
  TORCH_CHECK(smem <= CRFPAIR_LDS_BYTES, "CRF pair: LDS overflow (", smem,
              " bytes at ", seqs, " sequences per block)");
  hipLaunchKernelGGL((crf_pair_kernel<W, TC>), dim3((B + seqs - 1) / seqs),
                     dim3(seqs * 2 * WAVE), smem, cur_stream(emissions),
                     emissions.data_ptr<float>(), tags.data_ptr<int>(),
                     lens.data_ptr<int>(), trans.data_ptr<float>(),
                     ll.data_ptr<float>(), demis.data_ptr<float>(),
                     dtrans.data_ptr<float>(), B, L, T);
  HIP_CHECK_LAST();
}

// ------------------------------------------------------------ grad scale
constexpr int CRFGS_THREADS = 256;

// blocks [0, eb): demis_out = demis * dll[b], flat. Blocks from eb on:
// dtrans_out[c] = sum_b dtrans[b][c] * dll[b], b in index order.
__global__ __launch_bounds__(CRFGS_THREADS) void crf_grad_scale_kernel(
    const float* __restrict__ demis,   // [B,LT]
    const float* __restrict__ dtrans,  // [B,TT]
    const float* __restrict__ dll,     // [B]
    float* __restrict__ demis_out,     // [B,LT]
    float* __restrict__ dtrans_out,    // [TT]
    long ds,  // element stride of dll: 0 when autograd hands an expanded scalar
    int B, int LT, int TT, int eb) {
  if ((int)blockIdx.x < eb) {
    const long idx = (long)blockIdx.x * CRFGS_THREADS + threadIdx.x;
    if (idx < (long)B * LT) demis_out[idx] = demis[idx] * dll[(idx / LT) * ds];
    return;
  }
  const int c = ((int)blockIdx.x - eb) * CRFGS_THREADS + threadIdx.x;
  if (c >= TT) return;
  // the loads of a batch are issued together; the sum keeps index order
  constexpr int NB = 16;
  float acc = 0.f;
  for (int b0 = 0; b0 < B; b0 += NB) {
    float d[NB], w[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int b = min(b0 + u, B - 1);  // clamped address, unused past B
      d[u] = dtrans[(long)b * TT + c];
      w[u] = dll[b * ds];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u)
      if (b0 + u < B) acc += d[u] * w[u];
  }
  dtrans_out[c] = acc;
}

}  // namespace

// ===================================================================== host
// {pair (1/0), waves per block, LDS bytes}; off the pair route the last two
// are 0 (crf_wide.hip picks its own)
std::vector<int64_t> crf_fwd_route(int64_t L, int64_t T) {
  check_pair_range((int)L, (int)T);
  const CrfFwdRoute rt((int)L, (int)T);
  return {rt.pair ? 1 : 0, rt.pair ? rt.seqs * 2 : 0,
          rt.pair ? (int64_t)rt.smem : 0};
}

// seqs_per_block: 0 = the route's own choice; 1 or 2 force it (timing)
std::vector<at::Tensor> crf_pair_fwd(const at::Tensor& emissions,
                                     const at::Tensor& tags,
                                     const at::Tensor& lens,
                                     const at::Tensor& trans,
                                     int64_t seqs_per_block) {
  CHECK_CUDA_CONTIG(emissions);
  CHECK_CUDA_CONTIG(tags);
  CHECK_CUDA_CONTIG(lens);
  CHECK_CUDA_CONTIG(trans);
  TORCH_CHECK(emissions.dim() == 3, "CRF: emissions must be [B,L,T]");
  TORCH_CHECK(emissions.scalar_type() == at::kFloat &&
                  trans.scalar_type() == at::kFloat &&
                  lens.scalar_type() == at::kInt &&
                  tags.scalar_type() == at::kInt,
              "CRF: emissions/transitions must be float32, lens/tags int32");
  const int B = emissions.size(0), L = emissions.size(1), T = emissions.size(2);
  check_pair_range(L, T);
  TORCH_CHECK(tags.numel() == (int64_t)B * L && lens.numel() == B &&
                  trans.numel() == (int64_t)T * T,
              "CRF: tags/lens/transitions do not match emissions");
  const CrfFwdRoute rt(L, T);
  TORCH_CHECK(rt.pair, "CRF pair: seq_len ", L, " at label_size ", T,
              " is not on the pair route (label_size <= ", CRFPAIR_MAX_T,
              " and both tables in LDS)");
  TORCH_CHECK(seqs_per_block >= 0 && seqs_per_block <= CRFPAIR_MAX_SEQS,
              "CRF pair: seqs_per_block must be 0, 1 or 2");
  const int seqs = seqs_per_block ? (int)seqs_per_block : rt.seqs;
  // the kernel writes every cell, so no memset node ahead of it
  auto ll = at::empty({B}, emissions.options());
  auto demis = at::empty_like(emissions);
  auto dtrans = at::empty({B, T, T}, emissions.options());
  if (B == 0) return {ll, demis, dtrans};
#define CRFPAIR_LAUNCH(W, TC)                                              \
  launch_pair<W, TC>(emissions, tags, lens, trans, ll, demis, dtrans, B, L, \
                     T, seqs)
  CRFPAIR_DISPATCH(T, CRFPAIR_LAUNCH);
#undef CRFPAIR_LAUNCH
  return {ll, demis, dtrans};
}

// (demis [B,L,T] * dll[b], sum_b dtrans[b] * dll[b]) in one launch; new
// tensors, the inputs are left as they are
std::vector<at::Tensor> crf_grad_scale(const at::Tensor& demis,
                                       const at::Tensor& dtrans,
                                       const at::Tensor& dll) {
  CHECK_CUDA_CONTIG(demis);
  CHECK_CUDA_CONTIG(dtrans);
  TORCH_CHECK(dll.is_cuda(), "dll must be a GPU tensor");  // any stride
  TORCH_CHECK(demis.dim() == 3 && dtrans.dim() == 3 && dll.dim() == 1,
              "crf_grad_scale: demis [B,L,T], dtrans [B,T,T], dll [B]");
  TORCH_CHECK(demis.scalar_type() == at::kFloat &&
                  dtrans.scalar_type() == at::kFloat &&
                  dll.scalar_type() == at::kFloat,
              "crf_grad_scale: float32 only");
  const int64_t B = demis.size(0), L = demis.size(1), T = demis.size(2);
  TORCH_CHECK(dtrans.size(0) == B && dtrans.size(1) == T &&
                  dtrans.size(2) == T && dll.size(0) == B,
              "crf_grad_scale: shapes do not match");
  TORCH_CHECK(B * L * T < (int64_t)1 << 31, "crf_grad_scale: too large");
  auto demis_out = at::empty_like(demis);
  auto dtrans_out = at::empty({T, T}, demis.options());
  const int LT = (int)(L * T), TT = (int)(T * T);
  const int eb = (int)((B * LT + CRFGS_THREADS - 1) / CRFGS_THREADS);
  const int tb = (TT + CRFGS_THREADS - 1) / CRFGS_THREADS;
  if (eb + tb == 0) return {demis_out, dtrans_out};
  hipLaunchKernelGGL(crf_grad_scale_kernel, dim3(eb + tb), dim3(CRFGS_THREADS),
                     0, cur_stream(demis), demis.data_ptr<float>(),
                     dtrans.data_ptr<float>(), dll.data_ptr<float>(),
                     demis_out.data_ptr<float>(), dtrans_out.data_ptr<float>(),
                     (long)dll.stride(0), (int)B, LT, TT, eb);
  HIP_CHECK_LAST();
  return {demis_out, dtrans_out};
}
