// Constrained Viterbi decode for 1 <= T <= 64 tags and 1 <= L <= 512 tokens:
// the best tag path among those that stay inside a per-position set of
// allowed tags and use only allowed transitions.
//
//   allowed[b][t]     one 64-bit word: bit j set = tag j allowed at t. Bits
//                     at or above T are ignored; a word with no bit below T
//                     set stands for all T tags (crf_partial.hip's rule).
//   trans_allowed[i]  bit j set = transition i -> j allowed. Bits at or above
//                     T are ignored; there is no "empty means all" rule here,
//                     a tag may be terminal.
//
//   delta[t][j] = max_i(delta[t-1][i] + trans[i][j]) + e[t][j]
//
// in that association, first maximum in index order per step and for the
// final tag (crf_wide_viterbi_kernel, ops.reference.crf_decode). pred is the
// path, score its unnormalised score. A row without a path (len <= 0, or an
// infeasible constraint set) gets score = -inf and an all-zero pred row;
// cells at t >= len are 0. Every output cell is written, so the outputs are
// not zeroed.
//
// Masking is a select, never an addition: masked transition cells are NEG in
// the LDS image, and once per step a lane whose own bit is clear, or whose
// best predecessor term is not above NEG/2, gets delta = NEG assigned. So a
// tag with no allowed predecessor path holds exactly NEG and nothing
// accumulates on it. Contract: real path scores stay above -1e29.
//
// Layout: one wave per sequence, lane = tag. Tag width W (32 / 64) and the
// scanned width TC (12, 24, 32 | 48, 64; T <= TC) are compile-time constants,
// so a step scans exactly TC predecessors and has no branch on T: the cells
// of delta in [T, TC) hold NEG. Each lane keeps its column of the masked
// transition image in registers; delta is published per step as TC floats
// and read back as 16 B broadcasts; the next step's emission and word are
// fetched one step ahead (the word address is wave-uniform). Backpointers
// are int8 [L][TC] in LDS. The back-trace parks tag t in cell 0 of
// backpointer row t, which is dead by then (row 0 never held any), and the
// wave stores the pred row from there, coalesced.
//
// LDS per block: the transition image, plus per wave 16*ceil(TC/4) B of
// delta and 16*ceil(L*TC/16) B of backpointers. The largest carve (T = 64,
// L = 512, four waves) is 16,640 + 4 * 33,024 = 148,736 B, so the kernel
// always runs four waves per block: one route. No atomics, no scratch.
#include "crf_common.h"

namespace {

constexpr size_t CRFV_LDS_BYTES = 160 * 1024;
constexpr int CRFV_WAVES = 4;

// ---- LDS carve, shared by host and device. Offsets in bytes, every region
// a multiple of 16 B.
template <int W, int TC> struct CrfConstrainedCarve {
  static constexpr int TRS = CrfTransImage<W>::TRS;
  static constexpr int TR_BYTES =
      CrfTransImage<W>::TR_FLOATS * (int)sizeof(float);
  static constexpr int DELTA_BYTES = 16 * ((TC + 3) / 4);
  static __host__ __device__ int bp_bytes(int L) {
    return 16 * ((L * TC + 15) / 16);
  }
  static __host__ __device__ int wave_bytes(int L) {
    return DELTA_BYTES + bp_bytes(L);
  }
  static size_t bytes(int L) {
    return (size_t)TR_BYTES + (size_t)CRFV_WAVES * wave_bytes(L);
  }
};

// stage_trans with the transition mask applied: cell [i][j] is trans[i][j]
// where bit j of trans_allowed[i] is set, NEG elsewhere and in the pad
template <int W>
__device__ __forceinline__ void stage_trans_masked(
    float* tr_s, const float* __restrict__ trans,
    const unsigned long long* __restrict__ trans_allowed, int T) {
  constexpr int TRS = CrfTransImage<W>::TRS;
  for (int idx = threadIdx.x; idx < W * TRS; idx += blockDim.x) {
    const int i = idx / TRS, j = idx - i * TRS;
    float v = NEG;
    if (i < T && j < T && ((trans_allowed[i] >> j) & 1ull))
      v = trans[i * T + j];
    tr_s[idx] = v;
  }
}

// Is tag `lane` in the set the word stands for?
__device__ __forceinline__ bool tag_open(unsigned long long word,
                                         unsigned long long tmask, int lane) {
  unsigned long long w = word & tmask;
  if (w == 0ull) w = ~0ull;  // nothing known: all tags
  return (w >> lane) & 1ull;
}

template <int W, int TC>
__global__ __launch_bounds__(CRFV_WAVES* WAVE) void crf_constrained_kernel(
    const float* __restrict__ emis,                        // [B,L,T]
    const unsigned long long* __restrict__ allowed,        // [B,L]
    const int* __restrict__ lens,                          // [B]
    const float* __restrict__ trans,                       // [T,T]
    const unsigned long long* __restrict__ trans_allowed,  // [T]
    int* __restrict__ pred,                                // [B,L]
    float* __restrict__ score,                             // [B]
    int B, int L, int T) {
  using Carve = CrfConstrainedCarve<W, TC>;
  static_assert(TC % 4 == 0 && TC <= W, "scanned width");
  constexpr int Q = TC / 4;                 // quads of predecessors
  constexpr int NCH = (Q % 4 == 0) ? 4 : 3;  // independent scan chains
  constexpr int QC = Q / NCH;               // quads per chain
  static_assert(QC * NCH == Q, "chains must tile the scan");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tr_s = reinterpret_cast<float*>(smem_raw);  // [W][TRS]
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  char* wbase =
      smem_raw + Carve::TR_BYTES + (size_t)wid * Carve::wave_bytes(L);
  float* dl_s = reinterpret_cast<float*>(wbase);  // [TC]
  unsigned char* bp =
      reinterpret_cast<unsigned char*>(wbase + Carve::DELTA_BYTES);  // [L][TC]
  stage_trans_masked<W>(tr_s, trans, trans_allowed, T);
  __syncthreads();

  // the row index is the same in every lane: say so, and the length and the
  // words are fetched once per wave
  const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * CRFV_WAVES + wid);
  if (b >= B) return;
  const int n = min(max(lens[b], 0), L);
  const float* e = emis + (long)b * L * T;
  const unsigned long long* wd = allowed + (long)b * L;
  int* pr = pred + (long)b * L;
  const unsigned long long tmask = T >= 64 ? ~0ull : ((1ull << T) - 1ull);
  const int j = lane;  // tag owned by this lane
  const bool act = j < T;
  const int jc = lane & (W - 1);  // in-bounds LDS index for idle lanes

  bool feasible = false;
  float bv = NEG;
  if (n > 0) {
    float trc[TC];  // this lane's column of the masked transitions
    load_trans_col<W>(tr_s, jc, trc);

    bool ok = act && tag_open(wd[0], tmask, lane);
    float delta = ok ? e[j] : NEG;  // delta[0][j]
    float e_nxt = 0.f;
    bool ok_nxt = false;
    if (n > 1) {
      ok_nxt = act && tag_open(wd[1], tmask, lane);
      if (act) e_nxt = e[T + j];
    }
    for (int t = 1; t < n; ++t) {
      const float et = e_nxt;
      ok = ok_nxt;
      if (t + 1 < n) {
        ok_nxt = act && tag_open(wd[t + 1], tmask, lane);
        if (act) e_nxt = e[(t + 1) * T + j];
      }
      __builtin_amdgcn_wave_barrier();
      if (lane < TC) dl_s[lane] = delta;
      __builtin_amdgcn_wave_barrier();
      // NCH contiguous index blocks scanned independently, then merged in
      // index order with a strict '>' so the first maximum wins
      float best[NCH];
      int arg[NCH];
#pragma unroll
      for (int h = 0; h < NCH; ++h) {
        best[h] = NEG;
        arg[h] = h * QC * 4;
#pragma unroll
        for (int q = h * QC; q < (h + 1) * QC; ++q) {
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
      float bst = best[0];
      int ag = arg[0];
#pragma unroll
      for (int h = 1; h < NCH; ++h) {
        if (best[h] > bst) {
          bst = best[h];
          ag = arg[h];
        }
      }
      // the reset: a masked or unreachable tag holds exactly NEG
      delta = (ok && bst > 0.5f * NEG) ? bst + et : NEG;
      if (lane < TC) bp[t * TC + lane] = (unsigned char)ag;
    }
    // first maximum over the lanes: ties go to the lower tag
    bv = delta;
    int barg = j;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oa = __shfl_xor(barg, off);
      if (ov > bv || (ov == bv && oa < barg)) {
        bv = ov;
        barg = oa;
      }
    }
    feasible = bv > 0.5f * NEG;
    __builtin_amdgcn_wave_barrier();
    if (feasible && lane == 0) {
      // clamp: non-finite emissions must not turn into out-of-bounds
      // backtraces
      int cur = min(max(barg, 0), T - 1);
      for (int t = n - 1; t > 0; --t) {
        const int prev = min(max((int)bp[t * TC + cur], 0), T - 1);
        bp[t * TC] = (unsigned char)cur;  // row t is dead now
        cur = prev;
      }
      bp[0] = (unsigned char)cur;
    }
    __builtin_amdgcn_wave_barrier();
  }
  const int live = feasible ? n : 0;
  for (int t = lane; t < L; t += WAVE)
    pr[t] = t < live ? (int)bp[t * TC] : 0;
  if (lane == 0) score[b] = feasible ? bv : -INFINITY;
}

template <int W, int TC>
void launch_constrained(const at::Tensor& emissions, const at::Tensor& allowed,
                        const at::Tensor& lens, const at::Tensor& trans,
                        const at::Tensor& trans_allowed, at::Tensor& pred,
                        at::Tensor& score, int B, int L, int T) {
  const size_t smem = CrfConstrainedCarve<W, TC>::bytes(L);
  TORCH_CHECK(smem <= CRFV_LDS_BYTES, "CRF constrained: LDS overflow (", smem,
              " bytes)");
  hipLaunchKernelGGL(
      (crf_constrained_kernel<W, TC>), dim3((B + CRFV_WAVES - 1) / CRFV_WAVES),
      dim3(CRFV_WAVES * WAVE), smem, cur_stream(emissions),
      emissions.data_ptr<float>(),
      reinterpret_cast<const unsigned long long*>(allowed.data_ptr<int64_t>()),
      lens.data_ptr<int>(), trans.data_ptr<float>(),
      reinterpret_cast<const unsigned long long*>(
          trans_allowed.data_ptr<int64_t>()),
      pred.data_ptr<int>(), score.data_ptr<float>(), B, L, T);
  HIP_CHECK_LAST();
}

}  // namespace

// ===================================================================== host
std::vector<at::Tensor> crf_viterbi_constrained(const at::Tensor& emissions,
                                                const at::Tensor& allowed,
                                                const at::Tensor& lens,
                                                const at::Tensor& trans,
                                                const at::Tensor& trans_allowed) {
  CHECK_CUDA_CONTIG(emissions);
  CHECK_CUDA_CONTIG(allowed);
  CHECK_CUDA_CONTIG(lens);
  CHECK_CUDA_CONTIG(trans);
  CHECK_CUDA_CONTIG(trans_allowed);
  TORCH_CHECK(emissions.dim() == 3, "CRF: emissions must be [B,L,T]");
  TORCH_CHECK(emissions.scalar_type() == at::kFloat &&
                  trans.scalar_type() == at::kFloat &&
                  lens.scalar_type() == at::kInt &&
                  allowed.scalar_type() == at::kLong &&
                  trans_allowed.scalar_type() == at::kLong,
              "CRF: emissions/transitions must be float32, lens int32, "
              "allowed/trans_allowed int64");
  const int B = emissions.size(0), L = emissions.size(1), T = emissions.size(2);
  check_wide_range(L, T);
  TORCH_CHECK(allowed.numel() == (int64_t)B * L && lens.numel() == B &&
                  trans.numel() == (int64_t)T * T && trans_allowed.numel() == T,
              "CRF: allowed/lens/transitions/trans_allowed do not match "
              "emissions");
  // the kernel writes every cell, so no memset node ahead of it
  auto pred = at::empty({B, L}, emissions.options().dtype(at::kInt));
  auto score = at::empty({B}, emissions.options());
  if (B == 0) return {pred, score};
#define CRFV_LAUNCH(W, TC)                                                  \
  launch_constrained<W, TC>(emissions, allowed, lens, trans, trans_allowed, \
                            pred, score, B, L, T)
  if (T <= 12)
    CRFV_LAUNCH(32, 12);
  else if (T <= 24)
    CRFV_LAUNCH(32, 24);
  else if (T <= 32)
    CRFV_LAUNCH(32, 32);
  else if (T <= 48)
    CRFV_LAUNCH(64, 48);
  else
    CRFV_LAUNCH(64, 64);
#undef CRFV_LAUNCH
  return {pred, score};
}
