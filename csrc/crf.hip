// Linear-chain CRF entry points. crf_fwd (loss + analytic grads in one
// launch) only routes: crf_pair.hip wherever its tables fit LDS,
// crf_wide.hip everywhere else. crf_viterbi has the narrow decoders here
// (T is tiny (<= 20), sequences are independent -> one wave
// per sequence, or four at T <= 16, lane j owns tag j, transition matrix
// and backpointers in LDS) and hands every other shape to crf_wide.hip.
#include "crf_pair_route.h"

#define TMAX 20
#define T16 16

__global__ void crf_viterbi_kernel_x4(const float* __restrict__ emis,
                                      const int* __restrict__ lens,
                                      const float* __restrict__ trans,
                                      int* __restrict__ pred,  // zeroed
                                      int B, int L, int T) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tr_s = reinterpret_cast<float*>(smem_raw);
  const int nw = blockDim.x / WAVE;
  const size_t bp_stride = (size_t)L * T16;
  char* bp_all = smem_raw + T16 * T16 * sizeof(float);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int g = lane >> 4;
  const int base = lane & 48;
  for (int i = threadIdx.x; i < T * T; i += blockDim.x) tr_s[i] = trans[i];
  __syncthreads();

  const int b = blockIdx.x * nw * 4 + wid * 4 + g;
  if (b >= B) return;
  const int n = lens[b];
  if (n <= 0) return;
  const float* e = emis + (long)b * L * T;
  char* bp = bp_all + (size_t)(wid * 4 + g) * bp_stride;
  const int j = lane & 15;
  const bool act = j < T;
  float delta = act ? e[j] : NEG;
  for (int t = 1; t < n; ++t) {
    float best = NEG;
    int arg = 0;
    for (int i = 0; i < T; ++i) {
      const float dprev = __shfl(delta, base + i);
      const float v = dprev + (act ? tr_s[i * T + j] : NEG);
      if (v > best) {
        best = v;
        arg = i;
      }
    }
    delta = act ? best + e[t * T + j] : NEG;
    if (act) bp[t * T16 + j] = (char)arg;
  }
  float bv = delta;
  int barg = act ? j : 0;
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {   // within the 16-lane group
    const float ov = __shfl_xor(bv, off);
    const int oa = __shfl_xor(barg, off);
    if (ov > bv) {
      bv = ov;
      barg = oa;
    }
  }
  if (j == 0) {
    int* pr = pred + (long)b * L;
    int cur = min(max(barg, 0), T - 1);
    pr[n - 1] = cur;
    for (int t = n - 2; t >= 0; --t) {
      cur = min(max((int)bp[(t + 1) * T16 + cur], 0), T - 1);
      pr[t] = cur;
    }
  }
}

// Viterbi: same layout; backpointers in LDS (int8), lane-0 backtrace.
__global__ void crf_viterbi_kernel(const float* __restrict__ emis,
                                   const int* __restrict__ lens,
                                   const float* __restrict__ trans,
                                   int* __restrict__ pred,  // [B,L] zeroed
                                   int B, int L, int T) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tr_s = reinterpret_cast<float*>(smem_raw);          // [TMAX*TMAX]
  const int nw = blockDim.x / WAVE;
  // per-wave: delta row [T] floats + bp [L][T] int8 (rounded to 16)
  const size_t bp_stride = (size_t)L * TMAX;
  char* bp_all = smem_raw + TMAX * TMAX * sizeof(float);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  for (int i = threadIdx.x; i < T * T; i += blockDim.x) tr_s[i] = trans[i];
  __syncthreads();

  const int b = blockIdx.x * nw + wid;
  if (b >= B) return;
  const int n = lens[b];
  if (n <= 0) return;
  const float* e = emis + (long)b * L * T;
  char* bp = bp_all + (size_t)wid * bp_stride;
  const int j = lane;
  const bool act = j < T;
  float delta = act ? e[j] : NEG;  // delta[0][j]
  for (int t = 1; t < n; ++t) {
    // all lanes need delta[t-1][i] -> shfl broadcast
    float best = NEG;
    int arg = 0;
    for (int i = 0; i < T; ++i) {
      const float dprev = __shfl(delta, i);
      const float v = dprev + (act ? tr_s[i * T + j] : NEG);
      if (v > best) {
        best = v;
        arg = i;
      }
    }
    delta = act ? best + e[t * T + j] : NEG;
    if (act) bp[t * TMAX + j] = (char)arg;
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
  if (lane == 0) {
    int* pr = pred + (long)b * L;
    // clamp defensively: non-finite emissions (diverged training) must
    // not turn into out-of-bounds backtraces
    int cur = min(max(barg, 0), T - 1);
    pr[n - 1] = cur;
    for (int t = n - 2; t >= 0; --t) {
      cur = min(max((int)bp[(t + 1) * TMAX + cur], 0), T - 1);
      pr[t] = cur;
    }
  }
}

// ===================================================================== host
// crf_wide.hip: 1 <= T <= 64, 1 <= L <= 512
std::vector<at::Tensor> crf_wide_fwd(const at::Tensor&, const at::Tensor&,
                                     const at::Tensor&, const at::Tensor&);
at::Tensor crf_wide_viterbi(const at::Tensor&, const at::Tensor&,
                            const at::Tensor&);

// crf_pair.hip: every shape whose two scan tables fit LDS
std::vector<at::Tensor> crf_pair_fwd(const at::Tensor&, const at::Tensor&,
                                     const at::Tensor&, const at::Tensor&,
                                     int64_t);

std::vector<at::Tensor> crf_fwd(const at::Tensor& emissions,
                                const at::Tensor& tags, const at::Tensor& lens,
                                const at::Tensor& trans) {
  CHECK_CUDA_CONTIG(emissions);
  TORCH_CHECK(emissions.dim() == 3, "CRF: emissions must be [B,L,T]");
  const int L = emissions.size(1), T = emissions.size(2);
  check_pair_range(L, T);
  if (CrfFwdRoute(L, T).pair)
    return crf_pair_fwd(emissions, tags, lens, trans, 0);
  return crf_wide_fwd(emissions, tags, lens, trans);
}

at::Tensor crf_viterbi(const at::Tensor& emissions, const at::Tensor& lens,
                       const at::Tensor& trans) {
  CHECK_CUDA_CONTIG(emissions);
  const int B = emissions.size(0), L = emissions.size(1), T = emissions.size(2);
  const int nw = 4;
  const size_t smem4 = T16 * T16 * sizeof(float) + (size_t)nw * 4 * L * T16;
  const size_t smem = TMAX * TMAX * sizeof(float) + (size_t)nw * L * TMAX;
  const bool x4 = T <= T16 && smem4 <= 160 * 1024;
  if (!x4 && (T > TMAX || smem > 160 * 1024))
    return crf_wide_viterbi(emissions, lens, trans);
  auto pred = at::zeros({B, L}, emissions.options().dtype(at::kInt));
  if (x4) {
    hipLaunchKernelGGL(crf_viterbi_kernel_x4,
                       dim3((B + nw * 4 - 1) / (nw * 4)), dim3(nw * WAVE),
                       smem4, cur_stream(emissions),
                       emissions.data_ptr<float>(), lens.data_ptr<int>(),
                       trans.data_ptr<float>(), pred.data_ptr<int>(), B, L, T);
    HIP_CHECK_LAST();
    return pred;
  }
  hipLaunchKernelGGL(crf_viterbi_kernel, dim3((B + nw - 1) / nw),
                     dim3(nw * WAVE), smem, cur_stream(emissions),
                     emissions.data_ptr<float>(), lens.data_ptr<int>(),
                     trans.data_ptr<float>(), pred.data_ptr<int>(), B, L, T);
  HIP_CHECK_LAST();
  return pred;
}
