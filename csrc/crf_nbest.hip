// N-best (list-Viterbi) decode of a linear-chain CRF for 1 <= T <= 64 tags,
// 1 <= L <= 512 tokens and 1 <= k <= 8 paths per sequence: the k best tag
// paths of every row with their unnormalised scores, best first.
//
// Order (the same as ops.reference.crf_nbest, so exact ties decode alike):
// for tag j at step t the candidates (delta[t-1][i][r] + trans[i][j]) over
// predecessor i and rank r are ranked by value descending, then i, then r
// ascending; the first NK are kept and emis[t][j] is added afterwards. The
// final ranking over (j, r) is by value descending, then j, then r.
//
// Layout: one wave per sequence, lane = tag, as crf_wide.hip's Viterbi.
// Compile-time constants: the tag width W (32 or 64), the number of tags a
// step scans TC (12, 24, 32 | 48, 64; T <= TC, no branch on T in the step)
// and the list length NK (2, 4, 8; the requested k is rounded up and the
// first k ranks are returned). Each lane keeps its NK ranked scores in
// registers. Per step it publishes them to LDS as NK contiguous floats per
// tag; every lane then reads all TC*NK of them as broadcast 16 B reads and
// inserts candidate (i, r) into its new list with a strict '>' in (i asc,
// r asc) order. Candidate (i, r) cannot land above position r, because
// (i, 0..r-1) are no smaller and came first, so it is compared with
// positions r..NK-1 only. Every register-array index is a constant after
// unrolling. At W = 32 the whole step is unrolled over this lane's
// transition column in registers (crf_common.h); at W = 64 that would be up
// to 512 candidates of straight-line code per step, so the loop over
// predecessors stays rolled, four tags a trip, and reads the column from
// the LDS image instead.
//
// Backpointers: one code i*NK + r per (t, j, r), 8 bits at W = 32 and 16
// bits at W = 64, NK of them packed into one store per lane and step. The
// table [L][TC][NK] lives in LDS whenever one wave's table fits beside the
// transition image (4, 2 or 1 waves per block, from the byte count in
// CrfNbestCarve); otherwise (only W = 64 with NK >= 4 can get there) it
// goes to a global workspace that the host allocates, written with plain
// vector stores the scan never waits for and read back, after a
// workgroup-scope fence, by the wave that wrote it. Every row of that
// workspace is a multiple of 128 B, so no two waves share a cache line.
//
// Numerics: the lists are kept relative to a running offset, k[t] = the best
// score of step t-1 over all tags (every lane reads the whole published
// vector, so it costs no cross-lane op), taken out after the insertion and
// summed in fp64; the returned score is that sum plus the relative score.
// Plain fp32 accumulation reaches |score| ~ 1.5e3 at L = 512 and was
// measured 1.06e-3 off the fp64 score of its own path, past the 1e-3 bound.
// The offset is the same for every candidate of a step, so it changes no
// comparison, and with inputs whose sums are exact it is exact too.
//
// Absent ranks (a row has min(k, T^len) paths) carry the sentinel NEG
// inside the scan and leave as IEEE -inf with an all-zero path. The kernel
// writes every output cell. No atomics; the result is bitwise reproducible.
#include "crf_common.h"

#include <cmath>
#include <type_traits>

namespace {

constexpr size_t CRFN_LDS_BYTES = 160 * 1024;
constexpr int CRFN_MAX_K = 8;
// a list cell above this holds a real path score, one below it is absent
constexpr float CRFN_PRESENT = -1e29f;

// ---- LDS carve, shared by host and device so the byte count (and with it
// the routing) lives in one place.
template <int W, int TC, int NK> struct CrfNbestCarve {
  static constexpr int TRS = CrfTransImage<W>::TRS;
  static constexpr int TR_FLOATS = CrfTransImage<W>::TR_FLOATS;
  static constexpr int CB = W == 32 ? 1 : 2;  // bytes per backpointer code
  static constexpr int RB = NK * CB;          // bytes per lane and step
  // per wave: cur [W][NK] floats, then the final tag / rank / score of the
  // CRFN_MAX_K winners
  static constexpr int HEAD_FLOATS = W * NK + 3 * CRFN_MAX_K;
  static __host__ __device__ int table_bytes(int L) {
    return (L * TC * RB + 127) & ~127;
  }
  static __host__ __device__ int wave_bytes(int L, bool lds_table) {
    return HEAD_FLOATS * (int)sizeof(float) + (lds_table ? table_bytes(L) : 0);
  }
  static size_t bytes(int nw, int L, bool lds_table) {
    return sizeof(float) * (size_t)TR_FLOATS +
           (size_t)nw * wave_bytes(L, lds_table);
  }
};

// Insert candidate (v, code c) into the descending list s[R..NK) (it cannot
// belong above R). Strict '>': an equal, earlier candidate keeps its place.
template <int NK, int R>
__device__ __forceinline__ void nbest_insert(float (&s)[NK], int (&cd)[NK],
                                             float v, int c) {
  bool g[NK];
#pragma unroll
  for (int p = R; p < NK; ++p) g[p] = v > s[p];
#pragma unroll
  for (int p = NK - 1; p > R; --p) {
    cd[p] = g[p - 1] ? cd[p - 1] : (g[p] ? c : cd[p]);
    // s[p-1] >= s[p]: the median is v's neighbour-respecting place
    s[p] = __builtin_amdgcn_fmed3f(s[p - 1], s[p], v);
  }
  cd[R] = g[R] ? c : cd[R];
  s[R] = fmaxf(s[R], v);
}

// all NK candidates of one predecessor tag, rank ascending
template <int NK, int R = 0> struct NbestInsertTag {
  static __device__ __forceinline__ void run(float (&s)[NK], int (&cd)[NK],
                                             const float (&cv)[NK], float tri,
                                             int cbase) {
    nbest_insert<NK, R>(s, cd, cv[R] + tri, cbase + R);
    if constexpr (R + 1 < NK)
      NbestInsertTag<NK, R + 1>::run(s, cd, cv, tri, cbase);
  }
};

// the NK published scores of tags [i0, i0+4) as broadcast 16 B reads
template <int NK>
__device__ __forceinline__ void nbest_read4(const float* cur_s, int i0,
                                            float (&cv)[4][NK]) {
#pragma unroll
  for (int q = 0; q < NK; ++q) {  // 4*NK floats = NK reads
    const f32x4 a4 = lds_bcast4(cur_s, (i0 / 4) * NK + q);  // i0 % 4 == 0
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int f = q * 4 + c;  // float index inside the 4-tag group
      cv[f / NK][f % NK] = a4[c];
    }
  }
}

// NK codes of CB bytes each as one store
template <int RB>
__device__ __forceinline__ void nbest_store_codes(unsigned char* dst,
                                                  const unsigned (&pk)[4]) {
  if constexpr (RB == 2)
    *reinterpret_cast<unsigned short*>(dst) = (unsigned short)pk[0];
  else if constexpr (RB == 4)
    *reinterpret_cast<unsigned*>(dst) = pk[0];
  else if constexpr (RB == 8)
    *reinterpret_cast<uint2*>(dst) = make_uint2(pk[0], pk[1]);
  else
    *reinterpret_cast<uint4*>(dst) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
}

template <int W, int TC, int NK, bool GTAB>
__global__ __launch_bounds__(256) void crf_nbest_kernel(
    const float* __restrict__ emis,   // [B,L,T]
    const int* __restrict__ lens,     // [B]
    const float* __restrict__ trans,  // [T,T]
    int* __restrict__ paths,          // [B,k,L]
    float* __restrict__ scores,       // [B,k]
    unsigned char* __restrict__ gtab, // [B][table_bytes(L)] when GTAB
    int B, int L, int T, int k) {
  using Carve = CrfNbestCarve<W, TC, NK>;
  using code_t = typename std::conditional<W == 32, unsigned char,
                                           unsigned short>::type;
  constexpr int TRS = Carve::TRS;
  constexpr int RB = Carve::RB;
  constexpr bool ROLLED = W == 64;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tr_s = reinterpret_cast<float*>(smem_raw);  // [W][TRS]
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int nw = blockDim.x / WAVE;
  char* wbase = smem_raw + Carve::TR_FLOATS * sizeof(float) +
                (size_t)wid * Carve::wave_bytes(L, !GTAB);
  float* cur_s = reinterpret_cast<float*>(wbase);             // [W][NK]
  int* ftag_s = reinterpret_cast<int*>(cur_s + W * NK);       // [MAX_K]
  int* frank_s = ftag_s + CRFN_MAX_K;                         // [MAX_K]
  float* fsc_s = reinterpret_cast<float*>(frank_s + CRFN_MAX_K);
  stage_trans<W>(tr_s, trans, T);
  __syncthreads();

  const int b = blockIdx.x * nw + wid;
  if (b >= B) return;
  const int n = min(max(lens[b], 0), L);
  int* prow = paths + (long)b * k * L;
  float* srow = scores + (long)b * k;
  if (n == 0) {  // no path at all: every rank absent
    if (lane < k) srow[lane] = -INFINITY;
    for (int idx = lane; idx < k * L; idx += WAVE) prow[idx] = 0;
    return;
  }
  unsigned char* bp =
      GTAB ? gtab + (size_t)b * Carve::table_bytes(L)
           : reinterpret_cast<unsigned char*>(wbase) +
                 Carve::HEAD_FLOATS * sizeof(float);  // [L][TC][NK] codes
  const float* e = emis + (long)b * L * T;
  const int j = lane;
  const bool act = j < T;
  const int jc = lane & (W - 1);  // in-bounds LDS index for idle lanes

  float trc[ROLLED ? 1 : TC];
  if constexpr (!ROLLED) load_trans_col<W>(tr_s, jc, trc);

  float d[NK];  // this tag's ranked scores, best first
  d[0] = act ? e[j] : NEG;
#pragma unroll
  for (int r = 1; r < NK; ++r) d[r] = NEG;
  float e_nxt = (act && n > 1) ? e[T + j] : 0.f;
  double ksum = 0.0;  // sum of the offsets taken out of the lists
  for (int t = 1; t < n; ++t) {
    const float et = e_nxt;
    if (act && t + 1 < n) e_nxt = e[(t + 1) * T + j];
    __builtin_amdgcn_wave_barrier();
    if (lane < W) {
#pragma unroll
      for (int r = 0; r < NK; ++r) cur_s[lane * NK + r] = d[r];
    }
    __builtin_amdgcn_wave_barrier();
    float ns[NK];
    int nc[NK];
#pragma unroll
    for (int r = 0; r < NK; ++r) {
      ns[r] = NEG;
      nc[r] = 0;
    }
    float kt = NEG;  // max_i delta[t-1][i][0], the same in every lane
    if constexpr (ROLLED) {
#pragma unroll 1
      for (int i0 = 0; i0 < TC; i0 += 4) {
        float cv[4][NK];
        nbest_read4<NK>(cur_s, i0, cv);
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
          kt = fmaxf(kt, cv[ii][0]);
          NbestInsertTag<NK>::run(ns, nc, cv[ii], tr_s[(i0 + ii) * TRS + jc],
                                  (i0 + ii) * NK);
        }
      }
    } else {
#pragma unroll
      for (int i0 = 0; i0 < TC; i0 += 4) {
        float cv[4][NK];
        nbest_read4<NK>(cur_s, i0, cv);
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
          kt = fmaxf(kt, cv[ii][0]);
          NbestInsertTag<NK>::run(ns, nc, cv[ii], trc[i0 + ii],
                                  (i0 + ii) * NK);
        }
      }
    }
    unsigned pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < NK; ++r) {
      // absent cells go back to exactly NEG, so they never drift
      d[r] = (act && ns[r] > CRFN_PRESENT) ? (ns[r] - kt) + et : NEG;
      constexpr int PER = 4 / Carve::CB;  // codes per 32-bit word
      pk[r / PER] |= (unsigned)nc[r] << ((r % PER) * 8 * Carve::CB);
    }
    if (lane < TC)
      nbest_store_codes<RB>(bp + ((size_t)t * TC + lane) * RB, pk);
    ksum += (double)kt;
  }

  // ---- final ranking across lanes: NK rounds, each takes the best head
  // (ties: lowest tag) and the winning lane pops its list
  int popped = 0;
#pragma unroll
  for (int q = 0; q < NK; ++q) {
    float bv = d[0];
    int bl = lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int ol = __shfl_xor(bl, off);
      if (ov > bv || (ov == bv && ol < bl)) {
        bv = ov;
        bl = ol;
      }
    }
    if (lane == bl) {
      ftag_s[q] = lane;
      frank_s[q] = popped;
      fsc_s[q] = bv;
      ++popped;
#pragma unroll
      for (int p = 0; p + 1 < NK; ++p) d[p] = d[p + 1];
      d[NK - 1] = NEG;
    }
  }
  // the table was written by this wave's other lanes: global stores need
  // the fence, LDS stores the barrier
  if constexpr (GTAB) __threadfence_block();
  __builtin_amdgcn_wave_barrier();

  // ---- k back-traces in parallel, one lane per rank
  if (lane < k) {
    const float sc = fsc_s[lane];
    const bool present = sc > CRFN_PRESENT;
    srow[lane] = present ? (float)(ksum + (double)sc) : -INFINITY;
    if (present) {
      int* pr = prow + (long)lane * L;
      // clamp every field: non-finite inputs must not turn into
      // out-of-bounds reads
      int cj = min(max(ftag_s[lane], 0), T - 1);
      int cr = frank_s[lane] & (NK - 1);
      const code_t* tab = reinterpret_cast<const code_t*>(bp);
      for (int t = n - 1; t >= 1; --t) {
        pr[t] = cj;
        const int code = (int)tab[((size_t)t * TC + cj) * NK + cr];
        cj = min(code / NK, T - 1);
        cr = code & (NK - 1);
      }
      pr[0] = cj;
    }
  }
  // zeros past len, and whole rows of absent ranks
  for (int r = 0; r < k; ++r) {
    const int t0 = fsc_s[r] > CRFN_PRESENT ? n : 0;  // wave-uniform
    for (int t = t0 + lane; t < L; t += WAVE) prow[(long)r * L + t] = 0;
  }
}

template <int W, int TC, int NK> struct CrfNbestRoute {
  using Carve = CrfNbestCarve<W, TC, NK>;
  // only these instantiations can outgrow LDS (W = 32 peaks at 128 KiB)
  static constexpr bool HAS_GLOBAL = W == 64 && NK >= 4;
  int nw = 0;
  bool global = false;
  size_t smem = 0;
  explicit CrfNbestRoute(int L) {
    for (nw = 4; nw >= 1; nw >>= 1) {
      smem = Carve::bytes(nw, L, true);
      if (smem <= CRFN_LDS_BYTES) return;
    }
    TORCH_CHECK(HAS_GLOBAL, "CRF n-best: LDS overflow (", smem,
                " bytes at one wave)");
    global = true;
    nw = 4;
    smem = Carve::bytes(nw, L, false);
  }
};

template <int W, int TC, int NK>
void launch_nbest(const at::Tensor& emissions, const at::Tensor& lens,
                  const at::Tensor& trans, at::Tensor& paths,
                  at::Tensor& scores, int B, int L, int T, int k) {
  using Route = CrfNbestRoute<W, TC, NK>;
  const Route rt(L);
  const dim3 grid((B + rt.nw - 1) / rt.nw), block(rt.nw * WAVE);
  if (!rt.global) {
    hipLaunchKernelGGL((crf_nbest_kernel<W, TC, NK, false>), grid, block,
                       rt.smem, cur_stream(emissions),
                       emissions.data_ptr<float>(), lens.data_ptr<int>(),
                       trans.data_ptr<float>(), paths.data_ptr<int>(),
                       scores.data_ptr<float>(), nullptr, B, L, T, k);
  } else if constexpr (Route::HAS_GLOBAL) {
    auto work = at::empty({B, (int64_t)Route::Carve::table_bytes(L)},
                          emissions.options().dtype(at::kByte));
    hipLaunchKernelGGL((crf_nbest_kernel<W, TC, NK, true>), grid, block,
                       rt.smem, cur_stream(emissions),
                       emissions.data_ptr<float>(), lens.data_ptr<int>(),
                       trans.data_ptr<float>(), paths.data_ptr<int>(),
                       scores.data_ptr<float>(), work.data_ptr<uint8_t>(), B,
                       L, T, k);
  }
  HIP_CHECK_LAST();
}

void check_nbest_k(int64_t k) {
  TORCH_CHECK(k >= 1 && k <= CRFN_MAX_K, "CRF n-best: k ", k,
              " outside the supported range (1 <= k <= ", CRFN_MAX_K, ")");
}

// picks the instantiation for (T, k) and hands it to f
#define CRFN_DISPATCH_NK(W, TC, k, F)  \
  do {                                 \
    if ((k) <= 2) {                    \
      F(W, TC, 2);                     \
    } else if ((k) <= 4) {             \
      F(W, TC, 4);                     \
    } else {                           \
      F(W, TC, 8);                     \
    }                                  \
  } while (0)
#define CRFN_DISPATCH(T, k, F)         \
  do {                                 \
    if ((T) <= 12)                     \
      CRFN_DISPATCH_NK(32, 12, k, F);  \
    else if ((T) <= 24)                \
      CRFN_DISPATCH_NK(32, 24, k, F);  \
    else if ((T) <= 32)                \
      CRFN_DISPATCH_NK(32, 32, k, F);  \
    else if ((T) <= 48)                \
      CRFN_DISPATCH_NK(64, 48, k, F);  \
    else                               \
      CRFN_DISPATCH_NK(64, 64, k, F);  \
  } while (0)

}  // namespace

// ===================================================================== host
std::vector<at::Tensor> crf_nbest(const at::Tensor& emissions,
                                  const at::Tensor& lens,
                                  const at::Tensor& trans, int64_t k) {
  CHECK_CUDA_CONTIG(emissions);
  CHECK_CUDA_CONTIG(lens);
  CHECK_CUDA_CONTIG(trans);
  TORCH_CHECK(emissions.dim() == 3, "CRF: emissions must be [B,L,T]");
  TORCH_CHECK(emissions.scalar_type() == at::kFloat &&
                  trans.scalar_type() == at::kFloat &&
                  lens.scalar_type() == at::kInt,
              "CRF: emissions/transitions must be float32, lens int32");
  const int B = emissions.size(0), L = emissions.size(1), T = emissions.size(2);
  check_wide_range(L, T);
  check_nbest_k(k);
  TORCH_CHECK(lens.numel() == B && trans.numel() == (int64_t)T * T,
              "CRF: lens/transitions do not match emissions");
  // the kernel writes every cell, so no memset node ahead of it
  auto paths = at::empty({B, k, L}, emissions.options().dtype(at::kInt));
  auto scores = at::empty({B, k}, emissions.options());
  if (B == 0) return {paths, scores};
  const int kk = (int)k;
#define CRFN_LAUNCH(W, TC, NK) \
  launch_nbest<W, TC, NK>(emissions, lens, trans, paths, scores, B, L, T, kk)
  CRFN_DISPATCH(T, kk, CRFN_LAUNCH);
#undef CRFN_LAUNCH
  return {paths, scores};
}

// (global route?, waves per block) the launch above takes for this shape
std::vector<int64_t> crf_nbest_route(int64_t L, int64_t T, int64_t k) {
  check_wide_range((int)L, (int)T);
  check_nbest_k(k);
  std::vector<int64_t> out;
#define CRFN_ROUTE(W, TC, NK)                                  \
  do {                                                         \
    const CrfNbestRoute<W, TC, NK> rt((int)L);                 \
    out = {rt.global ? 1 : 0, rt.nw, (int64_t)rt.smem};        \
  } while (0)
  CRFN_DISPATCH(T, k, CRFN_ROUTE);
#undef CRFN_ROUTE
  return out;
}
