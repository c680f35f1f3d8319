// NT-layout MFMA GEMM for the BERT linear layers:
// C[M, N] = A[M, K] @ B[N, K]^T (+ bias[N]) with both operands K-major
// row-major — exactly torch's F.linear(x, w): A = activations, B = the
// [out, in] weight. Both MFMA fragments read 8 contiguous bf16 along K,
// so no transpose anywhere (the layout hipBLASLt calls NT). The backward
// products, whose contraction index is a row index in memory (gemm_tn for
// wgrad, gemm_nn for dgrad), are in the second half of this file.
//
// Structure (guide §5 "step-3" ladder stage, measured 874-912 TF/s at
// 4096^3 on this chip): 128x128 output tile per 256-thread workgroup
// (4 waves, 2x2 of 64x64), BK = 64, double-buffered LDS staged with
// global_load_lds width 16 (lane-linear image, XOR-swizzled SOURCE
// address so the MFMA fragment ds_read_b128s hit <=2-way banks),
// bijective XCD-aware workgroup remap (8 XCDs, private L2s).
//
// Full tiles only: the host wrapper dispatches here when M%128==0,
// N%128==0, K%64==0 (every BERT shape: K/N in {768, 2304, 3072},
// M = batch*seq); anything else falls back to the library GEMM.
#include "common.h"
#include "gelu.h"
#include "slab_colsum.h"

#define BM 128
#define BN 128
#define BK 64

using bfrag = mfma_bf16x8;
using cfrag = mfma_f32x4;

__device__ __forceinline__ cfrag mfma16(bfrag a, bfrag b, cfrag c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Source-address chunk swizzle: the LDS image is lane-linear (glds), so
// the bank-spread XOR moves to the per-lane GLOBAL address. A row is
// 64 bf16 = 128 B = one cache line, and the XOR permutes 16-B chunks
// WITHIN the row, so coalescing is preserved exactly.
__device__ __forceinline__ int swz_chunk(int row, int chunk) {
  return chunk ^ (row & 7);
}

// Stage one [128][BK] bf16 tile (rows r0.., K-major, row stride `ld`
// elements) into lds (lane-linear [128][BK]): 4 glds-b128 per wave.
__device__ __forceinline__ void stage_tile(const bf16* __restrict__ g,
                                           long ld, long r0, long k0,
                                           bf16* lds) {
  const int t = threadIdx.x;                 // 0..255
  // one glds instruction stages 64 lanes x 16 B = 1 KiB = 8 rows
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lds_off = (t / WAVE) * 4096 + i * 1024 + (t % WAVE) * 16;
    const int row = lds_off >> 7;            // 128 B per row
    const int chunk = (lds_off & 127) >> 4;  // 16-B chunk in row
    const long src = (r0 + row) * ld + k0 +
                     (long)(swz_chunk(row, chunk) << 3);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(g + src),
        (__attribute__((address_space(3))) void*)(lds + (lds_off >> 1)),
        16, 0, 0);
  }
}

// MFMA operand fragment from the lane-linear swizzled image:
// lane l -> tile[r0 + (l&15)][k0 + (l>>4)*8 .. +8]   (b128, <=2-way)
__device__ __forceinline__ bfrag frag(const bf16* tile, int r0, int k0) {
  const int l = threadIdx.x & (WAVE - 1);
  const int row = r0 + (l & 15);
  const int chunk = (k0 >> 3) + (l >> 4);
  return *reinterpret_cast<const bfrag*>(
      tile + ((long)row << 6) + (swz_chunk(row, chunk) << 3));
}

// BT: the bias in its stored dtype (fp32 or bf16, read in place and
// added in fp32); ignored without HAS_BIAS
template <typename OT, bool HAS_BIAS, typename BT>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(
    const bf16* __restrict__ A,   // [M, K]
    const bf16* __restrict__ B,   // [N, K]
    const BT* __restrict__ bias,  // [N] or null
    OT* __restrict__ C,           // [M, N]
    long M, long N, long K, int tiles_n) {
  __shared__ bf16 smem[2 * 2 * BM * BK];     // A/B double-buffered, 64 KiB
  bf16* a_s = smem;                          // [2][128][64]
  bf16* b_s = smem + 2 * BM * BK;

  // bijective XCD-aware remap (8 XCDs; guide T1)
  const int nwg = gridDim.x;
  int wg = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = wg & 7, idx = wg >> 3;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const long m0 = (long)(wg / tiles_n) * BM;
  const long n0 = (long)(wg % tiles_n) * BN;

  const int wid = threadIdx.x / WAVE;        // 2x2 wave grid
  const int wr = (wid >> 1) * 64, wc = (wid & 1) * 64;
  const int lane = threadIdx.x & (WAVE - 1);

  cfrag acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = cfrag{0.f, 0.f, 0.f, 0.f};

  stage_tile(A, K, m0, 0, a_s);
  stage_tile(B, K, n0, 0, b_s);
  __syncthreads();                           // drains glds (vmcnt 0)

  const int nkt = (int)(K / BK);
  int buf = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    if (kt + 1 < nkt) {                      // prefetch next K-tile
      const int nxt = buf ^ 1;
      stage_tile(A, K, m0, (long)(kt + 1) * BK, a_s + nxt * BM * BK);
      stage_tile(B, K, n0, (long)(kt + 1) * BK, b_s + nxt * BM * BK);
    }
    const bf16* at = a_s + buf * BM * BK;
    const bf16* bt = b_s + buf * BM * BK;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      bfrag af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = frag(at, wr + i * 16, kk * 32);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = frag(bt, wc + j * 16, kk * 32);
      // favor this wave while its MFMA cluster runs (guide T5)
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = mfma16(af[i], bfr[j], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();                         // joins + drains prefetch
    buf ^= 1;
  }

  // epilogue: C/D map col = lane&15, row = (lane>>4)*4 + r
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long row0 = m0 + wr + i * 16 + ((lane >> 4) << 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long col = n0 + wc + j * 16 + (lane & 15);
      const float bv = HAS_BIAS ? to_f32(bias[col]) : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        from_f32(acc[i][j][r] + bv, &C[(row0 + r) * N + col]);
    }
  }
}

template <typename OT>
static void launch_gemm_nt(const at::Tensor& a, const at::Tensor& b,
                           const c10::optional<at::Tensor>& bias,
                           at::Tensor& out, long M, long N, long K) {
  dim3 grid((unsigned)((M / BM) * (N / BN)));
  if (bias && bias->scalar_type() == at::kBFloat16)
    hipLaunchKernelGGL((gemm_nt_kernel<OT, true, bf16>), grid, dim3(256), 0,
                       cur_stream(a), (const bf16*)a.data_ptr(),
                       (const bf16*)b.data_ptr(),
                       (const bf16*)bias->data_ptr(), (OT*)out.data_ptr(),
                       M, N, K, (int)(N / BN));
  else if (bias)
    hipLaunchKernelGGL((gemm_nt_kernel<OT, true, float>), grid, dim3(256), 0,
                       cur_stream(a), (const bf16*)a.data_ptr(),
                       (const bf16*)b.data_ptr(), bias->data_ptr<float>(),
                       (OT*)out.data_ptr(), M, N, K, (int)(N / BN));
  else
    hipLaunchKernelGGL((gemm_nt_kernel<OT, false, float>), grid, dim3(256), 0,
                       cur_stream(a), (const bf16*)a.data_ptr(),
                       (const bf16*)b.data_ptr(), (const float*)nullptr,
                       (OT*)out.data_ptr(), M, N, K, (int)(N / BN));
}

// C = A @ B^T (+bias). A [M,K] bf16, B [N,K] bf16, bias fp32/bf16 optional;
// out bf16 (fp32_out=false) or fp32.
at::Tensor gemm_nt(const at::Tensor& a, const at::Tensor& b,
                   c10::optional<at::Tensor> bias, bool fp32_out) {
  CHECK_CUDA_CONTIG(a);
  CHECK_CUDA_CONTIG(b);
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 &&
                  b.scalar_type() == at::kBFloat16,
              "gemm_nt: bf16 operands");
  const long M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(b.size(1) == K, "gemm_nt: K mismatch");
  TORCH_CHECK(M % BM == 0 && N % BN == 0 && K % BK == 0,
              "gemm_nt: needs M%128==0, N%128==0, K%64==0 (got ", M, "x", N,
              "x", K, ")");
  if (bias) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() &&
                    (bias->scalar_type() == at::kFloat ||
                     bias->scalar_type() == at::kBFloat16) &&
                    bias->numel() == N,
                "gemm_nt: bias must be fp32 or bf16 [N]");
  }
  auto out = at::empty({M, N}, a.options().dtype(
                                   fp32_out ? at::kFloat : at::kBFloat16));
  if (fp32_out)
    launch_gemm_nt<float>(a, b, bias, out, M, N, K);
  else
    launch_gemm_nt<bf16>(a, b, bias, out, M, N, K);
  HIP_CHECK_LAST();
  return out;
}

// ===================================================================
// Transposed-operand variants for the backward products:
//   gemm_tn: C[M, N] = A[T, M]^T @ B[T, N]   (wgrad: dW = dy^T @ x)
//   gemm_nn: C[M, N] = A[M, K]   @ B[K, N]   (dgrad: dx = dy @ w)
// An operand whose contraction index is its ROW index in memory
// ("k-strided") is staged exactly like the k-major one -- coalesced full
// rows, glds width 16, lane-linear image, XOR on the source address --
// as a [BK = 64 rows of k][128 columns] tile with 256-byte rows, and is
// consumed column-wise with ds_read_b64_tr_b16 (two per fragment), so
// there is no transpose pass anywhere. The k-major A operand of gemm_nn
// reuses stage_tile/frag above. Both reads give lane (g, i) the k
// indices 8g .. 8g+7 of row/column i, so the two kinds mix freely.
//
// LDS image of a k-strided tile (guide T10 image (b)): byte offset of
// 16-byte chunk ch of row r is 256 r + 16 (ch ^ X(r)),
// X(r) = ((r & 3) << 2) | ((r >> 2) & 3). Bank check (bank = (a/4) % 64,
// conflicts per 32-lane half): in one transposed read a half holds
// groups g, g+1 = rows r0 + q and r0 + 8 + q (q = 0..3), chunks
// {2m, 2m+1}; the slot is (2m | p>>1) ^ (q << 2) ^ {0, 2} (+1 for the
// second read, rows + 4): 16 distinct slots, each split in two 8-byte
// halves by p & 1 -> 32 lanes x 8 B cover the 256-byte bank row exactly
// once. Both reads of a fragment are conflict-free.
__device__ __forceinline__ int swz_ks(int row) {
  return ((row & 3) << 2) | ((row >> 2) & 3);
}

// Stage one [BK][128] bf16 tile (rows k0.., columns c0.., row stride
// `ld` elements) into lds: one glds-b128 per wave fills 4 rows.
__device__ __forceinline__ void stage_tile_ks(const bf16* __restrict__ g,
                                              long ld, long k0, long c0,
                                              bf16* lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lds_off = (t / WAVE) * 4096 + i * 1024 + (t % WAVE) * 16;
    const int row = lds_off >> 8;            // 256 B per row
    const int slot = (lds_off & 255) >> 4;   // 16-B slot in row
    const long src = (k0 + row) * ld + c0 + (long)((slot ^ swz_ks(row)) << 3);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(g + src),
        (__attribute__((address_space(3))) void*)(lds + (lds_off >> 1)),
        16, 0, 0);
  }
}

// Element offset this lane supplies to the transposed read of the 4-row
// block starting at row `r0` (multiple of 4), 16 columns from `c0`
// (multiple of 16): lane 4q+p of a group -> row r0 + q, columns
// c0 + 4p .. +3. The XOR can swap the two chunks of a 32-byte span, so
// every lane goes through the image's own offset function.
__device__ __forceinline__ int tr_off(int r0, int c0) {
  const int l = threadIdx.x & (WAVE - 1);
  const int row = r0 + ((l & 15) >> 2);
  const int col = c0 + ((l & 3) << 2);
  return (row << 7) + (((col >> 3) ^ swz_ks(row)) << 3) + (col & 7);
}

// 16x16x32 operand, lane (g, i) element j = tile[k0 + 8g + j][c0 + i],
// from the two precomputed offsets (rows 8g.. and 8g+4..). Needs EXEC
// all ones and a 16-byte aligned tile.
__device__ __forceinline__ bfrag frag_tr(const bf16* tile, int off_lo,
                                         int off_hi) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + off_lo));
  const s16x4 hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + off_hi));
  const s16x8 f = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bfrag, f);
}

// A_KMAJOR: A is [M, K] (gemm_nn) else [K, M] (gemm_tn); B is [K, N].
// blockIdx covers tiles x split; split s contracts K-stages
// [s nkt / split, (s+1) nkt / split) and writes slab s of C.
template <bool A_KMAJOR, typename OT>
__global__ __launch_bounds__(256, 2) void gemm_ks_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B,
    OT* __restrict__ C,           // [split][M, N]
    long M, long N, long K, int tiles_n, int tiles, int split) {
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * 2 * BM * BK];
  bf16* a_s = smem;                          // [2][8192]
  bf16* b_s = smem + 2 * BM * BK;

  const int nwg = gridDim.x;
  int wg = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = wg & 7, idx = wg >> 3;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int s = wg / tiles, tile = wg - s * tiles;
  const long m0 = (long)(tile / tiles_n) * BM;
  const long n0 = (long)(tile % tiles_n) * BN;

  const int wid = threadIdx.x / WAVE;
  const int wr = (wid >> 1) * 64, wc = (wid & 1) * 64;
  const int lane = threadIdx.x & (WAVE - 1);
  const int g8 = (lane >> 4) << 3;

  int aoff[4][2], boff[4][2];                // kk = 0; kk adds 32 rows
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    aoff[i][0] = tr_off(g8, wr + i * 16);
    aoff[i][1] = tr_off(g8 + 4, wr + i * 16);
    boff[i][0] = tr_off(g8, wc + i * 16);
    boff[i][1] = tr_off(g8 + 4, wc + i * 16);
  }

  cfrag acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = cfrag{0.f, 0.f, 0.f, 0.f};

  const int nkt = (int)(K / BK);
  const int kb = (int)((long)s * nkt / split);
  const int ke = (int)((long)(s + 1) * nkt / split);

  if (A_KMAJOR) stage_tile(A, K, m0, (long)kb * BK, a_s);
  else stage_tile_ks(A, M, (long)kb * BK, m0, a_s);
  stage_tile_ks(B, N, (long)kb * BK, n0, b_s);
  __syncthreads();

  // Per stage: read every fragment of the current tile, then issue the
  // next tile's glds, then the 32 MFMAs. A transposed read issued while
  // glds writes are in flight makes the compiler drain vmcnt first (it
  // cannot tell the two LDS buffers apart), which would serialise the
  // prefetch; in this order the only vmcnt(0) is the one at the barrier.
  int buf = 0;
  for (int kt = kb; kt < ke; ++kt) {
    const bf16* at = a_s + buf * BM * BK;
    const bf16* bt = b_s + buf * BM * BK;
    bfrag af[BK / 32][4], bfr[BK / 32][4];
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[kk][i] = A_KMAJOR ? frag(at, wr + i * 16, kk * 32)
                             : frag_tr(at + kk * 32 * 128, aoff[i][0],
                                       aoff[i][1]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bfr[kk][j] = frag_tr(bt + kk * 32 * 128, boff[j][0], boff[j][1]);
    }
    if (kt + 1 < ke) {                       // prefetch next K-tile
      const int nxt = buf ^ 1;
      const long k1 = (long)(kt + 1) * BK;
      if (A_KMAJOR) stage_tile(A, K, m0, k1, a_s + nxt * BM * BK);
      else stage_tile_ks(A, M, k1, m0, a_s + nxt * BM * BK);
      stage_tile_ks(B, N, k1, n0, b_s + nxt * BM * BK);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = mfma16(af[kk][i], bfr[kk][j], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();                         // joins + drains prefetch
    buf ^= 1;
  }

  OT* Cs = C + (long)s * M * N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long row0 = m0 + wr + i * 16 + ((lane >> 4) << 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long col = n0 + wc + j * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        from_f32(acc[i][j][r], &Cs[(row0 + r) * N + col]);
    }
  }
}

// out[i] = sum over slabs in slab order (fixed order: reproducible)
template <typename OT>
__global__ __launch_bounds__(256) void splitk_finish_kernel(
    const float* __restrict__ part, OT* __restrict__ out, long n4,
    long slab, int split) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  f32x4 acc = reinterpret_cast<const f32x4*>(part)[i];
  for (int s = 1; s < split; ++s)
    acc += reinterpret_cast<const f32x4*>(part + (long)s * slab)[i];
#pragma unroll
  for (int e = 0; e < 4; ++e) from_f32(acc[e], &out[i * 4 + e]);
}

// Host split rule for gemm_tn (split == 0), from the measured per-shape
// table in profiles/gemm_tn_r08.md: a workgroup wave is 512 resident
// tiles (256 CUs x 2); cost = waves x stages per split, plus the
// partial-slab traffic of the finisher counted in stage units.
static int choose_split(long tiles, long nkt, long MN) {
  static const int cand[] = {1, 2, 3, 4, 6, 8};
  int best = 1;
  double best_cost = 1e30;
  for (int c : cand) {
    if (c > nkt) break;
    const double waves = (double)((tiles * c + 511) / 512);
    const double stages = (double)((nkt + c - 1) / c);
    // one stage of a resident pair ~0.7 us; slab write + read at ~6 TB/s
    double cost = waves * stages * 0.7;
    if (tiles * c < 256) cost *= 0.75;       // CUs not shared: faster stage
    if (c > 1) cost += 2.0 + (double)c * MN * 8.0 / 6.0e6;
    if (cost < best_cost) { best_cost = cost; best = c; }
  }
  return best;
}

template <bool A_KMAJOR>
static at::Tensor launch_gemm_ks(const at::Tensor& a, const at::Tensor& b,
                                 long M, long N, long K, int split,
                                 bool fp32_out) {
  const int tiles_n = (int)(N / BN), tiles = (int)((M / BM) * tiles_n);
  auto out = at::empty({M, N}, a.options().dtype(
                                   fp32_out ? at::kFloat : at::kBFloat16));
  auto st = cur_stream(a);
  const bf16* ap = (const bf16*)a.data_ptr();
  const bf16* bp = (const bf16*)b.data_ptr();
  if (split == 1) {
    if (fp32_out)
      hipLaunchKernelGGL((gemm_ks_kernel<A_KMAJOR, float>), dim3(tiles),
                         dim3(256), 0, st, ap, bp, out.data_ptr<float>(), M,
                         N, K, tiles_n, tiles, 1);
    else
      hipLaunchKernelGGL((gemm_ks_kernel<A_KMAJOR, bf16>), dim3(tiles),
                         dim3(256), 0, st, ap, bp, (bf16*)out.data_ptr(), M,
                         N, K, tiles_n, tiles, 1);
    HIP_CHECK_LAST();
    return out;
  }
  auto ws = at::empty({(long)split, M, N}, a.options().dtype(at::kFloat));
  hipLaunchKernelGGL((gemm_ks_kernel<A_KMAJOR, float>),
                     dim3((unsigned)(tiles * split)), dim3(256), 0, st, ap,
                     bp, ws.data_ptr<float>(), M, N, K, tiles_n, tiles,
                     split);
  HIP_CHECK_LAST();
  const long n4 = M * N / 4;
  dim3 fgrid((unsigned)((n4 + 255) / 256));
  if (fp32_out)
    hipLaunchKernelGGL((splitk_finish_kernel<float>), fgrid, dim3(256), 0, st,
                       ws.data_ptr<float>(), out.data_ptr<float>(), n4,
                       M * N, split);
  else
    hipLaunchKernelGGL((splitk_finish_kernel<bf16>), fgrid, dim3(256), 0, st,
                       ws.data_ptr<float>(), (bf16*)out.data_ptr(), n4,
                       M * N, split);
  HIP_CHECK_LAST();
  return out;
}

// C = A^T @ B. A [T,M] bf16, B [T,N] bf16; split-K over T with fp32
// partial slabs and a fixed-order finisher (split 1: direct; split 0:
// host rule). out bf16 or fp32.
at::Tensor gemm_tn(const at::Tensor& a, const at::Tensor& b, long split,
                   bool fp32_out) {
  CHECK_CUDA_CONTIG(a);
  CHECK_CUDA_CONTIG(b);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 &&
                  a.scalar_type() == at::kBFloat16 &&
                  b.scalar_type() == at::kBFloat16,
              "gemm_tn: 2-D bf16 operands");
  const long T = a.size(0), M = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == T, "gemm_tn: T mismatch");
  TORCH_CHECK(T > 0 && M > 0 && N > 0 && M % BM == 0 && N % BN == 0 &&
                  T % BK == 0,
              "gemm_tn: needs M%128==0, N%128==0, T%64==0 (got ", M, "x", N,
              "x", T, ")");
  const long nkt = T / BK;
  TORCH_CHECK(split >= 0 && split <= 16 && split <= nkt,
              "gemm_tn: split must be 0 (auto) or 1..min(16, T/64)");
  if (split == 0) split = choose_split((M / BM) * (N / BN), nkt, M * N);
  return launch_gemm_ks<false>(a, b, M, N, T, (int)split, fp32_out);
}

// C = A @ B. A [M,K] bf16, B [K,N] bf16 (a weight in its stored
// [out, in] layout for dgrad); out bf16 or fp32.
at::Tensor gemm_nn(const at::Tensor& a, const at::Tensor& b, bool fp32_out) {
  CHECK_CUDA_CONTIG(a);
  CHECK_CUDA_CONTIG(b);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 &&
                  a.scalar_type() == at::kBFloat16 &&
                  b.scalar_type() == at::kBFloat16,
              "gemm_nn: 2-D bf16 operands");
  const long M = a.size(0), K = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K, "gemm_nn: K mismatch");
  TORCH_CHECK(M > 0 && N > 0 && K > 0 && M % BM == 0 && N % BN == 0 &&
                  K % BK == 0,
              "gemm_nn: needs M%128==0, N%128==0, K%64==0 (got ", M, "x", N,
              "x", K, ")");
  return launch_gemm_ks<true>(a, b, M, N, K, 1, fp32_out);
}

// ===================================================================
// FFN GEMMs with the bias+GELU passes in their epilogues:
//   gemm_nt_bias_gelu: u = bf16(A @ B^T),  g = bf16(gelu(u + bias))
//   gemm_nn_dgelu:     dh = bf16(A @ B),   du = bf16(dh * gelu'(u + bias)),
//                      dbias = column sums of float(du)
// Sibling kernels of gemm_nt_kernel / gemm_ks_kernel<true>: same staging,
// same fragments, same K order. The one change in the loop is that the
// two MFMA operands trade places (D^T = B-frag x A-frag), which makes the
// C/D map  row m = lane & 15, columns n = (lane >> 4) * 4 + r: a lane
// owns 4 CONSECUTIVE columns of one row, so u is loaded and u / g / du
// are stored 8 bytes per lane (16 instead of 64 store instructions per
// wave and tile), straight from registers: no LDS round trip and no
// barrier in the forward epilogue. Each product a*b and the order in
// which an element's K terms are added are those of the plain kernels,
// and the rounding to bf16 before the bias is kept, so u, g and du are
// what gemm_nt -> bias_gelu_fwd and gemm_nn -> bias_gelu_bwd produce.

template <bool SAVE_PRE, typename BT>
__global__ __launch_bounds__(256, 2) void gemm_nt_gelu_kernel(
    const bf16* __restrict__ A,   // [M, K]
    const bf16* __restrict__ B,   // [N, K]
    const BT* __restrict__ bias,  // [N]
    bf16* __restrict__ U,         // [M, N] pre-activation (SAVE_PRE)
    bf16* __restrict__ G,         // [M, N] gelu(u + bias)
    long M, long N, long K, int tiles_n) {
  __shared__ bf16 smem[2 * 2 * BM * BK];
  bf16* a_s = smem;
  bf16* b_s = smem + 2 * BM * BK;

  const int nwg = gridDim.x;
  int wg = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = wg & 7, idx = wg >> 3;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const long m0 = (long)(wg / tiles_n) * BM;
  const long n0 = (long)(wg % tiles_n) * BN;

  const int wid = threadIdx.x / WAVE;
  const int wr = (wid >> 1) * 64, wc = (wid & 1) * 64;
  const int lane = threadIdx.x & (WAVE - 1);
  const int g4 = (lane >> 4) << 2;

  cfrag acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = cfrag{0.f, 0.f, 0.f, 0.f};

  stage_tile(A, K, m0, 0, a_s);
  stage_tile(B, K, n0, 0, b_s);
  // this lane's 16 bias values, in flight under the first stage
  float be[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) load_bias4(bias, n0 + wc + j * 16 + g4, be[j]);
  __syncthreads();

  const int nkt = (int)(K / BK);
  int buf = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    if (kt + 1 < nkt) {
      const int nxt = buf ^ 1;
      stage_tile(A, K, m0, (long)(kt + 1) * BK, a_s + nxt * BM * BK);
      stage_tile(B, K, n0, (long)(kt + 1) * BK, b_s + nxt * BM * BK);
    }
    const bf16* at = a_s + buf * BM * BK;
    const bf16* bt = b_s + buf * BM * BK;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      bfrag af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = frag(at, wr + i * 16, kk * 32);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = frag(bt, wc + j * 16, kk * 32);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = mfma16(bfr[j], af[i], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
    buf ^= 1;
  }

  // epilogue: acc[i][j][r] = C[m0+wr+16i + (lane&15)][n0+wc+16j + g4 + r]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long row = m0 + wr + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long off = row * N + n0 + wc + j * 16 + g4;
      bf16 uo[4], go[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        from_f32(acc[i][j][r], &uo[r]);
        const float u = to_f32(uo[r]) + be[j][r];
        from_f32(gelu_f(u), &go[r]);
      }
      if (SAVE_PRE)
        *reinterpret_cast<s16x4*>(U + off) = *reinterpret_cast<s16x4*>(uo);
      *reinterpret_cast<s16x4*>(G + off) = *reinterpret_cast<s16x4*>(go);
    }
  }
}

// slab: [M / 128][N] fp32, row = this block's tile row; every block
// writes all 128 columns of its tile, so the slab needs no zero-fill.
template <typename BT>
__global__ __launch_bounds__(256, 2) void gemm_nn_dgelu_kernel(
    const bf16* __restrict__ A,   // [M, K]  upstream gradient
    const bf16* __restrict__ B,   // [K, N]  weight as stored
    const bf16* __restrict__ U,   // [M, N]  saved pre-activation
    const BT* __restrict__ bias,  // [N]
    bf16* __restrict__ DU,        // [M, N]
    float* __restrict__ slab, long M, long N, long K, int tiles_n) {
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * 2 * BM * BK];
  bf16* a_s = smem;
  bf16* b_s = smem + 2 * BM * BK;

  const int nwg = gridDim.x;
  int wg = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = wg & 7, idx = wg >> 3;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int tile_m = wg / tiles_n;
  const long m0 = (long)tile_m * BM;
  const long n0 = (long)(wg % tiles_n) * BN;

  const int wid = threadIdx.x / WAVE;
  const int wr = (wid >> 1) * 64, wc = (wid & 1) * 64;
  const int lane = threadIdx.x & (WAVE - 1);
  const int g8 = (lane >> 4) << 3;
  const int g4 = (lane >> 4) << 2;

  int boff[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    boff[j][0] = tr_off(g8, wc + j * 16);
    boff[j][1] = tr_off(g8 + 4, wc + j * 16);
  }

  cfrag acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = cfrag{0.f, 0.f, 0.f, 0.f};

  const int nkt = (int)(K / BK);
  // the stage whose barrier also drains the u loads: two before the end
  const int kpre = nkt >= 2 ? nkt - 2 : 0;
  s16x4 uraw[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) uraw[i][j] = s16x4{0, 0, 0, 0};

  stage_tile(A, K, m0, 0, a_s);
  stage_tile_ks(B, N, 0, n0, b_s);
  float be[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) load_bias4(bias, n0 + wc + j * 16 + g4, be[j]);
  __syncthreads();

  // stage order as in gemm_ks_kernel: fragments, then the prefetch, then
  // the MFMAs
  int buf = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const bf16* at = a_s + buf * BM * BK;
    const bf16* bt = b_s + buf * BM * BK;
    bfrag af[BK / 32][4], bfr[BK / 32][4];
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
#pragma unroll
      for (int i = 0; i < 4; ++i) af[kk][i] = frag(at, wr + i * 16, kk * 32);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bfr[kk][j] = frag_tr(bt + kk * 32 * 128, boff[j][0], boff[j][1]);
    }
    if (kt + 1 < nkt) {
      const int nxt = buf ^ 1;
      const long k1 = (long)(kt + 1) * BK;
      stage_tile(A, K, m0, k1, a_s + nxt * BM * BK);
      stage_tile_ks(B, N, k1, n0, b_s + nxt * BM * BK);
    }
    if (kt == kpre) {                        // u: 16 x 8 bytes per lane
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long row = m0 + wr + i * 16 + (lane & 15);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          uraw[i][j] = *reinterpret_cast<const s16x4*>(
              U + row * N + n0 + wc + j * 16 + g4);
      }
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = mfma16(bfr[kk][j], af[kk][i], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    buf ^= 1;
  }

  // epilogue: du from registers; cs[j][r] = this lane's 4 rows of column
  // n0 + wc + 16j + g4 + r
  float cs[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) cs[j][r] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long row = m0 + wr + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16 o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bf16 dh;
        from_f32(acc[i][j][r], &dh);
        const float u =
            to_f32(reinterpret_cast<const bf16*>(&uraw[i][j])[r]) + be[j][r];
        const float g = to_f32(dh);
        from_f32(g * dgelu_f(u), &o[r]);
        cs[j][r] += to_f32(o[r]);
      }
      *reinterpret_cast<s16x4*>(DU + row * N + n0 + wc + j * 16 + g4) =
          *reinterpret_cast<s16x4*>(o);
    }
  }
  // column sums over the tile's 128 rows in a fixed order: the lane's 4
  // rows above, the 16 lanes of a group (xor tree), then the lower wave
  // row + the upper one through LDS (free after the loop's last barrier)
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) cs[j][r] = group16_reduce_sum(cs[j][r]);
  float* red = reinterpret_cast<float*>(smem);         // [128] columns
  if ((wid >> 1) == 1 && (lane & 15) == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<f32x4*>(red + wc + j * 16 + g4) =
          f32x4{cs[j][0], cs[j][1], cs[j][2], cs[j][3]};
  }
  __syncthreads();
  if ((wid >> 1) == 0 && (lane & 15) == 0) {
    float* srow = slab + (long)tile_m * N + n0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 hi = *reinterpret_cast<const f32x4*>(red + wc + j * 16 + g4);
      *reinterpret_cast<f32x4*>(srow + wc + j * 16 + g4) =
          f32x4{cs[j][0] + hi[0], cs[j][1] + hi[1], cs[j][2] + hi[2],
                cs[j][3] + hi[3]};
    }
  }
}

static void check_ffn_bias(const at::Tensor& bias, long N, const char* who) {
  TORCH_CHECK(bias.is_cuda() && bias.is_contiguous() && bias.dim() == 1 &&
                  bias.numel() == N &&
                  (bias.scalar_type() == at::kFloat ||
                   bias.scalar_type() == at::kBFloat16),
              who, ": bias must be a contiguous fp32 or bf16 [N]");
}

// (u, g) = (A @ B^T, gelu(u + bias)), both bf16; save_pre=false writes
// only g and returns an undefined u.
std::vector<at::Tensor> gemm_nt_bias_gelu(const at::Tensor& a,
                                          const at::Tensor& b,
                                          const at::Tensor& bias,
                                          bool save_pre) {
  CHECK_CUDA_CONTIG(a);
  CHECK_CUDA_CONTIG(b);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 &&
                  a.scalar_type() == at::kBFloat16 &&
                  b.scalar_type() == at::kBFloat16,
              "gemm_nt_bias_gelu: 2-D bf16 operands");
  const long M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(b.size(1) == K, "gemm_nt_bias_gelu: K mismatch");
  TORCH_CHECK(M > 0 && N > 0 && K > 0 && M % BM == 0 && N % BN == 0 &&
                  K % BK == 0,
              "gemm_nt_bias_gelu: needs M%128==0, N%128==0, K%64==0 (got ",
              M, "x", N, "x", K, ")");
  check_ffn_bias(bias, N, "gemm_nt_bias_gelu");
  at::Tensor u;
  if (save_pre) u = at::empty({M, N}, a.options());
  auto g = at::empty({M, N}, a.options());
  const dim3 grid((unsigned)((M / BM) * (N / BN)));
  const bf16* ap = (const bf16*)a.data_ptr();
  const bf16* bp = (const bf16*)b.data_ptr();
  bf16* up = save_pre ? (bf16*)u.data_ptr() : nullptr;
  bf16* gp = (bf16*)g.data_ptr();
  const int tn = (int)(N / BN);
  auto st = cur_stream(a);
  const bool bb = bias.scalar_type() == at::kBFloat16;
#define LAUNCH_NT_GELU(SP, BT)                                               \
  hipLaunchKernelGGL((gemm_nt_gelu_kernel<SP, BT>), grid, dim3(256), 0, st,  \
                     ap, bp, (const BT*)bias.data_ptr(), up, gp, M, N, K, tn)
  if (save_pre) {
    if (bb) LAUNCH_NT_GELU(true, bf16); else LAUNCH_NT_GELU(true, float);
  } else {
    if (bb) LAUNCH_NT_GELU(false, bf16); else LAUNCH_NT_GELU(false, float);
  }
#undef LAUNCH_NT_GELU
  HIP_CHECK_LAST();
  return {u, g};
}

// (du, dbias) = ((A @ B) * gelu'(u + bias), column sums of du); du bf16,
// dbias in the bias dtype.
std::vector<at::Tensor> gemm_nn_dgelu(const at::Tensor& a,
                                      const at::Tensor& b,
                                      const at::Tensor& u,
                                      const at::Tensor& bias) {
  CHECK_CUDA_CONTIG(a);
  CHECK_CUDA_CONTIG(b);
  CHECK_CUDA_CONTIG(u);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && u.dim() == 2 &&
                  a.scalar_type() == at::kBFloat16 &&
                  b.scalar_type() == at::kBFloat16 &&
                  u.scalar_type() == at::kBFloat16,
              "gemm_nn_dgelu: 2-D bf16 operands");
  const long M = a.size(0), K = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K, "gemm_nn_dgelu: K mismatch");
  TORCH_CHECK(u.size(0) == M && u.size(1) == N,
              "gemm_nn_dgelu: u must be [M, N]");
  TORCH_CHECK(M > 0 && N > 0 && K > 0 && M % BM == 0 && N % BN == 0 &&
                  K % BK == 0,
              "gemm_nn_dgelu: needs M%128==0, N%128==0, K%64==0 (got ", M,
              "x", N, "x", K, ")");
  check_ffn_bias(bias, N, "gemm_nn_dgelu");
  auto du = at::empty({M, N}, a.options());
  auto slab = at::empty({M / BM, N}, a.options().dtype(at::kFloat));
  auto dbias = at::empty({N}, bias.options());
  const dim3 grid((unsigned)((M / BM) * (N / BN)));
  auto st = cur_stream(a);
  if (bias.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL((gemm_nn_dgelu_kernel<bf16>), grid, dim3(256), 0, st,
                       (const bf16*)a.data_ptr(), (const bf16*)b.data_ptr(),
                       (const bf16*)u.data_ptr(),
                       (const bf16*)bias.data_ptr(), (bf16*)du.data_ptr(),
                       slab.data_ptr<float>(), M, N, K, (int)(N / BN));
    launch_slab_colsum<bf16, bf16>(slab, dbias.data_ptr(), (int)N, nullptr,
                                   st);
  } else {
    hipLaunchKernelGGL((gemm_nn_dgelu_kernel<float>), grid, dim3(256), 0, st,
                       (const bf16*)a.data_ptr(), (const bf16*)b.data_ptr(),
                       (const bf16*)u.data_ptr(), bias.data_ptr<float>(),
                       (bf16*)du.data_ptr(), slab.data_ptr<float>(), M, N, K,
                       (int)(N / BN));
    launch_slab_colsum<float, float>(slab, dbias.data_ptr(), (int)N, nullptr,
                                     st);
  }
  HIP_CHECK_LAST();
  return {du, dbias};
}
