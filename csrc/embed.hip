// Fused BERT embedding gather: one kernel computes
// out[b, l, :] = word[token[b,l]] + pos[l] + tok_type[seg[b,l]]
// replacing three separate gather launches + two adds (each a full
// [B, L, H] pass over HBM). Memory-bound by design: 3 row reads + 1 row
// write, vectorized b128. The LayerNorm + dropout that follow stay in
// the existing fused dropout_add_ln kernel.
#include "common.h"
#include "slab_colsum.h"
#include "sorted_index.h"

__global__ __launch_bounds__(256) void embed3_kernel(
    const bf16* __restrict__ word,  // [V, H]
    const bf16* __restrict__ pos,   // [P, H]
    const bf16* __restrict__ tok,   // [S, H]
    const long* __restrict__ ids,   // [R] flattened token ids
    const long* __restrict__ segs,  // [R] flattened segment ids
    bf16* __restrict__ out,         // [R, H]
    long R, int H, int L) {
  const long row = blockIdx.x;
  if (row >= R) return;
  const long wrow = ids[row];
  const long srow = segs[row];
  const int prow = (int)(row % L);
  const bf16* w = word + wrow * H;
  const bf16* p = pos + (long)prow * H;
  const bf16* s = tok + srow * H;
  bf16* o = out + row * H;
  for (int c = threadIdx.x * 8; c < H; c += blockDim.x * 8) {
    const bf16x8 wv = *reinterpret_cast<const bf16x8*>(w + c);
    const bf16x8 pv = *reinterpret_cast<const bf16x8*>(p + c);
    const bf16x8 sv = *reinterpret_cast<const bf16x8*>(s + c);
    bf16x8 ov;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      ov[e] = (__bf16)((float)wv[e] + (float)pv[e] + (float)sv[e]);
    *reinterpret_cast<bf16x8*>(o + c) = ov;
  }
}

// word/pos/tok [*, H] bf16; token_ids/segment_ids [B, L] int64 ->
// [B, L, H] bf16 (the position index is l, the row index mod L).
at::Tensor embed3_fwd(const at::Tensor& word, const at::Tensor& pos,
                      const at::Tensor& tok, const at::Tensor& token_ids,
                      const at::Tensor& segment_ids) {
  CHECK_CUDA_CONTIG(word);
  CHECK_CUDA_CONTIG(pos);
  CHECK_CUDA_CONTIG(tok);
  CHECK_CUDA_CONTIG(token_ids);
  CHECK_CUDA_CONTIG(segment_ids);
  TORCH_CHECK(word.scalar_type() == at::kBFloat16 &&
                  pos.scalar_type() == at::kBFloat16 &&
                  tok.scalar_type() == at::kBFloat16,
              "embed3: bf16 tables");
  const int H = word.size(1);
  TORCH_CHECK(H % 8 == 0, "embed3: hidden % 8");
  const long B = token_ids.size(0), L = token_ids.size(1);
  const long R = B * L;
  auto out = at::empty({B, L, (long)H}, word.options());
  hipLaunchKernelGGL(embed3_kernel, dim3((unsigned)R), dim3(256), 0,
                     cur_stream(word), (const bf16*)word.data_ptr(),
                     (const bf16*)pos.data_ptr(), (const bf16*)tok.data_ptr(),
                     token_ids.data_ptr<long>(), segment_ids.data_ptr<long>(),
                     (bf16*)out.data_ptr(), R, H, (int)L);
  HIP_CHECK_LAST();
  return out;
}

// ------------------------------------------------------------ backward
// dw[v] = sum of the dy rows whose token id is v (row 0 = PAD stays zero),
// dp[l] = sum over the batch, dt[s] = sum of the rows of segment s; fp32
// sums rounded to bf16 once. No float atomics: the word table goes through
// the inverted index of sorted_index.h (one wave per destination row sums
// its list in list order), dp and dt through a fixed-order pass over dy.
// Every output cell is written exactly once by exactly one kernel, so the
// outputs need no zero fill, and the summation order of every element is a
// function of the shapes and the ids alone.
#define EB_CHUNK 16     // a list of n rows is summed by max(1, n / EB_CHUNK)
                        // waves, so a wave sums at most 2 * EB_CHUNK - 1 rows
#define EB_INFLIGHT 8   // row loads a wave keeps in flight
#define EB_SEG_CAP 8    // token_type rows the dp/dt pass keeps in registers
#define EB_BSLICES 8    // batch slices of the dp/dt pass
#define EB_COLVECS 32   // 8-column vectors per block of the dp/dt pass

// Sum of rows order[s .. e) of dy in that order, columns strided over the
// lanes 8 at a time; bf16 to out_b or, for a chunk of a long list, fp32 to
// out_f.
template <bool PARTIAL>
__device__ __forceinline__ void eb_sum_rows(
    const bf16* __restrict__ dy, const int* __restrict__ order, int s, int e,
    int H, int lane, bf16* __restrict__ out_b, float* __restrict__ out_f) {
  for (int c = lane * 8; c < H; c += WAVE * 8) {
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    for (int p = s; p < e; p += EB_INFLIGHT) {
      bf16x8 x[EB_INFLIGHT];
#pragma unroll
      for (int u = 0; u < EB_INFLIGHT; ++u) {
        if (p + u < e) {
          const long r = order[p + u];
          x[u] = *reinterpret_cast<const bf16x8*>(dy + r * H + c);
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k) x[u][k] = (__bf16)0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < EB_INFLIGHT; ++u)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += (float)x[u][k];
    }
    if (PARTIAL) {
      f32x4 lo = {acc[0], acc[1], acc[2], acc[3]};
      f32x4 hi = {acc[4], acc[5], acc[6], acc[7]};
      *reinterpret_cast<f32x4*>(out_f + c) = lo;
      *reinterpret_cast<f32x4*>(out_f + c + 4) = hi;
    } else {
      bf16x8 ov;
#pragma unroll
      for (int k = 0; k < 8; ++k) ov[k] = (__bf16)acc[k];
      *reinterpret_cast<bf16x8*>(out_b + c) = ov;
    }
  }
}

// The chunk that slab slot j holds, if any. A list at sorted positions
// [s, s + n) with m = n / EB_CHUNK >= 2 is cut into m chunks, chunk k at
// [s + k*n/m, s + (k+1)*n/m), and its partial sums live in slots
// s / EB_CHUNK + k. Slots of different lists never meet (the last one is
// below (s + n) / EB_CHUNK), and position (j + 1) * EB_CHUNK - 1 lies in
// the list that owns slot j, which is how a slot finds its list. PAD
// (id 0) owns no slot: its sum is not wanted.
struct EbChunk {
  int v, k, m, s, n;
};
__device__ __forceinline__ bool eb_slot_chunk(const int* __restrict__ skey,
                                              const int* __restrict__ start,
                                              int j, EbChunk* ch) {
  const int v = skey[(j + 1) * EB_CHUNK - 1];
  if (v == 0) return false;
  const int s = start[v];
  const int n = start[v + 1] - s;
  const int m = n / EB_CHUNK;
  const int k = j - s / EB_CHUNK;
  if (m < 2 || k < 0 || k >= m) return false;
  ch->v = v; ch->k = k; ch->m = m; ch->s = s; ch->n = n;
  return true;
}

// One wave per work item, 4 per block. Items [0, V): destination row v.
// It stores zeros for PAD and for an empty list without reading dy, the
// sum for a list of fewer than 2 * EB_CHUNK rows, and nothing for a longer
// one (embed3_bwd_word_finish_kernel stores that row). Items [V, V + nslot):
// slab slot j, the fp32 partial sum of one chunk of a long list.
__global__ __launch_bounds__(256) void embed3_bwd_word_kernel(
    const bf16* __restrict__ dy, const int* __restrict__ order,
    const int* __restrict__ skey, const int* __restrict__ start,
    bf16* __restrict__ dw, float* __restrict__ slab, int V, int H,
    int nslot) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = blockIdx.x * 4 + threadIdx.x / WAVE;
  if (w < V) {
    const int s = start[w];
    const int n = start[w + 1] - s;
    bf16* o = dw + (long)w * H;
    if (w == 0 || n == 0) {
      bf16x8 z;
#pragma unroll
      for (int k = 0; k < 8; ++k) z[k] = (__bf16)0.f;
      for (int c = lane * 8; c < H; c += WAVE * 8)
        *reinterpret_cast<bf16x8*>(o + c) = z;
    } else if (n < 2 * EB_CHUNK) {
      eb_sum_rows<false>(dy, order, s, s + n, H, lane, o, nullptr);
    }
  } else if (w - V < nslot) {
    const int j = w - V;
    EbChunk ch;
    if (!eb_slot_chunk(skey, start, j, &ch)) return;
    const int cs = ch.s + (int)((long)ch.k * ch.n / ch.m);
    const int ce = ch.s + (int)((long)(ch.k + 1) * ch.n / ch.m);
    eb_sum_rows<true>(dy, order, cs, ce, H, lane, nullptr,
                      slab + (long)j * H);
  }
}

// grid (nslot, ceil(H / (8 * EB_COLVECS))), 256 threads = EB_COLVECS column
// vectors x EB_BSLICES slices. The blocks of a long list's first slot add
// the list's m partial sums and store the bf16 row: slice y adds partials
// y, y + 8, ... in that order, then the slices are added in slice order
// through LDS, so a list of thousands of rows costs m / 8 dependent adds,
// not m, and the order is still a function of m alone. Every other block
// returns at once.
__global__ __launch_bounds__(EB_COLVECS * EB_BSLICES) void embed3_bwd_word_finish_kernel(
    const float* __restrict__ slab, const int* __restrict__ skey,
    const int* __restrict__ start, bf16* __restrict__ dw, int H) {
  __shared__ float red[EB_BSLICES][EB_COLVECS][9];
  const int j = blockIdx.x;
  EbChunk ch;
  if (!eb_slot_chunk(skey, start, j, &ch) || ch.k != 0) return;  // per block
  const int tx = threadIdx.x % EB_COLVECS;
  const int ty = threadIdx.x / EB_COLVECS;
  const int c = (blockIdx.y * EB_COLVECS + tx) * 8;
  const bool live = c < H;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  if (live) {
    const float* p = slab + (long)j * H + c;
#pragma unroll 4
    for (int q = ty; q < ch.m; q += EB_BSLICES) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(p + (long)q * H);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(p + (long)q * H + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc[k] += lo[k];
        acc[4 + k] += hi[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) red[ty][tx][k] = acc[k];
  __syncthreads();
  if (ty == 0 && live) {
    bf16x8 ov;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float a = red[0][tx][k];
#pragma unroll
      for (int y = 1; y < EB_BSLICES; ++y) a += red[y][tx][k];
      ov[k] = (__bf16)a;
    }
    *reinterpret_cast<bf16x8*>(dw + (long)ch.v * H + c) = ov;
  }
}

// grid (P, ceil(H / (8 * EB_COLVECS))), 256 threads = EB_COLVECS column
// vectors x EB_BSLICES batch slices. Block (l, tile) with l < L sums
// dy[b, l, tile] over b = slice, slice + 8, ... in registers, once into
// the dp row and once into the accumulator of the row's segment, then adds
// the slices in slice order through LDS: dp[l] is final, the per-segment
// sums go to row l of the [L][S*H] slab that slab_colsum_kernel finishes.
// A segment id outside [0, S) adds to no segment. Blocks l >= L store the
// zero rows of dp.
__global__ __launch_bounds__(EB_COLVECS * EB_BSLICES) void embed3_bwd_pos_seg_kernel(
    const bf16* __restrict__ dy, const long* __restrict__ segs,
    bf16* __restrict__ dp, float* __restrict__ slab, int B, int L, int H,
    int S) {
  __shared__ float red[EB_BSLICES][EB_COLVECS][9];
  const int tx = threadIdx.x % EB_COLVECS;
  const int ty = threadIdx.x / EB_COLVECS;
  const int l = blockIdx.x;
  const int c = (blockIdx.y * EB_COLVECS + tx) * 8;
  const bool live = c < H;
  if (l >= L) {
    if (live && ty == 0) {
      bf16x8 z;
#pragma unroll
      for (int k = 0; k < 8; ++k) z[k] = (__bf16)0.f;
      *reinterpret_cast<bf16x8*>(dp + (long)l * H + c) = z;
    }
    return;
  }
  float acc[EB_SEG_CAP + 1][8];
#pragma unroll
  for (int q = 0; q <= EB_SEG_CAP; ++q)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[q][k] = 0.f;
  if (live) {
#pragma unroll 4
    for (int b = ty; b < B; b += EB_BSLICES) {
      const long r = (long)b * L + l;
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(dy + r * H + c);
      const long seg = segs[r];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[0][k] += (float)x[k];
#pragma unroll
      for (int q = 0; q < EB_SEG_CAP; ++q)
        if (q < S && seg == q) {
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[q + 1][k] += (float)x[k];
        }
    }
  }
#pragma unroll
  for (int q = 0; q <= EB_SEG_CAP; ++q) {
    if (q <= S) {  // the same for the whole block
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 8; ++k) red[ty][tx][k] = acc[q][k];
      __syncthreads();
      if (ty == 0 && live) {
        float a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = red[0][tx][k];
#pragma unroll
        for (int y = 1; y < EB_BSLICES; ++y)
#pragma unroll
          for (int k = 0; k < 8; ++k) a[k] += red[y][tx][k];
        if (q == 0) {
          bf16x8 ov;
#pragma unroll
          for (int k = 0; k < 8; ++k) ov[k] = (__bf16)a[k];
          *reinterpret_cast<bf16x8*>(dp + (long)l * H + c) = ov;
        } else {
          float* o = slab + ((long)l * S + (q - 1)) * H + c;
          f32x4 lo = {a[0], a[1], a[2], a[3]};
          f32x4 hi = {a[4], a[5], a[6], a[7]};
          *reinterpret_cast<f32x4*>(o) = lo;
          *reinterpret_cast<f32x4*>(o + 4) = hi;
        }
      }
    }
  }
}

// (list chunk, segment cap, row limit, limit of V * rows): the one place
// ops/functional.py and the tests take them from
std::vector<long> embed3_bwd_limits() {
  return {EB_CHUNK, EB_SEG_CAP, SIDX_MAX_ROWS, SIDX_MAX_KEYS};
}

static bool embed3_bwd_supported(long R, long V, long H, long S) {
  return H >= 8 && H % 8 == 0 && S >= 1 && S <= EB_SEG_CAP &&
         sidx_supported(R, V);
}

// dy [B, L, H] bf16; token_ids/segment_ids [B, L] int64, read as stored
// -> (dw [V, H], dp [P, H], dt [S, H]) bf16. Seven launches, all on the
// current stream, capturable.
std::vector<at::Tensor> embed3_bwd(const at::Tensor& dy,
                                   const at::Tensor& token_ids,
                                   const at::Tensor& segment_ids, long V,
                                   long P, long S) {
  CHECK_CUDA_CONTIG(dy);
  CHECK_CUDA_CONTIG(token_ids);
  CHECK_CUDA_CONTIG(segment_ids);
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 && dy.dim() == 3,
              "embed3_bwd: dy [B, L, H] bf16");
  TORCH_CHECK(token_ids.scalar_type() == at::kLong &&
                  segment_ids.scalar_type() == at::kLong,
              "embed3_bwd: int64 ids");
  const long B = dy.size(0), L = dy.size(1), H = dy.size(2);
  const long R = B * L;
  TORCH_CHECK(token_ids.numel() == R && segment_ids.numel() == R,
              "embed3_bwd: ids [B, L]");
  TORCH_CHECK(L <= P, "embed3_bwd: L <= P");
  TORCH_CHECK(embed3_bwd_supported(R, V, H, S),
              "embed3_bwd: need H % 8 == 0, S <= ", EB_SEG_CAP, ", B*L <= ",
              SIDX_MAX_ROWS, " and V*B*L <= 2^32");
  hipStream_t stream = cur_stream(dy);
  auto dw = at::empty({V, H}, dy.options());
  auto dp = at::empty({P, H}, dy.options());
  auto dt = at::empty({S, H}, dy.options());
  const bf16* dyp = (const bf16*)dy.data_ptr();

  SortedIndex si = build_sorted_index(token_ids, R, V, stream);
  const int nslot = (int)(R / EB_CHUNK);
  auto wslab = at::empty({std::max(nslot, 1), H},
                         dy.options().dtype(at::kFloat));
  hipLaunchKernelGGL(embed3_bwd_word_kernel,
                     dim3((unsigned)((V + nslot + 3) / 4)), dim3(256), 0,
                     stream, dyp, si.order, si.skey, si.start,
                     (bf16*)dw.data_ptr(), wslab.data_ptr<float>(), (int)V,
                     (int)H, nslot);
  if (nslot > 0)
    hipLaunchKernelGGL(
        embed3_bwd_word_finish_kernel,
        dim3((unsigned)nslot,
             (unsigned)((H + 8 * EB_COLVECS - 1) / (8 * EB_COLVECS))),
        dim3(EB_COLVECS * EB_BSLICES), 0, stream,
                       (const float*)wslab.data_ptr<float>(), si.skey,
                       si.start, (bf16*)dw.data_ptr(), (int)H);

  auto tslab = at::empty({L, S * H}, dy.options().dtype(at::kFloat));
  hipLaunchKernelGGL(
      embed3_bwd_pos_seg_kernel,
      dim3((unsigned)P, (unsigned)((H + 8 * EB_COLVECS - 1) / (8 * EB_COLVECS))),
      dim3(EB_COLVECS * EB_BSLICES), 0, stream, dyp,
      segment_ids.data_ptr<long>(), (bf16*)dp.data_ptr(),
      tslab.data_ptr<float>(), (int)B, (int)L, (int)H, (int)S);
  launch_slab_colsum<bf16, bf16>(tslab, dt.data_ptr(), (int)(S * H),
                                 dt.data_ptr(), stream);
  HIP_CHECK_LAST();
  return {dw, dp, dt};
}
