// Fused LayerNorm (fwd/bwd), residual-add+LayerNorm, bias+GELU, masked CE.
// SURVEY.md kernels K10/K11/K13: memory-bound rowwise ops, vectorized
// 8-wide bf16 loads (guide G13), fp32 statistics, one wave per row.
#include "common.h"
#include "gelu.h"
#include "slab_colsum.h"

// ---------------------------------------------------------------------
// LayerNorm forward: y = (x - mean) * rstd * w + b  (stats in fp32)
// one wave per row; H % 8 == 0
// ---------------------------------------------------------------------
template <typename T>
__global__ void layernorm_fwd_kernel(const T* __restrict__ x,
                                     const T* __restrict__ res,  // optional
                                     const float* __restrict__ w,
                                     const float* __restrict__ b,
                                     T* __restrict__ y,
                                     T* __restrict__ sum_out,  // optional x+res
                                     float* __restrict__ mean,
                                     float* __restrict__ rstd,
                                     int N, int H, float eps) {
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const long row = (long)blockIdx.x * (blockDim.x / WAVE) + wid;
  if (row >= N) return;
  const T* xr = x + row * H;
  const T* rr = res ? res + row * H : nullptr;
  float acc = 0.f, acc2 = 0.f;
  const int HV = H / 8;
  // static trip count keeps vals in registers (guide §5.4 rule 20)
  constexpr int MAXIT = 6;  // H <= 3072
  float vals[MAXIT][8];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int i = lane + it * WAVE;
    if (i < HV) {
    const s16x8 raw = reinterpret_cast<const s16x8*>(xr)[i];
    s16x8 raw2{};
    if (rr) raw2 = reinterpret_cast<const s16x8*>(rr)[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = to_f32(reinterpret_cast<const T*>(&raw)[e]);
      if (rr) v += to_f32(reinterpret_cast<const T*>(&raw2)[e]);
      vals[it][e] = v;
      acc += v;
      acc2 += v * v;
    }
    }
  }
  acc = wave_reduce_sum(acc);
  acc2 = wave_reduce_sum(acc2);
  const float m = acc / H;
  const float rs = rsqrtf(fmaxf(acc2 / H - m * m, 0.f) + eps);
  if (lane == 0) {
    mean[row] = m;
    rstd[row] = rs;
  }
  T* yr = y + row * H;
  T* sr = sum_out ? sum_out + row * H : nullptr;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int i = lane + it * WAVE;
    if (i < HV) {
    T out[8], sout[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = i * 8 + e;
      const float v = vals[it][e];
      from_f32((v - m) * rs * w[col] + b[col], &out[e]);
      if (sr) from_f32(v, &sout[e]);
    }
    reinterpret_cast<s16x8*>(yr)[i] = *reinterpret_cast<s16x8*>(out);
    if (sr) reinterpret_cast<s16x8*>(sr)[i] = *reinterpret_cast<s16x8*>(sout);
    }
  }
}

// fp32 specialization uses wider registers; keep one code path by
// reinterpreting through s16x8 only for 16-bit T. Provide a scalar body
// for float.
__global__ void layernorm_fwd_kernel_f32(const float* __restrict__ x,
                                         const float* __restrict__ res,
                                         const float* __restrict__ w,
                                         const float* __restrict__ b,
                                         float* __restrict__ y,
                                         float* __restrict__ sum_out,
                                         float* __restrict__ mean,
                                         float* __restrict__ rstd,
                                         int N, int H, float eps) {
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const long row = (long)blockIdx.x * (blockDim.x / WAVE) + wid;
  if (row >= N) return;
  const float* xr = x + row * H;
  const float* rr = res ? res + row * H : nullptr;
  float acc = 0.f, acc2 = 0.f;
  for (int i = lane; i < H; i += WAVE) {
    float v = xr[i] + (rr ? rr[i] : 0.f);
    acc += v;
    acc2 += v * v;
  }
  acc = wave_reduce_sum(acc);
  acc2 = wave_reduce_sum(acc2);
  const float m = acc / H;
  const float rs = rsqrtf(fmaxf(acc2 / H - m * m, 0.f) + eps);
  if (lane == 0) {
    mean[row] = m;
    rstd[row] = rs;
  }
  for (int i = lane; i < H; i += WAVE) {
    float v = xr[i] + (rr ? rr[i] : 0.f);
    if (sum_out) sum_out[row * H + i] = v;
    y[row * H + i] = (v - m) * rs * w[i] + b[i];
  }
}

// ---------------------------------------------------------------------
// LayerNorm backward.
// dx = rs * (dy*w - mean(dy*w) - xhat * mean(dy*w*xhat))
// dw += dy * xhat ; db += dy   (block-local LDS, then global atomics)
// ---------------------------------------------------------------------
template <typename T>
__global__ void layernorm_bwd_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const float* __restrict__ w,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     T* __restrict__ dx,
                                     float* __restrict__ dw,
                                     float* __restrict__ db,
                                     int N, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* dw_s = reinterpret_cast<float*>(smem_raw);
  float* db_s = dw_s + H;
  for (int i = threadIdx.x; i < 2 * H; i += blockDim.x) dw_s[i] = 0.f;
  __syncthreads();

  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int rows_per_blk = blockDim.x / WAVE;
  const long row = (long)blockIdx.x * rows_per_blk + wid;
  if (row < N) {
    const T* dyr = dy + row * H;
    const T* xr = x + row * H;
    const float m = mean[row], rs = rstd[row];
    float c1 = 0.f, c2 = 0.f;
    for (int i = lane; i < H; i += WAVE) {
      const float g = to_f32(dyr[i]) * w[i];
      const float xhat = (to_f32(xr[i]) - m) * rs;
      c1 += g * xhat;
      c2 += g;
    }
    c1 = wave_reduce_sum(c1) / H;
    c2 = wave_reduce_sum(c2) / H;
    T* dxr = dx + row * H;
    for (int i = lane; i < H; i += WAVE) {
      const float g = to_f32(dyr[i]) * w[i];
      const float d = to_f32(dyr[i]);
      const float xhat = (to_f32(xr[i]) - m) * rs;
      from_f32((g - c2 - xhat * c1) * rs, &dxr[i]);
      atomicAdd(&dw_s[i], d * xhat);
      atomicAdd(&db_s[i], d);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H; i += blockDim.x) {
    atomicAdd(&dw[i], dw_s[i]);
    atomicAdd(&db[i], db_s[i]);
  }
}


// fast bf16 backward, one pass, no global atomics. 16 rows per 4-wave
// block, 4 per wave, 2 blocks per CU at 8192 rows (holding two rows'
// loads explicitly, or 2 or 8 rows per wave, measured 2-5 us slower:
// profiles/fused_bwd_r03.md), vectorized loads.
// The column reductions (dw = sum dy*xhat, db = sum dy and, with DBIAS,
// the bias grad of the linear that feeds the dropout) accumulate in
// registers over a wave's rows, are combined across the block's waves
// through LDS in wave order, and leave as one fp32 partial row per
// block in slab[nblocks][K*H]; slab_colsum_kernel sums those per
// column. Plain stores instead of same-address atomics (guide G12), and
// the result is bitwise reproducible. H % 8 == 0, H <= 1024.
// DROPOUT also emits dx_drop = bf16(float(dsum_bf16) * mask * scale),
// the exact arithmetic of mask_scale_kernel on the stored dsum.
#define LNB_WAVES 4
#define LNB_RPW 4
#define LNB_ROWS (LNB_WAVES * LNB_RPW)

template <bool DROPOUT, bool DBIAS>
__global__ __launch_bounds__(LNB_WAVES * WAVE) void layernorm_bwd_bf16_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ x,
    const float* __restrict__ w, const float* __restrict__ mean,
    const float* __restrict__ rstd, const unsigned char* __restrict__ mask,
    bf16* __restrict__ dx, bf16* __restrict__ dx_drop,
    float* __restrict__ slab, long N, int H, float scale) {
  static_assert(DROPOUT || !DBIAS, "DBIAS needs DROPOUT");
  constexpr int K = DBIAS ? 3 : 2;
  constexpr int MAXC = 2;               // H <= 1024
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* part = reinterpret_cast<float*>(smem_raw);  // [LNB_WAVES][K*H]
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int HV = H / 8;                 // vec8 slots per row
  float dwp[MAXC][8] = {}, dbp[MAXC][8] = {}, dbiasp[MAXC][8] = {};
  float wv[MAXC][8];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int i = lane + c * WAVE;
    if (i < HV) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(w + i * 8);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(w + i * 8 + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) wv[c][e] = e < 4 ? lo[e] : hi[e - 4];
    }
  }
  const long row0 = (long)blockIdx.x * LNB_ROWS + wid * LNB_RPW;
#pragma unroll
  for (int rr = 0; rr < LNB_RPW; ++rr) {
    const long row = row0 + rr;
    if (row >= N) break;                // wave-uniform
    const float m = mean[row], rs = rstd[row];
    s16x8 rd[MAXC], rx[MAXC];
    f32x2 rm[MAXC];                     // 8 mask bytes
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int i = lane + c * WAVE;
      if (i < HV) {
        rd[c] = reinterpret_cast<const s16x8*>(dy + row * H)[i];
        rx[c] = reinterpret_cast<const s16x8*>(x + row * H)[i];
        if (DROPOUT) rm[c] = reinterpret_cast<const f32x2*>(mask + row * H)[i];
      }
    }
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int i = lane + c * WAVE;
      if (i < HV) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = to_f32(reinterpret_cast<const bf16*>(&rd[c])[e]);
          const float hx =
              (to_f32(reinterpret_cast<const bf16*>(&rx[c])[e]) - m) * rs;
          const float g = d * wv[c][e];
          c1 += g * hx;
          c2 += g;
        }
      }
    }
    c1 = wave_reduce_sum(c1) / H;
    c2 = wave_reduce_sum(c2) / H;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int i = lane + c * WAVE;
      if (i < HV) {
        bf16 outv[8], dropv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          // d, xhat re-derived from the raw bf16 (same values as above)
          // rather than held in 32 more registers
          const float d = to_f32(reinterpret_cast<const bf16*>(&rd[c])[e]);
          const float hx =
              (to_f32(reinterpret_cast<const bf16*>(&rx[c])[e]) - m) * rs;
          const float g = d * wv[c][e];
          from_f32((g - c2 - hx * c1) * rs, &outv[e]);
          dwp[c][e] += d * hx;
          dbp[c][e] += d;
          if (DROPOUT) {
            const unsigned char mk =
                reinterpret_cast<const unsigned char*>(&rm[c])[e];
            dropv[e] = __float2bfloat16(to_f32(outv[e]) * mk * scale);
            if (DBIAS) dbiasp[c][e] += to_f32(dropv[e]);
          }
        }
        reinterpret_cast<s16x8*>(dx + row * H)[i] =
            *reinterpret_cast<s16x8*>(outv);
        if (DROPOUT)
          reinterpret_cast<s16x8*>(dx_drop + row * H)[i] =
              *reinterpret_cast<s16x8*>(dropv);
      }
    }
  }
  // per-wave partials -> LDS (every wave, also one without a valid row:
  // its zeros are part of the sum), then a fixed wave-order sum per
  // column -> this block's slab row, all K*H columns of it
  float* mine = part + (long)wid * K * H;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int i = lane + c * WAVE;
    if (i < HV) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        mine[i * 8 + e] = dwp[c][e];
        mine[H + i * 8 + e] = dbp[c][e];
        if (DBIAS) mine[2 * H + i * 8 + e] = dbiasp[c][e];
      }
    }
  }
  __syncthreads();
  float* srow = slab + (long)blockIdx.x * K * H;
  for (int i = threadIdx.x; i < K * H; i += blockDim.x) {
    float a = part[i];
#pragma unroll
    for (int v = 1; v < LNB_WAVES; ++v) a += part[(long)v * K * H + i];
    srow[i] = a;
  }
}

// bias + GELU: gelu_f, dgelu_f and load_bias8 live in gelu.h, shared with the
// FFN GEMM epilogues of gemm_nt.hip
template <typename T, typename BT>
__global__ void bias_gelu_kernel(const T* __restrict__ x,
                                 const BT* __restrict__ bias,
                                 T* __restrict__ out, long n, int F) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nv = n / 8;
  for (long v = i; v < nv; v += (long)gridDim.x * blockDim.x) {
    const s16x8 raw = reinterpret_cast<const s16x8*>(x)[v];
    const int col0 = (int)((v * 8) % F);
    float be[8];
    load_bias8(bias, col0, be);
    T o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float u = to_f32(reinterpret_cast<const T*>(&raw)[e]) + be[e];
      from_f32(gelu_f(u), &o[e]);
    }
    reinterpret_cast<s16x8*>(out)[v] = *reinterpret_cast<s16x8*>(o);
  }
}

// backward with the bias grad fused: grid (column chunk, row chunk);
// a thread owns one vec8 column slot, walks the rows of its chunk and
// accumulates sum float(dx_bf16) in registers; the block's partial row
// goes to slab[row chunk][F] for slab_colsum_kernel. Every block writes
// all the columns of its chunk, so the slab needs no zero-fill.
#define BGB_THREADS 64
#define BGB_ROWS 16
template <typename T, typename BT>
__global__ __launch_bounds__(BGB_THREADS) void bias_gelu_bwd_kernel(
    const T* __restrict__ x, const BT* __restrict__ bias,
    const T* __restrict__ dy, T* __restrict__ dx, float* __restrict__ slab,
    long M, int F) {
  const int slot = blockIdx.x * BGB_THREADS + threadIdx.x;
  if (slot >= F / 8) return;
  const int col0 = slot * 8;
  float be[8], acc[8] = {};
  load_bias8(bias, col0, be);
  const long r0 = (long)blockIdx.y * BGB_ROWS;
  const long r1 = min(M, r0 + BGB_ROWS);
#pragma unroll 4
  for (long r = r0; r < r1; ++r) {
    const long off = r * F + col0;
    const s16x8 raw = *reinterpret_cast<const s16x8*>(x + off);
    const s16x8 draw = *reinterpret_cast<const s16x8*>(dy + off);
    T o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float u = to_f32(reinterpret_cast<const T*>(&raw)[e]) + be[e];
      const float g = to_f32(reinterpret_cast<const T*>(&draw)[e]);
      from_f32(g * dgelu_f(u), &o[e]);
      acc[e] += to_f32(o[e]);
    }
    *reinterpret_cast<s16x8*>(dx + off) = *reinterpret_cast<s16x8*>(o);
  }
  float* srow = slab + (long)blockIdx.y * F + col0;
  *reinterpret_cast<f32x4*>(srow) = f32x4{acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<f32x4*>(srow + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

__global__ void bias_gelu_kernel_f32(const float* __restrict__ x,
                                     const float* __restrict__ bias,
                                     const float* __restrict__ dy, bool bwd,
                                     float* __restrict__ out, long n, int F) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long v = i; v < n; v += (long)gridDim.x * blockDim.x) {
    const float u = x[v] + bias[v % F];
    out[v] = bwd ? dy[v] * dgelu_f(u) : gelu_f(u);
  }
}

// ---------------------------------------------------------------------
// masked softmax-CE over [N, T] logits (fp32), one thread per row.
// fwd also writes probs for bwd. loss = sum(per-row) / nvalid.
// ---------------------------------------------------------------------
__global__ void masked_ce_fwd_kernel(const float* __restrict__ logits,
                                     const int* __restrict__ labels,
                                     const int* __restrict__ mask,
                                     float* __restrict__ probs,
                                     float* __restrict__ loss_sum,
                                     int* __restrict__ nvalid, long N, int T) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* red = reinterpret_cast<float*>(smem_raw);
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float my_loss = 0.f;
  int my_valid = 0;
  if (r < N) {
    const float* lr = logits + r * T;
    float mx = -1e30f;
    for (int t = 0; t < T; ++t) mx = fmaxf(mx, lr[t]);
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += __expf(lr[t] - mx);
    // log-softmax as (x - max) - log(sum): adding max to log(sum) first
    // rounds at ulp(|max|) and costs that much in every prob (1e-5
    // relative at logits of +-100)
    const float ls = __logf(s);
    for (int t = 0; t < T; ++t) probs[r * T + t] = __expf((lr[t] - mx) - ls);
    if (mask[r]) {
      my_loss = ls - (lr[labels[r]] - mx);
      my_valid = 1;
    }
  }
  const float tot = block_reduce_sum(my_loss, red);
  __syncthreads();
  const float nv = block_reduce_sum((float)my_valid, red);
  if (threadIdx.x == 0) {
    atomicAdd(loss_sum, tot);
    atomicAdd(nvalid, (int)nv);
  }
}

__global__ void masked_ce_bwd_kernel(const float* __restrict__ probs,
                                     const int* __restrict__ labels,
                                     const int* __restrict__ mask,
                                     const float* __restrict__ dloss,
                                     const int* __restrict__ nvalid,
                                     float* __restrict__ dlogits, long N, int T) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= N) return;
  const float scale = mask[r] ? dloss[0] / (float)max(*nvalid, 1) : 0.f;
  for (int t = 0; t < T; ++t) {
    const float oh = (t == labels[r]) ? 1.f : 0.f;
    dlogits[r * T + t] = (probs[r * T + t] - oh) * scale;
  }
}

// =====================================================================
// host wrappers
// =====================================================================
static std::vector<at::Tensor> layernorm_fwd_impl(const at::Tensor& x,
                                                  const c10::optional<at::Tensor>& res,
                                                  const at::Tensor& w,
                                                  const at::Tensor& b,
                                                  double eps, bool want_sum) {
  CHECK_CUDA_CONTIG(x);
  const long N = x.size(0);
  const int H = x.size(1);
  TORCH_CHECK(H % 8 == 0, "layernorm: H % 8 != 0");
  auto y = at::empty_like(x);
  auto sum = want_sum ? at::empty_like(x) : at::Tensor();
  auto mean = at::empty({N}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({N}, x.options().dtype(at::kFloat));
  auto wf = w.to(at::kFloat).contiguous();
  auto bf = b.to(at::kFloat).contiguous();
  const int rows_per_blk = 4;
  const dim3 grid((N + rows_per_blk - 1) / rows_per_blk);
  const dim3 block(rows_per_blk * WAVE);
  auto stream = cur_stream(x);
  if (x.scalar_type() == at::kBFloat16) {
    TORCH_CHECK(H <= 3072, "layernorm bf16 kernel: H too large");
    hipLaunchKernelGGL(layernorm_fwd_kernel<bf16>, grid, block, 0, stream,
                       (const bf16*)x.data_ptr(),
                       res ? (const bf16*)res->data_ptr() : nullptr,
                       wf.data_ptr<float>(), bf.data_ptr<float>(),
                       (bf16*)y.data_ptr(),
                       want_sum ? (bf16*)sum.data_ptr() : nullptr,
                       mean.data_ptr<float>(), rstd.data_ptr<float>(), N, H,
                       (float)eps);
  } else {
    hipLaunchKernelGGL(layernorm_fwd_kernel_f32, grid, block, 0, stream,
                       x.data_ptr<float>(),
                       res ? res->data_ptr<float>() : nullptr,
                       wf.data_ptr<float>(), bf.data_ptr<float>(),
                       y.data_ptr<float>(),
                       want_sum ? sum.data_ptr<float>() : nullptr,
                       mean.data_ptr<float>(), rstd.data_ptr<float>(), N, H,
                       (float)eps);
  }
  HIP_CHECK_LAST();
  if (want_sum) return {y, sum, mean, rstd};
  return {y, mean, rstd};
}

std::vector<at::Tensor> layernorm_fwd(const at::Tensor& x, const at::Tensor& w,
                                      const at::Tensor& b, double eps) {
  return layernorm_fwd_impl(x, c10::nullopt, w, b, eps, false);
}

std::vector<at::Tensor> add_layernorm_fwd(const at::Tensor& x,
                                          const at::Tensor& res,
                                          const at::Tensor& w,
                                          const at::Tensor& b, double eps) {
  CHECK_CUDA_CONTIG(res);
  TORCH_CHECK(res.scalar_type() == x.scalar_type(),
              "add_layernorm: x/residual dtype mismatch");
  return layernorm_fwd_impl(x, res, w, b, eps, true);
}

// bf16 LN backward on the one-pass kernel. mask undefined: plain LN
// backward -> {dx, dw, db}; mask defined: the dropout+add+LN backward ->
// {dsum, dx_drop, dw, db, dbias-or-undefined}. dw/db come out in w's
// dtype, dbias in the activation dtype, straight from the finisher.
static std::vector<at::Tensor> layernorm_bwd_bf16(
    const at::Tensor& dy, const at::Tensor& x, const at::Tensor& w,
    const at::Tensor& mean, const at::Tensor& rstd, const at::Tensor& mask,
    double keep, bool want_dbias) {
  const long N = x.size(0);
  const int H = x.size(1);
  TORCH_CHECK(H % 8 == 0 && H <= 1024, "layernorm bwd bf16: bad H ", H);
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 && dy.numel() == x.numel(),
              "layernorm bwd bf16: dy must be bf16 of x's shape");
  TORCH_CHECK(mean.is_cuda() && mean.is_contiguous() &&
                  mean.scalar_type() == at::kFloat && mean.numel() == N &&
                  rstd.is_cuda() && rstd.is_contiguous() &&
                  rstd.scalar_type() == at::kFloat && rstd.numel() == N,
              "layernorm bwd bf16: mean/rstd must be fp32 [N]");
  TORCH_CHECK(w.is_cuda() && w.numel() == H, "layernorm bwd bf16: bad weight");
  const bool dropout = mask.defined();
  if (dropout) {
    TORCH_CHECK(mask.is_cuda() && mask.is_contiguous() &&
                    mask.scalar_type() == at::kByte &&
                    mask.numel() == x.numel(),
                "dropout_add_ln_bwd: mask must be uint8 of x's shape");
  }
  const int K = (dropout && want_dbias) ? 3 : 2;
  const long nblocks = std::max<long>((N + LNB_ROWS - 1) / LNB_ROWS, 1);
  auto dx = at::empty_like(x);
  auto dx_drop = dropout ? at::empty_like(x) : at::Tensor();
  auto wf = w.to(at::kFloat).contiguous();
  auto slab = at::empty({nblocks, (long)K * H}, x.options().dtype(at::kFloat));
  const bool w_bf16 = w.scalar_type() == at::kBFloat16;
  // other weight dtypes: finish in fp32 and cast
  auto dwdb = at::empty(
      {2, (long)H}, x.options().dtype(w_bf16 ? at::kBFloat16 : at::kFloat));
  auto dbias = K == 3 ? at::empty({(long)H}, x.options()) : at::Tensor();
  const size_t smem = (size_t)LNB_WAVES * K * H * sizeof(float);
  const float scale = (float)(1.0 / keep);
  auto stream = cur_stream(x);
#define LNB_LAUNCH(DROPOUT, DBIAS)                                           \
  hipLaunchKernelGGL((layernorm_bwd_bf16_kernel<DROPOUT, DBIAS>),            \
                     dim3((unsigned)nblocks), dim3(LNB_WAVES * WAVE), smem,  \
                     stream, (const bf16*)dy.data_ptr(),                     \
                     (const bf16*)x.data_ptr(), wf.data_ptr<float>(),        \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),         \
                     dropout ? mask.data_ptr<unsigned char>() : nullptr,     \
                     (bf16*)dx.data_ptr(),                                   \
                     dropout ? (bf16*)dx_drop.data_ptr() : nullptr,          \
                     slab.data_ptr<float>(), N, H, scale)
  if (K == 3) {
    LNB_LAUNCH(true, true);
  } else if (dropout) {
    LNB_LAUNCH(true, false);
  } else {
    LNB_LAUNCH(false, false);
  }
#undef LNB_LAUNCH
  void* ob = K == 3 ? dbias.data_ptr() : nullptr;
  if (w_bf16)
    launch_slab_colsum<bf16, bf16>(slab, dwdb.data_ptr(), 2 * H, ob, stream);
  else
    launch_slab_colsum<float, bf16>(slab, dwdb.data_ptr(), 2 * H, ob, stream);
  HIP_CHECK_LAST();
  auto dw = dwdb[0], db = dwdb[1];
  if (dw.scalar_type() != w.scalar_type()) {
    dw = dw.to(w.scalar_type());
    db = db.to(w.scalar_type());
  }
  if (dropout) return {dx, dx_drop, dw, db, dbias};
  return {dx, dw, db};
}

std::vector<at::Tensor> dropout_add_ln_bwd(
    const at::Tensor& dy, const at::Tensor& s, const at::Tensor& w,
    const at::Tensor& mean, const at::Tensor& rstd, const at::Tensor& mask,
    double keep, bool want_dbias) {
  CHECK_CUDA_CONTIG(dy);
  CHECK_CUDA_CONTIG(s);
  TORCH_CHECK(s.scalar_type() == at::kBFloat16 && s.dim() == 2,
              "dropout_add_ln_bwd: bf16 [N, H] only");
  TORCH_CHECK(mask.defined() && keep > 0.0,
              "dropout_add_ln_bwd: needs the saved mask and keep > 0");
  return layernorm_bwd_bf16(dy, s, w, mean, rstd, mask, keep, want_dbias);
}

std::vector<at::Tensor> layernorm_bwd(const at::Tensor& dy, const at::Tensor& x,
                                      const at::Tensor& w, const at::Tensor& mean,
                                      const at::Tensor& rstd) {
  CHECK_CUDA_CONTIG(dy);
  CHECK_CUDA_CONTIG(x);
  if (x.scalar_type() == at::kBFloat16)
    return layernorm_bwd_bf16(dy, x, w, mean, rstd, at::Tensor(), 1.0, false);
  const long N = x.size(0);
  const int H = x.size(1);
  auto dx = at::empty_like(x);
  auto dw = at::zeros({H}, x.options().dtype(at::kFloat));
  auto db = at::zeros({H}, x.options().dtype(at::kFloat));
  auto wf = w.to(at::kFloat).contiguous();
  const size_t smem = 2 * H * sizeof(float);
  auto stream = cur_stream(x);
  {
    const int rows_per_blk = 4;
    const dim3 grid((N + rows_per_blk - 1) / rows_per_blk);
    const dim3 block(rows_per_blk * WAVE);
    hipLaunchKernelGGL(layernorm_bwd_kernel<float>, grid, block, smem, stream,
                       dy.data_ptr<float>(), x.data_ptr<float>(),
                       wf.data_ptr<float>(), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), dx.data_ptr<float>(),
                       dw.data_ptr<float>(), db.data_ptr<float>(), N, H);
  }
  HIP_CHECK_LAST();
  return {dx, dw.to(w.scalar_type()), db.to(w.scalar_type())};
}

// bias in its stored dtype when the kernels can read it in place (bf16
// or fp32, contiguous), else an fp32 copy
static at::Tensor bias_gelu_bias(const at::Tensor& bias, int F) {
  TORCH_CHECK(bias.is_cuda() && bias.numel() == F, "bias_gelu: bad bias");
  if (bias.is_contiguous() && (bias.scalar_type() == at::kBFloat16 ||
                               bias.scalar_type() == at::kFloat))
    return bias;
  return bias.to(at::kFloat).contiguous();
}

at::Tensor bias_gelu_fwd(const at::Tensor& x, const at::Tensor& bias) {
  CHECK_CUDA_CONTIG(x);
  const long n = x.numel();
  const int F = x.size(-1);
  TORCH_CHECK(F % 8 == 0, "bias_gelu: F % 8 != 0");
  auto out = at::empty_like(x);
  auto stream = cur_stream(x);
  const int block = 256;
  if (x.scalar_type() == at::kBFloat16) {
    auto b = bias_gelu_bias(bias, F);
    const long grid = std::min<long>((n / 8 + block - 1) / block, 32768);
    if (b.scalar_type() == at::kBFloat16)
      hipLaunchKernelGGL((bias_gelu_kernel<bf16, bf16>), dim3(grid),
                         dim3(block), 0, stream, (const bf16*)x.data_ptr(),
                         (const bf16*)b.data_ptr(), (bf16*)out.data_ptr(), n,
                         F);
    else
      hipLaunchKernelGGL((bias_gelu_kernel<bf16, float>), dim3(grid),
                         dim3(block), 0, stream, (const bf16*)x.data_ptr(),
                         b.data_ptr<float>(), (bf16*)out.data_ptr(), n, F);
  } else {
    auto bf = bias.to(at::kFloat).contiguous();
    const long grid = std::min<long>((n + block - 1) / block, 4096);
    hipLaunchKernelGGL(bias_gelu_kernel_f32, dim3(grid), dim3(block), 0, stream,
                       x.data_ptr<float>(), bf.data_ptr<float>(), nullptr,
                       false, out.data_ptr<float>(), n, F);
  }
  HIP_CHECK_LAST();
  return out;
}

std::vector<at::Tensor> bias_gelu_bwd(const at::Tensor& dy, const at::Tensor& x,
                                      const at::Tensor& bias) {
  CHECK_CUDA_CONTIG(x);
  CHECK_CUDA_CONTIG(dy);
  const long n = x.numel();
  const int F = x.size(-1);
  TORCH_CHECK(F % 8 == 0, "bias_gelu: F % 8 != 0");
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() && dy.numel() == n,
              "bias_gelu_bwd: dy must match x");
  auto dx = at::empty_like(x);
  auto stream = cur_stream(x);
  if (x.scalar_type() != at::kBFloat16) {
    auto bf = bias.to(at::kFloat).contiguous();
    const int block = 256;
    const long grid = std::min<long>((n + block - 1) / block, 4096);
    hipLaunchKernelGGL(bias_gelu_kernel_f32, dim3(grid), dim3(block), 0, stream,
                       x.data_ptr<float>(), bf.data_ptr<float>(),
                       dy.data_ptr<float>(), true, dx.data_ptr<float>(), n, F);
    HIP_CHECK_LAST();
    auto dbias = at::sum(dx.reshape({-1, (long)F}), {0}, false, at::kFloat)
                     .to(bias.scalar_type());
    return {dx, dbias};
  }
  auto b = bias_gelu_bias(bias, F);
  const long M = n / F;
  const long nchunks = std::max<long>((M + BGB_ROWS - 1) / BGB_ROWS, 1);
  TORCH_CHECK(nchunks <= 65535, "bias_gelu_bwd: too many rows ", M);
  auto slab = at::empty({nchunks, (long)F}, x.options().dtype(at::kFloat));
  const bool b_bf16 = b.scalar_type() == at::kBFloat16;
  auto dbias = at::empty({(long)F},
                         x.options().dtype(b_bf16 ? at::kBFloat16 : at::kFloat));
  const dim3 grid((F / 8 + BGB_THREADS - 1) / BGB_THREADS, (unsigned)nchunks);
  if (b_bf16) {
    hipLaunchKernelGGL((bias_gelu_bwd_kernel<bf16, bf16>), grid,
                       dim3(BGB_THREADS), 0, stream, (const bf16*)x.data_ptr(),
                       (const bf16*)b.data_ptr(), (const bf16*)dy.data_ptr(),
                       (bf16*)dx.data_ptr(), slab.data_ptr<float>(), M, F);
    launch_slab_colsum<bf16, bf16>(slab, dbias.data_ptr(), F, nullptr, stream);
  } else {
    hipLaunchKernelGGL((bias_gelu_bwd_kernel<bf16, float>), grid,
                       dim3(BGB_THREADS), 0, stream, (const bf16*)x.data_ptr(),
                       b.data_ptr<float>(), (const bf16*)dy.data_ptr(),
                       (bf16*)dx.data_ptr(), slab.data_ptr<float>(), M, F);
    launch_slab_colsum<float, float>(slab, dbias.data_ptr(), F, nullptr,
                                     stream);
  }
  HIP_CHECK_LAST();
  if (dbias.scalar_type() != bias.scalar_type())
    dbias = dbias.to(bias.scalar_type());
  return {dx, dbias};
}

std::vector<at::Tensor> masked_ce_fwd(const at::Tensor& logits,
                                      const at::Tensor& labels,
                                      const at::Tensor& mask) {
  CHECK_CUDA_CONTIG(logits);
  const long N = logits.size(0);
  const int T = logits.size(1);
  auto probs = at::empty_like(logits);
  auto loss = at::zeros({}, logits.options());
  auto nvalid = at::zeros({}, logits.options().dtype(at::kInt));
  const int block = 256;
  const long grid = (N + block - 1) / block;
  hipLaunchKernelGGL(masked_ce_fwd_kernel, dim3(grid), dim3(block),
                     (block / WAVE) * sizeof(float) * 2, cur_stream(logits),
                     logits.data_ptr<float>(), labels.data_ptr<int>(),
                     mask.data_ptr<int>(), probs.data_ptr<float>(),
                     loss.data_ptr<float>(), nvalid.data_ptr<int>(), N, T);
  HIP_CHECK_LAST();
  auto mean = loss / at::clamp_min(nvalid, 1).to(at::kFloat);
  return {mean, probs, nvalid};
}

at::Tensor masked_ce_bwd(const at::Tensor& dloss, const at::Tensor& probs,
                         const at::Tensor& labels, const at::Tensor& mask,
                         const at::Tensor& nvalid) {
  const long N = probs.size(0);
  const int T = probs.size(1);
  auto dlogits = at::empty_like(probs);
  const int block = 256;
  hipLaunchKernelGGL(masked_ce_bwd_kernel, dim3((N + block - 1) / block),
                     dim3(block), 0, cur_stream(probs), probs.data_ptr<float>(),
                     labels.data_ptr<int>(), mask.data_ptr<int>(),
                     dloss.to(at::kFloat).contiguous().data_ptr<float>(),
                     nvalid.data_ptr<int>(), dlogits.data_ptr<float>(), N, T);
  HIP_CHECK_LAST();
  return dlogits;
}

// ---------------------------------------------------------------------
// column sum for bias gradients: dy [M,N] -> db [N] (fp32 accumulation,
// coalesced row-chunk blocks + one atomic per (block, column)).
// torch's generic reduce runs ~4.5x off memory bound for this shape.
// ---------------------------------------------------------------------
template <typename T>
__global__ void colsum_kernel(const T* __restrict__ dy, float* __restrict__ ws,
                              long M, int N, int rows_per_chunk) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= N) return;
  const long r0 = (long)blockIdx.y * rows_per_chunk;
  const long r1 = min(M, r0 + rows_per_chunk);
  float acc = 0.f;
  for (long r = r0; r < r1; ++r) acc += to_f32(dy[r * N + c]);
  atomicAdd(&ws[c], acc);
}

template <typename T>
__global__ void colsum_cast_kernel(const float* __restrict__ ws,
                                   T* __restrict__ out, int N) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < N) from_f32(ws[c], &out[c]);
}

at::Tensor colsum(const at::Tensor& dy) {
  CHECK_CUDA_CONTIG(dy);
  const long M = dy.size(0);
  const int N = dy.size(1);
  auto ws = at::zeros({N}, dy.options().dtype(at::kFloat));
  auto out = at::empty({N}, dy.options());
  const int block = 256;
  const int rows_per_chunk = 64;
  const dim3 grid((N + block - 1) / block,
                  (unsigned)((M + rows_per_chunk - 1) / rows_per_chunk));
  auto stream = cur_stream(dy);
  if (dy.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL(colsum_kernel<bf16>, grid, dim3(block), 0, stream,
                       (const bf16*)dy.data_ptr(), ws.data_ptr<float>(), M, N,
                       rows_per_chunk);
    hipLaunchKernelGGL(colsum_cast_kernel<bf16>, dim3((N + 255) / 256),
                       dim3(256), 0, stream, ws.data_ptr<float>(),
                       (bf16*)out.data_ptr(), N);
  } else {
    hipLaunchKernelGGL(colsum_kernel<float>, grid, dim3(block), 0, stream,
                       dy.data_ptr<float>(), ws.data_ptr<float>(), M, N,
                       rows_per_chunk);
    hipLaunchKernelGGL(colsum_cast_kernel<float>, dim3((N + 255) / 256),
                       dim3(256), 0, stream, ws.data_ptr<float>(),
                       out.data_ptr<float>(), N);
  }
  HIP_CHECK_LAST();
  return out;
}

// ---------------------------------------------------------------------
// fused dropout + residual-add + LayerNorm (the BERT post-LN pattern:
// LN(dropout(sublayer_out) + x)). Counter-based RNG (splitmix64 hash of
// (step_counter, element)) — the device counter is bumped by a 1-thread
// kernel after each call, so hipGraph replays draw fresh masks.
// ---------------------------------------------------------------------
__device__ __forceinline__ float hash_uniform(unsigned long long ctr,
                                              unsigned long long idx) {
  unsigned long long z = ctr * 0x9E3779B97F4A7C15ull ^ idx;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (float)(z >> 40) * (1.f / 16777216.f);  // top 24 bits -> [0,1)
}

__global__ void dropout_add_ln_fwd_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ res,
    const float* __restrict__ w, const float* __restrict__ b,
    bf16* __restrict__ y, bf16* __restrict__ sum_out,
    unsigned char* __restrict__ mask_out, float* __restrict__ mean,
    float* __restrict__ rstd, const unsigned long long* __restrict__ ctr,
    long N, int H, float eps, float keep) {
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const long row = (long)blockIdx.x * (blockDim.x / WAVE) + wid;
  if (row >= N) return;
  const unsigned long long c = *ctr;
  const float inv_keep = 1.f / keep;
  const bf16* xr = x + row * H;
  const bf16* rr = res + row * H;
  float acc = 0.f, acc2 = 0.f;
  const int HV = H / 8;
  constexpr int MAXIT = 6;  // H <= 3072
  float vals[MAXIT][8];
  unsigned char mks[MAXIT][8];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int i = lane + it * WAVE;
    if (i < HV) {
      const s16x8 rx = reinterpret_cast<const s16x8*>(xr)[i];
      const s16x8 rres = reinterpret_cast<const s16x8*>(rr)[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const long idx = row * H + i * 8 + e;
        const unsigned char m = hash_uniform(c, (unsigned long long)idx) < keep;
        mks[it][e] = m;
        const float xv =
            to_f32(reinterpret_cast<const bf16*>(&rx)[e]) * m * inv_keep +
            to_f32(reinterpret_cast<const bf16*>(&rres)[e]);
        vals[it][e] = xv;
        acc += xv;
        acc2 += xv * xv;
      }
    }
  }
  acc = wave_reduce_sum(acc);
  acc2 = wave_reduce_sum(acc2);
  const float mu = acc / H;
  const float var = fmaxf(acc2 / H - mu * mu, 0.f);
  const float rs = rsqrtf(var + eps);
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
  bf16* yr = y + row * H;
  bf16* sr = sum_out + row * H;
  unsigned char* mr = mask_out + row * H;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int i = lane + it * WAVE;
    if (i < HV) {
      bf16 ov[8], sv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float s = vals[it][e];
        sv[e] = __float2bfloat16(s);
        ov[e] = __float2bfloat16((s - mu) * rs * w[i * 8 + e] + b[i * 8 + e]);
        mr[i * 8 + e] = mks[it][e];
      }
      reinterpret_cast<s16x8*>(yr)[i] = *reinterpret_cast<s16x8*>(ov);
      reinterpret_cast<s16x8*>(sr)[i] = *reinterpret_cast<s16x8*>(sv);
    }
  }
}

__global__ void bump_counter_kernel(unsigned long long* ctr) { ++(*ctr); }

// dx_drop = dsum * mask / keep (the dropout half of the fused bwd; the
// LN half reuses layernorm_bwd on the stored sum, giving dsum = dres)
__global__ void mask_scale_kernel(const bf16* __restrict__ dsum,
                                  const unsigned char* __restrict__ mask,
                                  bf16* __restrict__ dx, long n, float scale) {
  const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i0 + 7 >= n) {
    for (long i = i0; i < n; ++i)
      dx[i] = __float2bfloat16(to_f32(dsum[i]) * mask[i] * scale);
    return;
  }
  const s16x8 d = *reinterpret_cast<const s16x8*>(dsum + i0);
  bf16 o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
    o[e] = __float2bfloat16(to_f32(reinterpret_cast<const bf16*>(&d)[e]) *
                            mask[i0 + e] * scale);
  *reinterpret_cast<s16x8*>(dx + i0) = *reinterpret_cast<const s16x8*>(o);
}

std::vector<at::Tensor> dropout_add_ln_fwd(const at::Tensor& x,
                                           const at::Tensor& res,
                                           const at::Tensor& w,
                                           const at::Tensor& b, double eps,
                                           double keep,
                                           const at::Tensor& counter) {
  CHECK_CUDA_CONTIG(x);
  CHECK_CUDA_CONTIG(res);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "dropout_add_ln: bf16 only");
  const long N = x.size(0);
  const int H = x.size(1);
  TORCH_CHECK(H % 8 == 0 && H <= 3072, "dropout_add_ln: bad H ", H);
  auto y = at::empty_like(x);
  auto sum = at::empty_like(x);
  auto mask = at::empty({N, (long)H}, x.options().dtype(at::kByte));
  auto mean = at::empty({N}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({N}, x.options().dtype(at::kFloat));
  auto wf = w.to(at::kFloat).contiguous();
  auto bf = b.to(at::kFloat).contiguous();
  const int rows_per_blk = 4;
  auto stream = cur_stream(x);
  hipLaunchKernelGGL(dropout_add_ln_fwd_kernel,
                     dim3((N + rows_per_blk - 1) / rows_per_blk),
                     dim3(rows_per_blk * WAVE), 0, stream,
                     (const bf16*)x.data_ptr(), (const bf16*)res.data_ptr(),
                     wf.data_ptr<float>(), bf.data_ptr<float>(),
                     (bf16*)y.data_ptr(), (bf16*)sum.data_ptr(),
                     mask.data_ptr<unsigned char>(), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(),
                     (const unsigned long long*)counter.data_ptr(), N, H,
                     (float)eps, (float)keep);
  hipLaunchKernelGGL(bump_counter_kernel, dim3(1), dim3(1), 0, stream,
                     (unsigned long long*)counter.data_ptr());
  HIP_CHECK_LAST();
  return {y, sum, mask, mean, rstd};
}

at::Tensor mask_scale(const at::Tensor& dsum, const at::Tensor& mask,
                      double scale) {
  CHECK_CUDA_CONTIG(dsum);
  auto dx = at::empty_like(dsum);
  const long n = dsum.numel();
  const int block = 256;
  const long grid = std::min<long>((n / 8 + block - 1) / block, 32768);
  hipLaunchKernelGGL(mask_scale_kernel, dim3(grid), dim3(block), 0,
                     cur_stream(dsum), (const bf16*)dsum.data_ptr(),
                     mask.data_ptr<unsigned char>(), (bf16*)dx.data_ptr(), n,
                     (float)scale);
  HIP_CHECK_LAST();
  return dx;
}

void bump_counter(const at::Tensor& ctr) {
  hipLaunchKernelGGL(bump_counter_kernel, dim3(1), dim3(1), 0,
                     cur_stream(ctr), (unsigned long long*)ctr.data_ptr());
  HIP_CHECK_LAST();
}
