// Multi-tensor AdamWeightDecay: one launch updates every
// parameter in a group. BERT AdamWeightDecay math (no bias correction,
// decoupled weight decay — reference tools/train_utils.py:276-284):
//   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g^2
//   p -= lr * (m / (sqrt(v)+eps) + wd*p)
//
// Two parameter modes:
//  - fp32 params: p/g/m/v all fp32 (CPU-parity path)
//  - bf16 params: model weights + grads bf16, fp32 MASTER copy updated in
//    fp32 and rounded back to the bf16 weight — the MI355X-native "pure
//    bf16" training mode (no autocast weight-cast kernels per step).
// Plus a fused multi-tensor L2 norm for the global-norm gradient clip.
#include "common.h"

#define MAX_TENSORS 512

struct ChunkMeta {
  void* p;        // bf16 or fp32 weight
  const void* g;  // grad, same dtype as p
  float* master;  // fp32 master (nullptr when p is fp32)
  float* m;
  float* v;
  long n;
  float lr;
  float wd;
};

// One element: updates m and v in place and returns the new weight.
// step = lr_mul * lr. The fused multiply-adds are spelled out and the
// compiler's own contraction is off: left to itself hipcc contracts the
// same expression differently from one instantiation or loop to the
// next (fma(b1, m, (1-b1)*g) here, fma(1-b1, g, b1*m) there), and the
// kernels below must agree to the bit. This is the form the 4-wide loop
// has always compiled to.
__device__ __forceinline__ float adamw_elem(float gv, float& m, float& v,
                                            float pv, float b1, float b2,
                                            float eps, float step, float wd) {
#pragma clang fp contract(off)
  m = fmaf(b1, m, (1.f - b1) * gv);
  v = fmaf(b2, v, ((1.f - b2) * gv) * gv);
  const float u = fmaf(wd, pv, m * __frcp_rn(sqrtf(v) + eps));
  return fmaf(-step, u, pv);
}

// One tensor's update, shared by both kernels. g is the grad pointer
// (HAS_G false: "no gradient", treated as g = 0 — m and v still decay and
// weight decay still applies). SCALE folds the global-norm clip into the
// load: bf16 grads become f32(bf16_round(f32(g) * c)), fp32 grads g * c,
// bit for bit what multi_tensor_scale_kernel followed by a plain load
// gives for the same c.
template <typename T, bool SCALE, bool HAS_G>
__device__ __forceinline__ void adamw_tensor(const ChunkMeta& mt, const T* g,
                                             float c, float b1, float b2,
                                             float eps, float mul) {
#pragma clang fp contract(off)
  // explicit 4-wide vector I/O on every stream (g/p via 4x16b or f32x4,
  // m/v/master via f32x4) — scalar per-lane math in registers
  T* p = reinterpret_cast<T*>(mt.p);
  const float step = mul * mt.lr;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  for (; i + 3 < mt.n; i += stride) {
    float gv[4], pv[4];
    if (!HAS_G) {
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = 0.f;
    } else if (sizeof(T) == 2) {
      const s16x4 g4 = *reinterpret_cast<const s16x4*>(g + i);
      const bf16* gb = reinterpret_cast<const bf16*>(&g4);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        gv[e] = SCALE ? to_f32(__float2bfloat16(to_f32(gb[e]) * c))
                      : to_f32(gb[e]);
    } else {
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(
          reinterpret_cast<const float*>(g) + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = SCALE ? g4[e] * c : g4[e];
    }
    f32x4 m4 = *reinterpret_cast<const f32x4*>(mt.m + i);
    f32x4 v4 = *reinterpret_cast<const f32x4*>(mt.v + i);
    if (mt.master) {
      const f32x4 ma = *reinterpret_cast<const f32x4*>(mt.master + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) pv[e] = ma[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        pv[e] = sizeof(T) == 2
                    ? to_f32(p[i + e])
                    : reinterpret_cast<const float*>(p)[i + e];
    }
    f32x4 up;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float m = m4[e], v = v4[e];
      up[e] = adamw_elem(gv[e], m, v, pv[e], b1, b2, eps, step, mt.wd);
      m4[e] = m;
      v4[e] = v;
    }
    *reinterpret_cast<f32x4*>(mt.m + i) = m4;
    *reinterpret_cast<f32x4*>(mt.v + i) = v4;
    if (mt.master) *reinterpret_cast<f32x4*>(mt.master + i) = up;
    if (sizeof(T) == 2) {
      s16x4 p4;
      bf16* pb = reinterpret_cast<bf16*>(&p4);
#pragma unroll
      for (int e = 0; e < 4; ++e) pb[e] = __float2bfloat16(up[e]);
      *reinterpret_cast<s16x4*>(p + i) = p4;
    } else {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p) + i) = up;
    }
  }
  for (; i < mt.n; ++i) {  // ragged tail
    float gv = 0.f;
    if (HAS_G) {
      gv = to_f32(g[i]);
      if (SCALE) {
        T r;
        from_f32(gv * c, &r);
        gv = to_f32(r);
      }
    }
    float m = mt.m[i], v = mt.v[i];
    const float pv = mt.master ? mt.master[i] : to_f32(p[i]);
    const float upd = adamw_elem(gv, m, v, pv, b1, b2, eps, step, mt.wd);
    mt.m[i] = m;
    mt.v[i] = v;
    if (mt.master) mt.master[i] = upd;
    from_f32(upd, &p[i]);
  }
}

// lr_mul: optional device scalar multiplied into every tensor's lr —
// lets a hipGraph-captured step keep a live LR schedule (the schedule
// writes the device scalar outside the graph; meta.lr holds the
// per-group scale).
template <typename T>
__global__ void multi_tensor_adamw_kernel(ChunkMeta* metas, int n_tensors,
                                          float b1, float b2, float eps,
                                          const float* lr_mul) {
  const float mul = lr_mul ? *lr_mul : 1.f;
  for (int ti = blockIdx.y; ti < n_tensors; ti += gridDim.y) {
    const ChunkMeta mt = metas[ti];
    adamw_tensor<T, false, true>(mt, reinterpret_cast<const T*>(mt.g), 1.f,
                                 b1, b2, eps, mul);
  }
}

// Grad addresses by value: autograd.grad hands back fresh tensors every
// step, so their addresses cannot live in the cached blob, and a
// host-to-device copy is not capture-safe. A kernel argument needs
// neither; it is baked into the graph node at capture. 256 slots = 2 KB,
// well inside HIP's 4 KB argument block next to the other arguments.
// A null slot means "this parameter got no gradient".
#define GRAD_SLOTS 256

struct GradTable {
  const void* g[GRAD_SLOTS];
};

// Same schedule as multi_tensor_adamw_kernel; grads come from the
// by-value table and are scaled by *coef (the clip) as they load.
// metas points at this launch's first tensor.
template <typename T>
__global__ void multi_tensor_adamw_tab_kernel(const ChunkMeta* metas,
                                              int n_tensors, GradTable tab,
                                              float b1, float b2, float eps,
                                              const float* lr_mul,
                                              const float* coef) {
  const float mul = lr_mul ? *lr_mul : 1.f;
  const float c = coef ? *coef : 1.f;
  for (int ti = blockIdx.y; ti < n_tensors; ti += gridDim.y) {
    const ChunkMeta mt = metas[ti];
    const T* g = reinterpret_cast<const T*>(tab.g[ti]);
    if (g)
      adamw_tensor<T, true, true>(mt, g, c, b1, b2, eps, mul);
    else
      adamw_tensor<T, true, false>(mt, g, c, b1, b2, eps, mul);
  }
}

static void launch_adamw(std::vector<ChunkMeta>& metas, long total,
                         bool is_bf16, const at::Tensor& ref, double b1,
                         double b2, double eps, const float* lr_mul) {
  const int n = metas.size();
  auto meta_blob = at::from_blob(metas.data(), {(long)(n * sizeof(ChunkMeta))},
                                 at::TensorOptions().dtype(at::kByte))
                       .to(ref.device(), /*non_blocking=*/false);
  const int block = 256;
  const int gx = std::min<long>((total / n + block - 1) / block, 512);
  dim3 grid(std::max(gx, 1), std::min(n, 64));
  auto stream = cur_stream(ref);
  if (is_bf16) {
    hipLaunchKernelGGL(multi_tensor_adamw_kernel<bf16>, grid, dim3(block), 0,
                       stream, (ChunkMeta*)meta_blob.data_ptr(), n, (float)b1,
                       (float)b2, (float)eps, lr_mul);
  } else {
    hipLaunchKernelGGL(multi_tensor_adamw_kernel<float>, grid, dim3(block), 0,
                       stream, (ChunkMeta*)meta_blob.data_ptr(), n, (float)b1,
                       (float)b2, (float)eps, lr_mul);
  }
  HIP_CHECK_LAST();
}

// Build the device-side ChunkMeta blob once (H2D copy here) so a
// hipGraph-captured step can run the kernel without any host transfer.
// Returns {blob, [total, n, is_bf16]}.
std::vector<at::Tensor> adamw_build_meta(
    std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
    std::vector<at::Tensor> masters, std::vector<at::Tensor> ms,
    std::vector<at::Tensor> vs, std::vector<double> lrs,
    std::vector<double> wds) {
  const int n = params.size();
  TORCH_CHECK(n > 0 && n <= MAX_TENSORS, "adamw_build_meta: bad count");
  const bool has_master = !masters.empty();
  const bool is_bf16 = params[0].scalar_type() == at::kBFloat16;
  // grads may be empty: the blob then serves multi_tensor_adamw_tab_run,
  // which takes the grad addresses by value
  TORCH_CHECK(grads.empty() || (int)grads.size() == n,
              "adamw_build_meta: grads must be empty or one per param");
  std::vector<ChunkMeta> metas(n);
  long total = 0;
  for (int i = 0; i < n; ++i) {
    metas[i] = {params[i].data_ptr(),
                grads.empty() ? nullptr : grads[i].data_ptr(),
                has_master ? masters[i].data_ptr<float>() : nullptr,
                ms[i].data_ptr<float>(), vs[i].data_ptr<float>(),
                params[i].numel(), (float)lrs[i], (float)wds[i]};
    total += metas[i].n;
  }
  auto blob = at::from_blob(metas.data(), {(long)(n * sizeof(ChunkMeta))},
                            at::TensorOptions().dtype(at::kByte))
                  .to(params[0].device(), false);
  auto info = at::tensor({total, (long)n, (long)(is_bf16 ? 1 : 0)},
                         at::TensorOptions().dtype(at::kLong));
  return {blob, info};
}

// Capture-safe launch from a prebuilt blob (no host transfers).
void multi_tensor_adamw_run(const at::Tensor& blob, long total, long n,
                            bool is_bf16, double b1, double b2, double eps,
                            c10::optional<at::Tensor> lr_mul) {
  const int block = 256;
  const int gx = std::min<long>((total / n + block - 1) / block, 512);
  dim3 grid(std::max(gx, 1), std::min<long>(n, 64));
  auto stream = cur_stream(blob);
  const float* mul = nullptr;
  if (lr_mul.has_value()) mul = lr_mul->data_ptr<float>();
  if (is_bf16) {
    hipLaunchKernelGGL(multi_tensor_adamw_kernel<bf16>, grid, dim3(block), 0,
                       stream, (ChunkMeta*)blob.data_ptr(), (int)n, (float)b1,
                       (float)b2, (float)eps, mul);
  } else {
    hipLaunchKernelGGL(multi_tensor_adamw_kernel<float>, grid, dim3(block), 0,
                       stream, (ChunkMeta*)blob.data_ptr(), (int)n, (float)b1,
                       (float)b2, (float)eps, mul);
  }
  HIP_CHECK_LAST();
}

// What a by-value slot may point at: a contiguous GPU tensor of the
// parameter's dtype and size whose address suits 16-byte vector loads.
// No gradient (None) gives a null slot. Callers route a grad that fails
// through a copy first; a failure here is an error, not a fallback.
static const void* tab_grad_ptr(const c10::optional<at::Tensor>& g,
                                bool is_bf16, long numel) {
  if (!g.has_value() || !g->defined()) return nullptr;
  TORCH_CHECK(g->is_cuda() && g->is_contiguous(),
              "grad table: grad must be a contiguous GPU tensor");
  TORCH_CHECK(g->scalar_type() == (is_bf16 ? at::kBFloat16 : at::kFloat),
              "grad table: grad dtype differs from its parameter's");
  TORCH_CHECK(g->numel() == numel,
              "grad table: grad size differs from its parameter's");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(g->data_ptr()) % 16 == 0,
              "grad table: grad address is not 16-byte aligned");
  return g->data_ptr();
}

// Capture-safe AdamW whose grads arrive as kernel arguments. blob comes
// from adamw_build_meta over the same params (its grad field is unused).
// grads[i] is None where params[i] got no gradient; coef (optional
// 1-element fp32 device tensor) is the clip factor applied on load.
void multi_tensor_adamw_tab_run(
    const at::Tensor& blob, long total, long n, bool is_bf16,
    std::vector<at::Tensor> params,
    std::vector<c10::optional<at::Tensor>> grads, double b1, double b2,
    double eps, c10::optional<at::Tensor> lr_mul,
    c10::optional<at::Tensor> coef) {
  TORCH_CHECK(n > 0 && n <= MAX_TENSORS && (long)params.size() == n &&
                  (long)grads.size() == n,
              "multi_tensor_adamw_tab_run: bad tensor count");
  TORCH_CHECK(blob.numel() == n * (long)sizeof(ChunkMeta),
              "multi_tensor_adamw_tab_run: blob does not match n");
  const float* mul = nullptr;
  const float* cf = nullptr;
  if (lr_mul.has_value()) {
    TORCH_CHECK(lr_mul->scalar_type() == at::kFloat && lr_mul->numel() == 1,
                "lr_mul must be a 1-element fp32 device tensor");
    mul = lr_mul->data_ptr<float>();
  }
  if (coef.has_value()) {
    TORCH_CHECK(coef->is_cuda() && coef->scalar_type() == at::kFloat &&
                    coef->numel() == 1,
                "coef must be a 1-element fp32 device tensor");
    cf = coef->data_ptr<float>();
  }
  const int n_launch = (n + GRAD_SLOTS - 1) / GRAD_SLOTS;
  std::vector<GradTable> tabs(n_launch);  // zero-initialised: null slots
  for (long i = 0; i < n; ++i) {
    TORCH_CHECK(params[i].scalar_type() ==
                    (is_bf16 ? at::kBFloat16 : at::kFloat),
                "adamw: mixed param dtypes in one call");
    tabs[i / GRAD_SLOTS].g[i % GRAD_SLOTS] =
        tab_grad_ptr(grads[i], is_bf16, params[i].numel());
  }
  const int block = 256;
  const int gx = std::min<long>((total / n + block - 1) / block, 512);
  auto stream = cur_stream(blob);
  const ChunkMeta* metas = (const ChunkMeta*)blob.data_ptr();
  for (int l = 0; l < n_launch; ++l) {
    const int cnt = std::min<long>(GRAD_SLOTS, n - (long)l * GRAD_SLOTS);
    dim3 grid(std::max(gx, 1), std::min(cnt, 64));
    if (is_bf16) {
      hipLaunchKernelGGL(multi_tensor_adamw_tab_kernel<bf16>, grid,
                         dim3(block), 0, stream, metas + l * GRAD_SLOTS, cnt,
                         tabs[l], (float)b1, (float)b2, (float)eps, mul, cf);
    } else {
      hipLaunchKernelGGL(multi_tensor_adamw_tab_kernel<float>, grid,
                         dim3(block), 0, stream, metas + l * GRAD_SLOTS, cnt,
                         tabs[l], (float)b1, (float)b2, (float)eps, mul, cf);
    }
    HIP_CHECK_LAST();
  }
}

// fp32 path (masters empty) or bf16 path (masters[i] fp32, same numel).
void multi_tensor_adamw(std::vector<at::Tensor> params,
                        std::vector<at::Tensor> grads,
                        std::vector<at::Tensor> masters,
                        std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
                        std::vector<double> lrs, std::vector<double> wds,
                        double b1, double b2, double eps,
                        c10::optional<at::Tensor> lr_mul) {
  const int n = params.size();
  TORCH_CHECK(n > 0 && n <= MAX_TENSORS, "multi_tensor_adamw: bad tensor count");
  const bool has_master = !masters.empty();
  const bool is_bf16 = params[0].scalar_type() == at::kBFloat16;
  TORCH_CHECK(!is_bf16 || has_master,
              "adamw: bf16 params need fp32 master weights");
  std::vector<ChunkMeta> metas(n);
  long total = 0;
  for (int i = 0; i < n; ++i) {
    TORCH_CHECK(params[i].scalar_type() ==
                    (is_bf16 ? at::kBFloat16 : at::kFloat),
                "adamw: mixed param dtypes in one call");
    TORCH_CHECK(grads[i].is_contiguous() &&
                    grads[i].scalar_type() == params[i].scalar_type(),
                "adamw: grad must be contiguous, same dtype as param");
    metas[i] = {params[i].data_ptr(), grads[i].data_ptr(),
                has_master ? masters[i].data_ptr<float>() : nullptr,
                ms[i].data_ptr<float>(), vs[i].data_ptr<float>(),
                params[i].numel(), (float)lrs[i], (float)wds[i]};
    total += metas[i].n;
  }
  const float* mul = nullptr;
  if (lr_mul.has_value()) {
    TORCH_CHECK(lr_mul->scalar_type() == at::kFloat && lr_mul->numel() == 1,
                "lr_mul must be a 1-element fp32 device tensor");
    mul = lr_mul->data_ptr<float>();
  }
  launch_adamw(metas, total, is_bf16, params[0], b1, b2, eps, mul);
}

// ------------------------------------------------------- global L2 norm
struct NormMeta {
  const void* g;
  long n;
  int is_bf16;
};

__global__ void multi_tensor_l2_kernel(NormMeta* metas, int n_tensors,
                                       float* out) {
  // every block walks every tensor (grid-stride over elements, 4-wide
  // vector loads); block-level LDS reduce -> ONE atomic per block
  __shared__ float warp_acc[16];
  float acc = 0.f;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (int ti = 0; ti < n_tensors; ++ti) {
    const NormMeta mt = metas[ti];
    const long base = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (mt.is_bf16) {
      const bf16* g = reinterpret_cast<const bf16*>(mt.g);
      long i = base;
      for (; i + 3 < mt.n; i += stride) {
        const s16x4 v4 = *reinterpret_cast<const s16x4*>(g + i);
        const bf16* vb = reinterpret_cast<const bf16*>(&v4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = to_f32(vb[e]);
          acc += v * v;
        }
      }
      for (; i < mt.n; ++i) {  // ragged tail (rare: params are 4-aligned)
        const float v = to_f32(g[i]);
        acc += v * v;
      }
    } else {
      const float* g = reinterpret_cast<const float*>(mt.g);
      long i = base;
      for (; i + 3 < mt.n; i += stride) {
        const f32x4 v4 = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += v4[e] * v4[e];
      }
      for (; i < mt.n; ++i) acc += g[i] * g[i];
    }
  }
  for (int off = WAVE / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, WAVE);
  const int wid = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) warp_acc[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < (int)(blockDim.x / WAVE); ++w) s += warp_acc[w];
    atomicAdd(out, s);
  }
}

std::vector<at::Tensor> norm_build_meta(std::vector<at::Tensor> grads) {
  const int n = grads.size();
  TORCH_CHECK(n > 0 && n <= MAX_TENSORS, "norm_build_meta: bad count");
  std::vector<NormMeta> metas(n);
  for (int i = 0; i < n; ++i)
    metas[i] = {grads[i].data_ptr(), grads[i].numel(),
                grads[i].scalar_type() == at::kBFloat16 ? 1 : 0};
  auto blob = at::from_blob(metas.data(), {(long)(n * sizeof(NormMeta))},
                            at::TensorOptions().dtype(at::kByte))
                  .to(grads[0].device(), false);
  auto info = at::tensor({(long)n}, at::TensorOptions().dtype(at::kLong));
  return {blob, info};
}

at::Tensor multi_tensor_sumsq_run(const at::Tensor& blob, long n,
                                  const at::Tensor& out) {
  hipLaunchKernelGGL(multi_tensor_l2_kernel, dim3(512, 1), dim3(256), 0,
                     cur_stream(blob), (NormMeta*)blob.data_ptr(), (int)n,
                     out.data_ptr<float>());
  HIP_CHECK_LAST();
  return out;
}


// Returns a 1-element fp32 tensor holding sum of squares (caller sqrts).
at::Tensor multi_tensor_sumsq(std::vector<at::Tensor> grads) {
  const int n = grads.size();
  TORCH_CHECK(n > 0 && n <= MAX_TENSORS, "multi_tensor_sumsq: bad count");
  std::vector<NormMeta> metas(n);
  long total = 0;
  for (int i = 0; i < n; ++i) {
    TORCH_CHECK(grads[i].is_contiguous(), "sumsq: non-contiguous grad");
    metas[i] = {grads[i].data_ptr(), grads[i].numel(),
                grads[i].scalar_type() == at::kBFloat16 ? 1 : 0};
    total += metas[i].n;
  }
  auto out = at::zeros({1}, grads[0].options().dtype(at::kFloat));
  auto meta_blob = at::from_blob(metas.data(), {(long)(n * sizeof(NormMeta))},
                                 at::TensorOptions().dtype(at::kByte))
                       .to(grads[0].device(), false);
  const int block = 256;
  // ~2048 waves total saturate HBM for a read-only reduction
  dim3 grid(512, 1);
  hipLaunchKernelGGL(multi_tensor_l2_kernel, grid, dim3(block), 0,
                     cur_stream(grads[0]), (NormMeta*)meta_blob.data_ptr(), n,
                     out.data_ptr<float>());
  HIP_CHECK_LAST();
  return out;
}

// Scale every grad in-place by *scale (1-element fp32 tensor, device side —
// no host sync in the clip path).
struct ScaleMeta {
  void* g;
  long n;
  int is_bf16;
};

__global__ void multi_tensor_scale_kernel(ScaleMeta* metas, int n_tensors,
                                          const float* scale) {
  const float s = *scale;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (int ti = blockIdx.y; ti < n_tensors; ti += gridDim.y) {
    const ScaleMeta mt = metas[ti];
    const long base = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (mt.is_bf16) {
      bf16* g = reinterpret_cast<bf16*>(mt.g);
      long i = base;
      for (; i + 3 < mt.n; i += stride) {
        s16x4 v4 = *reinterpret_cast<const s16x4*>(g + i);
        bf16* vb = reinterpret_cast<bf16*>(&v4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          vb[e] = __float2bfloat16(to_f32(vb[e]) * s);
        *reinterpret_cast<s16x4*>(g + i) = v4;
      }
      for (; i < mt.n; ++i) g[i] = __float2bfloat16(to_f32(g[i]) * s);
    } else {
      float* g = reinterpret_cast<float*>(mt.g);
      long i = base;
      for (; i + 3 < mt.n; i += stride) {
        f32x4 v4 = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v4[e] *= s;
        *reinterpret_cast<f32x4*>(g + i) = v4;
      }
      for (; i < mt.n; ++i) g[i] *= s;
    }
  }
}

void multi_tensor_scale(std::vector<at::Tensor> grads,
                        const at::Tensor& scale) {
  const int n = grads.size();
  TORCH_CHECK(n > 0 && n <= MAX_TENSORS, "multi_tensor_scale: bad count");
  std::vector<ScaleMeta> metas(n);
  long total = 0;
  for (int i = 0; i < n; ++i) {
    metas[i] = {grads[i].data_ptr(), grads[i].numel(),
                grads[i].scalar_type() == at::kBFloat16 ? 1 : 0};
    total += metas[i].n;
  }
  auto meta_blob = at::from_blob(metas.data(), {(long)(n * sizeof(ScaleMeta))},
                                 at::TensorOptions().dtype(at::kByte))
                       .to(grads[0].device(), false);
  const int block = 256;
  const int gx = std::min<long>((total / n + block - 1) / block, 256);
  dim3 grid(std::max(gx, 1), std::min(n, 64));
  hipLaunchKernelGGL(multi_tensor_scale_kernel, grid, dim3(block), 0,
                     cur_stream(grads[0]), (ScaleMeta*)meta_blob.data_ptr(), n,
                     scale.data_ptr<float>());
  HIP_CHECK_LAST();
}

void multi_tensor_scale_run(const at::Tensor& blob, long n,
                            const at::Tensor& scale) {
  // NormMeta and ScaleMeta share layout {ptr, n, is_bf16}
  hipLaunchKernelGGL(multi_tensor_scale_kernel, dim3(256, 64), dim3(256), 0,
                     cur_stream(blob), (ScaleMeta*)blob.data_ptr(), (int)n,
                     scale.data_ptr<float>());
  HIP_CHECK_LAST();
}

// ------------------------------- balanced sum of squares + clip finisher
// The tensors are cut into chunks of SUMSQ_CHUNK elements and block b
// takes chunks b, b + grid, ...: every block streams about the same
// number of bytes however the sizes are spread (multi_tensor_l2_kernel
// walks every tensor in every block, so the many 768-element tensors
// occupy a few threads of block 0 and idle the rest). The chunk list
// depends on sizes and dtypes only and is cached; the grad addresses come
// by value. Each block stores one fp32 partial in a slab and
// sumsq_finish_kernel sums the slab in fixed order: no atomics, no
// zero-fill, bitwise reproducible.
#define SUMSQ_CHUNK 8192
#define SUMSQ_GRID 1024
#define SUMSQ_BLOCK 256

struct SumsqChunk {
  long off;  // first element within the tensor (a multiple of SUMSQ_CHUNK)
  int n;     // elements in this chunk, 1..SUMSQ_CHUNK
  short slot;  // index into the launch's GradTable
  short is_bf16;
};

__global__ __launch_bounds__(SUMSQ_BLOCK) void grad_sumsq_kernel(
    const SumsqChunk* __restrict__ chunks, int c0, int c1, GradTable tab,
    float* __restrict__ slab) {
  __shared__ float red[SUMSQ_BLOCK / WAVE];
  float acc = 0.f;
  for (int c = c0 + blockIdx.x; c < c1; c += gridDim.x) {
    const SumsqChunk ck = chunks[c];
    const void* g = tab.g[ck.slot];
    if (!g) continue;  // no gradient: adds 0
    if (ck.is_bf16) {
      const bf16* p = reinterpret_cast<const bf16*>(g) + ck.off;
      const int nv = ck.n >> 3;
#pragma unroll 4
      for (int i = threadIdx.x; i < nv; i += SUMSQ_BLOCK) {
        const s16x8 v8 = *reinterpret_cast<const s16x8*>(p + 8 * i);
        const bf16* vb = reinterpret_cast<const bf16*>(&v8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = to_f32(vb[e]);
          acc += v * v;
        }
      }
      const int t = (nv << 3) + threadIdx.x;  // scalar tail, < 8 elements
      if (t < ck.n) {
        const float v = to_f32(p[t]);
        acc += v * v;
      }
    } else {
      const float* p = reinterpret_cast<const float*>(g) + ck.off;
      const int nv = ck.n >> 2;
#pragma unroll 4
      for (int i = threadIdx.x; i < nv; i += SUMSQ_BLOCK) {
        const f32x4 v4 = *reinterpret_cast<const f32x4*>(p + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += v4[e] * v4[e];
      }
      const int t = (nv << 2) + threadIdx.x;  // scalar tail, < 4 elements
      if (t < ck.n) acc += p[t] * p[t];
    }
  }
  const float s = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) slab[blockIdx.x] = s;
}

// out[0] = sum of the slab, out[1] = min(max_norm / (sqrt(out[0]) + 1e-6),
// 1) in fp32 — clip_gradients' formula. A NaN norm gives a NaN coef, as
// torch's clamp does.
__global__ __launch_bounds__(SUMSQ_BLOCK) void sumsq_finish_kernel(
    const float* __restrict__ slab, int n, float max_norm,
    float* __restrict__ out) {
  __shared__ float red[SUMSQ_BLOCK / WAVE];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += SUMSQ_BLOCK) acc += slab[i];
  const float s = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) {
    out[0] = s;
    const float c = max_norm / (sqrtf(s) + 1e-6f);
    out[1] = c > 1.f ? 1.f : c;
  }
}

// the two sizes tests and callers need to pick shapes at the edges
long grad_table_slots() { return GRAD_SLOTS; }
long sumsq_chunk_elems() { return SUMSQ_CHUNK; }

static long sumsq_chunks_of(long numel) {
  return (numel + SUMSQ_CHUNK - 1) / SUMSQ_CHUNK;
}

// Device chunk list for tensors of the given sizes (is_bf16[i] != 0:
// bf16, else fp32). Tensor i uses slot i % GRAD_SLOTS of launch
// i / GRAD_SLOTS.
at::Tensor sumsq_build_chunks(std::vector<long> numels,
                              std::vector<long> is_bf16,
                              const at::Tensor& ref) {
  const long n = numels.size();
  TORCH_CHECK(n > 0 && n <= MAX_TENSORS && (long)is_bf16.size() == n,
              "sumsq_build_chunks: bad count");
  std::vector<SumsqChunk> chunks;
  for (long i = 0; i < n; ++i) {
    TORCH_CHECK(numels[i] >= 0, "sumsq_build_chunks: negative size");
    for (long off = 0; off < numels[i]; off += SUMSQ_CHUNK)
      chunks.push_back({off, (int)std::min<long>(SUMSQ_CHUNK, numels[i] - off),
                        (short)(i % GRAD_SLOTS), (short)(is_bf16[i] ? 1 : 0)});
  }
  if (chunks.empty())
    return at::empty({0}, ref.options().dtype(at::kByte));
  return at::from_blob(chunks.data(),
                       {(long)(chunks.size() * sizeof(SumsqChunk))},
                       at::TensorOptions().dtype(at::kByte))
      .to(ref.device(), false);
}

// Capture-safe. chunks comes from sumsq_build_chunks over the same numels
// and is_bf16; grads[i] is None where there is no gradient. Returns a
// 2-element fp32 tensor {sumsq, coef}.
at::Tensor multi_tensor_sumsq_coef_run(
    const at::Tensor& chunks, std::vector<long> numels,
    std::vector<long> is_bf16, std::vector<c10::optional<at::Tensor>> grads,
    double max_norm) {
  const long n = numels.size();
  TORCH_CHECK(n > 0 && n <= MAX_TENSORS && (long)is_bf16.size() == n &&
                  (long)grads.size() == n,
              "multi_tensor_sumsq_coef_run: bad count");
  TORCH_CHECK(chunks.is_cuda(), "sumsq: chunk list must be on the GPU");
  const int n_launch = (n + GRAD_SLOTS - 1) / GRAD_SLOTS;
  std::vector<GradTable> tabs(n_launch);  // zero-initialised: null slots
  std::vector<long> c_end(n_launch, 0);
  long total_chunks = 0;
  for (long i = 0; i < n; ++i) {
    tabs[i / GRAD_SLOTS].g[i % GRAD_SLOTS] =
        tab_grad_ptr(grads[i], is_bf16[i] != 0, numels[i]);
    total_chunks += sumsq_chunks_of(numels[i]);
    c_end[i / GRAD_SLOTS] = total_chunks;
  }
  TORCH_CHECK(chunks.numel() == total_chunks * (long)sizeof(SumsqChunk),
              "sumsq: chunk list does not match the sizes");
  long n_part = 0;
  for (int l = 0; l < n_launch; ++l) {
    const long c0 = l ? c_end[l - 1] : 0;
    n_part += std::min<long>(SUMSQ_GRID, c_end[l] - c0);
  }
  auto opts = chunks.options().dtype(at::kFloat);
  auto slab = at::empty({std::max<long>(n_part, 1)}, opts);
  auto out = at::empty({2}, opts);
  auto stream = cur_stream(chunks);
  long s0 = 0;
  for (int l = 0; l < n_launch; ++l) {
    const long c0 = l ? c_end[l - 1] : 0;
    const int grid = std::min<long>(SUMSQ_GRID, c_end[l] - c0);
    if (grid == 0) continue;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(SUMSQ_BLOCK), 0,
                       stream, (const SumsqChunk*)chunks.data_ptr(), (int)c0,
                       (int)c_end[l], tabs[l], slab.data_ptr<float>() + s0);
    HIP_CHECK_LAST();
    s0 += grid;
  }
  hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(SUMSQ_BLOCK), 0,
                     stream, slab.data_ptr<float>(), (int)n_part,
                     (float)max_norm, out.data_ptr<float>());
  HIP_CHECK_LAST();
  return out;
}
