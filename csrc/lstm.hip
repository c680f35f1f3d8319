// Persistent BiLSTM recurrence (the "BiLSTM tagger" kernel
// named in BASELINE.json). The x-projection (x @ [W_ih_f|W_ih_b] + b) is a
// single library GEMM done by the Python wrapper; these kernels own the
// sequential part: per step  gates = gates_x[t] + h_{t-1} @ W_hh,
// LSTM cell update, variable-length masking.
//
// Design:
//  * BOTH directions run in ONE launch (blockIdx.y = direction) so their
//    sequence loops overlap on different CUs.
//  * Strided I/O: python layout is [B,L,8h] gates (fw|bw halves) and
//    [B,L,2h] hidden — the BiLSTM concat is free.
//  * The hidden size H is a template parameter (32, 64, ..., 256; the
//    wrapper zero-pads to a multiple of 32, exact: padded units stay 0
//    through time). Fragment counts, loop trips and LDS strides are
//    constants, so every per-lane array lives in registers and no slot
//    exists that the size does not use.
//  * Recurrent weights come through one `const bf16* __restrict__`
//    global pointer. For H <= 128 each wave loads its MFMA B operands
//    once and keeps them in registers for the whole sequence (measured
//    faster than re-reading an LDS image every step at every such H);
//    for H in (128, 256] they stream from global memory every step
//    (L2-resident: W_hh is <= 512 KiB). Chosen at compile time.
//  * One workgroup (NW = 4 or 8 waves, see LstmTile) owns a 16-row batch
//    tile and loops time in-kernel; MFMA 16x16x32 bf16 computes the
//    [16,4H] gate panel; column frag f (16 cols) is owned by wave f%NW,
//    so each lane locally combines its i/f/g/o gates and carries cell
//    state in registers. A timestep is mostly the cell arithmetic (IEEE
//    divides, exp), so more waves per tile shorten it.
//  * No lane is idle and no store is guarded: rows past B recompute row
//    B-1 and, where H/16 is no multiple of NW (H = 32, 96, 160, 224),
//    the waves without a last frag recompute frag H/16-1. They read the
//    same inputs and run the same instructions as the owner, so they
//    store the same bits to the same addresses. Guards would put the
//    stores under branches, and the compiler then waits for them
//    whenever it waits for a prefetched load.
//  * Only the recurrence is waited for. Forward: step t+1's gates_x
//    chunks are loaded at the top of step t and reach LDS after its
//    second barrier; the hs/cs/gates stores are never waited for.
//    Backward: every per-cell operand (gates, c, dh_out) of step t-1 is
//    loaded, unconditionally and with clamped addresses, at the top of
//    step t; c_prev of a step is kept as the next step's c_t. `valid` is
//    applied with selects. The barriers order LDS only. The activation
//    is a template parameter: one path through the loop body lets the
//    compiler count the stores issued after a prefetch, so its wait for
//    the prefetch (vmcnt(N)) leaves them in flight.
//
// fwd stores activated gates interleaved ([D,B,L,h,4] — one f32x4 per
// (row, j) in bwd) + cell states; bwd replays in reverse producing
// pre-activation gate grads; dW_hh / dW_ih / db / dx are library GEMMs
// in the wrapper.
#include <type_traits>

#include "common.h"

#define H_MAX 256

using bfrag = mfma_bf16x8;
using cfrag = mfma_f32x4;

// Tiling of one hidden size over the waves of a block. 8 waves where they
// divide the column frags evenly (measured: H = 128 and 256 faster than
// with 4, H = 192 slower), 4 otherwise.
template <int H>
struct LstmTile {
  static_assert(H % 32 == 0 && H >= 32 && H <= H_MAX, "bad hidden size");
  static constexpr int N16 = H / 16;         // column frags per gate
  static constexpr int NW = H % 128 == 0 ? 8 : 4;  // waves per block
  static constexpr int NT = NW * WAVE;             // threads per block
  static constexpr int NQ = (N16 + NW - 1) / NW;   // frags per wave
  // each wave keeps its MFMA B operands (its slice of W_hh) in registers
  // for the whole sequence: at most 96 VGPRs per lane (H = 96)
  static constexpr bool W_REG = H <= 128;
  // padded strides (odd 16B groups) keep operand reads conflict free
  static constexpr int HS_LD = H + 8;
  static constexpr int G_LD = 4 * H + 8;
};

// One MFMA 16x16x32 A/B operand: 8 consecutive bf16 of this lane's row.
__device__ __forceinline__ bfrag frag_at(const bf16* p) {
  return *reinterpret_cast<const bfrag*>(p);
}

// Workgroup barrier that orders LDS traffic only: outstanding global loads
// and stores stay in flight across it. The kernels below exchange data
// between waves through LDS alone.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Waits for every outstanding global load and store (s_waitcnt vmcnt(0),
// gfx9 encoding, the other counters left at their maximum). Placed in
// front of a time loop it makes the loop's own counted waits exact: the
// compiler otherwise merges the loop-entry state, where the prologue's
// loads are the youngest operations, into every wait inside the loop.
__device__ __forceinline__ void wait_global_all() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
}
// Consumes a loaded value in place, so the compiler cannot sink its load
// past this point (into the time loop's preheader, behind the wait above).
template <typename V>
__device__ __forceinline__ void pin_loaded(V& v) {
  asm volatile("" : "+v"(v));
}

__device__ __forceinline__ float act_f(float x, bool relu) {
  return relu ? fmaxf(x, 0.f) : tanhf(x);
}
__device__ __forceinline__ float dact_from_out(float y, bool relu) {
  // derivative expressed from the activated value y = act(x)
  return relu ? (y > 0.f ? 1.f : 0.f) : (1.f - y * y);
}

// dir = blockIdx.y. gates_x rows: stride gxs, this direction's slice at
// column offset dir*4H; hs rows: stride hss, offset dir*H. cs/gates_out
// per-direction contiguous ([D,B,L,H] / [D,B,L,H,4] interleaved).
// Direction 1 (when gridDim.y == 2) scans the sequence reversed.
template <typename T, int H, bool RELU>
__global__ __launch_bounds__(LstmTile<H>::NT) void lstm_fwd_kernel(
    const T* __restrict__ gates_x,    // [B,L,gxs]
    const bf16* __restrict__ w_hh_t,  // [D,4H,H] (transposed by wrapper)
    const int* __restrict__ lens, T* __restrict__ hs,  // [B,L,hss]
    float* __restrict__ cs,                            // [D,B,L,H]
    float* __restrict__ gates_out,                     // [D,B,L,H,4]
    int B, int L, int gxs, int hss, bool rev0, float cell_clip) {
  using TL = LstmTile<H>;
  constexpr int NQ = TL::NQ, NKK = H / 32, HS_LD = TL::HS_LD;
  constexpr int NC = 8 * H / TL::NT;  // 16-byte gates_x chunks per thread
  constexpr int K_UNROLL = TL::W_REG ? NKK : 1;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  bf16* hb = reinterpret_cast<bf16*>(smem_raw);  // [16][HS_LD] current h
  bf16* gx_s = hb + 16 * HS_LD;                  // [16][4H] staged gates_x
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int lane = threadIdx.x & (WAVE - 1);
  const int b0 = blockIdx.x * 16;
  const int dir = blockIdx.y;
  const bool reverse = dir ? true : rev0;
  const int hs_off = dir * H;
  const long dbase = (long)dir * B * L;  // row offset into cs/gates_out
  const bf16* __restrict__ wg = w_hh_t + (long)dir * 4 * H * H;

  for (int i = threadIdx.x; i < 16 * HS_LD / 8; i += TL::NT)
    reinterpret_cast<s16x8*>(hb)[i] = s16x8{};

  // column frag of slot q; waves without a last frag redo frag N16-1
  int fq[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) fq[q] = min(wid + TL::NW * q, TL::N16 - 1);
  // lane-owned cells: rows lrow + r (r = 0..3), column j = fq*16 + lcol
  const int lrow = (lane >> 4) << 2;
  const int lcol = lane & 15;
  const int frag_off = lcol * HS_LD + ((lane >> 4) << 3);  // operand row/k
  float c_reg[4][NQ] = {};
  float h_reg[4][NQ] = {};  // bf16-rounded h carried through invalid steps
  int mylen[4];
  long row_bl[4];  // batch row * L; tile rows past B redo row B-1
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = min(b0 + lrow + r, B - 1);
    mylen[r] = lens[b];
    row_bl[r] = (long)b * L;
    pin_loaded(mylen[r]);
  }

  // gates_x staging: chunk c of this thread is 8 values of tile row
  // (i*8)/(4H)
  const T* gx_p[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int i = threadIdx.x + c * TL::NT;
    const int row = (i * 8) / (4 * H);
    const int col = (i * 8) % (4 * H);
    gx_p[c] = gates_x + (long)min(b0 + row, B - 1) * L * gxs + dir * 4 * H +
              col;
  }
  s16x8 pre[NC];
  auto load_chunks = [&](int t) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const T* g = gx_p[c] + (long)t * gxs;
      if constexpr (sizeof(T) == 2) {
        pre[c] = *reinterpret_cast<const s16x8*>(g);
      } else {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(g);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(g + 4);
        bf16 packed[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          packed[e] = __float2bfloat16(lo[e]);
          packed[e + 4] = __float2bfloat16(hi[e]);
        }
        pre[c] = *reinterpret_cast<const s16x8*>(packed);
      }
    }
  };
  auto store_chunks = [&]() {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      reinterpret_cast<s16x8*>(gx_s)[threadIdx.x + c * TL::NT] = pre[c];
  };
  // B operand of gate g, slot q, k-chunk kk: row = gate column, k along H
  auto w_frag = [&](int kk, int g, int q) {
    return frag_at(wg + (g * H + fq[q] * 16 + lcol) * H + ((lane >> 4) << 3) +
                   kk * 32);
  };
  bfrag wreg[TL::W_REG ? NKK : 1][4][NQ];
  if constexpr (TL::W_REG) {
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int q = 0; q < NQ; ++q) wreg[kk][g][q] = w_frag(kk, g, q);
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int q = 0; q < NQ; ++q) pin_loaded(wreg[kk][g][q]);
  }

  const int tinc = reverse ? -1 : 1;
  int t = reverse ? L - 1 : 0;
  load_chunks(t);
  store_chunks();
  wait_global_all();
  __syncthreads();
  // cell update of one step
  auto cells = [&](const cfrag (&acc)[4][NQ], int t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool valid = t < mylen[r];
      const long row = row_bl[r] + t;
      const int lr4h = (lrow + r) * 4 * H;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = fq[q] * 16 + lcol;
        float gi = acc[0][q][r] + to_f32(gx_s[lr4h + 0 * H + j]);
        float gf = acc[1][q][r] + to_f32(gx_s[lr4h + 1 * H + j]);
        float gg = acc[2][q][r] + to_f32(gx_s[lr4h + 2 * H + j]);
        float go = acc[3][q][r] + to_f32(gx_s[lr4h + 3 * H + j]);
        gi = 1.f / (1.f + __expf(-gi));
        gf = 1.f / (1.f + __expf(-gf));
        go = 1.f / (1.f + __expf(-go));
        gg = act_f(gg, RELU);
        float c_new = gf * c_reg[r][q] + gi * gg;
        // TF LSTMCell cell_clip: bounds the (relu) recurrence
        if (cell_clip > 0.f)
          c_new = fminf(fmaxf(c_new, -cell_clip), cell_clip);
        const float h_new = go * act_f(c_new, RELU);
        c_reg[r][q] = valid ? c_new : c_reg[r][q];
        const bf16 hb_new =
            __float2bfloat16(valid ? h_new : h_reg[r][q]);
        h_reg[r][q] = to_f32(hb_new);
        hb[(lrow + r) * HS_LD + j] = hb_new;
        from_f32(valid ? h_new : 0.f, &hs[row * hss + hs_off + j]);
        cs[(dbase + row) * H + j] = c_reg[r][q];
        const f32x4 g4 = {gi, gf, gg, go};
        *reinterpret_cast<f32x4*>(gates_out + (dbase + row) * 4 * H + j * 4) =
            g4;
      }
    }
  };

  for (int step = 0; step < L; ++step, t += tinc) {
    // next step's gates_x (the last step reloads its own): in flight
    // until after the second barrier
    load_chunks(min(max(t + tinc, 0), L - 1));
    // gates = h_prev @ W_hh  (+ gates_x added in the cell update)
    cfrag acc[4][NQ];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[g][q] = cfrag{0.f, 0.f, 0.f, 0.f};
#pragma unroll K_UNROLL
    for (int kk = 0; kk < NKK; ++kk) {
      // all operand reads of the k-chunk first, then its MFMAs
      const bfrag ah = frag_at(hb + frag_off + kk * 32);
      bfrag bw[4][NQ];
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          if constexpr (TL::W_REG)
            bw[g][q] = wreg[kk][g][q];
          else
            bw[g][q] = w_frag(kk, g, q);
        }
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          acc[g][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              ah, bw[g][q], acc[g][q], 0, 0, 0);
    }
    lds_barrier();  // every wave's hb reads of this step are done
    cells(acc, t);
    lds_barrier();  // hb updated; gx_s safe to overwrite for next step
    store_chunks();
  }
}

template <typename T, int H, bool RELU>
__global__ __launch_bounds__(LstmTile<H>::NT) void lstm_bwd_kernel(
    const T* __restrict__ dhs,        // [B,L,hss] upstream grad (strided)
    const float* __restrict__ cs,     // [D,B,L,H] carried cell states
    const float* __restrict__ gates,  // [D,B,L,H,4] activated, interleaved
    const bf16* __restrict__ w_hh,    // [D,H,4H] (original layout)
    const int* __restrict__ lens, T* __restrict__ dgates_x,  // [B,L,gxs]
    int B, int L, int gxs, int hss, bool rev0, float cell_clip) {
  using TL = LstmTile<H>;
  constexpr int NQ = TL::NQ, NKK = 4 * H / 32, G_LD = TL::G_LD;
  constexpr int K_UNROLL = TL::W_REG ? NKK : 4;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  bf16* dg_s = reinterpret_cast<bf16*>(smem_raw);  // [16][G_LD]
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int lane = threadIdx.x & (WAVE - 1);
  const int b0 = blockIdx.x * 16;
  const int dir = blockIdx.y;
  const bool reverse = dir ? true : rev0;
  const int gx_off = dir * 4 * H;
  const int hs_off = dir * H;
  const long dbase = (long)dir * B * L;
  const bf16* __restrict__ wg = w_hh + (long)dir * 4 * H * H;
  int fq[NQ];  // waves without a last frag redo frag N16-1
#pragma unroll
  for (int q = 0; q < NQ; ++q) fq[q] = min(wid + TL::NW * q, TL::N16 - 1);
  const int lrow = (lane >> 4) << 2;
  const int lcol = lane & 15;
  const int frag_off = lcol * G_LD + ((lane >> 4) << 3);
  float dc_reg[4][NQ] = {};
  float dh_reg[4][NQ] = {};
  int mylen[4];
  long row_bl[4];  // batch row * L; tile rows past B redo row B-1
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = min(b0 + lrow + r, B - 1);
    mylen[r] = lens[b];
    row_bl[r] = (long)b * L;
    pin_loaded(mylen[r]);
  }

  // Per-cell operands of one step. None depends on the recurrence, so they
  // are loaded one step ahead, for every cell and from a clamped (always
  // readable) address; `valid` is applied where they are used.
  struct CellIn {
    f32x4 g[4][NQ];   // activated gates i, f, g, o
    T dh[4][NQ];      // upstream grad
    float cp[4][NQ];  // cell state of the forward predecessor step
  };
  // time runs against the forward order: t + tdec is the forward
  // predecessor of t, i.e. the step this loop handles next
  const int tdec = reverse ? 1 : -1;
  auto cs_at = [&](int r, int q, int t) {
    const int tc = min(max(t, 0), L - 1);
    return cs[(dbase + row_bl[r] + tc) * H + fq[q] * 16 + lcol];
  };
  auto load_cells = [&](int t, CellIn& in) {
    const int tc = min(max(t, 0), L - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = row_bl[r] + tc;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = fq[q] * 16 + lcol;
        in.g[r][q] = *reinterpret_cast<const f32x4*>(
            gates + (dbase + row) * 4 * H + j * 4);
        in.dh[r][q] = dhs[row * hss + hs_off + j];
        in.cp[r][q] = cs_at(r, q, t + tdec);
      }
    }
  };

  // c_t of the current step: loaded once, afterwards the previous step's
  // c_prev (same value, one load fewer per cell and step)
  float c_t[4][NQ];

  // gate grads of step t from `in`
  auto cells = [&](int t, const CellIn& in) {
    const int t_prev = t + tdec;
    const bool prev_in = t_prev >= 0 && t_prev < L;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool valid = t < mylen[r];
      const bool prev_valid = prev_in && t_prev < mylen[r];
      const long xbase = (row_bl[r] + t) * gxs + gx_off;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = fq[q] * 16 + lcol;
        const f32x4 g4 = in.g[r][q];
        const float gi = g4[0], gf = g4[1], gg = g4[2], go = g4[3];
        const float ct = c_t[r][q];
        const float cp = prev_valid ? in.cp[r][q] : 0.f;
        const float ac = act_f(ct, RELU);
        const float dh = dh_reg[r][q] + to_f32(in.dh[r][q]);
        float dc = dc_reg[r][q] + dh * go * dact_from_out(ac, RELU);
        float dgo = dh * ac * go * (1.f - go);
        // clamp boundary: no grad through a clipped cell state
        if (cell_clip > 0.f && fabsf(ct) >= cell_clip) dc = 0.f;
        float dgi = dc * gg * gi * (1.f - gi);
        float dgf = dc * cp * gf * (1.f - gf);
        float dgg = dc * gi * dact_from_out(gg, RELU);
        dc_reg[r][q] = valid ? dc * gf : dc_reg[r][q];  // carry to prev step
        dgi = valid ? dgi : 0.f;
        dgf = valid ? dgf : 0.f;
        dgg = valid ? dgg : 0.f;
        dgo = valid ? dgo : 0.f;
        // pre-activation gate grads (global + LDS for the MFMA)
        from_f32(dgi, &dgates_x[xbase + 0 * H + j]);
        from_f32(dgf, &dgates_x[xbase + 1 * H + j]);
        from_f32(dgg, &dgates_x[xbase + 2 * H + j]);
        from_f32(dgo, &dgates_x[xbase + 3 * H + j]);
        const int lr = lrow + r;
        dg_s[lr * G_LD + 0 * H + j] = __float2bfloat16(dgi);
        dg_s[lr * G_LD + 1 * H + j] = __float2bfloat16(dgf);
        dg_s[lr * G_LD + 2 * H + j] = __float2bfloat16(dgg);
        dg_s[lr * G_LD + 3 * H + j] = __float2bfloat16(dgo);
        c_t[r][q] = in.cp[r][q];
      }
    }
  };

  // B operand of slot q, k-chunk kk: row = hidden unit, k along 4H
  auto w_frag = [&](int kk, int q) {
    return frag_at(wg + (fq[q] * 16 + lcol) * 4 * H + ((lane >> 4) << 3) +
                   kk * 32);
  };
  bfrag wreg[TL::W_REG ? NKK : 1][NQ];
  if constexpr (TL::W_REG) {
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
#pragma unroll
      for (int q = 0; q < NQ; ++q) wreg[kk][q] = w_frag(kk, q);
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
#pragma unroll
      for (int q = 0; q < NQ; ++q) pin_loaded(wreg[kk][q]);
  }
  // One timestep: consumes `in`, leaves the next step's operands in `nx`.
  auto one_step = [&](int t, const CellIn& in, CellIn& nx) {
    // clamped and unused after the last step; in flight over this whole step
    load_cells(t + tdec, nx);
    cells(t, in);
    lds_barrier();
    // dh_prev = dgates @ W_hh^T : [16,4H] @ [4H,H]; col frag f = wid+NW*q
    cfrag acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = cfrag{0.f, 0.f, 0.f, 0.f};
#pragma unroll K_UNROLL
    for (int kk = 0; kk < NKK; ++kk) {
      // all operand reads of the k-chunk first, then its MFMAs
      const bfrag adg = frag_at(dg_s + frag_off + kk * 32);
      bfrag bw[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if constexpr (TL::W_REG)
          bw[q] = wreg[kk][q];
        else
          bw[q] = w_frag(kk, q);
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(adg, bw[q], acc[q],
                                                         0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool valid = t < mylen[r];
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        dh_reg[r][q] = valid ? acc[q][r] : dh_reg[r][q];
      // invalid step: h passed through unchanged -> dh carries unchanged
    }
    lds_barrier();  // dg_s reads done before next step overwrites
  };

  // two steps per trip, so the operand sets swap roles without copies
  int t = reverse ? 0 : L - 1;
  CellIn in_a, in_b;
  load_cells(t, in_a);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < NQ; ++q) c_t[r][q] = cs_at(r, q, t);
  wait_global_all();
  for (int left = L; left > 0; left -= 2, t += 2 * tdec) {
    one_step(t, in_a, in_b);
    if (left == 1) break;
    one_step(t + tdec, in_b, in_a);
  }
}

// ===================================================================== host
static size_t lstm_fwd_smem(int h) {  // hb + gx_s
  return ((size_t)16 * (h + 8) + (size_t)16 * 4 * h) * sizeof(bf16);
}
static size_t lstm_bwd_smem(int h) {  // dg_s
  return (size_t)16 * (4 * h + 8) * sizeof(bf16);
}

// Calls fn(integral_constant<int, H>, bool_constant<RELU>) for the kernel
// instantiation of hidden size h and activation.
template <typename Fn>
static void dispatch_shape(int h, bool relu, Fn&& fn) {
  switch (h) {
#define LSTM_H_CASE(HH)                                            \
  case HH:                                                         \
    if (relu)                                                      \
      fn(std::integral_constant<int, HH>{}, std::true_type{});     \
    else                                                           \
      fn(std::integral_constant<int, HH>{}, std::false_type{});    \
    break;
    LSTM_H_CASE(32) LSTM_H_CASE(64) LSTM_H_CASE(96) LSTM_H_CASE(128)
    LSTM_H_CASE(160) LSTM_H_CASE(192) LSTM_H_CASE(224) LSTM_H_CASE(256)
#undef LSTM_H_CASE
    default:
      TORCH_CHECK(false,
                  "lstm kernel: hidden must be a multiple of 32 and <= 256, "
                  "got ", h);
  }
}

// D directions (grid.y) over gates_x rows of stride gxs, hs rows of stride
// hss; w_t is bf16 [D,4h,h].
template <typename T>
static void launch_fwd(const at::Tensor& gates_x, const at::Tensor& w_t,
                       const at::Tensor& lens, at::Tensor& hs, at::Tensor& cs,
                       at::Tensor& gates, int D, int h, int gxs, int hss,
                       bool rev0, bool relu, float cell_clip) {
  const int B = gates_x.size(0), L = gates_x.size(1);
  const size_t smem = lstm_fwd_smem(h);
  const dim3 grid((B + 15) / 16, D);
  auto stream = cur_stream(gates_x);
  dispatch_shape(h, relu, [&](auto hc, auto rc) {
    hipLaunchKernelGGL(
        (lstm_fwd_kernel<T, decltype(hc)::value, decltype(rc)::value>), grid,
        dim3(LstmTile<decltype(hc)::value>::NT), smem, stream,
        (const T*)gates_x.data_ptr(),
        (const bf16*)w_t.data_ptr(), lens.data_ptr<int>(), (T*)hs.data_ptr(),
        cs.data_ptr<float>(), gates.data_ptr<float>(), B, L, gxs, hss, rev0,
        cell_clip);
  });
  HIP_CHECK_LAST();
}

// w is bf16 [D,h,4h].
template <typename T>
static void launch_bwd(const at::Tensor& dhs, const at::Tensor& cs,
                       const at::Tensor& gates, const at::Tensor& w,
                       const at::Tensor& lens, at::Tensor& dgates_x, int D,
                       int h, int gxs, int hss, bool rev0, bool relu,
                       float cell_clip) {
  const int B = dhs.size(0), L = dhs.size(1);
  const size_t smem = lstm_bwd_smem(h);
  const dim3 grid((B + 15) / 16, D);
  auto stream = cur_stream(dhs);
  dispatch_shape(h, relu, [&](auto hc, auto rc) {
    hipLaunchKernelGGL(
        (lstm_bwd_kernel<T, decltype(hc)::value, decltype(rc)::value>), grid,
        dim3(LstmTile<decltype(hc)::value>::NT), smem, stream,
        (const T*)dhs.data_ptr(),
        cs.data_ptr<float>(), gates.data_ptr<float>(),
        (const bf16*)w.data_ptr(), lens.data_ptr<int>(),
        (T*)dgates_x.data_ptr(), B, L, gxs, hss, rev0, cell_clip);
  });
  HIP_CHECK_LAST();
}

// Bidirectional fused path: gates_x [B,L,8h] (fw|bw), w_hh_t2 [2,4h,h].
// Returns hs [B,L,2h] (concat free), cs [2,B,L,h], gates [2,B,L,h,4].
std::vector<at::Tensor> bilstm_fwd_l(const at::Tensor& gates_x,
                                     const at::Tensor& w_hh_t2,
                                     const at::Tensor& lens, bool relu,
                                     double cell_clip) {
  CHECK_CUDA_CONTIG(gates_x);
  const int B = gates_x.size(0), L = gates_x.size(1);
  const int h = gates_x.size(2) / 8;
  TORCH_CHECK(w_hh_t2.size(0) == 2 && w_hh_t2.scalar_type() == at::kBFloat16,
              "w_hh_t2 must be bf16 [2,4h,h]");
  auto hs = at::empty({B, L, 2 * h}, gates_x.options());
  auto cs = at::empty({2, B, L, h}, gates_x.options().dtype(at::kFloat));
  auto gates = at::empty({2, B, L, 4 * h},
                         gates_x.options().dtype(at::kFloat));
  if (gates_x.scalar_type() == at::kBFloat16)
    launch_fwd<bf16>(gates_x, w_hh_t2, lens, hs, cs, gates, 2, h, 8 * h,
                     2 * h, /*rev0=*/false, relu, (float)cell_clip);
  else
    launch_fwd<float>(gates_x, w_hh_t2, lens, hs, cs, gates, 2, h, 8 * h,
                      2 * h, /*rev0=*/false, relu, (float)cell_clip);
  return {hs, cs, gates};
}

at::Tensor bilstm_bwd_l(const at::Tensor& dhs, const at::Tensor& cs,
                        const at::Tensor& gates, const at::Tensor& w_hh2,
                        const at::Tensor& lens, bool relu, double cell_clip) {
  const int B = dhs.size(0), L = dhs.size(1);
  const int h = dhs.size(2) / 2;
  TORCH_CHECK(w_hh2.size(0) == 2 && w_hh2.scalar_type() == at::kBFloat16,
              "w_hh2 must be bf16 [2,h,4h]");
  auto dhs_c = dhs.contiguous();
  auto dgates_x = at::empty({B, L, 8 * h}, dhs.options());
  if (dhs.scalar_type() == at::kBFloat16)
    launch_bwd<bf16>(dhs_c, cs, gates, w_hh2, lens, dgates_x, 2, h, 8 * h,
                     2 * h, /*rev0=*/false, relu, (float)cell_clip);
  else
    launch_bwd<float>(dhs_c, cs, gates, w_hh2, lens, dgates_x, 2, h, 8 * h,
                      2 * h, /*rev0=*/false, relu, (float)cell_clip);
  return dgates_x;
}

// Single-direction path (kept for the kernel unit tests: one direction,
// reverse selectable, gates_x [B,L,4h] contiguous).
std::vector<at::Tensor> lstm_fwd(const at::Tensor& gates_x,
                                 const at::Tensor& w_hh,
                                 const at::Tensor& lens, bool reverse,
                                 bool relu) {
  CHECK_CUDA_CONTIG(gates_x);
  const int B = gates_x.size(0), L = gates_x.size(1);
  const int h4 = gates_x.size(2), h = h4 / 4;
  auto hs = at::empty({B, L, h}, gates_x.options());
  auto cs = at::empty({1, B, L, h}, gates_x.options().dtype(at::kFloat));
  auto gates = at::empty({1, B, L, h4}, gates_x.options().dtype(at::kFloat));
  auto w_t = w_hh.t().contiguous().to(at::kBFloat16);  // [4h,h]
  if (gates_x.scalar_type() == at::kBFloat16)
    launch_fwd<bf16>(gates_x, w_t, lens, hs, cs, gates, 1, h, h4, h, reverse,
                     relu, 0.f);
  else
    launch_fwd<float>(gates_x, w_t, lens, hs, cs, gates, 1, h, h4, h, reverse,
                      relu, 0.f);
  return {hs, cs.squeeze(0), gates.squeeze(0)};
}

std::vector<at::Tensor> lstm_bwd(const at::Tensor& dhs, const at::Tensor& hs,
                                 const at::Tensor& cs, const at::Tensor& gates,
                                 const at::Tensor& w_hh, const at::Tensor& lens,
                                 bool reverse, bool relu) {
  const int B = dhs.size(0), L = dhs.size(1), h = dhs.size(2);
  auto dgates_x = at::empty({B, L, 4 * h}, dhs.options());
  auto w_b = w_hh.contiguous().to(at::kBFloat16);  // [h,4h]
  auto dhs_c = dhs.contiguous();
  if (dhs.scalar_type() == at::kBFloat16)
    launch_bwd<bf16>(dhs_c, cs, gates, w_b, lens, dgates_x, 1, h, 4 * h, h,
                     reverse, relu, 0.f);
  else
    launch_bwd<float>(dhs_c, cs, gates, w_b, lens, dgates_x, 1, h, 4 * h, h,
                      reverse, relu, 0.f);
  return {dgates_x};
}
