// Inverted index of a row -> id map, integers only: the stable order of
// the rows by (id, row) and a start table per id, so that a scatter-add
// over ids becomes a per-id sum over a list in a fixed order (no float
// atomics, bitwise reproducible). Used by the embedding backward
// (embed.hip); kept free of it so other scatters can share it.
//
// Three launches, no atomics of any kind, nothing kept between calls:
//   sidx_count_kernel  partial ranks: for a tile of rows and a slice of
//                      the other rows, how many keys are smaller
//   sidx_place_kernel  rank = sum of the partials; order[rank] = row,
//                      skey[rank] = id
//   sidx_start_kernel  start[v] = first sorted position with id >= v,
//                      for v in [0, V]; list of v is
//                      order[start[v] .. start[v+1])
//
// The key of row r is id[r] * R + r in 32 bits, unique and ordered by
// (id, r). Limits: R <= SIDX_MAX_ROWS and V * R <= 2^32. An id outside
// [0, V) is taken as id 0.
#pragma once

#include "common.h"

#define SIDX_MAX_ROWS 32768
#define SIDX_MAX_KEYS (1l << 32)  // V * R, the range of the 32-bit key
#define SIDX_TILE 256        // rows per block of the count kernel
#define SIDX_SLICE_MAX 2048  // other rows per block (LDS: 8 KiB)

static inline bool sidx_supported(long R, long V) {
  return R >= 1 && V >= 1 && R <= SIDX_MAX_ROWS &&
         R * V <= SIDX_MAX_KEYS;
}

__device__ __forceinline__ int sidx_id(const long* __restrict__ ids, int r,
                                       int V) {
  const long id = ids[r];
  return (id < 0 || id >= V) ? 0 : (int)id;
}

__device__ __forceinline__ unsigned sidx_key(const long* __restrict__ ids,
                                             int r, int R, int V) {
  return (unsigned)sidx_id(ids, r, V) * (unsigned)R + (unsigned)r;
}

// grid (ceil(R / SIDX_TILE), NS); slice y holds rows [y*SL, (y+1)*SL),
// SL a multiple of 4 and <= SIDX_SLICE_MAX. One thread per row of the
// tile; the slice's keys are read from LDS as broadcasts.
__global__ __launch_bounds__(SIDX_TILE) void sidx_count_kernel(
    const long* __restrict__ ids, int R, int V, int SL,
    int* __restrict__ cnt) {  // [NS][R]
  __shared__ __attribute__((aligned(16))) unsigned keys[SIDX_SLICE_MAX];
  const int j0 = blockIdx.y * SL;
  for (int j = threadIdx.x; j < SL; j += SIDX_TILE) {
    const int rr = j0 + j;
    // the padding compares greater than or equal to every real key
    keys[j] = rr < R ? sidx_key(ids, rr, R, V) : 0xFFFFFFFFu;
  }
  __syncthreads();
  const int r = blockIdx.x * SIDX_TILE + threadIdx.x;
  if (r >= R) return;
  const unsigned ki = sidx_key(ids, r, R, V);
  int c = 0;
#pragma unroll 4
  for (int j = 0; j < SL; j += 4) {
    const uint4 k = *reinterpret_cast<const uint4*>(&keys[j]);
    c += (int)(k.x < ki) + (int)(k.y < ki) + (int)(k.z < ki) +
         (int)(k.w < ki);
  }
  cnt[(long)blockIdx.y * R + r] = c;
}

__global__ __launch_bounds__(256) void sidx_place_kernel(
    const long* __restrict__ ids, int R, int V, int NS,
    const int* __restrict__ cnt, int* __restrict__ order,
    int* __restrict__ skey) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  int pos = 0;
  for (int y = 0; y < NS; ++y) pos += cnt[(long)y * R + r];
  if (pos < R) {  // always: the keys are distinct
    order[pos] = r;
    skey[pos] = sidx_id(ids, r, V);
  }
}

// One thread per sorted position p in [0, R]: it owns the ids v with
// skey[p-1] < v <= skey[p] (skey[-1] = -1, skey[R] = V) and writes
// start[v] = p for them. These ranges tile [0, V], so every entry of
// start[0..V] is written exactly once. A range longer than 8 is written
// by the whole wave, so that one id far from its neighbour (or the tail
// behind the largest id) does not serialise on one lane.
__global__ __launch_bounds__(256) void sidx_start_kernel(
    const int* __restrict__ skey, int R, int V, int* __restrict__ start) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  int a = 0, b = 0;  // p > R: empty range
  if (p <= R) {
    a = p > 0 ? skey[p - 1] + 1 : 0;
    b = p < R ? skey[p] + 1 : V + 1;
  }
  // start[v] = p for v in [a, b)
  const bool wide = b - a > 8;
  if (!wide)
    for (int v = a; v < b; ++v) start[v] = p;
  unsigned long long todo = __ballot(wide);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int aa = __shfl(a, src), bb = __shfl(b, src), pp = __shfl(p, src);
    for (int v = aa + lane; v < bb; v += WAVE) start[v] = pp;
  }
}

struct SortedIndex {
  at::Tensor buf;  // owns the three arrays below and the partial ranks
  const int* order;  // [R] rows sorted by (id, row)
  const int* skey;   // [R] their ids, ascending
  const int* start;  // [V + 1]
};

// ids: R int64 on the device, read as stored. Workspace from the torch
// allocator, no host synchronisation.
static inline SortedIndex build_sorted_index(const at::Tensor& ids, long R,
                                             long V, hipStream_t stream) {
  TORCH_CHECK(sidx_supported(R, V), "sorted index: need 1 <= R <= ",
              SIDX_MAX_ROWS, " and V * R <= 2^32, got R = ", R, ", V = ", V);
  const int SL = R <= 8192 ? 512 : SIDX_SLICE_MAX;
  const int NS = (int)((R + SL - 1) / SL);
  SortedIndex si;
  si.buf = at::empty({(long)NS * R + 2 * R + V + 1},
                     ids.options().dtype(at::kInt));
  int* cnt = si.buf.data_ptr<int>();
  int* order = cnt + (long)NS * R;
  int* skey = order + R;
  int* start = skey + R;
  const long* idp = ids.data_ptr<long>();
  hipLaunchKernelGGL(sidx_count_kernel,
                     dim3((unsigned)((R + SIDX_TILE - 1) / SIDX_TILE), NS),
                     dim3(SIDX_TILE), 0, stream, idp, (int)R, (int)V, SL, cnt);
  hipLaunchKernelGGL(sidx_place_kernel, dim3((unsigned)((R + 255) / 256)),
                     dim3(256), 0, stream, idp, (int)R, (int)V, NS,
                     (const int*)cnt, order, skey);
  hipLaunchKernelGGL(sidx_start_kernel, dim3((unsigned)((R + 1 + 255) / 256)),
                     dim3(256), 0, stream, (const int*)skey, (int)R, (int)V,
                     start);
  si.order = order;
  si.skey = skey;
  si.start = start;
  return si;
}
