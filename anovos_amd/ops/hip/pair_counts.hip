// K22: contingency tables for pairs of dictionary-code columns.
//
// Table of pair (i, j): [sizes[i] + 1][sizes[j] + 1] row-major int64; a
// code v of column c goes to slot v when 0 <= v < sizes[c] and to the null
// slot sizes[c] otherwise (NULL_CODE, any other negative code, any code
// >= size) — the rule of code_counts_multi_kernel (K5), in two dimensions.
//
// One block per pair would read two columns per table. Instead the host
// packs work items "anchor column + up to PAIR_PMAX partner columns" whose
// tables together fit PAIR_LDS_SLOTS uint32 counters: a block streams its
// row chunk of the anchor once and of each partner once (16-byte
// nontemporal loads), bumps the partner tables in LDS and flushes every
// non-zero counter with one 64-bit global atomic. A table with more cells
// than the LDS budget is an item of its own (one partner) and is counted
// with 64-bit global atomics straight into its output table. Both kinds
// of item sit in one launch; grid = items x nchunks. Counts are integers,
// so the result does not depend on the order of the atomics.
//
// Item descriptor: PAIR_ITEM_WORDS int64 words
//   [0] anchor column  [1] anchor size  [2] partners
//   [3] LDS counters the item stages (0: global-atomic item)
//   [4 + 4p ..] partner p: column, size, LDS offset, output offset

#include <hip/hip_runtime.h>
#include <cstdint>

#include "anovos_kernels.h"  // PAIR_PMAX, PAIR_LDS_SLOTS, PAIR_ITEM_WORDS

#define THREADS 256
#define DEV_INLINE __device__ __forceinline__

typedef int nat_i4 __attribute__((ext_vector_type(4)));

DEV_INLINE int pair_slot(int c, int size) { return (c >= 0 && c < size) ? c : size; }

// element offset (0..3) of p inside its 16-byte line; columns are int32,
// so p is 4-byte aligned
DEV_INLINE int pair_misalign(const int32_t *p) {
  return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);
}

__global__ __launch_bounds__(THREADS) void pair_code_counts_kernel(
    const int32_t *const *cols, const int64_t *items, int64_t n, int64_t per,
    int nchunks, uint64_t *out) {
  const int item = blockIdx.x / nchunks;
  const int chunk = blockIdx.x % nchunks;
  const int64_t *__restrict__ it = items + (int64_t)item * PAIR_ITEM_WORDS;
  const int32_t *__restrict__ ac = cols[it[0]];
  const int sa = (int)it[1];
  const int np = (int)it[2];
  const int staged = (int)it[3];
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  if (s >= e) return;  // whole block: per is rounded up, late chunks can be empty

  if (!staged) {
    // oversized table: one partner, counted in global memory
    const int32_t *__restrict__ bc = cols[it[4]];
    const int sb = (int)it[5];
    uint64_t *o = out + it[7];
    const int64_t stride = (int64_t)sb + 1;
    for (int64_t r = s + threadIdx.x; r < e; r += THREADS) {
      const int64_t cell = (int64_t)pair_slot(ac[r], sa) * stride + pair_slot(bc[r], sb);
      atomicAdd((unsigned long long *)&o[cell], 1ull);
    }
    return;
  }

  extern __shared__ uint32_t cnt[];
  for (int i = threadIdx.x; i < staged; i += THREADS) cnt[i] = 0;

  // partner descriptors: block-uniform, the loops below are fully
  // unrolled so these stay in registers
  const int32_t *__restrict__ pc[PAIR_PMAX];
  int ps[PAIR_PMAX], pl[PAIR_PMAX];
  bool same = true;
  const int mis = pair_misalign(ac + s);
#pragma unroll
  for (int p = 0; p < PAIR_PMAX; ++p) {
    if (p < np) {
      pc[p] = cols[it[4 + 4 * p]];
      ps[p] = (int)it[5 + 4 * p];
      pl[p] = (int)it[6 + 4 * p];
      same = same && (pair_misalign(pc[p] + s) == mis);
    } else {
      pc[p] = ac;
      ps[p] = 0;
      pl[p] = 0;
    }
  }
  __syncthreads();

  auto count_row = [&](int64_t r) {
    const int a = pair_slot(ac[r], sa);
#pragma unroll
    for (int p = 0; p < PAIR_PMAX; ++p)
      if (p < np) atomicAdd(&cnt[pl[p] + a * (ps[p] + 1) + pair_slot(pc[p][r], ps[p])], 1u);
  };

  if (same) {
    // every column of the item starts the chunk at the same offset inside
    // a 16-byte line: peel rows up to the line boundary, then aligned
    // 16-byte loads, then the tail
    const int64_t head = min((int64_t)((4 - mis) & 3), e - s);
    const int64_t vs = s + head;
    const int64_t nv = (e - vs) / 4;
    if ((int64_t)threadIdx.x < head) count_row(s + threadIdx.x);
    const nat_i4 *__restrict__ av = reinterpret_cast<const nat_i4 *>(ac + vs);
    for (int64_t i = threadIdx.x; i < nv; i += THREADS) {
      const nat_i4 a = __builtin_nontemporal_load(&av[i]);
      nat_i4 b[PAIR_PMAX];
#pragma unroll
      for (int p = 0; p < PAIR_PMAX; ++p)
        if (p < np) b[p] = __builtin_nontemporal_load(reinterpret_cast<const nat_i4 *>(pc[p] + vs) + i);
      const int a0 = pair_slot(a.x, sa), a1 = pair_slot(a.y, sa);
      const int a2 = pair_slot(a.z, sa), a3 = pair_slot(a.w, sa);
#pragma unroll
      for (int p = 0; p < PAIR_PMAX; ++p) {
        if (p < np) {
          uint32_t *t = cnt + pl[p];
          const int sb = ps[p], st = ps[p] + 1;
          atomicAdd(&t[a0 * st + pair_slot(b[p].x, sb)], 1u);
          atomicAdd(&t[a1 * st + pair_slot(b[p].y, sb)], 1u);
          atomicAdd(&t[a2 * st + pair_slot(b[p].z, sb)], 1u);
          atomicAdd(&t[a3 * st + pair_slot(b[p].w, sb)], 1u);
        }
      }
    }
    for (int64_t r = vs + nv * 4 + threadIdx.x; r < e; r += THREADS) count_row(r);
  } else {
    // views at different offsets inside a line: no common peel exists,
    // 4-byte loads (still coalesced)
    for (int64_t r = s + threadIdx.x; r < e; r += THREADS) count_row(r);
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < PAIR_PMAX; ++p) {
    if (p < np) {
      uint64_t *o = out + it[7 + 4 * p];
      const uint32_t *t = cnt + pl[p];
      const int cells = (sa + 1) * (ps[p] + 1);
      for (int i = threadIdx.x; i < cells; i += THREADS)
        if (t[i]) atomicAdd((unsigned long long *)&o[i], (unsigned long long)t[i]);
    }
  }
}

extern "C" int anovos_pair_code_counts(const int32_t *const *cols, const int64_t *items,
                                       int nitems, int64_t n, int64_t per, int nchunks,
                                       int lds_slots, uint64_t *out, hipStream_t stream) {
  // lds_slots: the most counters any staged item of the launch needs (0
  // when every item counts in global memory)
  if (lds_slots < 0 || lds_slots > PAIR_LDS_SLOTS) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pair_code_counts_kernel, dim3((unsigned)nitems * (unsigned)nchunks),
                     dim3(THREADS), (size_t)lds_slots * 4, stream, cols, items, n, per,
                     nchunks, out);
  return (int)hipGetLastError();
}
