// K23: moments of numeric columns grouped by a dictionary-code column.
//
// Block of pair (c, v): [sizes[c] + 1][3] fp64, slot-major; slot g holds
// (n, s1, s2) = (#rows, sum d, sum d^2) with d = (double)x - shift[v] over
// the rows whose code maps to slot g and whose x is not NaN. The slot rule
// is K5's and K22's: code v takes slot v when 0 <= v < size, the null slot
// `size` otherwise. +-inf is counted and goes through the sums as IEEE says.
//
// No floating-point atomic anywhere: every thread owns private
// accumulators in LDS, laid out [cell][thread] (the address differs per
// thread by 8 * tid only, so an update is conflict-free whatever the slot)
// and touched with plain loads and stores. After its rows the block sums
// over threads in a fixed tree order and writes [item][chunk][cell][3]
// partials; a second kernel sums the chunks in ascending order. The same
// call on the same input therefore returns the same bits.
//
// Work item: one code column, a slot window [g0, g0 + w) and P value
// columns of one dtype with w * P <= GRP_CELLS. A dictionary whose slots
// fit GRP_CELLS is one window, and the host packs up to GRP_PMAX value
// columns that share the code column into the item: the codes are read
// once for all of them. A larger dictionary becomes ceil(slots /
// GRP_CELLS) items with P = 1, each skipping the rows outside its window.
// grid = items x row chunks. Codes and values come in with 16-byte
// nontemporal loads (scalar head and tail); an item whose columns sit at
// different offsets inside a 16-byte line loads element by element.
//
// Item descriptor: GRP_ITEM_WORDS int64 words
//   [0] code column  [1] dictionary size  [2] P  [3] g0  [4] w
//   [5 + 2p ..] value column p: index into the launch's value table,
//               output offset of its pair's block

#include <hip/hip_runtime.h>
#include <cstdint>

#include "anovos_kernels.h"  // GRP_CELLS, GRP_PMAX, GRP_THREADS, GRP_ITEM_WORDS

#define DEV_INLINE __device__ __forceinline__

typedef int nat_i4 __attribute__((ext_vector_type(4)));
typedef float nat_f4 __attribute__((ext_vector_type(4)));
typedef double nat_d2 __attribute__((ext_vector_type(2)));

DEV_INLINE int grp_slot(int c, int size) { return (c >= 0 && c < size) ? c : size; }

// The columns arrive through a pointer table, so the compiler would treat
// them as flat pointers: flat loads count on the LDS counter as well, and
// every accumulator update would wait for all outstanding column loads.
// Global-address-space pointers give global_load with a counter of its own.
#define GRP_GLOBAL __attribute__((address_space(1)))

DEV_INLINE bool grp_aligned16(const GRP_GLOBAL void *p) { return ((uintptr_t)p & 15) == 0; }

// four consecutive rows of a value column from a 16-byte aligned address
DEV_INLINE void grp_load4(const float GRP_GLOBAL *p, float (&x)[4]) {
  const nat_f4 v = __builtin_nontemporal_load((const nat_f4 GRP_GLOBAL *)p);
  x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
}
DEV_INLINE void grp_load4(const double GRP_GLOBAL *p, double (&x)[4]) {
  const nat_d2 a = __builtin_nontemporal_load((const nat_d2 GRP_GLOBAL *)p);
  const nat_d2 b = __builtin_nontemporal_load((const nat_d2 GRP_GLOBAL *)p + 1);
  x[0] = a.x, x[1] = a.y, x[2] = b.x, x[3] = b.y;
}

template <typename T>
__global__ __launch_bounds__(GRP_THREADS) void grouped_moments_kernel(
    const int32_t *const *codes, const T *const *vals, const double *shifts,
    const int64_t *items, int64_t n, int64_t per, int nchunks, double *partials) {
  const int item = blockIdx.x / nchunks;
  const int chunk = blockIdx.x % nchunks;
  const int tid = threadIdx.x;
  const int64_t *__restrict__ it = items + (int64_t)item * GRP_ITEM_WORDS;
  const int32_t GRP_GLOBAL *__restrict__ cc = (const int32_t GRP_GLOBAL *)codes[it[0]];
  const int size = (int)it[1];
  const int np = (int)it[2];
  const int g0 = (int)it[3];
  const int w = (int)it[4];
  const int cells = np * w;  // <= GRP_CELLS, checked by the host
  const int64_t s = min(n, (int64_t)chunk * per);
  const int64_t e = min(n, s + per);  // per is rounded up: late chunks can be empty

  // [cells][THREADS] s1, [cells][THREADS] s2, [cells][THREADS] row counts
  extern __shared__ double acc[];
  double *s1 = acc;
  double *s2 = acc + cells * GRP_THREADS;
  uint32_t *cn = reinterpret_cast<uint32_t *>(acc + 2 * cells * GRP_THREADS);
  for (int c = 0; c < cells; ++c) {
    s1[c * GRP_THREADS + tid] = 0.0;
    s2[c * GRP_THREADS + tid] = 0.0;
    cn[c * GRP_THREADS + tid] = 0u;
  }

  // value descriptors: block-uniform, the loops below are fully unrolled
  // so these stay in registers
  const T GRP_GLOBAL *__restrict__ vp[GRP_PMAX];
  double sh[GRP_PMAX];
#pragma unroll
  for (int p = 0; p < GRP_PMAX; ++p) {
    if (p < np) {
      vp[p] = (const T GRP_GLOBAL *)vals[it[5 + 2 * p]];
      sh[p] = shifts[it[5 + 2 * p]];
    } else {
      vp[p] = nullptr;
      sh[p] = 0.0;
    }
  }

  // owner-only update of cell (p, gl) with one value
  auto add = [&](int p, int gl, T xv) {
    if (xv == xv) {
      const double d = (double)xv - sh[p];
      const int i = (p * w + gl) * GRP_THREADS + tid;
      cn[i] += 1u;
      s1[i] += d;
      s2[i] += d * d;
    }
  };
  auto add_row = [&](int64_t r) {
    const int gl = grp_slot(cc[r], size) - g0;
    if ((unsigned)gl < (unsigned)w) {
#pragma unroll
      for (int p = 0; p < GRP_PMAX; ++p)
        if (p < np) add(p, gl, vp[p][r]);
    }
  };

  // rows up to the codes' next 16-byte line; the vector path needs every
  // value column of the item on a 16-byte line there as well (the chunk
  // length is a multiple of 4 rows, so this holds for all chunks or none)
  const int64_t head = min((int64_t)((4 - (int)(((uintptr_t)(cc + s) >> 2) & 3)) & 3), e - s);
  const int64_t vs = s + head;
  bool same = true;
#pragma unroll
  for (int p = 0; p < GRP_PMAX; ++p)
    if (p < np) same = same && grp_aligned16(vp[p] + vs);

  if (same) {
    const int64_t nv = (e - vs) / 4;
    if ((int64_t)tid < head) add_row(s + tid);
    const nat_i4 GRP_GLOBAL *__restrict__ cv = (const nat_i4 GRP_GLOBAL *)(cc + vs);
    int64_t i = tid;
    if (np == 1) {
      // one value column (every item of a dictionary with several windows):
      // two streams per block leave too few bytes in flight to cover the
      // latency of HBM, so four trips' loads are issued before the first
      // is used
      const T GRP_GLOBAL *__restrict__ v0 = vp[0] + vs;
      for (; i + 3 * GRP_THREADS < nv; i += 4 * GRP_THREADS) {
        nat_i4 c4[4];
        T x[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          c4[u] = __builtin_nontemporal_load(&cv[i + u * GRP_THREADS]);
          grp_load4(v0 + 4 * (i + u * GRP_THREADS), x[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int gl[4] = {grp_slot(c4[u].x, size) - g0, grp_slot(c4[u].y, size) - g0,
                             grp_slot(c4[u].z, size) - g0, grp_slot(c4[u].w, size) - g0};
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if ((unsigned)gl[k] < (unsigned)w) add(0, gl[k], x[u][k]);
        }
      }
    }
    for (; i < nv; i += GRP_THREADS) {
      const nat_i4 c4 = __builtin_nontemporal_load(&cv[i]);
      T x[GRP_PMAX][4];
#pragma unroll
      for (int p = 0; p < GRP_PMAX; ++p)
        if (p < np) grp_load4(vp[p] + vs + 4 * i, x[p]);
      const int gl[4] = {grp_slot(c4.x, size) - g0, grp_slot(c4.y, size) - g0,
                         grp_slot(c4.z, size) - g0, grp_slot(c4.w, size) - g0};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if ((unsigned)gl[k] < (unsigned)w) {
#pragma unroll
          for (int p = 0; p < GRP_PMAX; ++p)
            if (p < np) add(p, gl[k], x[p][k]);
        }
      }
    }
    for (int64_t r = vs + nv * 4 + tid; r < e; r += GRP_THREADS) add_row(r);
  } else {
    // views at different offsets inside a line: no common peel exists,
    // one element per load (still coalesced)
    for (int64_t r = s + tid; r < e; r += GRP_THREADS) add_row(r);
  }

  // sum over threads in a fixed tree order
  __syncthreads();
  for (int stride = GRP_THREADS / 2; stride > 0; stride >>= 1) {
    if (tid < stride) {
      for (int c = 0; c < cells; ++c) {
        const int i = c * GRP_THREADS + tid;
        s1[i] += s1[i + stride];
        s2[i] += s2[i + stride];
        cn[i] += cn[i + stride];
      }
    }
    __syncthreads();
  }
  if (tid < cells) {
    double *o = partials + (((int64_t)item * nchunks + chunk) * GRP_CELLS + tid) * 3;
    o[0] = (double)cn[tid * GRP_THREADS];
    o[1] = s1[tid * GRP_THREADS];
    o[2] = s2[tid * GRP_THREADS];
  }
}

// Second stage: one thread per (item, cell, statistic) sums the chunks in
// ascending order into the pair's output block.
__global__ __launch_bounds__(256) void grouped_moments_merge_kernel(
    const int64_t *items, int nitems, int nchunks, const double *partials, double *out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)nitems * GRP_CELLS * 3) return;
  const int k = (int)(idx % 3);
  const int cell = (int)((idx / 3) % GRP_CELLS);
  const int64_t item = idx / (3 * GRP_CELLS);
  const int64_t *__restrict__ it = items + item * GRP_ITEM_WORDS;
  const int np = (int)it[2];
  const int w = (int)it[4];
  if (cell >= np * w) return;
  const int p = cell / w;
  const int64_t g = it[3] + cell % w;
  if (g > it[1]) return;
  const double *src = partials + (item * nchunks * GRP_CELLS + cell) * 3 + k;
  double sum = 0.0;
  for (int c = 0; c < nchunks; ++c) sum += src[(int64_t)c * GRP_CELLS * 3];
  out[it[6 + 2 * p] + g * 3 + k] = sum;
}

extern "C" int anovos_grouped_moments(const int32_t *const *codes, const void *const *vals,
                                      const double *shifts, const int64_t *items, int nitems,
                                      int64_t n, int64_t per, int nchunks, int cells, int dtype,
                                      double *partials, double *out, hipStream_t stream) {
  // cells: the most accumulator cells (w * P) any item of the launch needs
  if (cells < 1 || cells > GRP_CELLS || nitems < 1 || nchunks < 1) return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)cells * GRP_THREADS * GRP_CELL_BYTES;
  const dim3 grid((unsigned)nitems * (unsigned)nchunks);
  hipError_t err;
  if (dtype == 0) {
    auto kern = grouped_moments_kernel<float>;
    err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(kern, grid, dim3(GRP_THREADS), lds, stream, codes,
                       reinterpret_cast<const float *const *>(vals), shifts, items, n, per,
                       nchunks, partials);
  } else {
    auto kern = grouped_moments_kernel<double>;
    err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(kern, grid, dim3(GRP_THREADS), lds, stream, codes,
                       reinterpret_cast<const double *const *>(vals), shifts, items, n, per,
                       nchunks, partials);
  }
  err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  const int64_t total = (int64_t)nitems * GRP_CELLS * 3;
  hipLaunchKernelGGL(grouped_moments_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256),
                     0, stream, items, nitems, nchunks, partials, out);
  return (int)hipGetLastError();
}
