// K24: rank grades of numerical columns on a grid of cells.
//
// A column comes with ascending cutoffs c_0 < ... < c_{q-1}, q <=
// GRADE_MAX_CELLS - 1, and a value x lies in cell(x) = #{j : c_j < x} in
// [0, q] — the placement of bucketize_float_kernel (K6), right-closed, the
// comparison exact as if both sides were fp64: an f32 column scans f32
// cutoffs that were stepped down one ulp where (double)(float)c > c, which
// gives (c < (double)v) <=> (cf < v) for every f32 v. NaN is null.
//
//   grade_counts_kernel  read-only: per column, slot 0 = nulls and slot
//                        1 + j = rows of cell j. Counters in LDS — a
//                        private stride-17 row per thread when every column
//                        of the launch has <= 15 cutoffs (binary and
//                        low-cardinality columns would serialise on two
//                        shared counters), shared LDS atomics above — and
//                        one 64-bit global atomic per non-zero slot per
//                        block. Integer counts: the same on every call.
//   grade_apply_kernel   out = table[cell(x)], null_grade for NaN; f32 out.
//
// Both: one block per (column, chunk), chunk-major block order, rows up to
// the first 16-byte line of the input peeled, then 16-byte nontemporal loads
// of four rows per thread (f64: two loads), then a scalar tail. Columns are
// read through global address-space pointers so the loads do not wait on
// the LDS counter with the cutoff reads between them. No alignment beyond
// the element's is assumed for the output: its 16-byte stores sit at the
// input's offset inside a line only when both views start alike.

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "anovos_kernels.h"  // GRADE_MAX_CELLS

#define THREADS 256
#define DEV_INLINE __device__ __forceinline__
#define GLOBAL_AS __attribute__((address_space(1)))
// rule and stride of BKT_PRIV_STRIDE (K6 with counts)
#define GRADE_PRIV_STRIDE 17
// linear scan with a wave-uniform index up to this many cutoffs
#define GRADE_LINEAR_NCUT 32

typedef float nat_f4 __attribute__((ext_vector_type(4)));
typedef double nat_d2 __attribute__((ext_vector_type(2)));
// 16-byte store at the alignment of a float
typedef nat_f4 __attribute__((aligned(4))) nat_f4_a4;

DEV_INLINE int grade_block_column(int nchunks) { return blockIdx.x % (gridDim.x / nchunks); }
DEV_INLINE int grade_block_chunk(int nchunks) { return blockIdx.x / (gridDim.x / nchunks); }

DEV_INLINE int64_t grade_chunk_rows(int64_t n, int nchunks) {
  const uint64_t t = (uint64_t)n + (uint64_t)(nchunks - 1);
  if (t <= 0xFFFFFFFFull) return (int64_t)((uint32_t)t / (uint32_t)nchunks);
  return (int64_t)(t / (uint64_t)nchunks);
}

template <typename T>
struct Quad {
  T x, y, z, w;
};

// four rows from a 16-byte aligned address
DEV_INLINE Quad<float> grade_load4(const float GLOBAL_AS *p) {
  const nat_f4 v = __builtin_nontemporal_load((const nat_f4 GLOBAL_AS *)p);
  return {v.x, v.y, v.z, v.w};
}
DEV_INLINE Quad<double> grade_load4(const double GLOBAL_AS *p) {
  const nat_d2 a = __builtin_nontemporal_load((const nat_d2 GLOBAL_AS *)p);
  const nat_d2 b = __builtin_nontemporal_load((const nat_d2 GLOBAL_AS *)p + 1);
  return {a.x, a.y, b.x, b.y};
}

// rows before the first 16-byte line boundary at or after p
template <typename T>
DEV_INLINE int64_t grade_head(const T *p) {
  return (int64_t)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T));
}

// Cutoff j sits at LDS entry j + j / 32: one pad entry after every 32. The
// first steps of a binary search over a sorted array probe entries a power
// of two apart (511, 255, 767, 127, ...), which without the pad all lie in
// one LDS bank, so the 2, 4, 8, ... addresses of a step are served one
// after the other. Lists of up to 32 cutoffs (the linear scan) are laid
// out unchanged. 150 f32 columns x 32M rows at 1023 cutoffs: grade_counts
// 17.4 -> 12.4 ms with the pad, 10.0 ms with the lane-uniform step of
// grade_cell as well (docs/BENCHMARKS.md).
DEV_INLINE int grade_pos(int j) { return j + (j >> 5); }
// entries a list of ncut cutoffs takes
__host__ __device__ constexpr int grade_cut_entries(int ncut) { return ncut + (ncut >> 5) + 1; }

// The column's cutoffs in LDS, in the column's own type.
template <typename T>
DEV_INLINE void grade_stage_cutoffs(T *cuts, const double *src, int ncut) {
  for (int i = threadIdx.x; i < ncut; i += THREADS) {
    const double c = src[i];
    if (sizeof(T) == 4) {
      float cf = (float)c;
      if ((double)cf > c) cf = nextafterf(cf, -INFINITY);
      cuts[grade_pos(i)] = (T)cf;
    } else {
      cuts[grade_pos(i)] = (T)c;
    }
  }
}

// #{j : cuts[j] < v}; v is not NaN
template <typename T>
DEV_INLINE int grade_cell(const T *cuts, int ncut, T v) {
  int lo = 0;
  if (ncut <= GRADE_LINEAR_NCUT) {
    // cuts[j] is an LDS broadcast, the adds are branchless
    for (int j = 0; j < ncut; ++j) lo += (cuts[j] < v) ? 1 : 0;
  } else {
    // branchless lower bound over [lo, lo + len]: len and half take the
    // same values in every lane, so they stay in scalar registers and a
    // step is one probe, one compare and one select
    int len = ncut;
    while (len > 1) {
      const int half = len >> 1;
      lo = (cuts[grade_pos(lo + half - 1)] < v) ? lo + half : lo;
      len -= half;
    }
    lo += (cuts[grade_pos(lo)] < v) ? 1 : 0;
  }
  return lo;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void grade_counts_kernel(
    const T *const *cols, const int64_t *lens, const double *cutflat,
    const int64_t *cutoff_off, const int *cutoff_len, int nchunks, int max_ncut,
    uint64_t *counts, const int64_t *count_off) {
  // [max_ncut + 2] shared counters, [THREADS][17] privates (private mode),
  // then the cutoffs, grade_cut_entries(max_ncut) entries (8-byte aligned:
  // the counters before them are rounded up to an even number of words)
  extern __shared__ uint32_t grade_lds[];
  const int col = grade_block_column(nchunks);
  const int chunk = grade_block_chunk(nchunks);
  const int ncut = cutoff_len[col];
  const int64_t n = lens[col];
  const int64_t per = grade_chunk_rows(n, nchunks);
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  if (s >= e) return;  // whole block: late chunks can be empty

  const bool use_priv = (max_ncut + 2 <= GRADE_PRIV_STRIDE);
  uint32_t *cnt = grade_lds;
  int words = (max_ncut + 2 + 1) & ~1;
  uint32_t *priv = cnt + words + (uint32_t)threadIdx.x * GRADE_PRIV_STRIDE;
  if (use_priv) words += (THREADS * GRADE_PRIV_STRIDE + 1) & ~1;
  T *cuts = reinterpret_cast<T *>(grade_lds + words);
  for (int i = threadIdx.x; i < max_ncut + 2; i += THREADS) cnt[i] = 0;
  if (use_priv)
    for (int j = 0; j < GRADE_PRIV_STRIDE; ++j) priv[j] = 0;
  grade_stage_cutoffs<T>(cuts, cutflat + cutoff_off[col], ncut);
  __syncthreads();

  const T *__restrict__ x = cols[col];
  auto count = [&](T v) {
    const int slot = (v != v) ? 0 : 1 + grade_cell<T>(cuts, ncut, v);
    if (use_priv) priv[slot] += 1u;
    else atomicAdd(&cnt[slot], 1u);
  };

  const int64_t head = min(grade_head<T>(x + s), e - s);
  const int64_t vs = s + head;
  const int64_t nv = (e - vs) / 4;
  if ((int64_t)threadIdx.x < head) count(x[s + threadIdx.x]);
  const T GLOBAL_AS *xv = (const T GLOBAL_AS *)(x + vs);
  // the next four rows are in flight while these go through the counters
  int64_t i = threadIdx.x;
  Quad<T> nx = {0, 0, 0, 0};
  if (i < nv) nx = grade_load4(xv + 4 * i);
  for (; i < nv; i += THREADS) {
    const Quad<T> q = nx;
    if (i + THREADS < nv) nx = grade_load4(xv + 4 * (i + THREADS));
    count(q.x);
    count(q.y);
    count(q.z);
    count(q.w);
  }
  for (int64_t r = vs + nv * 4 + threadIdx.x; r < e; r += THREADS) count(x[r]);

  __syncthreads();
  const int slots = ncut + 2;
  if (use_priv) {
    for (int b = 0; b < slots; ++b) {
      const uint32_t v = priv[b];
      if (v) atomicAdd(&cnt[b], v);
    }
    __syncthreads();
  }
  uint64_t *g = counts + count_off[col];
  for (int b = threadIdx.x; b < slots; b += THREADS)
    if (cnt[b]) atomicAdd((unsigned long long *)&g[b], (unsigned long long)cnt[b]);
}

template <typename T>
__global__ __launch_bounds__(THREADS) void grade_apply_kernel(
    const T *const *cols, const int64_t *lens, const double *cutflat,
    const int64_t *cutoff_off, const int *cutoff_len, const float *tabflat,
    const int64_t *tab_off, float null_grade, int nchunks, int max_ncut,
    float *const *outs) {
  // [max_ncut + 1] table entries (rounded up to an even number of words),
  // then the cutoffs, grade_cut_entries(max_ncut) entries
  extern __shared__ uint32_t grade_lds[];
  const int col = grade_block_column(nchunks);
  const int chunk = grade_block_chunk(nchunks);
  const int ncut = cutoff_len[col];
  const int64_t n = lens[col];
  const int64_t per = grade_chunk_rows(n, nchunks);
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  if (s >= e) return;

  float *table = reinterpret_cast<float *>(grade_lds);
  T *cuts = reinterpret_cast<T *>(grade_lds + ((max_ncut + 1 + 1) & ~1));
  const float *tsrc = tabflat + tab_off[col];
  for (int i = threadIdx.x; i < ncut + 1; i += THREADS) table[i] = tsrc[i];
  grade_stage_cutoffs<T>(cuts, cutflat + cutoff_off[col], ncut);
  __syncthreads();

  const T *__restrict__ x = cols[col];
  float *__restrict__ out = outs[col];
  auto grade = [&](T v) -> float {
    return (v != v) ? null_grade : table[grade_cell<T>(cuts, ncut, v)];
  };
  auto grade4 = [&](const Quad<T> &q) -> nat_f4 {
    nat_f4 r;
    r.x = grade(q.x);
    r.y = grade(q.y);
    r.z = grade(q.z);
    r.w = grade(q.w);
    return r;
  };

  const int64_t head = min(grade_head<T>(x + s), e - s);
  const int64_t vs = s + head;
  const int64_t nv = (e - vs) / 4;
  if ((int64_t)threadIdx.x < head) out[s + threadIdx.x] = grade(x[s + threadIdx.x]);
  const T GLOBAL_AS *xv = (const T GLOBAL_AS *)(x + vs);
  nat_f4_a4 GLOBAL_AS *ov = (nat_f4_a4 GLOBAL_AS *)(out + vs);
  int64_t i = threadIdx.x;
  for (; i + THREADS < nv; i += 2 * THREADS) {
    const Quad<T> a = grade_load4(xv + 4 * i);
    const Quad<T> b = grade_load4(xv + 4 * (i + THREADS));
    const nat_f4 ra = grade4(a);
    const nat_f4 rb = grade4(b);
    __builtin_nontemporal_store(ra, &ov[i]);
    __builtin_nontemporal_store(rb, &ov[i + THREADS]);
  }
  for (; i < nv; i += THREADS) {
    const nat_f4 ra = grade4(grade_load4(xv + 4 * i));
    __builtin_nontemporal_store(ra, &ov[i]);
  }
  for (int64_t r = vs + nv * 4 + threadIdx.x; r < e; r += THREADS) out[r] = grade(x[r]);
}

static size_t grade_cut_bytes(int max_ncut, int dtype) {
  return (size_t)grade_cut_entries(max_ncut) * (dtype == 0 ? sizeof(float) : sizeof(double));
}

// counts is zeroed by the caller; column c of the launch owns the
// cutoff_len[c] + 2 slots at counts[count_off[c]]; 1 <= max_ncut sizes the
// LDS and cutoff_len[c] <= max_ncut <= GRADE_MAX_CELLS - 1.
extern "C" int anovos_grade_counts(const void *const *cols, const int64_t *lens, int ncols,
                                   const double *cutflat, const int64_t *cutoff_off,
                                   const int *cutoff_len, int max_ncut, int nchunks, int dtype,
                                   uint64_t *counts, const int64_t *count_off,
                                   hipStream_t stream) {
  if (max_ncut < 1 || max_ncut > GRADE_MAX_CELLS - 1 || ncols < 1 || nchunks < 1)
    return (int)hipErrorInvalidValue;
  size_t words = (size_t)((max_ncut + 2 + 1) & ~1);
  if (max_ncut + 2 <= GRADE_PRIV_STRIDE) words += (size_t)((THREADS * GRADE_PRIV_STRIDE + 1) & ~1);
  const size_t lds = words * sizeof(uint32_t) + grade_cut_bytes(max_ncut, dtype);
  const dim3 grid((unsigned)ncols * (unsigned)nchunks);
  if (dtype == 0)
    hipLaunchKernelGGL(grade_counts_kernel<float>, grid, dim3(THREADS), lds, stream,
                       (const float *const *)cols, lens, cutflat, cutoff_off, cutoff_len, nchunks,
                       max_ncut, counts, count_off);
  else
    hipLaunchKernelGGL(grade_counts_kernel<double>, grid, dim3(THREADS), lds, stream,
                       (const double *const *)cols, lens, cutflat, cutoff_off, cutoff_len, nchunks,
                       max_ncut, counts, count_off);
  return (int)hipGetLastError();
}

// column c's table: the cutoff_len[c] + 1 floats at tabflat[tab_off[c]]
extern "C" int anovos_grade_apply(const void *const *cols, const int64_t *lens, int ncols,
                                  const double *cutflat, const int64_t *cutoff_off,
                                  const int *cutoff_len, const float *tabflat,
                                  const int64_t *tab_off, float null_grade, int max_ncut,
                                  int nchunks, int dtype, float *const *outs,
                                  hipStream_t stream) {
  if (max_ncut < 1 || max_ncut > GRADE_MAX_CELLS - 1 || ncols < 1 || nchunks < 1)
    return (int)hipErrorInvalidValue;
  const size_t lds =
      (size_t)((max_ncut + 1 + 1) & ~1) * sizeof(uint32_t) + grade_cut_bytes(max_ncut, dtype);
  const dim3 grid((unsigned)ncols * (unsigned)nchunks);
  if (dtype == 0)
    hipLaunchKernelGGL(grade_apply_kernel<float>, grid, dim3(THREADS), lds, stream,
                       (const float *const *)cols, lens, cutflat, cutoff_off, cutoff_len, tabflat,
                       tab_off, null_grade, nchunks, max_ncut, outs);
  else
    hipLaunchKernelGGL(grade_apply_kernel<double>, grid, dim3(THREADS), lds, stream,
                       (const double *const *)cols, lens, cutflat, cutoff_off, cutoff_len, tabflat,
                       tab_off, null_grade, nchunks, max_ncut, outs);
  return (int)hipGetLastError();
}
