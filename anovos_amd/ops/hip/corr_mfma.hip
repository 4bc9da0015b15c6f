// K8: centered Gram matrix (correlation/covariance) on MFMA matrix cores.
//
// gram[i][j] = sum_r (x_i[r] - mean_i)(x_j[r] - mean_j), NaN -> 0 contribution.
// Reference semantics: association_evaluator.py:118-123 (MLlib Correlation
// .corr = one pass over the assembled vector column); here the pass is a
// tall-skinny X^T X on v_mfma_f32_16x16x32_bf16 (bf16 in, fp32 accumulate).
//
// Shape: k columns (tens..hundreds) x n rows (millions) -> HBM-bound
// (read n*k floats); MFMA keeps compute off the critical path.
//
// Two kernels. k <= 208 runs the single-read kernel further down (every
// column is read from HBM exactly once). Wider matrices run the
// pair-parallel kernel that follows:
//
// Tiling: columns padded to 16-col tiles; one workgroup per
// (tile-pair (i, j >= i), row-chunk). Each of the 4 waves strides
// 32-row MFMA steps across the chunk (wave w rows r0+32w, step 128) and
// accumulates its own f32x4 fragment; fragments are loaded STRAIGHT from
// global (8 consecutive rows of one column = 16 B per lane, coalesced
// across the 16 lanes of a row-group) — no LDS staging needed because
// each element is touched once per tile-pair. Per-block partials land in
// a [pairs*chunks][256] buffer; a second deterministic kernel reduces
// chunks in fp64 and mirrors the symmetric half (same no-atomics
// convention as anovos_kernels.hip).

#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>
#include <cmath>

#include "anovos_kernels.h"

#define THREADS 256

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ short to_bf16(float v) {
  union {
    float f;
    uint32_t u;
  } c{v};
  // round-to-nearest-even into the upper 16 bits
  uint32_t r = c.u + 0x7FFFu + ((c.u >> 16) & 1u);
  return (short)(r >> 16);
}

// Load one lane's A/B fragment: 8 consecutive rows of column `col`,
// centered, NaN->0, zero outside [0,k) x [0,limit).
__device__ __forceinline__ bf16x8 load_frag(const float *const *cols, int k,
                                            const float *means, int col,
                                            int64_t row, int64_t limit) {
  bf16x8 f;
  if (col < k) {
    const float *__restrict__ x = cols[col];
    const float m = means[col];
    if (row + 8 <= limit) {
      const float4 *p = reinterpret_cast<const float4 *>(x + row);
      float4 a = p[0], b = p[1];
      float v0 = a.x - m, v1 = a.y - m, v2 = a.z - m, v3 = a.w - m;
      float v4 = b.x - m, v5 = b.y - m, v6 = b.z - m, v7 = b.w - m;
      f[0] = to_bf16(isnan(v0) ? 0.f : v0);
      f[1] = to_bf16(isnan(v1) ? 0.f : v1);
      f[2] = to_bf16(isnan(v2) ? 0.f : v2);
      f[3] = to_bf16(isnan(v3) ? 0.f : v3);
      f[4] = to_bf16(isnan(v4) ? 0.f : v4);
      f[5] = to_bf16(isnan(v5) ? 0.f : v5);
      f[6] = to_bf16(isnan(v6) ? 0.f : v6);
      f[7] = to_bf16(isnan(v7) ? 0.f : v7);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = (row + e < limit) ? x[row + e] - m : 0.f;
        f[e] = to_bf16(isnan(v) ? 0.f : v);
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = 0;
  }
  return f;
}

__global__ __launch_bounds__(THREADS) void gram_partials_kernel(
    const float *const *cols, int64_t n, int k, const float *means,
    const int *pair_i, const int *pair_j, int row_chunks, float *partials) {
  const int pair = blockIdx.x / row_chunks;
  const int chunk = blockIdx.x % row_chunks;
  const int i0 = pair_i[pair] * 16;
  const int j0 = pair_j[pair] * 16;

  // 32-row-aligned chunk bounds
  const int64_t steps_total = (n + 31) / 32;
  const int64_t steps_per = (steps_total + row_chunks - 1) / row_chunks;
  const int64_t step_s = (int64_t)chunk * steps_per;
  const int64_t step_e = min(steps_total, step_s + steps_per);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int m = lane & 15;         // tile row (A) / tile col (B)
  const int ko = (lane >> 4) * 8;  // K offset within the 32-row step

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int64_t s = step_s + wave; s < step_e; s += 4) {
    const int64_t r = s * 32 + ko;
    bf16x8 a = load_frag(cols, k, means, i0 + m, r, n);
    bf16x8 b = (j0 == i0) ? a : load_frag(cols, k, means, j0 + m, r, n);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }

  // combine the 4 waves' [16,16] fragments via LDS (C/D layout:
  // col = lane&15, row = (lane>>4)*4 + reg)
  __shared__ float lds[4][256];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = (lane >> 4) * 4 + reg;
    lds[wave][row * 16 + (lane & 15)] = acc[reg];
  }
  __syncthreads();
  const int c = threadIdx.x;
  partials[(int64_t)blockIdx.x * 256 + c] =
      lds[0][c] + lds[1][c] + lds[2][c] + lds[3][c];
}

__global__ __launch_bounds__(THREADS) void gram_reduce_kernel(
    const float *partials, int row_chunks, const int *pair_i,
    const int *pair_j, int k, float *gram) {
  const int pair = blockIdx.x;
  const int c = threadIdx.x;
  const int row = c >> 4, col = c & 15;
  double s = 0.0;
  for (int ch = 0; ch < row_chunks; ++ch)
    s += (double)partials[((int64_t)pair * row_chunks + ch) * 256 + c];
  const int gi = pair_i[pair] * 16 + row;
  const int gj = pair_j[pair] * 16 + col;
  if (gi < k && gj < k) {
    gram[(int64_t)gi * k + gj] = (float)s;
    gram[(int64_t)gj * k + gi] = (float)s;
  }
}

extern "C" int anovos_centered_gram(const void *const *cols, int64_t n, int k,
                                    const float *means, const int *pair_i,
                                    const int *pair_j, int npairs,
                                    int row_chunks, float *partials,
                                    float *gram, hipStream_t stream) {
  dim3 grid1((uint32_t)(npairs * row_chunks));
  hipLaunchKernelGGL(gram_partials_kernel, grid1, dim3(THREADS), 0, stream,
                     (const float *const *)cols, n, k, means, pair_i, pair_j,
                     row_chunks, partials);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((uint32_t)npairs), dim3(THREADS),
                     0, stream, partials, row_chunks, pair_i, pair_j, k, gram);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------
// Single-read Gram variant. The pair-parallel kernel above re-reads
// every column once per tile-pair it appears in (~kt times, 11.7x HBM
// traffic at k=150 — measured 197 ms in the bench step). Here ONE block
// stages a 128-row macro-slab (4 MFMA k-steps of 32 rows) of ALL kt*16
// columns through LDS once per round (centered bf16), then its 4 waves
// compute EVERY 16x16 tile-pair from LDS: HBM traffic = n*k*4 bytes
// exactly. Block b owns the macro-slabs [b*macro_per, (b+1)*macro_per),
// a function of n and row_chunks only.
//
// LDS layout: [4 stages][4 ko-groups][kstride cols][8 rows] bf16 — one
// 16-byte block per (stage, ko-group, col), so an MFMA A/B fragment (8
// K-rows of one column) is a single aligned ds_read_b128; consecutive
// columns are 16 B apart (minimum-phase bank pattern for the 16 lanes
// of a row-group).
//
// Staging. Thread t stages the 4-row segment (t & 31) of the columns
// (t >> 5) + 8*it, it = 0..KT*2-1, every round: the same columns and
// the same LDS slots each time. So the column base pointers are
// resolved once per block into registers (as global-address-space
// pointers, so the loads are global_load_dwordx4, not flat), the means
// once into a small LDS table, and the padding columns' slots are
// zeroed once and never written again; a padding column is never
// dereferenced. A round over a full macro-slab then has no bounds
// checks and a compile-time trip count: all of a thread's 16-byte loads
// are issued back to back, and for KT <= 10 the loads of round s+1 are
// issued into registers BEFORE the MFMA phase of round s and converted
// and written to LDS after the barrier that ends it, so the HBM read
// stays in flight through the whole round. (The previous kernel fetched
// cols[c] and means[c] again for every 16 bytes and waited for each data
// load before issuing the next — two dependent round trips per 16
// bytes, ~12 KB in flight per CU; it was latency-bound at 2.4 TB/s, not
// bound by DRAM pages as an earlier note here claimed.) Only the one
// partial macro-slab at the end of the column takes the guarded
// element-wise path.
//
// Pairs are assigned to waves in CONTIGUOUS chunks of PPW pairs of the
// i-major upper-tri order. Accumulators live in registers via a
// compile-time-unrolled pair loop (PPW = 14 at kt = 10, 23 at kt = 13;
// larger k falls back). Slots past the last pair (only in the last
// wave) recompute pair 0 and are never written, which keeps the MFMA
// phase branch-free.
// Deterministic: fixed block/step split, each accumulator takes its
// block's 32-row steps in ascending row order, fp64 block-order reduce.
// ------------------------------------------------------------------

typedef short bf16x4_t __attribute__((ext_vector_type(4)));
typedef float nat_f4c __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1))) *gcolptr;
typedef const nat_f4c __attribute__((address_space(1))) *gvecptr;

// centered values -> bf16, NaN -> 0
__device__ __forceinline__ bf16x4_t pack_bf16x4(float v0, float v1, float v2,
                                                float v3) {
  bf16x4_t pack;
  pack.x = to_bf16(isnan(v0) ? 0.f : v0);
  pack.y = to_bf16(isnan(v1) ? 0.f : v1);
  pack.z = to_bf16(isnan(v2) ? 0.f : v2);
  pack.w = to_bf16(isnan(v3) ? 0.f : v3);
  return pack;
}

// KT = 16-column tiles (ktot = KT*16 padded columns). 2 waves per SIMD
// (2 blocks per CU) is the register budget the prefetch is sized for.
template <int KT>
__global__ __launch_bounds__(THREADS, 2) void gram_singleread_kernel(
    const float *const *cols, int64_t n, int k, const float *means,
    const int *pair_i, const int *pair_j, int npairs, int row_chunks,
    float *partials) {
  constexpr int STAGES = 4;      // 128-row macro-slab
  constexpr int KTOT = KT * 16;  // padded column count
  constexpr int NIT = KTOT / 8;  // 16-byte loads per thread per round
  constexpr int PPW = (KT * (KT + 1) / 2 + 3) / 4;  // pairs per wave
  // Wide instances have no registers left for a whole round of
  // prefetch next to 23 accumulators: they load in batches of NB at
  // staging time instead.
  constexpr bool PREFETCH = KT <= 10;
  constexpr int NB = 8;
  // KSTRIDE pads each (stage, ko-group) plane by 3 column slots: the
  // un-padded plane stride (KTOT*16 B = 640 words for KT=10) is 0 mod
  // 32 banks, so the 16 planes' writes all landed in the same 4 banks
  // (16-way conflict — measured 2.1 TB/s for a 75 GB pass). +3 slots
  // shifts consecutive planes by 12 banks (worst case 2-way).
  constexpr int KSTRIDE = KTOT + 3;
  __shared__ __attribute__((aligned(16))) short slab[STAGES * 4 * KSTRIDE * 8];
  __shared__ float smean[KTOT];
  // wide instances keep the column pointers here, not in registers
  __shared__ gcolptr sptr[PREFETCH ? 1 : KTOT];

  const int block = blockIdx.x;
  const int64_t macro_total = (n + STAGES * 32 - 1) / (STAGES * 32);
  const int64_t macro_per = (macro_total + row_chunks - 1) / row_chunks;
  const int64_t mac_s = (int64_t)block * macro_per;
  const int64_t mac_e = min(macro_total, mac_s + macro_per);
  // macro-slabs below full_e lie entirely below n; at most one more
  // (the partial one) follows, in the last non-empty block
  const int64_t full_e = min(mac_e, n / (STAGES * 32));

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int m = lane & 15;    // tile row (A) / tile col (B)
  const int kog = lane >> 4;  // this lane's 8-row K group

  // ---- staging set-up: once per block ----
  const int cw = threadIdx.x >> 5;   // first column of this thread
  const int seg = threadIdx.x & 31;  // 4-row segment in the macro-slab
  const int sst = seg >> 3;          // stage (32-row step) 0..STAGES-1
  const int ssi = seg & 7;           // 4-row segment within the stage
  // slot of column cw; column cw + 8*it is 8*it*8 shorts further on
  short *const dst0 =
      slab + ((sst * 4 + (ssi >> 1)) * KSTRIDE + cw) * 8 + (ssi & 1) * 4;
  // Column cw + 8*it is real for every thread when it < k/8, and for
  // the threads with cw < k%8 when it == k/8; beyond that it is padding.
  // The first test is block-uniform (a scalar branch, no lane mask); the
  // one partly real step gets a pointer, a slot and a lane mask of its
  // own, so the unrolled steps need no per-lane predicate at all.
  int kfull = k >> 3;
  const bool part = cw < (k & 7);
  gcolptr xp[NIT];  // column base + this thread's segment
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = cw + 8 * it;
    // padding steps get a real column's pointer and never use it
    if (PREFETCH) xp[it] = (gcolptr)cols[min(c, k - 1)] + seg * 4;
    if (c >= k)
      *reinterpret_cast<bf16x4_t *>(dst0 + it * 64) = bf16x4_t{0, 0, 0, 0};
  }
  if (!PREFETCH)
    for (int c = threadIdx.x; c < KTOT; c += THREADS)
      sptr[c] = (gcolptr)cols[min(c, k - 1)];
  const int cpart = cw + 8 * kfull;  // < k exactly where `part` holds
  const gcolptr xpart = (gcolptr)cols[min(cpart, k - 1)] + seg * 4;
  short *const dpart = dst0 + kfull * 64;
  for (int c = threadIdx.x; c < KTOT; c += THREADS)
    smean[c] = (c < k) ? means[c] : 0.f;

  const int p0 = wave * PPW;  // contiguous pair chunk per wave
  int i0s[PPW], j0s[PPW];     // LDS column offsets of the pair's tiles
#pragma unroll
  for (int u = 0; u < PPW; ++u) {
    const int p = (p0 + u < npairs) ? p0 + u : 0;
    i0s[u] = __builtin_amdgcn_readfirstlane(pair_i[p] * 16);
    j0s[u] = __builtin_amdgcn_readfirstlane(pair_j[p] * 16);
  }
  f32x4 acc[PPW];
#pragma unroll
  for (int u = 0; u < PPW; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};

  nat_f4c pre[NIT], prepart;
  // issue the loads of steps [b0, b1) of the full macro-slab at row
  // offset `off`; the partly real step goes first with step 0
  auto issue = [&](int b0, int b1, int64_t off) {
    if (b0 == 0 && part)
      prepart = __builtin_nontemporal_load((gvecptr)(xpart + off));
#pragma unroll
    for (int it = b0; it < b1; ++it)
      if (it < kfull) {
        const gcolptr x = PREFETCH ? xp[it] : sptr[cw + 8 * it] + seg * 4;
        pre[it] = __builtin_nontemporal_load((gvecptr)(x + off));
      }
  };
  // center, pack and write them to this thread's LDS slots
  auto stage = [&](const nat_f4c t, float mean, short *dst) {
    *reinterpret_cast<bf16x4_t *>(dst) =
        pack_bf16x4(t.x - mean, t.y - mean, t.z - mean, t.w - mean);
  };
  auto convert = [&](int b0, int b1) {
    if (b0 == 0 && part) stage(prepart, smean[cpart], dpart);
    float mean = smean[cw + 8 * b0];
#pragma unroll
    for (int it = b0; it < b1; ++it)
      if (it < kfull) {
        // next step's mean is read ahead of this step's arithmetic
        const float mnext = smean[cw + 8 * (it + 1 < b1 ? it + 1 : it)];
        stage(pre[it], mean, dst0 + it * 64);
        mean = mnext;
      }
    // s_waitcnt vmcnt(0): every load issued so far has been consumed
    // above, so this costs nothing; stating it keeps the compiler from
    // guarding the next issue's destination registers with waits of its
    // own in between the loads.
    __builtin_amdgcn_s_waitcnt(0x0F70);
  };
  auto mfma_phase = [&]() {
#pragma unroll
    for (int st = 0; st < STAGES; ++st) {
      const short *sbase = slab + ((st * 4 + kog) * KSTRIDE + m) * 8;
#pragma unroll
      for (int u = 0; u < PPW; ++u) {
        const bf16x8 a = *reinterpret_cast<const bf16x8 *>(sbase + i0s[u] * 8);
        const bf16x8 b = *reinterpret_cast<const bf16x8 *>(sbase + j0s[u] * 8);
        acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[u], 0, 0, 0);
      }
    }
  };
  // ---- steady state: full macro-slabs ----
  if (PREFETCH && mac_s < full_e) issue(0, NIT, mac_s * (STAGES * 32));
  for (int64_t s = mac_s; s < full_e; ++s) {
    // opaque to the optimiser: keeps the per-step tests on kfull as
    // scalar compares in the loop instead of NIT hoisted conditions
    asm volatile("" : "+s"(kfull));
    __syncthreads();  // previous round's LDS reads complete (and smean set)
    if (PREFETCH) {
      convert(0, NIT);
    } else {
#pragma unroll
      for (int b = 0; b < NIT; b += NB) {
        issue(b, b + NB < NIT ? b + NB : NIT, s * (STAGES * 32));
        convert(b, b + NB < NIT ? b + NB : NIT);
      }
    }
    __syncthreads();
    if (PREFETCH && s + 1 < full_e) issue(0, NIT, (s + 1) * (STAGES * 32));
    mfma_phase();
  }

  // ---- tail: the one partial macro-slab, guarded per element ----
  if (mac_s < mac_e && full_e < mac_e) {
    const int64_t r = full_e * (STAGES * 32) + (int64_t)seg * 4;
    __syncthreads();
#pragma unroll 1
    for (int it = 0; it < NIT; ++it) {
      const int c = cw + 8 * it;
      if (c < k) {
        const gcolptr x = (gcolptr)cols[c] + r;
        const float mean = smean[c];
        float v0, v1, v2, v3;
        if (r + 4 <= n) {
          const nat_f4c t = __builtin_nontemporal_load((gvecptr)x);
          v0 = t.x - mean; v1 = t.y - mean; v2 = t.z - mean; v3 = t.w - mean;
        } else {
          v0 = (r + 0 < n) ? x[0] - mean : 0.f;
          v1 = (r + 1 < n) ? x[1] - mean : 0.f;
          v2 = (r + 2 < n) ? x[2] - mean : 0.f;
          v3 = (r + 3 < n) ? x[3] - mean : 0.f;
        }
        *reinterpret_cast<bf16x4_t *>(dst0 + it * 64) =
            pack_bf16x4(v0, v1, v2, v3);
      }
    }
    __syncthreads();
    mfma_phase();
  }

  // each pair is owned by exactly one wave: write fragments directly
  // (C layout: row = (lane>>4)*4 + reg, col = lane&15)
  const int row = (lane >> 4) * 4;
  // opaque, so the store predicates and addresses are formed here and
  // not held in registers across the round loop
  int np = npairs;
  asm volatile("" : "+s"(np));
#pragma unroll
  for (int u = 0; u < PPW; ++u) {
    const int p = p0 + u;
    if (p < np) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        partials[((int64_t)block * np + p) * 256 + (row + reg) * 16 + m] =
            acc[u][reg];
    }
  }
}

__global__ __launch_bounds__(THREADS) void gram_reduce_sr_kernel(
    const float *partials, int nblocks, int npairs, const int *pair_i,
    const int *pair_j, int k, float *gram) {
  const int pair = blockIdx.x;
  const int c = threadIdx.x;
  double s = 0.0;
  for (int ch = 0; ch < nblocks; ++ch)
    s += (double)partials[((int64_t)ch * npairs + pair) * 256 + c];
  const int row = c >> 4, col = c & 15;
  const int gi = pair_i[pair] * 16 + row;
  const int gj = pair_j[pair] * 16 + col;
  if (gi < k && gj < k) {
    gram[(int64_t)gi * k + gj] = (float)s;
    gram[(int64_t)gj * k + gi] = (float)s;
  }
}

using SrKernel = void (*)(const float *const *, int64_t, int, const float *,
                          const int *, const int *, int, int, float *);

// the instance for kt 16-column tiles; null past the single-read range
static SrKernel gram_sr_instance(int kt) {
  switch (kt) {
    case 1: return gram_singleread_kernel<1>;
    case 2: return gram_singleread_kernel<2>;
    case 3: return gram_singleread_kernel<3>;
    case 4: return gram_singleread_kernel<4>;
    case 5: return gram_singleread_kernel<5>;
    case 6: return gram_singleread_kernel<6>;
    case 7: return gram_singleread_kernel<7>;
    case 8: return gram_singleread_kernel<8>;
    case 9: return gram_singleread_kernel<9>;
    case 10: return gram_singleread_kernel<10>;
    case 11: return gram_singleread_kernel<11>;
    case 12: return gram_singleread_kernel<12>;
    case 13: return gram_singleread_kernel<13>;
    default: return nullptr;
  }
}

extern "C" int anovos_centered_gram_sr(const void *const *cols, int64_t n,
                                       int k, const float *means,
                                       const int *pair_i, const int *pair_j,
                                       int npairs, int row_chunks,
                                       float *partials, float *gram,
                                       hipStream_t stream) {
  const SrKernel fn = gram_sr_instance((k + 15) / 16);
  if (!fn) return -2;  // caller dispatches the pair-parallel kernel instead
  hipLaunchKernelGGL(fn, dim3(row_chunks), dim3(THREADS), 0, stream,
                     (const float *const *)cols, n, k, means, pair_i, pair_j,
                     npairs, row_chunks, partials);
  hipLaunchKernelGGL(gram_reduce_sr_kernel, dim3((uint32_t)npairs),
                     dim3(THREADS), 0, stream, partials, row_chunks, npairs,
                     pair_i, pair_j, k, gram);
  return (int)hipGetLastError();
}

extern "C" int anovos_gram_sr_grid(int k) {
  // Preferred grid = EXACTLY the resident block capacity (one wave of
  // blocks): every block starts at once and owns the longest possible
  // contiguous row range of each column (sweep at 20M x 150 with the
  // previous kernel: 256 blocks 0.95 TB/s, 768 = its capacity 2.20
  // TB/s, 2048 1.93, 16384 1.01).
  static int cached_k = -1, cached_grid = 0;
  if (k == cached_k) return cached_grid;
  const SrKernel fn = gram_sr_instance((k + 15) / 16);
  int per_cu = 0;
  if (fn)
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, reinterpret_cast<const void *>(fn), THREADS, 0);
  if (per_cu <= 0) per_cu = 2;
  hipDeviceProp_t prop;
  int dev = 0;
  hipGetDevice(&dev);
  hipGetDeviceProperties(&prop, dev);
  int grid = per_cu * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256);
  cached_k = k;
  cached_grid = grid;
  return grid;
}
