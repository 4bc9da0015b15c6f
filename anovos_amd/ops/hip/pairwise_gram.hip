// K25: pairwise-complete Gram sums on MFMA matrix cores.
//
// Per column let m = 1 where the value is present (not NaN), else 0, and
// z = x - mean on present rows, 0 on null rows. The kernel returns four
// k x k matrices, fp64 [4, k, k]:
//   N[i][j] = sum m_i m_j      rows where both are present   (symmetric)
//   P[i][j] = sum z_i z_j                                    (symmetric)
//   S[i][j] = sum z_i m_j      sum of i over the rows of j   (not symmetric)
//   Q[i][j] = sum z_i^2 m_j                                  (not symmetric)
// which hold everything a pairwise-complete Pearson r needs (ops/corr.py).
// All four are blocks of the Gram matrix of [Z | Z^2 | M], on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation as in K8 (corr_mfma.hip).
// Operands: zb = bf16(z) round-to-nearest-even, the square plane is
// bf16(zb * zb) - the square of the ROUNDED value, so that Q stays
// consistent with P's diagonal - and m is 0 / 1, exact in bf16.
//
// Layout. Columns are padded to 16-column tiles and tiles are taken in
// groups of PAIRGRAM_GROUP_TILES = 4 (64 columns). A work item is a pair
// of groups (gi <= gj); a block owns one item and one contiguous range of
// PAIRGRAM_SLAB_ROWS = 64-row macro-slabs (2 MFMA k-steps of 32 rows).
// Each round the block stages the macro-slab of both groups (of one, when
// gi == gj) through LDS as three bf16 planes formed in registers from the
// ONE read of x, then wave w multiplies tile w of group gi with every tile
// of group gj: its three A fragments are read once per k-step and serve
// up to four B tiles. An off-diagonal tile pair takes six products
// (ZZ, ZM, Z^2M, MM, MZ, MZ^2), a diagonal tile pair four (MZ and MZ^2
// would only repeat ZM and Z^2M transposed); inside a diagonal item the
// tile pairs below the diagonal are skipped.
// HBM read multiple: a column is read once per item its group is in,
// ceil(k / 64) times (3x at k = 150, against 11.7x for a kernel that
// re-reads per tile pair); blocks are ordered chunk-major, so the items
// that share a group read the same rows at about the same time.
//
// LDS: [2 groups][3 planes][2 k-steps][4 ko-groups][KSTRIDE cols][8 rows]
// bf16 - one 16-byte slot per (k-step, ko-group, col), so an MFMA fragment
// is one aligned ds_read_b128, as in K8. KSTRIDE = 64 + 3 slots: the
// unpadded plane stride (1024 B) is 0 mod 64 banks, +3 slots shifts
// consecutive ko-group planes by 12 banks. 51 456 B per block.
//
// Staging as in K8: thread t stages the 4-row segment (t & 15) of the
// columns (t >> 4) + 16 * it; column base pointers are resolved once per
// block as global-address-space pointers, means once into registers,
// padding columns' slots are zeroed once and never dereferenced. Full
// macro-slabs take an unguarded path of 16-byte nontemporal loads, issued
// two rounds ahead (a round is short, so one round of loads in flight
// leaves the kernel waiting on memory latency); the one partial
// macro-slab at the end of the column takes the guarded element path.
//
// Every block writes its fp32 tiles to `partials`; a second kernel sums
// the row chunks in ascending order in fp64 and writes both triangles
// (for S and Q the (J, I) tile is the transposed MZ / MZ^2 product, not a
// mirror). No floating-point atomics: the same call returns the same
// bits. Counts: a block's fp32 accumulator of M.M is exact while it sees
// fewer than 2^24 rows - the binding sizes row_chunks accordingly
// (PAIRGRAM_MAX_BLOCK_ROWS) - and the fp64 stage keeps N exact to 2^53.

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "anovos_kernels.h"

namespace {

constexpr int PG_THREADS = 256;
constexpr int PG_STAGES = PAIRGRAM_SLAB_ROWS / 32;
constexpr int PG_GT = PAIRGRAM_GROUP_TILES;
constexpr int PG_GCOLS = PG_GT * 16;
constexpr int PG_KSTRIDE = PG_GCOLS + 3;
constexpr int PG_NIT = 2 * PG_GCOLS / 16;  // 16-byte loads per thread per round
constexpr int PG_PLANE = PG_STAGES * 4 * PG_KSTRIDE * 8;  // shorts per (group, plane)

static_assert(PG_THREADS == 4 * 64 && PG_GT == 4, "one wave per A tile of the group");
static_assert(PAIRGRAM_SLAB_ROWS == 64, "16 four-row segments per column and round");
static_assert(PAIRGRAM_ITEM_FLOATS == PG_GT * PG_GT * 6 * 256, "partials layout");

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using bf16x4 = __attribute__((ext_vector_type(4))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef float nat_f4 __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1))) *gcolptr;
typedef const nat_f4 __attribute__((address_space(1))) *gvecptr;

// round-to-nearest-even into the upper 16 bits, as K8's to_bf16
__device__ __forceinline__ uint32_t bf16_bits(float v) {
  union {
    float f;
    uint32_t u;
  } c{v};
  return (c.u + 0x7FFFu + ((c.u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ float bf16_value(uint32_t bits) {
  union {
    uint32_t u;
    float f;
  } c{bits << 16};
  return c.f;
}

// one element -> its entries of the three planes
__device__ __forceinline__ void planes_of(float x, float mean, short &z, short &q, short &m) {
  const bool present = !isnan(x);
  const uint32_t zb = bf16_bits(present ? x - mean : 0.f);
  const float zr = bf16_value(zb);
  z = (short)zb;
  q = (short)bf16_bits(zr * zr);
  m = present ? (short)0x3F80 : (short)0;  // bf16 1.0
}

__device__ __forceinline__ void stage4(float v0, float v1, float v2, float v3, float mean,
                                       short *dst) {
  short z[4], q[4], m[4];
  planes_of(v0, mean, z[0], q[0], m[0]);
  planes_of(v1, mean, z[1], q[1], m[1]);
  planes_of(v2, mean, z[2], q[2], m[2]);
  planes_of(v3, mean, z[3], q[3], m[3]);
  *reinterpret_cast<bf16x4 *>(dst) = bf16x4{z[0], z[1], z[2], z[3]};
  *reinterpret_cast<bf16x4 *>(dst + PG_PLANE) = bf16x4{q[0], q[1], q[2], q[3]};
  *reinterpret_cast<bf16x4 *>(dst + 2 * PG_PLANE) = bf16x4{m[0], m[1], m[2], m[3]};
}

// The work of one block. DIAG (gi == gj) is a template parameter so that
// the number of loads per round is a compile-time constant on both paths.
template <bool DIAG>
__device__ __forceinline__ void pairwise_gram_block(
    short *slab, const float *const *cols, int64_t n, int k, const float *means, int gi, int gj,
    int item, int chunk, int nitems, int row_chunks, float *partials) {
  constexpr bool diag = DIAG;
  constexpr int NIT = DIAG ? PG_NIT / 2 : PG_NIT;  // a diagonal item stages one group

  const int64_t macro_total = (n + PAIRGRAM_SLAB_ROWS - 1) / PAIRGRAM_SLAB_ROWS;
  const int64_t macro_per = (macro_total + row_chunks - 1) / row_chunks;
  const int64_t mac_s = (int64_t)chunk * macro_per;
  const int64_t mac_e = min(macro_total, mac_s + macro_per);
  // macro-slabs below full_e lie entirely below n; at most one more (the
  // partial one) follows, in the last non-empty block
  const int64_t full_e = min(mac_e, n / PAIRGRAM_SLAB_ROWS);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = lane & 15;    // tile row (A) / tile col (B)
  const int kog = lane >> 4;  // this lane's 8-row K group

  // ---- staging set-up: once per block ----
  const int cw = threadIdx.x >> 4;   // first local column of this thread
  const int seg = threadIdx.x & 15;  // 4-row segment in the macro-slab
  // slot of local column cw in plane 0 of group 0; local column
  // cw + 16 * it lies (it & 3) * 16 columns and (it >> 2) groups further on
  short *const dst0 =
      slab + (((seg >> 3) * 4 + ((seg & 7) >> 1)) * PG_KSTRIDE + cw) * 8 + (seg & 1) * 4;
  gcolptr xp[NIT];
  float mu[NIT];
  unsigned real = 0;  // bit it: this thread's column of step it exists
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int g = it >> 2;
    const int c = (g ? gj : gi) * PG_GCOLS + (it & 3) * 16 + cw;
    short *const d = dst0 + g * 3 * PG_PLANE + (it & 3) * 16 * 8;
    // a padding step stands on a real column, loads it in the full rounds
    // and drops the value; its slots are zeroed here, once
    xp[it] = (gcolptr)cols[min(c, k - 1)] + seg * 4;
    mu[it] = means[min(c, k - 1)];
    if (c < k) real |= 1u << it;
    else {
      *reinterpret_cast<bf16x4 *>(d) = bf16x4{0, 0, 0, 0};
      *reinterpret_cast<bf16x4 *>(d + PG_PLANE) = bf16x4{0, 0, 0, 0};
      *reinterpret_cast<bf16x4 *>(d + 2 * PG_PLANE) = bf16x4{0, 0, 0, 0};
    }
  }

  // ---- MFMA set-up: wave w owns A tile w of group gi ----
  const bool a_live = (gi * PG_GT + wave) * 16 < k;
  unsigned jact = 0;  // bit j: B tile j of group gj is multiplied by this wave
#pragma unroll
  for (int j = 0; j < PG_GT; ++j)
    if (a_live && (gj * PG_GT + j) * 16 < k && !(diag && j < wave)) jact |= 1u << j;
  jact = __builtin_amdgcn_readfirstlane(jact);
  const short *const abase = slab + (kog * PG_KSTRIDE + wave * 16 + m) * 8;
  const short *const bbase = slab + (diag ? 0 : 3 * PG_PLANE) + (kog * PG_KSTRIDE + m) * 8;

  f32x4 acc[PG_GT][6];
#pragma unroll
  for (int j = 0; j < PG_GT; ++j)
#pragma unroll
    for (int p = 0; p < 6; ++p) acc[j][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Two rounds of loads are in flight: what a CU has outstanding, not the
  // MFMA phase, sets the pace. Every lane issues NIT loads per round,
  // padding steps included, and every issue in the loop is unconditional
  // (past the last full macro-slab it repeats that one), so the wait before
  // a conversion can leave the NIT younger loads outstanding.
  nat_f4 pre0[NIT], pre1[NIT];
  auto issue = [&](nat_f4(&pre)[NIT], int64_t slab_index) {
    const int64_t off = min(slab_index, full_e - 1) * PAIRGRAM_SLAB_ROWS;
#pragma unroll
    for (int it = 0; it < NIT; ++it) pre[it] = __builtin_nontemporal_load((gvecptr)(xp[it] + off));
  };
  auto convert = [&](const nat_f4(&pre)[NIT]) {
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      if ((real >> it) & 1u)
        stage4(pre[it].x, pre[it].y, pre[it].z, pre[it].w, mu[it],
               dst0 + (it >> 2) * 3 * PG_PLANE + (it & 3) * 16 * 8);
  };
  auto mfma_phase = [&]() {
#pragma unroll
    for (int st = 0; st < PG_STAGES; ++st) {
      const short *const ap = abase + st * 4 * PG_KSTRIDE * 8;
      const short *const bp = bbase + st * 4 * PG_KSTRIDE * 8;
      const bf16x8 az = *reinterpret_cast<const bf16x8 *>(ap);
      const bf16x8 aq = *reinterpret_cast<const bf16x8 *>(ap + PG_PLANE);
      const bf16x8 am = *reinterpret_cast<const bf16x8 *>(ap + 2 * PG_PLANE);
#pragma unroll
      for (int j = 0; j < PG_GT; ++j) {
        if ((jact >> j) & 1u) {
          const bf16x8 bz = *reinterpret_cast<const bf16x8 *>(bp + j * 16 * 8);
          const bf16x8 bq = *reinterpret_cast<const bf16x8 *>(bp + j * 16 * 8 + PG_PLANE);
          const bf16x8 bm = *reinterpret_cast<const bf16x8 *>(bp + j * 16 * 8 + 2 * PG_PLANE);
          acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az, bz, acc[j][0], 0, 0, 0);
          acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az, bm, acc[j][1], 0, 0, 0);
          acc[j][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq, bm, acc[j][2], 0, 0, 0);
          acc[j][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bm, acc[j][3], 0, 0, 0);
          if (!(diag && j == wave)) {
            acc[j][4] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bz, acc[j][4], 0, 0, 0);
            acc[j][5] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bq, acc[j][5], 0, 0, 0);
          }
        }
      }
    }
  };

  // ---- steady state: full macro-slabs, two per trip ----
  if (mac_s < full_e) {
    issue(pre0, mac_s);
    issue(pre1, mac_s + 1);
    int64_t s = mac_s;
    for (; s + 1 < full_e; s += 2) {
      __syncthreads();  // previous round's LDS reads complete
      convert(pre0);
      __syncthreads();
      issue(pre0, s + 2);
      mfma_phase();
      __syncthreads();
      convert(pre1);
      __syncthreads();
      issue(pre1, s + 3);
      mfma_phase();
    }
    if (s < full_e) {  // odd count: the last full macro-slab is in pre0
      __syncthreads();
      convert(pre0);
      __syncthreads();
      mfma_phase();
    }
  }

  // ---- tail: the one partial macro-slab, guarded per element ----
  if (mac_s < mac_e && full_e < mac_e) {
    const int64_t r = full_e * PAIRGRAM_SLAB_ROWS + (int64_t)seg * 4;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if ((real >> it) & 1u) {
        const gcolptr x = xp[it] + full_e * PAIRGRAM_SLAB_ROWS;
        // rows at and past n count as null
        const float nanv = __builtin_nanf("");
        const float v0 = (r + 0 < n) ? x[0] : nanv;
        const float v1 = (r + 1 < n) ? x[1] : nanv;
        const float v2 = (r + 2 < n) ? x[2] : nanv;
        const float v3 = (r + 3 < n) ? x[3] : nanv;
        stage4(v0, v1, v2, v3, mu[it], dst0 + (it >> 2) * 3 * PG_PLANE + (it & 3) * 16 * 8);
      }
    }
    __syncthreads();
    mfma_phase();
  }

  // each tile pair is owned by exactly one wave: write fragments directly
  // (C layout: row = (lane >> 4) * 4 + reg, col = lane & 15)
  float *const out = partials + ((int64_t)chunk * nitems + item) * PAIRGRAM_ITEM_FLOATS +
                     (int64_t)wave * PG_GT * 6 * 256 + (lane >> 4) * 4 * 16 + m;
#pragma unroll
  for (int j = 0; j < PG_GT; ++j) {
    if ((jact >> j) & 1u) {
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        if (p < 4 || !(diag && j == wave)) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) out[(j * 6 + p) * 256 + reg * 16] = acc[j][p][reg];
        }
      }
    }
  }
}

__global__ __launch_bounds__(PG_THREADS, 2) void pairwise_gram_kernel(
    const float *const *cols, int64_t n, int k, const float *means, const int *item_gi,
    const int *item_gj, int nitems, int row_chunks, float *partials) {
  __shared__ __attribute__((aligned(16))) short slab[2 * 3 * PG_PLANE];
  // chunk-major: neighbouring blocks read the same rows for different items
  const int item = blockIdx.x % nitems;
  const int chunk = blockIdx.x / nitems;
  const int gi = item_gi[item];
  const int gj = item_gj[item];
  if (gi == gj)
    pairwise_gram_block<true>(slab, cols, n, k, means, gi, gj, item, chunk, nitems, row_chunks,
                              partials);
  else
    pairwise_gram_block<false>(slab, cols, n, k, means, gi, gj, item, chunk, nitems, row_chunks,
                               partials);
}

// One block per (item, tile pair): chunk sums in ascending order, fp64.
__global__ __launch_bounds__(PG_THREADS) void pairwise_gram_reduce_kernel(
    const float *partials, int row_chunks, int nitems, const int *item_gi, const int *item_gj,
    int k, double *out) {
  const int item = blockIdx.x / (PG_GT * PG_GT);
  const int w = (blockIdx.x / PG_GT) % PG_GT;
  const int j = blockIdx.x % PG_GT;
  const int ti = item_gi[item] * PG_GT + w;
  const int tj = item_gj[item] * PG_GT + j;
  if (ti * 16 >= k || tj * 16 >= k || tj < ti) return;  // never computed
  const bool same = ti == tj;
  const int c = threadIdx.x;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int ch = 0; ch < row_chunks; ++ch) {
    const float *p = partials + ((int64_t)ch * nitems + item) * PAIRGRAM_ITEM_FLOATS +
                     (int64_t)(w * PG_GT + j) * 6 * 256 + c;
#pragma unroll
    for (int q = 0; q < 6; ++q)
      if (q < 4 || !same) s[q] += (double)p[q * 256];
  }
  const int row = c >> 4, col = c & 15;
  const int64_t i = (int64_t)ti * 16 + row;
  const int64_t jj = (int64_t)tj * 16 + col;
  if (i >= k || jj >= k) return;
  const int64_t kk = (int64_t)k * k;
  double *const N = out, *const P = out + kk, *const S = out + 2 * kk, *const Q = out + 3 * kk;
  const int64_t ij = i * k + jj, ji = jj * k + i;
  S[ij] = s[1];
  Q[ij] = s[2];
  if (!same) {
    P[ij] = s[0];
    P[ji] = s[0];
    N[ij] = s[3];
    N[ji] = s[3];
    S[ji] = s[4];
    Q[ji] = s[5];
  } else if (row <= col) {
    // one writer per symmetric entry pair of a diagonal tile
    P[ij] = s[0];
    P[ji] = s[0];
    N[ij] = s[3];
    N[ji] = s[3];
  }
}

}  // namespace

extern "C" int anovos_pairwise_gram(const void *const *cols, int64_t n, int k, const float *means,
                                    const int *item_gi, const int *item_gj, int nitems,
                                    int row_chunks, float *partials, double *out,
                                    hipStream_t stream) {
  hipLaunchKernelGGL(pairwise_gram_kernel, dim3((uint32_t)nitems * (uint32_t)row_chunks),
                     dim3(PG_THREADS), 0, stream, (const float *const *)cols, n, k, means,
                     item_gi, item_gj, nitems, row_chunks, partials);
  hipLaunchKernelGGL(pairwise_gram_reduce_kernel, dim3((uint32_t)nitems * PG_GT * PG_GT),
                     dim3(PG_THREADS), 0, stream, partials, row_chunks, nitems, item_gi, item_gj,
                     k, out);
  return (int)hipGetLastError();
}

extern "C" int anovos_pairwise_gram_grid() {
  // one wave of resident blocks, as anovos_gram_sr_grid
  static int cached_grid = 0;
  if (cached_grid) return cached_grid;
  int per_cu = 0;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, reinterpret_cast<const void *>(pairwise_gram_kernel), PG_THREADS, 0);
  if (per_cu <= 0) per_cu = 2;
  hipDeviceProp_t prop;
  prop.multiProcessorCount = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  (void)hipGetDeviceProperties(&prop, dev);
  cached_grid = per_cu * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256);
  return cached_grid;
}
