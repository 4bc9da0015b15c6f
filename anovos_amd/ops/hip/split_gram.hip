// K28: centred Gram matrix a model can be fitted on - split-bf16 MFMA
// products, bounded fp32 chains, fp64 sums.
//
// Per column j (f32, length n) with the fp64 mean split on the host into
// mh = f32(mean), ml = f32(mean - mh):
//   z  = isnan(x) ? 0 : (x - mh) - ml      f32; the first subtraction is exact
//                                          near the mean, so centring costs
//                                          2^-24 |z|, not 2^-25 |mean|
//   zh = bf16(z)  round-to-nearest-even,   zl = bf16(z - zh)  (z - zh is exact)
//   G[i][j] = sum_rows zh_i zh_j + zh_i zl_j + zl_i zh_j
// on v_mfma_f32_16x16x32_bf16; the zl zl term (2^-18 relative) is dropped,
// as in K26 and K27. Returned as fp64 [k, k], exactly symmetric.
//
// The sum over rows. An fp32 accumulator takes the products of at most
// SPLITGRAM_FLUSH_ROWS rows (flush_slabs macro-slabs); then the lane adds it
// into an fp64 accumulator it owns (its "shadow") and zeroes it. So the fp32
// rounding of an entry is that of a chain of 3 * SPLITGRAM_FLUSH_ROWS terms
// however long the column is, and everything beyond is fp64. Per entry, on
// sum |z_i| |z_j|:  3 * 2^-18 (zh + zl = z (1 + d), |d| <= 2^-18, on either
// side, and the dropped zl zl <= 2^-18)  +  (3 * SPLITGRAM_FLUSH_ROWS + 4) *
// 2^-24 (the fp32 chain, and two subtractions per centring).
//
// Layout: K25's (pairwise_gram.hip) with two planes instead of three.
// Columns pad to 16-column tiles, tiles go in groups of SPLITGRAM_GROUP_TILES
// = 4 (64 columns). A work item is a pair of groups (gi <= gj); a 256-thread
// block owns one item and one contiguous range of SPLITGRAM_SLAB_ROWS =
// 64-row macro-slabs (2 MFMA k-steps). Blocks are ordered chunk-major, so
// the items that share a group read the same rows at about the same time;
// the grid is one wave of resident blocks.
// HBM read multiple: a column is read once per item its group is in,
// ceil(k / 64) times (3x at k = 150).
//
// LDS: [2 groups][2 planes: Zh, Zl][2 k-steps][4 ko-groups][KSTRIDE cols]
// [8 rows] bf16 - one 16-byte slot per (k-step, ko-group, col), so an MFMA
// fragment is one aligned ds_read_b128. KSTRIDE = 64 + 3 slots (K8 / K25's
// plane padding: the unpadded 1024 B stride is 0 mod 64 banks). 34 304 B.
//
// Staging: thread t stages the 4-row segment (t & 15) of the columns
// (t >> 4) + 16 * it. Both planes are formed in registers from the ONE read
// of x (two hardware pair conversions per plane). Column pointers are
// resolved once per block as global-address-space pointers, mh / ml once
// into registers; padding columns' slots are zeroed once and never
// dereferenced. Full macro-slabs take unguarded 16-byte nontemporal loads
// issued two rounds ahead, every issue unconditional; the one partial
// macro-slab at the end of the column takes the guarded element path.
//
// Products: wave w multiplies tile w of gi with every tile of gj. Its two A
// fragments are read once per k-step; a tile pair takes three products into
// ONE fp32 accumulator: four live f32x4 and their sixteen fp64 shadows per
// lane. Inside a diagonal item tile pairs below the diagonal are skipped.
//
// Every block writes its fp64 tiles to `partials`; a second kernel sums the
// row chunks in ascending order in fp64, writes the upper triangle and
// mirrors it. No floating-point atomics: the same call returns the same bits.
//
// Resources (hipcc -O3, gfx950, 256 threads): see docs/KERNELS.md, K28; no
// scratch in either instantiation.

#include <hip/hip_runtime.h>
#include <cstdint>

#include "anovos_kernels.h"

// Compiled without the packed fp32 instructions, for the reason given in
// project_columns.hip; the staging below is subtractions of neighbouring
// rows, exactly what the vectorizer pairs. The attribute has to be on every
// device function of the file, lambdas included, and the barrier is the
// builtin (the runtime header's carries the default target).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_STAGES = SPLITGRAM_SLAB_ROWS / 32;
constexpr int SG_GT = SPLITGRAM_GROUP_TILES;
constexpr int SG_GCOLS = SG_GT * 16;
constexpr int SG_KSTRIDE = SG_GCOLS + 3;
constexpr int SG_NIT = 2 * SG_GCOLS / 16;  // 16-byte loads per thread per round
constexpr int SG_PLANE = SG_STAGES * 4 * SG_KSTRIDE * 8;  // shorts per (group, plane)

static_assert(SG_THREADS == 4 * 64 && SG_GT == 4, "one wave per A tile of the group");
static_assert(SPLITGRAM_SLAB_ROWS == 64, "16 four-row segments per column and round");
static_assert(SPLITGRAM_FLUSH_ROWS % SPLITGRAM_SLAB_ROWS == 0 && SPLITGRAM_FLUSH_ROWS > 0,
              "a flush falls between macro-slabs");
static_assert(SPLITGRAM_ITEM_DOUBLES == SG_GT * SG_GT * 256, "partials layout");

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef float nat_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t nat_u2 __attribute__((ext_vector_type(2)));
typedef const float __attribute__((address_space(1))) *gcolptr;
typedef const nat_f4 __attribute__((address_space(1))) *gvecptr;

__device__ __forceinline__ float bf16_value(uint32_t bits) {
  union {
    uint32_t u;
    float f;
  } c{bits << 16};
  return c.f;
}

// two f32 -> two bf16 (a in the low half), round-to-nearest-even by the
// hardware's packed conversion, as K26
typedef __bf16 hw_bf16x2 __attribute__((ext_vector_type(2)));
typedef float nat_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
  const hw_bf16x2 r = __builtin_convertvector(nat_f2{a, b}, hw_bf16x2);
  uint32_t u;
  __builtin_memcpy(&u, &r, 4);
  return u;
}

// __syncthreads()
__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

__device__ __forceinline__ float centred(float x, float mh, float ml) {
  return x != x ? 0.f : (x - mh) - ml;
}

// four rows of one column -> their 8-byte entries of the Zh and Zl planes
__device__ __forceinline__ void stage4(float v0, float v1, float v2, float v3, float mh, float ml,
                                       short *dst) {
  const float z0 = centred(v0, mh, ml), z1 = centred(v1, mh, ml);
  const float z2 = centred(v2, mh, ml), z3 = centred(v3, mh, ml);
  const uint32_t h01 = pack_bf16(z0, z1), h23 = pack_bf16(z2, z3);
  const uint32_t l01 = pack_bf16(z0 - bf16_value(h01 & 0xFFFFu), z1 - bf16_value(h01 >> 16));
  const uint32_t l23 = pack_bf16(z2 - bf16_value(h23 & 0xFFFFu), z3 - bf16_value(h23 >> 16));
  *reinterpret_cast<nat_u2 *>(dst) = nat_u2{h01, h23};
  *reinterpret_cast<nat_u2 *>(dst + SG_PLANE) = nat_u2{l01, l23};
}

// The work of one block. DIAG (gi == gj) is a template parameter so that
// the number of loads per round is a compile-time constant on both paths.
template <bool DIAG>
__device__ __forceinline__ void split_gram_block(
    short *slab, const float *const *cols, int64_t n, int k, const float *mean_hi,
    const float *mean_lo, int gi, int gj, int item, int chunk, int nitems, int row_chunks,
    int flush_slabs, double *partials) {
  constexpr bool diag = DIAG;
  constexpr int NIT = DIAG ? SG_NIT / 2 : SG_NIT;  // a diagonal item stages one group

  const int64_t macro_total = (n + SPLITGRAM_SLAB_ROWS - 1) / SPLITGRAM_SLAB_ROWS;
  const int64_t macro_per = (macro_total + row_chunks - 1) / row_chunks;
  const int64_t mac_s = (int64_t)chunk * macro_per;
  const int64_t mac_e = min64(macro_total, mac_s + macro_per);
  // macro-slabs below full_e lie entirely below n; at most one more (the
  // partial one) follows, in the last non-empty block
  const int64_t full_e = min64(mac_e, n / SPLITGRAM_SLAB_ROWS);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = lane & 15;    // tile row (A) / tile col (B)
  const int kog = lane >> 4;  // this lane's 8-row K group

  // ---- staging set-up: once per block ----
  const int cw = threadIdx.x >> 4;   // first local column of this thread
  const int seg = threadIdx.x & 15;  // 4-row segment in the macro-slab
  // slot of local column cw in the Zh plane of group 0; local column
  // cw + 16 * it lies (it & 3) * 16 columns and (it >> 2) groups further on
  short *const dst0 =
      slab + (((seg >> 3) * 4 + ((seg & 7) >> 1)) * SG_KSTRIDE + cw) * 8 + (seg & 1) * 4;
  gcolptr xp[NIT];
  float mh[NIT], ml[NIT];
  unsigned real = 0;  // bit it: this thread's column of step it exists
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int g = it >> 2;
    const int c = (g ? gj : gi) * SG_GCOLS + (it & 3) * 16 + cw;
    const int cc = c < k ? c : k - 1;
    short *const d = dst0 + g * 2 * SG_PLANE + (it & 3) * 16 * 8;
    // a padding step stands on a real column, loads it in the full rounds
    // and drops the value; its slots are zeroed here, once
    xp[it] = (gcolptr)cols[cc] + seg * 4;
    mh[it] = mean_hi[cc];
    ml[it] = mean_lo[cc];
    if (c < k) real |= 1u << it;
    else {
      *reinterpret_cast<nat_u2 *>(d) = nat_u2{0u, 0u};
      *reinterpret_cast<nat_u2 *>(d + SG_PLANE) = nat_u2{0u, 0u};
    }
  }

  // ---- MFMA set-up: wave w owns A tile w of group gi ----
  const bool a_live = (gi * SG_GT + wave) * 16 < k;
  unsigned jact = 0;  // bit j: B tile j of group gj is multiplied by this wave
#pragma unroll
  for (int j = 0; j < SG_GT; ++j)
    if (a_live && (gj * SG_GT + j) * 16 < k && !(diag && j < wave)) jact |= 1u << j;
  jact = __builtin_amdgcn_readfirstlane(jact);
  const short *const abase = slab + (kog * SG_KSTRIDE + wave * 16 + m) * 8;
  const short *const bbase = slab + (diag ? 0 : 2 * SG_PLANE) + (kog * SG_KSTRIDE + m) * 8;

  f32x4 acc[SG_GT];       // at most flush_slabs macro-slabs of products
  double sum[SG_GT][4];   // their fp64 shadows
#pragma unroll
  for (int j = 0; j < SG_GT; ++j) {
    acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[j][r] = 0.0;
  }
  int pending = 0;  // macro-slabs in acc since the last flush

  // Two rounds of loads are in flight, as in K25: every lane issues NIT
  // loads per round, padding steps included, and every issue in the loop is
  // unconditional (past the last full macro-slab it repeats that one), so
  // the wait before a conversion can leave the NIT younger loads outstanding.
  nat_f4 pre0[NIT], pre1[NIT];
  auto issue = [&](nat_f4(&pre)[NIT], int64_t slab_index) {
    const int64_t off = min64(slab_index, full_e - 1) * SPLITGRAM_SLAB_ROWS;
#pragma unroll
    for (int it = 0; it < NIT; ++it) pre[it] = __builtin_nontemporal_load((gvecptr)(xp[it] + off));
  };
  auto convert = [&](const nat_f4(&pre)[NIT]) {
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      if ((real >> it) & 1u)
        stage4(pre[it].x, pre[it].y, pre[it].z, pre[it].w, mh[it], ml[it],
               dst0 + (it >> 2) * 2 * SG_PLANE + (it & 3) * 16 * 8);
  };
  auto flush = [&]() {
#pragma unroll
    for (int j = 0; j < SG_GT; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[j][r] += (double)acc[j][r];
      acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    pending = 0;
  };
  // the products of the macro-slab in LDS, then the flush rule
  auto mfma_phase = [&]() {
#pragma unroll
    for (int st = 0; st < SG_STAGES; ++st) {
      const short *const ap = abase + st * 4 * SG_KSTRIDE * 8;
      const short *const bp = bbase + st * 4 * SG_KSTRIDE * 8;
      const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(ap);
      const bf16x8 al = *reinterpret_cast<const bf16x8 *>(ap + SG_PLANE);
#pragma unroll
      for (int j = 0; j < SG_GT; ++j) {
        if ((jact >> j) & 1u) {
          const bf16x8 bh = *reinterpret_cast<const bf16x8 *>(bp + j * 16 * 8);
          const bf16x8 bl = *reinterpret_cast<const bf16x8 *>(bp + j * 16 * 8 + SG_PLANE);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc[j], 0, 0, 0);
        }
      }
    }
    if (++pending >= flush_slabs) flush();
  };

  // ---- steady state: full macro-slabs, two per trip ----
  if (mac_s < full_e) {
    issue(pre0, mac_s);
    issue(pre1, mac_s + 1);
    int64_t s = mac_s;
    for (; s + 1 < full_e; s += 2) {
      block_barrier();  // previous round's LDS reads complete
      convert(pre0);
      block_barrier();
      issue(pre0, s + 2);
      mfma_phase();
      block_barrier();
      convert(pre1);
      block_barrier();
      issue(pre1, s + 3);
      mfma_phase();
    }
    if (s < full_e) {  // odd count: the last full macro-slab is in pre0
      block_barrier();
      convert(pre0);
      block_barrier();
      mfma_phase();
    }
  }

  // ---- tail: the one partial macro-slab, guarded per element ----
  if (mac_s < mac_e && full_e < mac_e) {
    const int64_t r = full_e * SPLITGRAM_SLAB_ROWS + (int64_t)seg * 4;
    block_barrier();
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if ((real >> it) & 1u) {
        const gcolptr x = xp[it] + full_e * SPLITGRAM_SLAB_ROWS;
        // rows at and past n count as null
        const float nanv = __builtin_nanf("");
        const float v0 = (r + 0 < n) ? x[0] : nanv;
        const float v1 = (r + 1 < n) ? x[1] : nanv;
        const float v2 = (r + 2 < n) ? x[2] : nanv;
        const float v3 = (r + 3 < n) ? x[3] : nanv;
        stage4(v0, v1, v2, v3, mh[it], ml[it],
               dst0 + (it >> 2) * 2 * SG_PLANE + (it & 3) * 16 * 8);
      }
    }
    block_barrier();
    mfma_phase();
  }
  flush();

  // each tile pair is owned by exactly one wave: write fragments directly
  // (C layout: row = (lane >> 4) * 4 + reg, col = lane & 15); a block that
  // owns no macro-slab writes zeros
  double *const out = partials + ((int64_t)chunk * nitems + item) * SPLITGRAM_ITEM_DOUBLES +
                      (int64_t)wave * SG_GT * 256 + (lane >> 4) * 4 * 16 + m;
#pragma unroll
  for (int j = 0; j < SG_GT; ++j) {
    if ((jact >> j) & 1u) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) out[j * 256 + reg * 16] = sum[j][reg];
    }
  }
}

__global__ __launch_bounds__(SG_THREADS, 2) void split_gram_kernel(
    const float *const *cols, int64_t n, int k, const float *mean_hi, const float *mean_lo,
    const int *item_gi, const int *item_gj, int nitems, int row_chunks, int flush_slabs,
    double *partials) {
  __shared__ __attribute__((aligned(16))) short slab[2 * 2 * SG_PLANE];
  // chunk-major: neighbouring blocks read the same rows for different items
  const int item = blockIdx.x % nitems;
  const int chunk = blockIdx.x / nitems;
  const int gi = item_gi[item];
  const int gj = item_gj[item];
  if (gi == gj)
    split_gram_block<true>(slab, cols, n, k, mean_hi, mean_lo, gi, gj, item, chunk, nitems,
                           row_chunks, flush_slabs, partials);
  else
    split_gram_block<false>(slab, cols, n, k, mean_hi, mean_lo, gi, gj, item, chunk, nitems,
                            row_chunks, flush_slabs, partials);
}

// One block per (item, tile pair): chunk sums in ascending order, fp64;
// the upper triangle and its mirror.
__global__ __launch_bounds__(SG_THREADS) void split_gram_reduce_kernel(
    const double *partials, int row_chunks, int nitems, const int *item_gi, const int *item_gj,
    int k, double *out) {
  const int item = blockIdx.x / (SG_GT * SG_GT);
  const int w = (blockIdx.x / SG_GT) % SG_GT;
  const int j = blockIdx.x % SG_GT;
  const int ti = item_gi[item] * SG_GT + w;
  const int tj = item_gj[item] * SG_GT + j;
  if (ti * 16 >= k || tj * 16 >= k || tj < ti) return;  // never computed
  const int c = threadIdx.x;
  double s = 0.0;
  for (int ch = 0; ch < row_chunks; ++ch)
    s += partials[((int64_t)ch * nitems + item) * SPLITGRAM_ITEM_DOUBLES +
                  (int64_t)(w * SG_GT + j) * 256 + c];
  const int row = c >> 4, col = c & 15;
  const int64_t i = (int64_t)ti * 16 + row;
  const int64_t jj = (int64_t)tj * 16 + col;
  if (i >= k || jj >= k) return;
  // one writer per symmetric entry pair: inside a diagonal tile the lower
  // triangle's own (differently rounded) sums are dropped
  if (ti == tj && row > col) return;
  out[i * k + jj] = s;
  out[jj * k + i] = s;
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" int anovos_split_gram(const void *const *cols, int64_t n, int k, const float *mean_hi,
                                 const float *mean_lo, const int *item_gi, const int *item_gj,
                                 int nitems, int row_chunks, int flush_slabs, double *partials,
                                 double *out, hipStream_t stream) {
  if (n < 1 || k < 1 || nitems < 1 || row_chunks < 1 || flush_slabs < 1)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(split_gram_kernel, dim3((uint32_t)nitems * (uint32_t)row_chunks),
                     dim3(SG_THREADS), 0, stream, (const float *const *)cols, n, k, mean_hi,
                     mean_lo, item_gi, item_gj, nitems, row_chunks, flush_slabs, partials);
  hipLaunchKernelGGL(split_gram_reduce_kernel, dim3((uint32_t)nitems * SG_GT * SG_GT),
                     dim3(SG_THREADS), 0, stream, partials, row_chunks, nitems, item_gi, item_gj,
                     k, out);
  return (int)hipGetLastError();
}

extern "C" int anovos_split_gram_grid() {
  // one wave of resident blocks, as anovos_pairwise_gram_grid
  static int cached_grid = 0;
  if (cached_grid) return cached_grid;
  int per_cu = 0;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, reinterpret_cast<const void *>(split_gram_kernel), SG_THREADS, 0);
  if (per_cu <= 0) per_cu = 2;
  hipDeviceProp_t prop;
  prop.multiProcessorCount = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  (void)hipGetDeviceProperties(&prop, dev);
  cached_grid = per_cu * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256);
  return cached_grid;
}
