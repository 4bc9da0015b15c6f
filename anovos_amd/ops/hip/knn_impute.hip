// K29: the apply step of KNN imputation - nan-euclidean distances of every
// task row to all fitted donor rows on MFMA matrix cores, with the k nearest
// donors selected in registers and re-ranked exactly (ops/knn.py).
//
// One call serves the tasks of ONE target column j: the rows whose x_j is
// null. With m columns, donors F [s, m] (f32, NaN = null), masks
// mx = !isnan(x), mf = !isnan(F) and a per-column centre c (fp64, split on
// the host into mh = f32(c), ml = f32(c - mh); any centre gives the same
// distances, the donor mean removes the |mean|^2 cancellation):
//   z   = isnan(v) ? 0 : (v - mh) - ml                  rows and donors alike
//   ov  = sum_c mx_c mf_c
//   sq  = sum_c mx_c mf_c (zx_c - zf_c)^2
//   d2  = (float(m) * sq) / ov      ov > 0, IEEE multiply, correctly rounded divide
// The donors of a task have column j present and ov > 0; its neighbours are
// the k smallest under the total order (d2, donor index); est is the f32 sum
// of their column-j values in that order over their count. Fewer than k
// donors: the rest is reported as idx -1, d2 +inf; none: est NaN.
//
// Filter pass (MFMA). sq = sum mf zx^2 + mx zf^2 - 2 zx zf is a Gram of the
// planes [Z | Z^2 | M] (K25's trick) with split-bf16 operands (K26 - K28):
// v = vh + vl, vh = bf16(v) round-to-nearest-even, vl = bf16(v - vh). Per
// k-step of 32 columns seven v_mfma_f32_16x16x32_bf16 add into ONE fp32
// accumulator, which is sq itself,
//   (-2fh) xh + (-2fh) xl + (-2fl) xh + mf (x^2)h + mf (x^2)l + (f^2)h mx + (f^2)l mx
// and an eighth, mf mx, into a second one, ov (a count: exact). The fl xl
// term is dropped. A = donor tile (16 donors x 32 columns), B = row tile
// (32 columns x 16 rows), so a lane's accumulator holds the donors
// (lane >> 4) * 4 + reg of the tile for the row (lane & 15).
//
// Error of the filter pass, per task and donor, on S = sum_overlap
// (|zx| + |zf|)^2 = sum x^2 + f^2 + 2 |x| |f|:
//   - 2 f x: fh + fl = f (1 + d), |d| <= 2^-18, likewise x, and the dropped
//     fl xl <= 2^-18 |f| |x|:                           3 * 2^-18 * 2 |f| |x|
//   - x^2 and f^2 are formed in f32 (2^-24) and split (2^-18):
//                                              (2^-18 + 2^-24) (x^2 + f^2)
//   - the fp32 sum: the 7 * m_pad products (each exact in fp32: 8 x 8
//     significant bits) reach the accumulator through 7 * m_pad / 32 MFMAs;
//     whatever the order inside one, a sum of N terms is off by at most
//     (N - 1) * 2^-24 * sum |terms| to first order, and sum |terms| <= S
//   |sq_filter - sq| <= gamma * S,  gamma = 3 * 2^-18 + (7 * m_pad + 1) * 2^-24
// (ops/knn.py KNN_FILTER_GAMMA repeats the figure). The filter only has to
// put the true neighbours among its k + 8 nearest (KNN_CAND in
// anovos_kernels.h): that holds wherever the gap between the k-th and the
// (k + 8)-th true distance exceeds 2 gamma S.
//
// Donor image: built once per call by knn_donor_image_kernel, in A-fragment
// order - [tile][plane][k-step][lane][8 columns] bf16, planes -2 zh, -2 zl,
// (z^2)h, (z^2)l, mf (the -2 is a power of two: exact) - so a fragment is one
// 16-byte load. Donors pad to 16 and to whole ring stages, columns to 32.
// Validity is folded into the planes: a padding donor and a donor without
// column j get all five planes zero, so their ov is 0 and the one test
// "ov > 0" that no-overlap donors need anyway rejects them too - no validity
// vector is read in the loop. The re-rank and est read the donors' f32
// values themselves.
//
// Work split. A 256-thread block owns 64-row slabs of `rows`, wave w the
// row tile w. A lane gathers its 8 * KS values of its row through `rows`
// and the column table and forms the five B planes zh, zl, (z^2)h, (z^2)l,
// mx in registers (20 * KS VGPRs, held for the slab's lifetime); then ALL
// donor tiles stream past. They come from L2 through a two-buffer LDS ring
// shared by the four waves, KNN_STAGE_TILES tiles per stage: the 16-byte
// loads of stage t + 1 are issued before the MFMAs of stage t, land in the
// other buffer after them, one barrier per stage. Every issue is
// unconditional (past the last stage it repeats it; a thread without a
// chunk of its own in the last round repeats the stage's last chunk - both
// store what is there already). Blocks are persistent over one wave of
// resident blocks, each with one contiguous range of slabs.
//
// Selection. A lane keeps KNN_CAND (filter d2, donor) pairs sorted ascending
// in registers. Donor indices only grow along the stream, so a newcomer
// goes behind its equals and the order is (d2, index) with one compare per
// entry. Per tile and register a conservative pre-test without a divide,
//   float(m) * sq <= worst * ov * (1 + 2^-22)
// and ov > 0 (worst = the list's last d2, +inf while it is not full; without
// the second test every padding or target-less donor would pass as 0 <= 0
// once the list is full), decides whether the value can enter;
// only if some lane of the wave passes (a wave-uniform branch) is the divide
// done and the branch-free insertion chain run, once per register that some
// lane needs. The pre-test is sound because rounding is monotone:
// RN(t / ov) < worst implies t < worst * ov, and the factor covers the two
// roundings of the right-hand side.
//
// Exact re-rank - what makes the GEMM form safe. After the last tile every
// lane recomputes sq of its KNN_CAND candidates in the direct form
// sum mx mf (((x - mh) - ml) - zf)^2 in f32 from the gathered row and the
// donors' f32 values, and their d2 as above. Then k rounds pick the
// smallest (d2, index) of the row: each lane its own, the four lanes of a
// row through two ds_bpermute exchanges in a fixed order, and the winner is
// struck from its owner's list. No atomics: the same call returns the same
// bits.
//
// Resources (hipcc -O3, gfx950, 256 threads): see docs/KERNELS.md, K29; no
// scratch in any instantiation.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "anovos_kernels.h"

// Compiled without the packed fp32 instructions, for the reason given in
// project_columns.hip. The attribute has to be on every device function of
// the file, lambdas included; barrier, ballot and lane permute are builtins
// (the runtime header's functions carry the default target).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int KN_THREADS = 256;
constexpr int KN_NOIDX = 0x7FFFFFFF;  // sorts behind every donor

static_assert(KNN_SLAB_ROWS == 64 && KN_THREADS == 4 * 64, "one wave per 16-row tile");
static_assert(KNN_CAND >= KNN_MAX_K + 8, "see anovos_kernels.h");
static_assert(KNN_MAX_COLS == 4 * 32, "KS = 1 .. 4");

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef uint32_t nat_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf16_value(uint32_t bits) {
  union {
    uint32_t u;
    float f;
  } c{bits << 16};
  return c.f;
}

// round-to-nearest-even into the upper 16 bits, as K25's bf16_bits
__device__ __forceinline__ uint32_t bf16_bits(float v) {
  union {
    float f;
    uint32_t u;
  } c{v};
  return (c.u + 0x7FFFu + ((c.u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ void split_bf16(float v, uint32_t &hi, uint32_t &lo) {
  hi = bf16_bits(v);
  lo = bf16_bits(v - bf16_value(hi));
}

__device__ __forceinline__ float inf_f() { return __builtin_inff(); }

__device__ __forceinline__ int as_int(float v) { return __builtin_bit_cast(int, v); }
__device__ __forceinline__ float as_float(int v) { return __builtin_bit_cast(float, v); }

// __syncthreads()
__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

// (a, ai) before (b, bi) in the order (d2, index)
__device__ __forceinline__ bool before(float a, int ai, float b, int bi) {
  return a < b || (a == b && ai < bi);
}

// eight columns of one row or donor -> the 16 bytes of one plane
__device__ __forceinline__ bf16x8 pack8(const uint32_t (&b)[8]) {
  nat_u4 v;
  v.x = b[0] | (b[1] << 16);
  v.y = b[2] | (b[3] << 16);
  v.z = b[4] | (b[5] << 16);
  v.w = b[6] | (b[7] << 16);
  return __builtin_bit_cast(bf16x8, v);
}

// The five planes of eight columns: z scaled by `zscale` (1 for rows, -2
// for donors) hi and lo, z^2 hi and lo, and the mask.
__device__ __forceinline__ void planes8(const float (&v)[8], const float *mh, const float *ml,
                                        float zscale, bf16x8 (&out)[5]) {
  uint32_t p[5][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const bool have = v[e] == v[e];
    const float z = have ? (v[e] - mh[e]) - ml[e] : 0.f;
    split_bf16(z * zscale, p[0][e], p[1][e]);  // a power of two: the split of z, scaled
    split_bf16(z * z, p[2][e], p[3][e]);
    p[4][e] = have ? 0x3F80u : 0u;  // bf16 1.0
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) out[q] = pack8(p[q]);
}

// One thread per (tile, k-step, lane) of the image: donor tile * 16 +
// (lane & 15), columns ks * 32 + (lane >> 4) * 8 + e. mh / ml hold m_pad
// entries. A donor past s or without column `target` is all zero.
__global__ __launch_bounds__(KN_THREADS) void knn_donor_image_kernel(
    const float *donors, int s, int m, int target, const float *mh, const float *ml, int ks_count,
    int tiles, uint16_t *img) {
  const int t = blockIdx.x * KN_THREADS + threadIdx.x;
  if (t >= tiles * ks_count * 64) return;
  const int lane = t & 63;
  const int ks = (t >> 6) % ks_count;
  const int tile = (t >> 6) / ks_count;
  const int d = tile * 16 + (lane & 15);
  const int c0 = ks * 32 + (lane >> 4) * 8;
  const float nanv = __builtin_nanf("");
  bool valid = d < s;
  if (valid) {
    const float tv = donors[(int64_t)d * m + target];
    valid = tv == tv;
  }
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (valid && c0 + e < m) ? donors[(int64_t)d * m + c0 + e] : nanv;
  bf16x8 out[5];
  planes8(v, mh + c0, ml + c0, -2.f, out);
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int64_t slot = (((int64_t)tile * 5 + q) * ks_count + ks) * 64 + lane;
    *reinterpret_cast<bf16x8 *>(img + slot * 8) = out[q];
  }
}

template <int KS>
__global__ __launch_bounds__(KN_THREADS, KS <= 2 ? 2 : 1) void knn_impute_kernel(
    const float *const *cols, int64_t n, int m, const int64_t *rows, int64_t r, const float *mh,
    const float *ml, const float *donors, int target, int k, const uint16_t *img, int nstages,
    float *est, int *idx, float *d2out, int *cand_idx, float *cand_d2) {
  extern __shared__ __attribute__((aligned(16))) short kn_lds[];
  constexpr int TILE = 5 * KS * 512;             // shorts per donor tile
  constexpr int STAGE = KNN_STAGE_TILES * TILE;  // shorts per ring stage
  constexpr int NCH = STAGE / 8;                 // 16-byte chunks per stage
  constexpr int NLD = (NCH + KN_THREADS - 1) / KN_THREADS;

  const int64_t slabs = (r + KNN_SLAB_ROWS - 1) / KNN_SLAB_ROWS;
  const int64_t per = (slabs + gridDim.x - 1) / gridDim.x;
  const int64_t slab_s = (int64_t)blockIdx.x * per;
  const int64_t slab_e = slab_s + per < slabs ? slab_s + per : slabs;
  if (slab_s >= slab_e) return;  // whole block, before any barrier

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row16 = lane & 15;  // row of the tile (B, C columns)
  const int grp = lane >> 4;    // column octet of a k-step (A, B) / donor quad (C)
  const float fm = (float)m;
  const float inf = inf_f();

  // ring: the chunks this thread moves per stage
  int chunk[NLD];
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int c = (int)threadIdx.x + i * KN_THREADS;
    chunk[i] = (c < NCH ? c : NCH - 1) * 8;
  }
  nat_u4 pre[NLD];
  auto issue = [&](int stage) {
    const uint16_t *const src = img + (int64_t)(stage < nstages ? stage : nstages - 1) * STAGE;
#pragma unroll
    for (int i = 0; i < NLD; ++i) pre[i] = *reinterpret_cast<const nat_u4 *>(src + chunk[i]);
  };
  auto land = [&](int buf) {
    short *const dst = kn_lds + buf * STAGE;
#pragma unroll
    for (int i = 0; i < NLD; ++i) *reinterpret_cast<nat_u4 *>(dst + chunk[i]) = pre[i];
  };

  for (int64_t slab = slab_s; slab < slab_e; ++slab) {
    // ---- this lane's row and its B fragments ----
    const int64_t q = slab * KNN_SLAB_ROWS + wave * 16 + row16;
    const int64_t ridx = rows[q < r ? q : r - 1];
    const bool live = q < r && (uint64_t)ridx < (uint64_t)n;  // else: a row of nulls
    bf16x8 xh[KS], xl[KS], x2h[KS], x2l[KS], xm[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int c0 = ks * 32 + grp * 8;
      float v[8], h[8], l[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = c0 + e < m ? c0 + e : m - 1;
        const float got = live ? cols[c][ridx] : 0.f;
        v[e] = (live && c0 + e < m) ? got : __builtin_nanf("");
        h[e] = mh[c];
        l[e] = ml[c];
      }
      bf16x8 out[5];
      planes8(v, h, l, 1.f, out);
      xh[ks] = out[0];
      xl[ks] = out[1];
      x2h[ks] = out[2];
      x2l[ks] = out[3];
      xm[ks] = out[4];
    }

    // ---- filter pass over all donor tiles ----
    float cd[KNN_CAND];
    int ci[KNN_CAND];
#pragma unroll
    for (int j = 0; j < KNN_CAND; ++j) {
      cd[j] = inf;
      ci[j] = -1;
    }
    // (d, i) into the sorted list; d = +inf or NaN changes nothing
    auto insert = [&](float d, int i) {
      // going down: entry j takes entry j - 1 if d goes before that one,
      // d itself if it goes before entry j only
#pragma unroll
      for (int j = KNN_CAND - 1; j > 0; --j) {
        const bool prev = d < cd[j - 1], here = d < cd[j];
        cd[j] = prev ? cd[j - 1] : (here ? d : cd[j]);
        ci[j] = prev ? ci[j - 1] : (here ? i : ci[j]);
      }
      const bool first = d < cd[0];
      cd[0] = first ? d : cd[0];
      ci[0] = first ? i : ci[0];
    };

    issue(0);
    land(0);
    block_barrier();
    for (int st = 0; st < nstages; ++st) {
      issue(st + 1);
      const short *const buf = kn_lds + (st & 1) * STAGE;
#pragma unroll
      for (int t = 0; t < KNN_STAGE_TILES; ++t) {
        f32x4 sq = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 ov = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const short *const ap = buf + t * TILE + ks * 512 + lane * 8;
          const bf16x8 fh = *reinterpret_cast<const bf16x8 *>(ap);
          const bf16x8 fl = *reinterpret_cast<const bf16x8 *>(ap + KS * 512);
          const bf16x8 f2h = *reinterpret_cast<const bf16x8 *>(ap + 2 * KS * 512);
          const bf16x8 f2l = *reinterpret_cast<const bf16x8 *>(ap + 3 * KS * 512);
          const bf16x8 fmk = *reinterpret_cast<const bf16x8 *>(ap + 4 * KS * 512);
          sq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh, xh[ks], sq, 0, 0, 0);
          sq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh, xl[ks], sq, 0, 0, 0);
          sq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fl, xh[ks], sq, 0, 0, 0);
          sq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fmk, x2h[ks], sq, 0, 0, 0);
          sq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fmk, x2l[ks], sq, 0, 0, 0);
          sq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f2h, xm[ks], sq, 0, 0, 0);
          sq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f2l, xm[ks], sq, 0, 0, 0);
          ov = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fmk, xm[ks], ov, 0, 0, 0);
        }
        const float worst = cd[KNN_CAND - 1];
        const int base = (st * KNN_STAGE_TILES + t) * 16 + grp * 4;
        float num[4];
        unsigned pend = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          num[e] = fm * sq[e];
          const float lim = worst * ov[e];
          const bool can = ov[e] > 0.f && num[e] <= __builtin_fmaf(__builtin_fabsf(lim), 0x1p-22f, lim);
          pend |= (can ? 1u : 0u) << e;
        }
        if (wave_any(pend != 0)) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool mine = (pend >> e) & 1u;
            if (wave_any(mine))
              insert(mine ? num[e] / ov[e] : inf, base + e);
          }
        }
      }
      land((st + 1) & 1);
      block_barrier();
    }

    // what the filter pass found, for the tests of its error bound
    if (cand_idx != nullptr && q < r) {
#pragma unroll
      for (int j = 0; j < KNN_CAND; ++j) {
        cand_idx[(q * 4 + grp) * KNN_CAND + j] = ci[j];
        cand_d2[(q * 4 + grp) * KNN_CAND + j] = cd[j];
      }
    }

    // ---- exact re-rank of this lane's candidates ----
    float esq[KNN_CAND], eov[KNN_CAND];
#pragma unroll
    for (int j = 0; j < KNN_CAND; ++j) esq[j] = eov[j] = 0.f;
    for (int c = 0; c < m; ++c) {
      const float xv = live ? cols[c][ridx] : __builtin_nanf("");
      const float h = mh[c], l = ml[c];
      const bool px = xv == xv;
      const float zx = (xv - h) - l;
#pragma unroll
      for (int j = 0; j < KNN_CAND; ++j) {
        const float f = donors[(int64_t)(ci[j] < 0 ? 0 : ci[j]) * m + c];
        const float dd = zx - ((f - h) - l);
        const bool both = px && f == f && ci[j] >= 0;
        esq[j] += both ? dd * dd : 0.f;
        eov[j] += both ? 1.f : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < KNN_CAND; ++j) {
      const bool ok = ci[j] >= 0 && eov[j] > 0.f;
      cd[j] = ok ? (fm * esq[j]) / eov[j] : inf;
      ci[j] = ok ? ci[j] : KN_NOIDX;
    }

    // ---- k rounds: the row's next neighbour under (d2, index) ----
    float sum = 0.f;
    int cnt = 0;
    const bool writer = grp == 0 && q < r;
    for (int t = 0; t < k; ++t) {
      float bd = inf;
      int bi = KN_NOIDX;
#pragma unroll
      for (int j = 0; j < KNN_CAND; ++j) {
        const bool b = before(cd[j], ci[j], bd, bi);
        bd = b ? cd[j] : bd;
        bi = b ? ci[j] : bi;
      }
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const int src = (lane ^ off) * 4;
        const float od = as_float(__builtin_amdgcn_ds_bpermute(src, as_int(bd)));
        const int oi = __builtin_amdgcn_ds_bpermute(src, bi);
        const bool b = before(od, oi, bd, bi);
        bd = b ? od : bd;
        bi = b ? oi : bi;
      }
      const bool found = bd < inf;
#pragma unroll
      for (int j = 0; j < KNN_CAND; ++j) {
        const bool hit = found && ci[j] == bi;
        cd[j] = hit ? inf : cd[j];
        ci[j] = hit ? KN_NOIDX : ci[j];
      }
      if (writer) {
        idx[q * k + t] = found ? bi : -1;
        d2out[q * k + t] = found ? bd : inf;
        if (found) {
          sum += donors[(int64_t)bi * m + target];
          ++cnt;
        }
      }
    }
    if (writer) est[q] = cnt > 0 ? sum / (float)cnt : __builtin_nanf("");
  }
}

int knn_cus() {
  static int cached = 0;
  if (cached) return cached;
  hipDeviceProp_t prop;
  prop.multiProcessorCount = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  (void)hipGetDeviceProperties(&prop, dev);
  cached = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  return cached;
}

template <int KS>
int launch_knn_impute(const float *const *cols, int64_t n, int m, const int64_t *rows, int64_t r,
                      const float *mh, const float *ml, const float *donors, int s, int target,
                      int k, const uint16_t *img, int blocks, float *est, int *idx, float *d2,
                      int *cand_idx, float *cand_d2, hipStream_t stream) {
  auto kern = knn_impute_kernel<KS>;
  const size_t lds = 2 * (size_t)KNN_STAGE_TILES * knn_tile_shorts(KS * 32) * sizeof(uint16_t);
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return (int)err;
  if (blocks <= 0) {
    // one wave of resident blocks, as K26
    int per_cu = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, reinterpret_cast<const void *>(kern), KN_THREADS, lds);
    if (per_cu <= 0) per_cu = 1;
    blocks = per_cu * knn_cus();
  }
  const int64_t slabs = (r + KNN_SLAB_ROWS - 1) / KNN_SLAB_ROWS;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(blocks, slabs));
  hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(KN_THREADS), lds, stream, cols, n, m, rows, r,
                     mh, ml, donors, target, k, img, knn_tiles(s) / KNN_STAGE_TILES, est, idx, d2,
                     cand_idx, cand_d2);
  return (int)hipGetLastError();
}

bool knn_args_ok(int s, int m, int target) {
  return m >= 1 && m <= KNN_MAX_COLS && s >= 1 && s <= KNN_MAX_DONORS && target >= 0 && target < m;
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" int anovos_knn_donor_image(const float *donors, int s, int m, int target,
                                      const float *mean_hi, const float *mean_lo, uint16_t *img,
                                      hipStream_t stream) {
  if (!knn_args_ok(s, m, target)) return (int)hipErrorInvalidValue;
  const int ks_count = knn_mpad(m) / 32, tiles = knn_tiles(s);
  const int total = tiles * ks_count * 64;
  hipLaunchKernelGGL(knn_donor_image_kernel, dim3((uint32_t)((total + KN_THREADS - 1) / KN_THREADS)),
                     dim3(KN_THREADS), 0, stream, donors, s, m, target, mean_hi, mean_lo, ks_count,
                     tiles, img);
  return (int)hipGetLastError();
}

extern "C" int anovos_knn_impute(const void *const *cols, int64_t n, int m, const int64_t *rows,
                                 int64_t r, const float *mean_hi, const float *mean_lo,
                                 const float *donors, int s, int target, int k, const uint16_t *img,
                                 int blocks, float *est, int *idx, float *d2, int *cand_idx,
                                 float *cand_d2, hipStream_t stream) {
  if (!knn_args_ok(s, m, target) || n < 1 || r < 1 || k < 1 || k > KNN_MAX_K)
    return (int)hipErrorInvalidValue;
  const float *const *c = (const float *const *)cols;
  switch (knn_mpad(m) / 32) {
    case 1: return launch_knn_impute<1>(c, n, m, rows, r, mean_hi, mean_lo, donors, s, target, k, img, blocks, est, idx, d2, cand_idx, cand_d2, stream);
    case 2: return launch_knn_impute<2>(c, n, m, rows, r, mean_hi, mean_lo, donors, s, target, k, img, blocks, est, idx, d2, cand_idx, cand_d2, stream);
    case 3: return launch_knn_impute<3>(c, n, m, rows, r, mean_hi, mean_lo, donors, s, target, k, img, blocks, est, idx, d2, cand_idx, cand_d2, stream);
    case 4: return launch_knn_impute<4>(c, n, m, rows, r, mean_hi, mean_lo, donors, s, target, k, img, blocks, est, idx, d2, cand_idx, cand_d2, stream);
  }
  return (int)hipErrorInvalidValue;
}
