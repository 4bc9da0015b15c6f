// K31: the apply step of regression imputation (sklearn IterativeImputer with
// linear estimators) as a row-local chain, in one read of the frame
// (ops/chain.py states the model side).
//
//   z0_i = isnan(x_i) ? 0 : (x_i - mh_i) - ml_i                     (f32)
//   P'[r, p] = beta[r, p] + sum_i C[r, p, i] z0_i                   observed part
//   for r < R, p < m_s, j = order[p] null in the row (Omega = the row's nulls):
//     z_j <- clip(P'[r, p] + sum_{i in Omega, i != j} C[r, p, i] z_i, lo_j, hi_j)
//   outs[j][row] = z_j + mh_j                                       null entries only
//
// z_i of a null starts at 0, so a null and its initial fill are the same
// value and the observed part does not depend on the chain: it is a dense
// [rows x m] . [m x R m_s] product, and only the R |Omega| steps of a row's
// own nulls are sequential.
//
// Observed part: split bf16 on v_mfma_f32_16x16x32_bf16 with fp32
// accumulation, operands split as in K26 - K30 (hi = bf16(v), lo =
// bf16(v - hi), both round-to-nearest-even), but with all FOUR products
// ch.zh + ch.zl + cl.zh + cl.zl. hi + lo carries 16 significant bits, so an
// operand's residual is at most 2^-17 |v|, while the cl.zl term reaches
// 2^-16 |c z|: dropping it, as the three-product kernels do, leaves up to
// 2^-15 on a single product, above the bound this kernel is held to,
// (3 * 2^-18 + (3 m_pad + 1) * 2^-24) sum |c| |z0| (ops.chain.CHAIN_GAMMA).
// With three products a 6-column model whose step has one dominant term
// measured 1.15 of that bound on 18 of 18 005 entries; with four the split
// costs at most 2^-16. The MFMAs are not what the kernel waits for.
// The intercept is the accumulator's initial value. A = a coefficient tile
// (16 steps x 32 columns), B = a Z tile (32 columns x 16 rows): a lane's C
// registers hold, for the row (lane & 15), the steps (lane >> 4) * 4 + reg.
//
// Coefficient image: built once per call by chain_image_kernel in A-fragment
// order, [stage][plane][k-step][lane][8] bf16, one stage per (round, step
// tile), the intercepts behind it as f32, 16 per stage.
//
// Work split: persistent 256-thread blocks in one wave of resident blocks,
// each owning a contiguous range of 64-row slabs. Per slab
//   1. all threads stage x into K26's two-plane bf16 Z image (unguarded
//      16-byte nontemporal loads; the one partial slab guarded) and write a
//      null flag per (row, column);
//   2. wave w compacts, for each of its 16 rows, the steps whose target is
//      null into a list in order sequence (one ballot per 64 steps), packed
//      (step | column << 8), and zeroes the row's state zc[row][k];
//   3. per round: the step tiles are dealt to the waves, tile T to wave
//      T & 3, which multiplies it with all four row tiles - so a stage of
//      the image is read from L2 once per block, straight into registers,
//      the next tile's fragments requested before this tile's products, with
//      no LDS ring and no barrier per stage - and writes P' to an LDS patch
//      P[64][m_s_pad]; the Z fragments are read from LDS (two ds_read_b128
//      per four MFMAs). One barrier, then wave w runs the chain
//      of its own 16 rows: the four lanes of a row walk its list in order,
//      split the sum over Omega between them (C as f32 straight from the
//      global table: one step reads within one row of it), combine as
//      (g0 + g1) + (g2 + g3) through two ds_bpermute, add P', clip, store the
//      state. A wave without nulls skips the chain. One barrier, next round.
//   4. the row's lanes store zc + mh to the null entries, 4 bytes each.
// The null flags share the LDS of P (dead before round 0 writes it). No
// atomics: the same call returns the same bits.
//
// Resources (hipcc -O3, gfx950, 256 threads): see docs/KERNELS.md, K31; no
// scratch in any instantiation.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "anovos_kernels.h"

// Compiled without the packed fp32 instructions, for the reason given in
// project_columns.hip: the staging step pairs two columns exactly as K27's
// does.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int CI_THREADS = 256;
constexpr int CI_ZSTRIDE = ROWQUAD_Z_SLOTS;

static_assert(CHAIN_SLAB_ROWS == 64 && CI_THREADS == 4 * 64, "one wave per 16-row tile");
static_assert(CI_ZSTRIDE == CHAIN_SLAB_ROWS + CHAIN_SLAB_ROWS / 16, "one spare slot per tile");
static_assert(CHAIN_MAX_COLS == 5 * 32, "KS = 1 .. 5");
static_assert(CHAIN_MAX_COLS <= 256, "a list entry packs step and column into 8 bits each");

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef uint32_t nat_u4 __attribute__((ext_vector_type(4)));
typedef float nat_f4 __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1))) *gcolptr;
typedef const nat_u4 __attribute__((address_space(1))) *gvecptr;
typedef float __attribute__((address_space(1))) *goutptr;

__device__ __forceinline__ float bf16_value(uint32_t bits) {
  return __builtin_bit_cast(float, bits << 16);
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

// LDS written by one lane of a wave, read by another
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float lane_xor(float v, int lane, int mask) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ mask) << 2, __builtin_bit_cast(int, v)));
}

// bytes of LDS of one block: Z image, P patch (the null flags share it),
// chain state, lists, counts, and per padded column two pointers, the order
// entry, centre (two floats) and clip bounds
__host__ __device__ constexpr size_t chain_lds_bytes(int ks) {
  return (size_t)rowquad_z_bytes(32 * ks) + 64 * (32 * ks + 4) * 4 + 64 * (32 * ks + 1) * 4 +
         64 * 32 * ks * 2 + 64 * 4 + 32 * ks * (8 + 8 + 4 + 4 * 4);
}
static_assert(chain_lds_bytes(5) <= 160 * 1024, "one block fits a CU's LDS");

// One thread per (stage, k-step, lane) of the image: the eight columns of
// k-group g = lane >> 4 of step tile * 16 + (lane & 15), both planes.
// Out-of-range steps and columns are zero. The first 16 * stages threads
// also write one intercept each.
__global__ __launch_bounds__(CI_THREADS) void chain_image_kernel(const float *C, const float *beta,
                                                                 int m, int m_s, int R, int ks_count,
                                                                 int tiles, uint16_t *img) {
  const int t = blockIdx.x * CI_THREADS + threadIdx.x;
  const int ns = R * tiles;
  if (t >= ns * ks_count * 64) return;
  if (t < ns * 16) {
    const int st = t >> 4, p = (st % tiles) * 16 + (t & 15);
    reinterpret_cast<float *>(img + (int64_t)ns * ks_count * 1024)[t] =
        p < m_s ? beta[(st / tiles) * m_s + p] : 0.f;
  }
  const int lane = t & 63;
  const int ks = (t >> 6) % ks_count;
  const int st = (t >> 6) / ks_count;
  const int r = st / tiles, p = (st % tiles) * 16 + (lane & 15), g = lane >> 4;
  uint32_t h[4], l[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int c = 32 * ks + 8 * g + 2 * q + e;
      v[e] = (p < m_s && c < m) ? C[((int64_t)r * m_s + p) * m + c] : 0.f;
    }
    h[q] = pack_bf16(v[0], v[1]);
    l[q] = pack_bf16(v[0] - bf16_value(h[q] & 0xFFFFu), v[1] - bf16_value(h[q] >> 16));
  }
  uint16_t *const dst = img + ((int64_t)st * 2 * ks_count + ks) * 512 + lane * 8;
  *reinterpret_cast<nat_u4 *>(dst) = nat_u4{h[0], h[1], h[2], h[3]};
  *reinterpret_cast<nat_u4 *>(dst + ks_count * 512) = nat_u4{l[0], l[1], l[2], l[3]};
}

template <int KS>
__global__ __launch_bounds__(CI_THREADS, KS <= 2 ? 2 : 1) void chain_impute_kernel(
    const float *const *cols, int64_t n, int m, int m_s, int R, const float *mean_hi,
    const float *mean_lo, const int *order, const float *Ctab, const uint16_t *img,
    const float *lo, const float *hi, float *const *outs) {
  extern __shared__ __attribute__((aligned(16))) short ci_lds[];
  constexpr int MP = 32 * KS;                   // padded columns = most steps of a round
  constexpr int OCT = 4 * KS;                   // column octets
  constexpr int ZPLANE = OCT * CI_ZSTRIDE * 8;  // shorts per Z plane
  constexpr int STAGE = KS * 1024;              // shorts per image stage
  constexpr int PST = MP + 4;                   // floats per row of P
  constexpr int ZCS = MP + 1;                   // floats per row of the chain state
  constexpr int NX = 2 * KS;                    // 16-byte loads per thread and slab
  short *const zs = ci_lds;
  float *const Pp = reinterpret_cast<float *>(zs + 2 * ZPLANE);  // [64][PST]
  uint8_t *const flags = reinterpret_cast<uint8_t *>(Pp);        // [64][MP], dead before P
  float *const zc = Pp + 64 * PST;                               // [64][ZCS], by list position
  uint16_t *const lst = reinterpret_cast<uint16_t *>(zc + 64 * ZCS);  // [64][MP] step | col << 8
  int *const cnt = reinterpret_cast<int *>(lst + 64 * MP);            // [64]
  uint64_t *const colp = reinterpret_cast<uint64_t *>(cnt + 64);      // [MP]
  uint64_t *const outp = colp + MP;                                   // [MP]
  int *const ords = reinterpret_cast<int *>(outp + MP);               // [MP]
  float *const mhs = reinterpret_cast<float *>(ords + MP);            // [MP]
  float *const mls = mhs + MP;
  float *const los = mls + MP;
  float *const his = los + MP;

  const int64_t macro_total = (n + CHAIN_SLAB_ROWS - 1) / CHAIN_SLAB_ROWS;
  const int64_t macro_per = (macro_total + gridDim.x - 1) / gridDim.x;
  const int64_t mac_s = (int64_t)blockIdx.x * macro_per;
  const int64_t mac_e = min(macro_total, mac_s + macro_per);
  if (mac_s >= mac_e) return;  // whole block, before any barrier
  const int64_t full_e = min(mac_e, n / CHAIN_SLAB_ROWS);  // slabs entirely below n

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rw = lane & 15;   // row of a tile
  const int kog = lane >> 4;  // k-group of a k-step; 4-step group of C; quarter of a row's list
  const int tiles = chain_tiles(m_s);
  const float *const betap = reinterpret_cast<const float *>(img + (int64_t)R * tiles * STAGE);

  // ---- once per block: tables to LDS, the Z image cleared (a padding
  // column of a k-step is never written again) ----
  for (int i = threadIdx.x; i < MP; i += CI_THREADS) {
    const int c = min(i, m - 1);  // a padding column stands on a real one
    colp[i] = (uint64_t)(uintptr_t)cols[c];
    outp[i] = i < m ? (uint64_t)(uintptr_t)outs[i] : 0ull;
    ords[i] = i < m_s ? order[i] : 0;
    mhs[i] = mean_hi[c];
    mls[i] = mean_lo[c];
    los[i] = lo[c];
    his[i] = hi[c];
  }
  for (int i = threadIdx.x; i < 2 * ZPLANE / 8; i += CI_THREADS)
    reinterpret_cast<nat_u4 *>(zs)[i] = nat_u4{0u, 0u, 0u, 0u};
  block_barrier();

  // ---- x staging: thread t takes the 4-row segment t & 15 of the slab and
  // the column pair t >> 4 of every k-step ----
  const int seg = threadIdx.x & 15;
  const int pq = threadIdx.x >> 4;
  // one pair of one k-step: 4 rows x 2 columns -> both planes and the flags
  auto stage = [&](int it, const float (&a)[4], const float (&b)[4]) {
    const int col = it * 32 + pq * 2;
    short *const dst =
        zs + ((((pq >> 2) + it * 4) * CI_ZSTRIDE + seg * 4 + (seg >> 2)) * 8 + (pq & 3) * 2);
    const float ha = mhs[col], la = mls[col], hb = mhs[col + 1], lb = mls[col + 1];
    const bool b_real = col + 1 < m;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const bool na = isnan(a[rr]), nb = b_real && isnan(b[rr]);
      const float za = na ? 0.f : (a[rr] - ha) - la;
      const float zb = (!b_real || nb) ? 0.f : (b[rr] - hb) - lb;
      const uint32_t hw = pack_bf16(za, zb);
      const uint32_t lw = pack_bf16(za - bf16_value(hw & 0xFFFFu), zb - bf16_value(hw >> 16));
      *reinterpret_cast<uint32_t *>(dst + rr * 8) = hw;
      *reinterpret_cast<uint32_t *>(dst + ZPLANE + rr * 8) = lw;
      *reinterpret_cast<uint16_t *>(flags + (seg * 4 + rr) * MP + col) =
          (uint16_t)((na ? 1u : 0u) | (nb ? 0x100u : 0u));
    }
  };
  auto stage_full = [&](int64_t slab) {
    const int64_t off = slab * CHAIN_SLAB_ROWS + seg * 4;
    nat_u4 pre[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int col = (i >> 1) * 32 + pq * 2 + (i & 1);
      pre[i] = __builtin_nontemporal_load((gvecptr)((gcolptr)(uintptr_t)colp[col] + off));
    }
#pragma unroll
    for (int it = 0; it < KS; ++it) {
      if (it * 32 + pq * 2 < m) {
        const nat_f4 va = __builtin_bit_cast(nat_f4, pre[2 * it]);
        const nat_f4 vb = __builtin_bit_cast(nat_f4, pre[2 * it + 1]);
        const float a[4] = {va.x, va.y, va.z, va.w};
        const float b[4] = {vb.x, vb.y, vb.z, vb.w};
        stage(it, a, b);
      }
    }
  };
  // the partial slab: rows at and past n count as present, with value 0
  auto stage_partial = [&](int64_t slab) {
    const int64_t row = slab * CHAIN_SLAB_ROWS + seg * 4;
#pragma unroll
    for (int it = 0; it < KS; ++it) {
      const int col = it * 32 + pq * 2;
      if (col < m) {
        const gcolptr xa = (gcolptr)(uintptr_t)colp[col] + row;
        const gcolptr xb = (gcolptr)(uintptr_t)colp[col + 1] + row;
        float a[4], b[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          a[rr] = (row + rr < n) ? xa[rr] : 0.f;
          b[rr] = (row + rr < n) ? xb[rr] : 0.f;
        }
        stage(it, a, b);
      }
    }
  };

  // this lane's A fragments of one stage of the image
  auto load_a = [&](int st, bf16x8 (&h)[KS], bf16x8 (&l)[KS]) {
    const uint16_t *const src = img + (int64_t)st * STAGE + lane * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      h[ks] = *reinterpret_cast<const bf16x8 *>(src + ks * 512);
      l[ks] = *reinterpret_cast<const bf16x8 *>(src + (KS + ks) * 512);
    }
  };

  const int row = wave * 16 + rw;  // the row of the slab this lane chains
  for (int64_t slab = mac_s; slab < mac_e; ++slab) {
    // ---- 1. stage the slab ----
    if (slab < full_e)
      stage_full(slab);
    else
      stage_partial(slab);
    block_barrier();

    // ---- 2. the wave's 16 lists, in order sequence ----
    int maxc = 0;
    for (int rr = 0; rr < 16; ++rr) {
      const int q = wave * 16 + rr;
      int count = 0;
      for (int p0 = 0; p0 < m_s; p0 += 64) {
        const int p = p0 + lane;
        const int col = p < m_s ? ords[p] : 0;
        const bool isn = p < m_s && flags[q * MP + col] != 0;
        const uint64_t mask = __builtin_amdgcn_ballot_w64(isn);
        const int below = __builtin_amdgcn_mbcnt_hi(
            (uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (isn) lst[q * MP + count + below] = (uint16_t)(p | (col << 8));
        count += __builtin_popcountll(mask);
      }
      for (int k = lane; k < count; k += 64) zc[q * ZCS + k] = 0.f;
      if (lane == 0) cnt[q] = count;
      maxc = max(maxc, count);
    }
    block_barrier();  // the flags are dead: P may be written
    const int c = cnt[row];

    for (int r = 0; r < R; ++r) {
      // ---- 3a. observed part of the round: tile T on wave T & 3 ----
      {
        bf16x8 ah[KS], al[KS];
        if (wave < tiles) load_a(r * tiles + wave, ah, al);
        for (int T = wave; T < tiles; T += 4) {
          bf16x8 nh[KS], nl[KS];
          load_a(r * tiles + (T + 4 < tiles ? T + 4 : T), nh, nl);
          const f32x4 b4 = *reinterpret_cast<const f32x4 *>(betap + (r * tiles + T) * 16 + kog * 4);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const short *const zb = zs + (kog * CI_ZSTRIDE + q * 17 + rw) * 8;
            f32x4 acc = b4;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
              const bf16x8 zh = *reinterpret_cast<const bf16x8 *>(zb + ks * 4 * CI_ZSTRIDE * 8);
              const bf16x8 zl =
                  *reinterpret_cast<const bf16x8 *>(zb + ks * 4 * CI_ZSTRIDE * 8 + ZPLANE);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[ks], zh, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[ks], zl, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[ks], zh, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[ks], zl, acc, 0, 0, 0);
            }
            *reinterpret_cast<f32x4 *>(Pp + (q * 16 + rw) * PST + T * 16 + kog * 4) = acc;
          }
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) ah[ks] = nh[ks], al[ks] = nl[ks];
        }
      }
      block_barrier();

      // ---- 3b. the chain of the wave's rows ----
      if (maxc > 0) {
        const float *const Cr = Ctab + (int64_t)r * m_s * m;
        for (int s = 0; s < maxc; ++s) {
          const bool act = s < c;
          const int e = act ? lst[row * MP + s] : 0;
          const int p = e & 0xFF, j = e >> 8;
          const float *const crow = Cr + p * m;
          float part = 0.f;
          if (act) {
            for (int k = kog; k < c; k += 4) {
              if (k != s) part = fmaf(crow[lst[row * MP + k] >> 8], zc[row * ZCS + k], part);
            }
          }
          float t = part + lane_xor(part, lane, 16);  // g0 + g1, g2 + g3
          t = t + lane_xor(t, lane, 32);              // (g0 + g1) + (g2 + g3)
          if (act && kog == 0) {
            const float v = Pp[row * PST + p] + t;
            zc[row * ZCS + s] = fminf(fmaxf(v, los[j]), his[j]);
          }
          wave_sync();
        }
      }
      block_barrier();  // P is free for the next round, or for the next slab's flags
    }

    // ---- 4. the null entries of the wave's rows ----
    const int64_t grow = slab * CHAIN_SLAB_ROWS + row;
    for (int k = kog; k < c; k += 4) {
      const int j = lst[row * MP + k] >> 8;
      const uint64_t o = outp[j];
      if (o != 0) ((goutptr)(uintptr_t)o)[grow] = zc[row * ZCS + k] + mhs[j];
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

int chain_cus() {
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
int launch_chain_impute(const float *const *cols, int64_t n, int m, int m_s, int R,
                        const float *mean_hi, const float *mean_lo, const int *order,
                        const float *C, const uint16_t *img, const float *lo, const float *hi,
                        int blocks, float *const *outs, hipStream_t stream) {
  auto kern = chain_impute_kernel<KS>;
  const size_t lds = chain_lds_bytes(KS);
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return (int)err;
  if (blocks <= 0) {
    // one wave of resident blocks, as K26
    int per_cu = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, reinterpret_cast<const void *>(kern), CI_THREADS, lds);
    if (per_cu <= 0) per_cu = 1;
    blocks = per_cu * chain_cus();
  }
  const int64_t macro_total = (n + CHAIN_SLAB_ROWS - 1) / CHAIN_SLAB_ROWS;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(blocks, macro_total));
  hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(CI_THREADS), lds, stream, cols, n, m, m_s, R,
                     mean_hi, mean_lo, order, C, img, lo, hi, outs);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int anovos_chain_image(const float *C, const float *beta, int m, int m_s, int R,
                                  uint16_t *img, hipStream_t stream) {
  if (!chain_shape_ok(m, m_s, R)) return (int)hipErrorInvalidValue;
  const int total = R * chain_tiles(m_s) * chain_ks(m) * 64;
  hipLaunchKernelGGL(chain_image_kernel, dim3((uint32_t)((total + CI_THREADS - 1) / CI_THREADS)),
                     dim3(CI_THREADS), 0, stream, C, beta, m, m_s, R, chain_ks(m), chain_tiles(m_s),
                     img);
  return (int)hipGetLastError();
}

extern "C" int anovos_chain_impute(const void *const *cols, int64_t n, int m, int m_s, int R,
                                   const float *mean_hi, const float *mean_lo, const int *order,
                                   const float *C, const uint16_t *img, const float *lo,
                                   const float *hi, int blocks, float *const *outs,
                                   hipStream_t stream) {
  if (n < 1 || !chain_shape_ok(m, m_s, R)) return (int)hipErrorInvalidValue;
  const float *const *c = (const float *const *)cols;
  switch (chain_ks(m)) {
    case 1: return launch_chain_impute<1>(c, n, m, m_s, R, mean_hi, mean_lo, order, C, img, lo, hi, blocks, outs, stream);
    case 2: return launch_chain_impute<2>(c, n, m, m_s, R, mean_hi, mean_lo, order, C, img, lo, hi, blocks, outs, stream);
    case 3: return launch_chain_impute<3>(c, n, m, m_s, R, mean_hi, mean_lo, order, C, img, lo, hi, blocks, outs, stream);
    case 4: return launch_chain_impute<4>(c, n, m, m_s, R, mean_hi, mean_lo, order, C, img, lo, hi, blocks, outs, stream);
    case 5: return launch_chain_impute<5>(c, n, m, m_s, R, mean_hi, mean_lo, order, C, img, lo, hi, blocks, outs, stream);
  }
  return (int)hipErrorInvalidValue;
}
