// K26: per-row quadratic form d2 = |W z|^2 on MFMA matrix cores - the
// Mahalanobis distance of every row once W is a whitening matrix
// (ops/mahalanobis.py).
//
//   z_j = isnan(x_j) ? 0 : (x_j - shift_j) * scale_j     (f32, subtract then multiply)
//   y_i = sum_j W[i][j] z_j                               i < r
//   d2  = sum_i y_i^2
//
// Numerics: split bf16, three products. Every operand is taken as hi + lo,
// hi = bf16(v) round-to-nearest-even, lo = bf16(v - hi) (the difference is
// exact in f32), and y accumulates wh.zh + wh.zl + wl.zh on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulators; the wl.zl term (2^-18
// relative) is dropped. A plain bf16 operand would leave 2^-9, which the
// whitening amplifies by lambda_min^-1/2. W is split once per call by
// row_quadform_split_kernel into the image the blocks copy to LDS.
//
// MFMA roles: A = W tile (16 output components x 32 columns), B = Z tile
// (32 columns x 16 rows of the frame), so a C fragment holds, for the row
// (lane & 15), the components (lane >> 4) * 4 + reg. A lane squares and
// adds its registers over all component tiles in ascending order; the four
// 16-lane groups of a row are then combined as (g0 + g1) + (g2 + g3). No
// floating-point atomics: the same call returns the same bits.
//
// Layout. Columns are padded to k_pad, a multiple of 32 (KS = k_pad / 32
// MFMA k-steps, a template parameter: the register arrays below are sized
// by it), in octets of 8. A block stages a ROWQUAD_SLAB_ROWS = 64-row slab
// of ALL columns through LDS as two bf16 planes formed in registers from
// the one read of x:
//   Z: [2 planes][k_pad / 8 octets][RQ_ZSTRIDE slots][8 columns] bf16
// one 16-byte slot per (octet, row), so a B fragment is one aligned
// ds_read_b128. The slot of row q is q + (q >> 4): one spare slot per
// 16-row tile keeps the staging stores (ds_write_b32, 32 banks) 2-way at
// most, which costs nothing.
//   W: [2 planes][k_pad / 8 octets][rw_pad rows][8 columns] bf16
// stays in LDS for the block's lifetime; rw_pad is a multiple of 16, so
// the octet stride is a multiple of 256 B and an A-fragment ds_read_b128
// (lane groups mix two octets on disjoint rows) is conflict-free.
// Blocks are persistent: the grid is one wave of resident blocks and each
// block owns one contiguous range of slabs, so W is read from L2 once per
// block, not once per slab.
//
// Staging: thread t stages the 4-row segment (t & 15) of the column pair
// (t >> 4) of every k-step, i.e. wave w fills octet w of each k-step and
// packs the pair's two bf16 into one 32-bit store per row and plane.
// Column base pointers (global address space), shifts and scales are
// resolved once per block; padding columns' slots are zeroed once and never
// dereferenced. Full slabs take an unguarded path of 16-byte nontemporal
// loads issued two rounds ahead, as in K25; the one partial slab at the end
// of the frame takes the guarded element path (rows past n count as null
// and are not written).
//
// Per wave: wave w owns row tile w of the slab. It reads its Z fragments
// (both planes, all k-steps: 8 * KS VGPRs) into registers once per slab and
// streams only W from LDS - two ds_read_b128 per three MFMAs. Once every
// wave holds its fragments the slab in LDS is free, so the conversion of
// the next slab runs between the products of this one: with one wave per
// SIMD the conversion's VALU work would otherwise leave the matrix core
// idle for as long as the products take.
//
// Wider W than LDS holds: the binding launches once per window of W's rows
// [r0, r0 + rw_pad) (rowquad_window_rows in anovos_kernels.h); d2 is a sum
// over output components, so later windows add into out. A row of out is
// written by exactly one lane per launch and launches are stream-ordered.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cmath>

#include "anovos_kernels.h"

namespace {

constexpr int RQ_THREADS = 256;
constexpr int RQ_ZSTRIDE = ROWQUAD_Z_SLOTS;

static_assert(ROWQUAD_SLAB_ROWS == 64 && RQ_THREADS == 4 * 64, "one wave per 16-row tile");
static_assert(RQ_ZSTRIDE == ROWQUAD_SLAB_ROWS + ROWQUAD_SLAB_ROWS / 16, "one spare slot per tile");

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef float nat_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t nat_u4 __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1))) *gcolptr;
typedef const nat_f4 __attribute__((address_space(1))) *gvecptr;

// round-to-nearest-even into the upper 16 bits, as K25's bf16_bits
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

// two f32 -> two bf16 (a in the low half), round-to-nearest-even by the
// hardware's packed conversion: the same rounding as bf16_bits
typedef __bf16 hw_bf16x2 __attribute__((ext_vector_type(2)));
typedef float nat_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
  const hw_bf16x2 r = __builtin_convertvector(nat_f2{a, b}, hw_bf16x2);
  uint32_t u;
  __builtin_memcpy(&u, &r, 4);
  return u;
}

// v -> bf16 hi, bf16 lo with v = hi + lo + O(2^-18 |v|)
__device__ __forceinline__ void split_bf16(float v, uint32_t &hi, uint32_t &lo) {
  hi = bf16_bits(v);
  lo = bf16_bits(v - bf16_value(hi));
}

// W [r, k] f32 row-major -> the two bf16 planes, [plane][octet][r_pad][8],
// zero in the padding rows and columns. One thread per (octet, row).
__global__ __launch_bounds__(RQ_THREADS) void row_quadform_split_kernel(
    const float *W, int r, int k, int r_pad, int k_pad, uint16_t *img) {
  const int idx = blockIdx.x * RQ_THREADS + threadIdx.x;
  const int octets = k_pad / 8;
  if (idx >= octets * r_pad) return;
  const int o = idx / r_pad, i = idx % r_pad;
  uint16_t *const hi = img + (int64_t)idx * 8;
  uint16_t *const lo = hi + (int64_t)octets * r_pad * 8;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int j = o * 8 + e;
    const float v = (i < r && j < k) ? W[(int64_t)i * k + j] : 0.f;
    uint32_t h, l;
    split_bf16(v, h, l);
    hi[e] = (uint16_t)h;
    lo[e] = (uint16_t)l;
  }
}

template <int KS>
__global__ __launch_bounds__(RQ_THREADS, 1) void row_quadform_kernel(
    const float *const *cols, int64_t n, int k, const float *shift, const float *scale,
    const uint16_t *wimg, int r_pad, int r0, int rw_pad, int accumulate, float *out) {
  extern __shared__ __attribute__((aligned(16))) short rq_lds[];
  constexpr int NIT = 2 * KS;   // 16-byte loads per thread per round
  constexpr int OCT = 4 * KS;   // column octets
  constexpr int ZPLANE = OCT * RQ_ZSTRIDE * 8;  // shorts per Z plane
  short *const zs = rq_lds;
  short *const ws = rq_lds + 2 * ZPLANE;
  const int wplane = OCT * rw_pad * 8;  // shorts per W plane

  const int64_t macro_total = (n + ROWQUAD_SLAB_ROWS - 1) / ROWQUAD_SLAB_ROWS;
  const int64_t macro_per = (macro_total + gridDim.x - 1) / gridDim.x;
  const int64_t mac_s = (int64_t)blockIdx.x * macro_per;
  const int64_t mac_e = min(macro_total, mac_s + macro_per);
  if (mac_s >= mac_e) return;  // whole block, before any barrier
  // slabs below full_e lie entirely below n; at most one more (the partial
  // one) follows, in the last non-empty block
  const int64_t full_e = min(mac_e, n / ROWQUAD_SLAB_ROWS);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = lane & 15;    // component in the W tile (A) / row in the Z tile (B)
  const int kog = lane >> 4;  // this lane's octet of the k-step

  // ---- W window -> LDS, once per block ----
  {
    const int64_t img_plane = (int64_t)OCT * r_pad * 8;
    const int per_plane = OCT * rw_pad;  // 16-byte slots
    for (int s = threadIdx.x; s < 2 * per_plane; s += RQ_THREADS) {
      const int p = s >= per_plane;
      const int q = s - p * per_plane;
      const int o = q / rw_pad, i = q - o * rw_pad;
      const nat_u4 v = *reinterpret_cast<const nat_u4 *>(
          wimg + p * img_plane + ((int64_t)o * r_pad + r0 + i) * 8);
      *reinterpret_cast<nat_u4 *>(ws + p * wplane + q * 8) = v;
    }
  }

  // ---- staging set-up: once per block ----
  const int seg = threadIdx.x & 15;  // 4-row segment of the slab
  const int pq = threadIdx.x >> 4;   // column pair of the k-step: octet pq >> 2 (= wave)
  // hi-plane entry of row seg * 4 of this thread's pair in k-step 0; k-step
  // `it` lies 4 octets further on, row +1 one slot, the lo plane ZPLANE
  short *const dst0 =
      zs + (((pq >> 2) * RQ_ZSTRIDE + seg * 4 + (seg >> 2)) * 8 + (pq & 3) * 2);
  gcolptr xp[NIT];
  float sh[NIT], sc[NIT];
  unsigned real = 0;  // bit 2 * it + c: column c of this thread's pair of step it exists
#pragma unroll
  for (int it = 0; it < KS; ++it) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int col = it * 32 + pq * 2 + c;
      const int cc = min(col, k - 1);
      // a padding column stands on a real one, loads it in the full rounds
      // and drops the value
      xp[2 * it + c] = (gcolptr)cols[cc] + seg * 4;
      sh[2 * it + c] = shift[cc];
      sc[2 * it + c] = scale[cc];
      if (col < k) real |= 1u << (2 * it + c);
    }
    if (!((real >> (2 * it)) & 1u)) {  // both columns are padding: zeroed here, once
      short *const d = dst0 + it * 4 * RQ_ZSTRIDE * 8;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        *reinterpret_cast<uint32_t *>(d + rr * 8) = 0u;
        *reinterpret_cast<uint32_t *>(d + ZPLANE + rr * 8) = 0u;
      }
    }
  }

  // one pair of one k-step: 4 rows x 2 columns -> both planes
  auto stage = [&](int it, const float (&a)[4], const float (&b)[4]) {
    short *const d = dst0 + it * 4 * RQ_ZSTRIDE * 8;
    const bool b_real = (real >> (2 * it + 1)) & 1u;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const float za = isnan(a[rr]) ? 0.f : (a[rr] - sh[2 * it]) * sc[2 * it];
      const float zb = (!b_real || isnan(b[rr])) ? 0.f : (b[rr] - sh[2 * it + 1]) * sc[2 * it + 1];
      const uint32_t h = pack_bf16(za, zb);
      const uint32_t l = pack_bf16(za - bf16_value(h & 0xFFFFu), zb - bf16_value(h >> 16));
      *reinterpret_cast<uint32_t *>(d + rr * 8) = h;
      *reinterpret_cast<uint32_t *>(d + ZPLANE + rr * 8) = l;
    }
  };

  // Two rounds of loads are in flight, as in K25: every lane issues NIT
  // loads per round, padding columns included, and every issue in the loop
  // is unconditional (past the last full slab it repeats that one), so the
  // wait before a conversion can leave the NIT younger loads outstanding.
  nat_f4 pre0[NIT], pre1[NIT];
  auto issue = [&](nat_f4(&pre)[NIT], int64_t slab_index) {
    const int64_t off = min(slab_index, full_e - 1) * ROWQUAD_SLAB_ROWS;
#pragma unroll
    for (int i = 0; i < NIT; ++i) pre[i] = __builtin_nontemporal_load((gvecptr)(xp[i] + off));
  };
  auto convert_step = [&](int it, const nat_f4(&pre)[NIT]) {
    if ((real >> (2 * it)) & 1u) {
      const float a[4] = {pre[2 * it].x, pre[2 * it].y, pre[2 * it].z, pre[2 * it].w};
      const float b[4] = {pre[2 * it + 1].x, pre[2 * it + 1].y, pre[2 * it + 1].z,
                          pre[2 * it + 1].w};
      stage(it, a, b);
    }
  };

  // ---- MFMA set-up: wave w owns row tile w of the slab ----
  const short *const zbase = zs + (kog * RQ_ZSTRIDE + wave * 17 + m) * 8;
  const short *const wbase = ws + (kog * rw_pad + m) * 8;
  const int rw_tiles = rw_pad / 16;
  bf16x8 zh[KS], zl[KS];

  // this wave's Z fragments of the staged slab -> registers; once every
  // wave has them (a barrier) the slab in LDS is free for the next one
  auto read_frags = [&]() {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      zh[ks] = *reinterpret_cast<const bf16x8 *>(zbase + ks * 4 * RQ_ZSTRIDE * 8);
      zl[ks] = *reinterpret_cast<const bf16x8 *>(zbase + ks * 4 * RQ_ZSTRIDE * 8 + ZPLANE);
    }
  };
  // sum of squares of the 4 components this lane holds of W tile ti
  auto tile = [&](int ti) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const short *const wp = wbase + (ks * 4 * rw_pad + ti * 16) * 8;
      const bf16x8 wh = *reinterpret_cast<const bf16x8 *>(wp);
      const bf16x8 wl = *reinterpret_cast<const bf16x8 *>(wp + wplane);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, zh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, zl[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, zh[ks], acc, 0, 0, 0);
    }
    float t = acc.x * acc.x;
    t += acc.y * acc.y;
    t += acc.z * acc.z;
    t += acc.w * acc.w;
    return t;
  };
  // The products of the slab held in zh / zl and, with `conv`, the
  // conversion of the next slab from `pre` into LDS: the first KS tiles and
  // the KS conversion steps alternate in one straight-line stretch, so the
  // conversion's VALU work issues while the matrix core runs. With fewer
  // than KS tiles the last one is repeated and its sum dropped.
  auto phase = [&](int64_t slab_index, const nat_f4(&pre)[NIT], bool conv) {
    float d2 = 0.f;
#pragma unroll
    for (int it = 0; it < KS; ++it) {
      const float t = tile(min(it, rw_tiles - 1));
      d2 += it < rw_tiles ? t : 0.f;
      if (conv) convert_step(it, pre);
    }
    for (int ti = KS; ti < rw_tiles; ++ti) d2 += tile(ti);
    // the four 16-lane groups hold components 4g .. 4g + 3 (mod 16) of row m
    d2 = d2 + __shfl_xor(d2, 16);
    d2 = d2 + __shfl_xor(d2, 32);
    const int64_t row = slab_index * ROWQUAD_SLAB_ROWS + wave * 16 + lane;
    if (lane < 16 && row < n) out[row] = accumulate ? out[row] + d2 : d2;
  };

  // ---- steady state: full slabs, two per trip ----
  // Entering a half trip for slab s: LDS holds slab s, one prefetch buffer
  // slab s + 1, the other slab s + 2. Barrier, fragments of s to registers,
  // barrier, then products of s interleaved with the conversion of s + 1.
  if (mac_s < full_e) {
    issue(pre0, mac_s);
    issue(pre1, mac_s + 1);
#pragma unroll
    for (int it = 0; it < KS; ++it) convert_step(it, pre0);
    issue(pre0, mac_s + 2);
    int64_t s = mac_s;
    for (; s + 1 < full_e; s += 2) {
      __syncthreads();  // slab s (and, the first time, W) is in LDS
      read_frags();
      __syncthreads();  // every wave holds its fragments: the slab is free
      phase(s, pre1, true);
      issue(pre1, s + 3);
      __syncthreads();
      read_frags();
      __syncthreads();
      phase(s + 1, pre0, true);  // past the last full slab: a repeat of it, unused
      issue(pre0, s + 4);
    }
    if (s < full_e) {  // odd count: the last full slab is in LDS
      __syncthreads();
      read_frags();
      __syncthreads();
      phase(s, pre0, false);
    }
  }

  // ---- tail: the one partial slab, guarded per element ----
  if (full_e < mac_e) {
    const int64_t row = full_e * ROWQUAD_SLAB_ROWS + (int64_t)seg * 4;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < KS; ++it) {
      if ((real >> (2 * it)) & 1u) {
        const float nanv = __builtin_nanf("");
        float a[4], b[4];
        const gcolptr xa = xp[2 * it] + full_e * ROWQUAD_SLAB_ROWS;
        const gcolptr xb = xp[2 * it + 1] + full_e * ROWQUAD_SLAB_ROWS;
        const bool b_real = (real >> (2 * it + 1)) & 1u;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          // rows at and past n count as null
          a[rr] = (row + rr < n) ? xa[rr] : nanv;
          b[rr] = (b_real && row + rr < n) ? xb[rr] : nanv;
        }
        stage(it, a, b);
      }
    }
    __syncthreads();
    read_frags();
    phase(full_e, pre0, false);
  }
}

int rowquad_cus() {
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
int launch_row_quadform(const float *const *cols, int64_t n, int k, const float *shift,
                        const float *scale, const uint16_t *wimg, int r_pad, int r0, int rw_pad,
                        int accumulate, int blocks, float *out, hipStream_t stream) {
  auto kern = row_quadform_kernel<KS>;
  const size_t lds = rowquad_z_bytes(KS * 32) + (size_t)rw_pad * rowquad_w_row_bytes(KS * 32);
  if (lds > (size_t)ROWQUAD_LDS_BYTES) return (int)hipErrorInvalidValue;
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return (int)err;
  if (blocks <= 0) {
    // one wave of resident blocks, as anovos_pairwise_gram_grid
    int per_cu = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, reinterpret_cast<const void *>(kern), RQ_THREADS, lds);
    if (per_cu <= 0) per_cu = 1;
    blocks = per_cu * rowquad_cus();
  }
  const int64_t macro_total = (n + ROWQUAD_SLAB_ROWS - 1) / ROWQUAD_SLAB_ROWS;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(blocks, macro_total));
  hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(RQ_THREADS), lds, stream, cols, n, k, shift,
                     scale, wimg, r_pad, r0, rw_pad, accumulate, out);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int anovos_row_quadform_split(const float *W, int r, int k, uint16_t *wimg,
                                         hipStream_t stream) {
  if (r < 1 || k < 1 || r > k || k > ROWQUAD_MAX_COLS) return (int)hipErrorInvalidValue;
  const int r_pad = rowquad_rpad(r), k_pad = rowquad_kpad(k);
  const int total = k_pad / 8 * r_pad;
  hipLaunchKernelGGL(row_quadform_split_kernel, dim3((uint32_t)((total + RQ_THREADS - 1) / RQ_THREADS)),
                     dim3(RQ_THREADS), 0, stream, W, r, k, r_pad, k_pad, wimg);
  return (int)hipGetLastError();
}

extern "C" int anovos_row_quadform(const void *const *cols, int64_t n, int k, const float *shift,
                                   const float *scale, const uint16_t *wimg, int r, int r0,
                                   int rw_pad, int accumulate, int blocks, float *out,
                                   hipStream_t stream) {
  const int r_pad = rowquad_rpad(r);
  if (n < 1 || k < 1 || k > ROWQUAD_MAX_COLS || r < 1 || r > k || r0 < 0 || rw_pad < 16 ||
      (r0 | rw_pad) % 16 != 0 || r0 + rw_pad > r_pad)
    return (int)hipErrorInvalidValue;
  const float *const *c = (const float *const *)cols;
  switch (rowquad_kpad(k) / 32) {
    case 1: return launch_row_quadform<1>(c, n, k, shift, scale, wimg, r_pad, r0, rw_pad, accumulate, blocks, out, stream);
    case 2: return launch_row_quadform<2>(c, n, k, shift, scale, wimg, r_pad, r0, rw_pad, accumulate, blocks, out, stream);
    case 3: return launch_row_quadform<3>(c, n, k, shift, scale, wimg, r_pad, r0, rw_pad, accumulate, blocks, out, stream);
    case 4: return launch_row_quadform<4>(c, n, k, shift, scale, wimg, r_pad, r0, rw_pad, accumulate, blocks, out, stream);
    case 5: return launch_row_quadform<5>(c, n, k, shift, scale, wimg, r_pad, r0, rw_pad, accumulate, blocks, out, stream);
    case 6: return launch_row_quadform<6>(c, n, k, shift, scale, wimg, r_pad, r0, rw_pad, accumulate, blocks, out, stream);
    case 7: return launch_row_quadform<7>(c, n, k, shift, scale, wimg, r_pad, r0, rw_pad, accumulate, blocks, out, stream);
    case 8: return launch_row_quadform<8>(c, n, k, shift, scale, wimg, r_pad, r0, rw_pad, accumulate, blocks, out, stream);
  }
  return (int)hipErrorInvalidValue;
}
