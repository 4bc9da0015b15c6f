// K30: a three-layer ReLU MLP applied to every row on MFMA matrix cores, the
// hidden activations never leaving the register file - the encode step of
// the autoencoder (ops/mlp.py), written as n3 separate columns.
//
//   z_j = isnan(x_j) ? 0 : (x_j - shift_j) * scale_j     (f32, subtract then multiply)
//   a1  = relu(W1 z  + b1)      W1 [n1, d]
//   a2  = relu(W2 a1 + b2)      W2 [n2, n1]
//   y   =      W3 a2 + b3       W3 [n3, n2]
//   out_c[row] = y_c            n3 contiguous f32 columns
//
// Numerics: split bf16, three products, as K26 - K28. Every operand is
// hi + lo, hi = bf16(v) round-to-nearest-even, lo = bf16(v - hi); a layer
// accumulates wh.ah + wh.al + wl.ah on v_mfma_f32_16x16x32_bf16 in fp32, the
// wl.al term (2^-18 relative) is dropped. The bias is the accumulator's
// initial value; ReLU and the hi / lo split of the next layer's input run on
// the accumulator in registers.
//
// MFMA roles and the register hand-over. Layers 1 and 2 take A = a W tile
// (16 components x 32 inputs) and B = the activations (32 inputs x 16 rows),
// K26's arrangement: a lane's C registers hold, for the row (lane & 15), the
// components (lane >> 4) * 4 + reg of the tile. The next layer's B fragment
// wants, for the same row, the eight inputs of the k-group (lane >> 4) - and
// which inputs those are is free, as long as A agrees. So k-step s of the
// next layer is defined over the components 32 s .. 32 s + 31 with slot
// (g, j) standing for
//   j <  4: component 32 s + 4 g + j
//   j >= 4: component 32 s + 16 + 4 g + (j - 4)
// and two consecutive C tiles (2 s, 2 s + 1) are, after ReLU and the split,
// one hi and one lo B fragment in place: no LDS round trip, no cross-lane
// move. The weight image carries the columns of W2 and W3 in that order.
// Padding components have zero weights and zero bias and stay 0 through
// ReLU. Layer 3 swaps the roles as K27 does - the activation fragments serve
// unchanged as A, W3 is B - so a lane's accumulator holds four consecutive
// rows of one output column and the epilogue is K27's: one 16-byte
// nontemporal store per lane and tile; a lane whose four rows are not all
// below n stores element by element, and nothing at or beyond n is written.
//
// Weight image: built once per call by mlp_weight_image_kernel, hi and lo
// planes in fragment order, [stage][plane][k-step][lane][8] bf16, so a
// fragment is one 16-byte LDS read. A stage is one output tile with KS
// k-steps (KS = d_pad / 32, the one template parameter): one stage per tile
// of layer 1 (KS k-steps) and of layer 3 (n2 / 32 <= KS), and for layer 2,
// whose n1 / 32 k-steps can number 2 * KS, two stages per tile when they
// exceed KS. The biases follow as f32, 16 per tile. At d = 150 (n1 = 300,
// n2 = n3 = 75) that is 20 + 12 + 5 stages of 10 KiB - more than a CU's LDS,
// so the image is not resident: all blocks stream it from L2, once per
// 64-row slab, through a two-buffer LDS ring shared by the four waves (as
// K29's donor tiles): the loads of stage t + 1 are issued before the MFMAs
// of stage t and land in the other buffer after them, one barrier per
// stage. The stream wraps: the last stage of a slab prefetches stage 0 for
// the next. Small images take the same path.
//
// Who loads what. Vector memory loads of a wave return in order, so a wave
// that had both the frame's loads (HBM, a microsecond) and the ring's (L2)
// in flight would wait for the frame at every ring stage. They are kept
// apart: waves 2 and 3 move the ring (KS 16-byte chunks per thread and
// stage), waves 0 and 1 stage the next slab of x, in two rounds of 2 KS
// unguarded 16-byte nontemporal loads per thread (columns' first and second
// half of every k-step), issued a round ahead of their conversion, both
// sharing one register buffer. The conversion - standardize, split, write the
// two bf16 planes of K26's Z image (ROWQUAD_Z_SLOTS slotting) - is spread
// over the tiles of layers 1 and 3, between the products. Column pointers,
// shifts and scales live in LDS, not in registers. The one partial slab at
// the end of the frame is staged with guarded loads.
//
// Work split: persistent 256-thread blocks in one wave of resident blocks,
// each owning a contiguous range of 64-row slabs; wave w owns row tile w and
// keeps its z fragments (8 KS registers, dead after layer 1), a1 (16 KS) and
// a2 (8 KS) as fragments in registers. Tile loops run to the maximum of the
// instantiation behind block-uniform guards, so every register index is
// static. No atomics: the same call returns the same bits.
//
// Resources (hipcc -O3, gfx950, 256 threads): see docs/KERNELS.md, K30; no
// scratch in any instantiation.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "anovos_kernels.h"

// Compiled without the packed fp32 instructions, for the reason given in
// project_columns.hip: the staging step pairs two columns exactly as K27's
// does. The attribute has to be on every device function of the file,
// lambdas included; the barrier is a builtin (the runtime header's function
// carries the default target).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int ME_THREADS = 256;
constexpr int ME_ZSTRIDE = ROWQUAD_Z_SLOTS;

static_assert(MLP_SLAB_ROWS == 64 && ME_THREADS == 4 * 64, "one wave per 16-row tile");
static_assert(ME_ZSTRIDE == MLP_SLAB_ROWS + MLP_SLAB_ROWS / 16, "one spare slot per tile");
static_assert(MLP_MAX_COLS == 5 * 32, "KS = 1 .. 5");

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef float nat_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t nat_u4 __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1))) *gcolptr;
typedef const nat_u4 __attribute__((address_space(1))) *gvecptr;
typedef float __attribute__((address_space(1))) *goutptr;
typedef nat_f4 __attribute__((address_space(1))) *goutvecptr;

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

// Two C tiles of a layer (components 4 g + reg of tiles 2 s and 2 s + 1 of
// this lane's row) -> ReLU -> the hi and lo B fragments of k-step s of the
// next layer.
__device__ __forceinline__ void relu_split(const f32x4 &c0, const f32x4 &c1, bf16x8 &hi, bf16x8 &lo) {
  const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaxf(c[e], 0.f);
  uint32_t h[4], l[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    h[p] = pack_bf16(v[2 * p], v[2 * p + 1]);
    l[p] = pack_bf16(v[2 * p] - bf16_value(h[p] & 0xFFFFu), v[2 * p + 1] - bf16_value(h[p] >> 16));
  }
  hi = __builtin_bit_cast(bf16x8, nat_u4{h[0], h[1], h[2], h[3]});
  lo = __builtin_bit_cast(bf16x8, nat_u4{l[0], l[1], l[2], l[3]});
}

// One thread per (stage, k-step, lane) of the image: the eight inputs of
// slot group g = lane >> 4 of output component tile * 16 + (lane & 15), both
// planes. Layer 1 takes its inputs in natural order (column 32 s + 8 g + e),
// layers 2 and 3 in the order the C tiles of the layer before hand them
// over. Out-of-range rows and inputs are zero. The first 16 * (t1 + t2 + t3)
// threads also write one bias each.
__global__ __launch_bounds__(ME_THREADS) void mlp_weight_image_kernel(
    const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
    const float *b3, int d, int n1, int n2, int n3, int ks_count, int t1, int t2, int l2s, int t3,
    uint16_t *img) {
  const int t = blockIdx.x * ME_THREADS + threadIdx.x;
  const int ns = t1 + t2 * l2s + t3;
  if (t >= ns * ks_count * 64) return;
  if (t < (t1 + t2 + t3) * 16) {
    const int tile = t >> 4, i = t & 15;
    float b;
    if (tile < t1) {
      const int c = tile * 16 + i;
      b = c < n1 ? b1[c] : 0.f;
    } else if (tile < t1 + t2) {
      const int c = (tile - t1) * 16 + i;
      b = c < n2 ? b2[c] : 0.f;
    } else {
      const int c = (tile - t1 - t2) * 16 + i;
      b = c < n3 ? b3[c] : 0.f;
    }
    reinterpret_cast<float *>(img + (int64_t)ns * ks_count * 1024)[t] = b;
  }
  const int lane = t & 63;
  const int ks = (t >> 6) % ks_count;
  const int st = (t >> 6) / ks_count;
  const int m = lane & 15, g = lane >> 4;
  const float *W;
  int rows, width, row, s;
  if (st < t1) {
    W = W1, rows = n1, width = d, row = st * 16 + m, s = ks;
  } else if (st < t1 + t2 * l2s) {
    const int q = st - t1;
    W = W2, rows = n2, width = n1, row = (q / l2s) * 16 + m, s = (q % l2s) * ks_count + ks;
  } else {
    W = W3, rows = n3, width = n2, row = (st - t1 - t2 * l2s) * 16 + m, s = ks;
  }
  uint32_t h[4], l[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    float v[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = 2 * p + q;
      const int c = st < t1 ? 32 * s + 8 * g + e
                            : (e < 4 ? 32 * s + 4 * g + e : 32 * s + 16 + 4 * g + (e - 4));
      v[q] = (row < rows && c < width) ? W[(int64_t)row * width + c] : 0.f;
    }
    h[p] = pack_bf16(v[0], v[1]);
    l[p] = pack_bf16(v[0] - bf16_value(h[p] & 0xFFFFu), v[1] - bf16_value(h[p] >> 16));
  }
  uint16_t *const dst = img + ((int64_t)st * 2 * ks_count + ks) * 512 + lane * 8;
  *reinterpret_cast<nat_u4 *>(dst) = nat_u4{h[0], h[1], h[2], h[3]};
  *reinterpret_cast<nat_u4 *>(dst + ks_count * 512) = nat_u4{l[0], l[1], l[2], l[3]};
}

template <int KS>
__global__ __launch_bounds__(ME_THREADS, KS <= 2 ? 2 : 1) void mlp_encode_kernel(
    const float *const *cols, int64_t n, int d, const float *shift, const float *scale,
    const uint16_t *img, int t1, int t2, int l2s, int t3, int n3, float *const *outs) {
  extern __shared__ __attribute__((aligned(16))) short me_lds[];
  constexpr int OCT = 4 * KS;                   // column octets
  constexpr int ZPLANE = OCT * ME_ZSTRIDE * 8;  // shorts per Z plane
  constexpr int STAGE = KS * 1024;              // shorts per ring stage
  constexpr int NX = 2 * KS;                    // 16-byte loads per thread and round of x
  short *const zs = me_lds;
  short *const ring = me_lds + 2 * ZPLANE;
  float *const bias = reinterpret_cast<float *>(ring + 2 * STAGE);          // [8 KS tiles][16]
  uint64_t *const colp = reinterpret_cast<uint64_t *>(bias + 8 * KS * 16);  // [32 KS]
  uint64_t *const optr = colp + 32 * KS;                                    // [32 KS]
  float *const shf = reinterpret_cast<float *>(optr + 32 * KS);             // [32 KS]
  float *const scl = shf + 32 * KS;                                         // [32 KS]

  const int64_t macro_total = (n + MLP_SLAB_ROWS - 1) / MLP_SLAB_ROWS;
  const int64_t macro_per = (macro_total + gridDim.x - 1) / gridDim.x;
  const int64_t mac_s = (int64_t)blockIdx.x * macro_per;
  const int64_t mac_e = min(macro_total, mac_s + macro_per);
  if (mac_s >= mac_e) return;  // whole block, before any barrier
  // slabs below full_e lie entirely below n; at most one more (the partial
  // one) follows, in the last non-empty block
  const int64_t full_e = min(mac_e, n / MLP_SLAB_ROWS);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool xw = wave < 2;   // stages x; the other two waves move the ring
  const int m = lane & 15;    // row of the tile (layers 1, 2: B, C) / component (layer 3: B, C)
  const int kog = lane >> 4;  // slot group of a k-step; 4-component (4-row) group of C
  const int k2 = t1 >> 1, k3 = t2 >> 1;  // k-steps of layers 2 and 3
  const int ns = t1 + t2 * l2s + t3;

  // ---- once per block: tables to LDS, the Z image cleared (a padding
  // column of a k-step is never written again) ----
  {
    const float *const gb = reinterpret_cast<const float *>(img + (int64_t)ns * STAGE);
    for (int i = threadIdx.x; i < (t1 + t2 + t3) * 16; i += ME_THREADS) bias[i] = gb[i];
    for (int i = threadIdx.x; i < 32 * KS; i += ME_THREADS) {
      const int c = min(i, d - 1);  // a padding column stands on a real one
      colp[i] = (uint64_t)(uintptr_t)cols[c];
      shf[i] = shift[c];
      scl[i] = scale[c];
      optr[i] = i < n3 ? (uint64_t)(uintptr_t)outs[i] : 0ull;
    }
    for (int i = threadIdx.x; i < 2 * ZPLANE / 8; i += ME_THREADS)
      reinterpret_cast<nat_u4 *>(zs)[i] = nat_u4{0u, 0u, 0u, 0u};
  }
  block_barrier();

  // ---- x staging (waves 0, 1): thread t of the 128 takes the 4-row
  // segment t & 15 of the slab and, in round h, the column pair
  // (t >> 4) + 8 h of every k-step ----
  const int seg = threadIdx.x & 15;
  const int pq8 = (threadIdx.x >> 4) & 7;
  nat_u4 pre[NX];  // x of one round (waves 0, 1) / the chunks of a ring stage (waves 2, 3)
  auto issue_x = [&](int h, int64_t slab) {
    const int64_t off = slab * MLP_SLAB_ROWS + seg * 4;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int col = (i >> 1) * 32 + (pq8 + 8 * h) * 2 + (i & 1);
      pre[i] = __builtin_nontemporal_load((gvecptr)((gcolptr)(uintptr_t)colp[col] + off));
    }
  };
  // one pair of one k-step: 4 rows x 2 columns -> both planes
  auto stage = [&](int h, int it, const float (&a)[4], const float (&b)[4]) {
    const int pq = pq8 + 8 * h;
    const int col = it * 32 + pq * 2;
    short *const dst =
        zs + ((((pq >> 2) + it * 4) * ME_ZSTRIDE + seg * 4 + (seg >> 2)) * 8 + (pq & 3) * 2);
    const float sa = shf[col], ca = scl[col], sb = shf[col + 1], cb = scl[col + 1];
    const bool b_real = col + 1 < d;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const float za = isnan(a[rr]) ? 0.f : (a[rr] - sa) * ca;
      const float zb = (!b_real || isnan(b[rr])) ? 0.f : (b[rr] - sb) * cb;
      const uint32_t hw = pack_bf16(za, zb);
      const uint32_t lw = pack_bf16(za - bf16_value(hw & 0xFFFFu), zb - bf16_value(hw >> 16));
      *reinterpret_cast<uint32_t *>(dst + rr * 8) = hw;
      *reinterpret_cast<uint32_t *>(dst + ZPLANE + rr * 8) = lw;
    }
  };
  auto convert_step = [&](int h, int it) {
    if (it * 32 + (pq8 + 8 * h) * 2 < d) {
      const nat_f4 va = __builtin_bit_cast(nat_f4, pre[2 * it]);
      const nat_f4 vb = __builtin_bit_cast(nat_f4, pre[2 * it + 1]);
      const float a[4] = {va.x, va.y, va.z, va.w};
      const float b[4] = {vb.x, vb.y, vb.z, vb.w};
      stage(h, it, a, b);
    }
  };
  // the partial slab: rows at and past n count as null
  auto stage_partial = [&](int64_t slab) {
    const int64_t row = slab * MLP_SLAB_ROWS + seg * 4;
    const float nanv = __builtin_nanf("");
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int it = 0; it < KS; ++it) {
        const int col = it * 32 + (pq8 + 8 * h) * 2;
        if (col < d) {
          const gcolptr xa = (gcolptr)(uintptr_t)colp[col] + row;
          const gcolptr xb = (gcolptr)(uintptr_t)colp[col + 1] + row;
          float a[4], b[4];
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            a[rr] = (row + rr < n) ? xa[rr] : nanv;
            b[rr] = (row + rr < n) ? xb[rr] : nanv;
          }
          stage(h, it, a, b);
        }
      }
    }
  };

  // ---- weight ring (waves 2, 3): KS chunks per thread and stage ----
  const int rchunk = (threadIdx.x & 127) * 8;
  auto issue_w = [&](int stage_index) {
    const uint16_t *const src = img + (int64_t)stage_index * STAGE + rchunk;
#pragma unroll
    for (int i = 0; i < KS; ++i) pre[i] = *reinterpret_cast<const nat_u4 *>(src + i * 1024);
  };
  auto land_w = [&](int buf) {
    short *const dst = ring + buf * STAGE + rchunk;
#pragma unroll
    for (int i = 0; i < KS; ++i) *reinterpret_cast<nat_u4 *>(dst + i * 1024) = pre[i];
  };
  int st = 0;   // stage of the image the buffer `par` holds
  int par = 0;
  // this lane's fragments of the current stage: plane p, k-step ks at
  // (p * KS + ks) * 512; the next stage is requested first
  auto stage_begin = [&]() -> const short * {
    if (!xw) issue_w(st + 1 == ns ? 0 : st + 1);
    return ring + par * STAGE + lane * 8;
  };
  auto stage_end = [&]() {
    if (!xw) land_w(par ^ 1);
    block_barrier();
    par ^= 1;
    st = st + 1 == ns ? 0 : st + 1;
  };

  // ---- first slab of the block and first stage of the image ----
  if (xw) {
    if (mac_s < full_e) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        issue_x(h, mac_s);
#pragma unroll
        for (int it = 0; it < KS; ++it) convert_step(h, it);
      }
    } else {
      stage_partial(mac_s);
    }
  } else {
    issue_w(0);
    land_w(0);
  }

  const short *const zbase = zs + (kog * ME_ZSTRIDE + wave * 17 + m) * 8;
  bf16x8 a1h[2 * KS], a1l[2 * KS], a2h[KS], a2l[KS];
#pragma unroll
  for (int s = 0; s < 2 * KS; ++s) a1h[s] = a1l[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < KS; ++s) a2h[s] = a2l[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};

  for (int64_t slab = mac_s; slab < mac_e; ++slab) {
    block_barrier();  // the slab (and, the first time, stage 0) is in LDS
    bf16x8 zh[KS], zl[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      zh[ks] = *reinterpret_cast<const bf16x8 *>(zbase + ks * 4 * ME_ZSTRIDE * 8);
      zl[ks] = *reinterpret_cast<const bf16x8 *>(zbase + ks * 4 * ME_ZSTRIDE * 8 + ZPLANE);
    }
    // The Z image is free once every wave has passed the barrier of the first
    // stage below; the conversions of the next slab come later than that.
    const bool conv = xw && slab + 1 < full_e;
    if (conv) issue_x(0, slab + 1);

    // ---- layer 1: a1 = relu(W1 z + b1) ----
    f32x4 held = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int T = 0; T < 4 * KS; ++T) {
      if (T < t1) {
        const short *const ap = stage_begin();
        f32x4 acc = *reinterpret_cast<const f32x4 *>(bias + T * 16 + kog * 4);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bf16x8 wh = *reinterpret_cast<const bf16x8 *>(ap + ks * 512);
          const bf16x8 wl = *reinterpret_cast<const bf16x8 *>(ap + (KS + ks) * 512);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, zh[ks], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, zl[ks], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, zh[ks], acc, 0, 0, 0);
        }
        if (T & 1)
          relu_split(held, acc, a1h[T >> 1], a1l[T >> 1]);
        else
          held = acc;
        stage_end();
      }
      // first round of the next slab's x: converted over the third quarter
      // of the tiles, then the second round is requested
      if (T >= 2 * KS && T < 3 * KS && conv) convert_step(0, T - 2 * KS);
      if (T == 3 * KS - 1 && conv) issue_x(1, slab + 1);
    }

    // ---- layer 2: a2 = relu(W2 a1 + b2) ----
#pragma unroll
    for (int T = 0; T < 2 * KS; ++T) {
      if (T < t2) {
        f32x4 acc = *reinterpret_cast<const f32x4 *>(bias + (t1 + T) * 16 + kog * 4);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          if (hf < l2s) {
            const short *const ap = stage_begin();
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
              if (hf * KS + ks < k2) {
                const bf16x8 wh = *reinterpret_cast<const bf16x8 *>(ap + ks * 512);
                const bf16x8 wl = *reinterpret_cast<const bf16x8 *>(ap + (KS + ks) * 512);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, a1h[hf * KS + ks], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, a1l[hf * KS + ks], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, a1h[hf * KS + ks], acc, 0, 0, 0);
              }
            }
            stage_end();
          }
        }
        if (T & 1)
          relu_split(held, acc, a2h[T >> 1], a2l[T >> 1]);
        else
          held = acc;
      }
    }

    // ---- layer 3: y = W3 a2 + b3, four rows of one column per lane ----
    const int64_t row = slab * MLP_SLAB_ROWS + wave * 16 + kog * 4;
#pragma unroll
    for (int T = 0; T < 2 * KS; ++T) {
      if (T < t3) {
        const short *const bp = stage_begin();
        const float b = bias[(t1 + t2 + T) * 16 + m];
        f32x4 acc = f32x4{b, b, b, b};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          if (ks < k3) {
            const bf16x8 wh = *reinterpret_cast<const bf16x8 *>(bp + ks * 512);
            const bf16x8 wl = *reinterpret_cast<const bf16x8 *>(bp + (KS + ks) * 512);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2h[ks], wh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2l[ks], wh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2h[ks], wl, acc, 0, 0, 0);
          }
        }
        const uint64_t p = optr[T * 16 + m];
        if (p != 0) {  // else a padding component
          const goutptr o = (goutptr)(uintptr_t)p + row;
          if (row + 4 <= n) {
            __builtin_nontemporal_store(nat_f4{acc.x, acc.y, acc.z, acc.w}, (goutvecptr)o);
          } else {
            if (row < n) o[0] = acc.x;
            if (row + 1 < n) o[1] = acc.y;
            if (row + 2 < n) o[2] = acc.z;
          }
        }
        stage_end();
      }
      // second round of the next slab's x
      if (T < KS && conv) convert_step(1, T);
    }
    if (xw && slab + 1 == full_e && slab + 1 < mac_e) stage_partial(slab + 1);
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

int mlp_cus() {
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
int launch_mlp_encode(const float *const *cols, int64_t n, int d, const float *shift,
                      const float *scale, const uint16_t *img, int n1, int n2, int n3, int blocks,
                      float *const *outs, hipStream_t stream) {
  auto kern = mlp_encode_kernel<KS>;
  // Z slab, two ring stages, biases, and per padded column a pointer, an
  // output pointer, a shift and a scale
  const size_t lds = rowquad_z_bytes(KS * 32) + 2 * (size_t)mlp_stage_shorts(KS * 32) * 2 +
                     8 * KS * 16 * 4 + 32 * KS * (8 + 8 + 4 + 4);
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return (int)err;
  if (blocks <= 0) {
    // one wave of resident blocks, as K26
    int per_cu = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, reinterpret_cast<const void *>(kern), ME_THREADS, lds);
    if (per_cu <= 0) per_cu = 1;
    blocks = per_cu * mlp_cus();
  }
  const int64_t macro_total = (n + MLP_SLAB_ROWS - 1) / MLP_SLAB_ROWS;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(blocks, macro_total));
  hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(ME_THREADS), lds, stream, cols, n, d, shift,
                     scale, img, mlp_tiles12(n1), mlp_tiles12(n2), mlp_l2_stages(d, n1),
                     mlp_tiles3(n3), n3, outs);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int anovos_mlp_weight_image(const float *W1, const float *b1, const float *W2,
                                       const float *b2, const float *W3, const float *b3, int d,
                                       int n1, int n2, int n3, uint16_t *img, hipStream_t stream) {
  if (!mlp_widths_ok(d, n1, n2, n3)) return (int)hipErrorInvalidValue;
  const int total = mlp_stages(d, n1, n2, n3) * mlp_ks(d) * 64;
  hipLaunchKernelGGL(mlp_weight_image_kernel, dim3((uint32_t)((total + ME_THREADS - 1) / ME_THREADS)),
                     dim3(ME_THREADS), 0, stream, W1, b1, W2, b2, W3, b3, d, n1, n2, n3, mlp_ks(d),
                     mlp_tiles12(n1), mlp_tiles12(n2), mlp_l2_stages(d, n1), mlp_tiles3(n3), img);
  return (int)hipGetLastError();
}

extern "C" int anovos_mlp_encode(const void *const *cols, int64_t n, int d, const float *shift,
                                 const float *scale, const uint16_t *img, int n1, int n2, int n3,
                                 int blocks, float *const *outs, hipStream_t stream) {
  if (n < 1 || !mlp_widths_ok(d, n1, n2, n3)) return (int)hipErrorInvalidValue;
  const float *const *c = (const float *const *)cols;
  switch (mlp_ks(d)) {
    case 1: return launch_mlp_encode<1>(c, n, d, shift, scale, img, n1, n2, n3, blocks, outs, stream);
    case 2: return launch_mlp_encode<2>(c, n, d, shift, scale, img, n1, n2, n3, blocks, outs, stream);
    case 3: return launch_mlp_encode<3>(c, n, d, shift, scale, img, n1, n2, n3, blocks, outs, stream);
    case 4: return launch_mlp_encode<4>(c, n, d, shift, scale, img, n1, n2, n3, blocks, outs, stream);
    case 5: return launch_mlp_encode<5>(c, n, d, shift, scale, img, n1, n2, n3, blocks, outs, stream);
  }
  return (int)hipErrorInvalidValue;
}
