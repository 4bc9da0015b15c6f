// K32: the two halves of an ALS-WR sweep of matrix-factorization imputation
// (ops/als.py states the method), one kernel per half.
//
//   m_rj = !isnan(x_rj),  z_rj = m_rj ? ((x_rj - mh_j) - ml_j) * s_j : 0     (f32)
//   row half:     A_r = sum_j m_rj v_j v_j^T,  b_r = sum_j z_rj v_j,
//                 u_r = (A_r + reg max(n_r, 1) I)^-1 b_r
//   column half:  H_j = sum_r m_rj u_r u_r^T,  g_j = sum_r z_rj u_r
//
// The rank pads to KR in {4, 8, 12, 16}, a template parameter; a padding
// component has v = 0, hence a diagonal of reg n, a zero right-hand side and
// u = 0. A symmetric KR x KR matrix travels as its T = KR (KR + 1) / 2 lower
// entries, (a, b) with a >= b at a (a + 1) / 2 + b, followed by the KR entries
// of the right-hand side: NT = T + KR numbers per row, or per column.
//
// Both kernels run on v_mfma_f32_16x16x32_bf16 with operands split as in
// K26 - K31 (hi = bf16(v), lo = bf16(v - hi)). The mask plane M is 0 / 1 and
// exact in bf16, so a masked product v_a v_b (u_a u_b) is formed ONCE in f32,
// split, and multiplied with M in two products (hi, lo); the right-hand
// sides take the three products hi.hi + hi.lo + lo.hi of K26 / K28.
//
// als_row_kernel<KR> (row half, one read of the frame). K26's / K31's block
// skeleton: persistent 256-thread blocks in one wave of resident blocks, each
// owning a contiguous range of 64-row slabs; unguarded 16-byte nontemporal
// loads and one guarded partial slab; x staged into K26's Z image with a
// third plane for M. The entries are dealt in tiles of 16: TP = ceil((T + 1)
// / 16) tiles of products against M - the spare slot T holds ones, so n_r
// comes out of the same products, exact - and one tile of V against Z. The
// image, [tile][plane][k-step][lane][8] bf16 in A-fragment order, is built
// once per call by als_row_image_kernel and read from L2 straight into
// registers, the next fragments requested before this step's products: at
// KR = 16, m = 160 it is 100 KiB, which does not fit beside the slab (65 KiB)
// and the patch (41 KiB). Tile t goes to wave t & 3, which multiplies it with
// all four row tiles and writes the accumulators to the LDS patch
// P[64][16 TT + 1] f32. One barrier; then the four lanes (lane & 15, lane >>
// 4 = q) of a row solve it: a right-looking Cholesky over the packed triangle
// in registers, lane q owning the columns c = q (mod 4), the pivot column
// broadcast inside the quad (ds_bpermute), the forward substitution riding
// on the broadcast columns, the back substitution one broadcast per
// component. All of it unrolls at compile-time KR. Outputs: U as KR f32
// component columns (transposed through LDS, one 16-byte store per lane and
// four rows); fmaf(u . v_j, sd_j, mh_j) into outs[j] at the null entries only
// (V as f32 in LDS; the M plane still in LDS names the nulls); the patch
// before the regulariser (normal). No atomics: the same call returns the
// same bits.
//
// als_col_kernel<KR> (column half). The reduction runs over rows, so the
// layout is K25's / K28's: 16-column tiles in groups of 4, a block owns one
// group and one contiguous range of 64-row macro-slabs (2 k-steps), wave w
// owns column tile w. Staged per macro-slab, all as [k-step][ko-group][slots
// + 3][8 rows] bf16: the frame's planes M, Zh, Zl (64 slots); U's slab as f32
// [KR][64 + 4]; from it the products u_a u_b (f32, then split) and U itself
// as hi / lo planes of 16 TT entry slots. Per entry tile M x (UU)h + M x (UU)l,
// and for the U tile Zh.Uh + Zh.Ul + Zl.Uh. K28's flush rule with a chain of
// exactly one macro-slab: the fp32 accumulator of at most 64 rows is added
// into an fp64 shadow the lane owns. Blocks write fp64 partials, a second
// kernel sums the row chunks in ascending order: no floating-point atomic.
//
// Resources (hipcc -O3, gfx950, 256 threads): see docs/KERNELS.md, K32; no
// scratch in any instantiation.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "anovos_kernels.h"

// Compiled without the packed fp32 instructions, for the reason given in
// project_columns.hip: the staging steps pair neighbouring rows and columns.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_ZSTRIDE = ROWQUAD_Z_SLOTS;
constexpr int AL_MAXKS = ALS_MAX_COLS / 32;
constexpr uint32_t BF16_ONE = 0x3F80u;

static_assert(ALS_SLAB_ROWS == 64 && AL_THREADS == 4 * 64, "one wave per 16-row tile");
static_assert(AL_ZSTRIDE == ALS_SLAB_ROWS + ALS_SLAB_ROWS / 16, "one spare slot per tile");
static_assert(ALS_MAX_COLS == 5 * 32 && ALS_MAX_RANK == 16, "KS = 1 .. 5, KR = 4 .. 16");

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef uint32_t nat_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t nat_u2 __attribute__((ext_vector_type(2)));
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

// four values -> their 8-byte entries of a hi and a lo plane
__device__ __forceinline__ void split4(float v0, float v1, float v2, float v3, short *hi,
                                       short *lo) {
  const uint32_t h01 = pack_bf16(v0, v1), h23 = pack_bf16(v2, v3);
  const uint32_t l01 = pack_bf16(v0 - bf16_value(h01 & 0xFFFFu), v1 - bf16_value(h01 >> 16));
  const uint32_t l23 = pack_bf16(v2 - bf16_value(h23 & 0xFFFFu), v3 - bf16_value(h23 >> 16));
  *reinterpret_cast<nat_u2 *>(hi) = nat_u2{h01, h23};
  *reinterpret_cast<nat_u2 *>(lo) = nat_u2{l01, l23};
}

// __syncthreads()
__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// v of the lane whose byte address (lane * 4) is src
__device__ __forceinline__ float lane_get(float v, int src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// (a, b), a >= b, of the packed index e
__device__ __forceinline__ void unpack_pair(int e, int &a, int &b) {
  a = 0;
  while ((a + 1) * (a + 2) / 2 <= e) ++a;
  b = e - a * (a + 1) / 2;
}

// ---------------------------------------------------------------------------
// row half
// ---------------------------------------------------------------------------

// One thread per (tile, k-step, lane) of the image: the eight columns of
// k-group lane >> 4 of entry tile * 16 + (lane & 15), both planes. V is f32
// [m, KR]. Product tiles: v_ja v_jb in f32 at the packed entries, ones at
// entry T, zero beyond; the last tile holds V. Padding columns are zero.
__global__ __launch_bounds__(AL_THREADS) void als_row_image_kernel(const float *V, int m, int KR,
                                                                   int ks_count, uint16_t *img) {
  const int T = als_tri(KR), TT = als_tiles(KR);
  const int t = blockIdx.x * AL_THREADS + threadIdx.x;
  if (t >= TT * ks_count * 64) return;
  const int lane = t & 63;
  const int ks = (t >> 6) % ks_count;
  const int tile = (t >> 6) / ks_count;
  const int e = tile * 16 + (lane & 15), g = lane >> 4;
  int a = 0, b = 0;
  if (tile < TT - 1 && e < T) unpack_pair(e, a, b);
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = 32 * ks + 8 * g + i;
    float x = 0.f;
    if (c < m) {
      if (tile == TT - 1) x = (lane & 15) < KR ? V[c * KR + (lane & 15)] : 0.f;
      else if (e < T) x = V[c * KR + a] * V[c * KR + b];
      else if (e == T) x = 1.f;
    }
    v[i] = x;
  }
  uint16_t *const dst = img + ((int64_t)tile * 2 * ks_count + ks) * 512 + lane * 8;
  split4(v[0], v[1], v[2], v[3], reinterpret_cast<short *>(dst),
         reinterpret_cast<short *>(dst + ks_count * 512));
  split4(v[4], v[5], v[6], v[7], reinterpret_cast<short *>(dst + 4),
         reinterpret_cast<short *>(dst + ks_count * 512 + 4));
}

// bytes of LDS of one block: Z image (three planes), patch, transposed U, V
// as f32, and per padded column two pointers and four floats
__host__ __device__ constexpr size_t als_row_lds_bytes(int ks, int kr) {
  return (size_t)3 * (4 * ks) * AL_ZSTRIDE * 16 + 64 * (als_tiles(kr) * 16 + 1) * 4 +
         (size_t)kr * 68 * 4 + (size_t)32 * ks * (kr + 1) * 4 + 32 * ks * (8 + 8 + 4 * 4);
}
static_assert(als_row_lds_bytes(5, 16) <= 160 * 1024, "one block fits a CU's LDS");

// Solves (A + lam I) u = b for one row, A and b in its patch row `pr`, by the
// four lanes of the row (q = lane >> 4; the quad's lane k is at byte address
// quad0 + 64 * k). Every lane returns all of u.
template <int KR>
__device__ __forceinline__ void als_solve(const float *pr, float lam, int q, int quad0,
                                          float (&u)[KR]) {
  constexpr int NC = KR / 4;
  constexpr int RHS = (als_tiles(KR) - 1) * 16;
  float col[NC][KR];  // slot s: column 4 s + q, rows below it; row i at [i]
  float y[KR];
#pragma unroll
  for (int s = 0; s < NC; ++s) {
    const int c = 4 * s + q;
#pragma unroll
    for (int i = 4 * s; i < KR; ++i) {
      float v = i >= c ? pr[i * (i + 1) / 2 + c] : 0.f;
      if (i == c) v += lam;
      col[s][i] = v;
    }
  }
#pragma unroll
  for (int i = 0; i < KR; ++i) y[i] = pr[RHS + i];

#pragma unroll
  for (int c = 0; c < KR; ++c) {
    const int cs = c / 4, cq = c % 4;
    const int src = quad0 + 64 * cq;
    float L[KR];
#pragma unroll
    for (int i = 0; i < KR; ++i) L[i] = i >= c ? lane_get(col[cs][i], src) : 0.f;
    const float d = sqrtf(L[c]);
    const float inv = 1.0f / d;
    // forward substitution on the column every lane now holds
    y[c] *= inv;
#pragma unroll
    for (int i = 0; i < KR; ++i) {
      if (i > c) {
        L[i] *= inv;
        y[i] = fmaf(-L[i], y[c], y[i]);
        if (q == cq) col[cs][i] = L[i];  // the owner keeps the finished column
      }
    }
    if (q == cq) col[cs][c] = d;
    L[c] = 0.f;  // from here L[i] = 0 for i <= c: columns up to c take no update
#pragma unroll
    for (int s = 0; s < NC; ++s) {
      if (s >= cs) {
        const float lq =
            q == 0 ? L[4 * s] : q == 1 ? L[4 * s + 1] : q == 2 ? L[4 * s + 2] : L[4 * s + 3];
#pragma unroll
        for (int i = 4 * s; i < KR; ++i)
          if (i > c) col[s][i] = fmaf(-L[i], lq, col[s][i]);
      }
    }
  }
  // back substitution: the owner's lane has the column, the quad gets u_c
#pragma unroll
  for (int c = KR - 1; c >= 0; --c) {
    const int cs = c / 4, cq = c % 4;
    float s = y[c];
#pragma unroll
    for (int i = 0; i < KR; ++i)
      if (i > c) s = fmaf(-col[cs][i], u[i], s);
    u[c] = lane_get(s / col[cs][c], quad0 + 64 * cq);
  }
}

template <int KR>
__global__ __launch_bounds__(AL_THREADS) void als_row_kernel(
    const float *const *cols, int64_t n, int m, int KS, const float *mean_hi, const float *mean_lo,
    const float *scale, const float *sd, const float *V, const uint16_t *img, float reg,
    float *const *outs, float *U, int64_t ldu, float *normal) {
  extern __shared__ __attribute__((aligned(16))) short al_lds[];
  constexpr int T = als_tri(KR);
  constexpr int TT = als_tiles(KR);
  constexpr int NT = T + KR;
  constexpr int PS = TT * 16 + 1;  // floats per row of the patch (odd)
  constexpr int VST = KR + 1;
  const int MP = 32 * KS;
  const int ZPLANE = 4 * KS * AL_ZSTRIDE * 8;  // shorts per plane
  short *const zs = al_lds;
  float *const Pp = reinterpret_cast<float *>(zs + 3 * ZPLANE);  // [64][PS]
  float *const Ut = Pp + 64 * PS;                                // [KR][68]
  float *const Vs = Ut + KR * 68;                                // [MP][VST]
  uint64_t *const colp = reinterpret_cast<uint64_t *>(Vs + MP * VST);
  uint64_t *const outp = colp + MP;
  float *const mhs = reinterpret_cast<float *>(outp + MP);
  float *const mls = mhs + MP;
  float *const scs = mls + MP;
  float *const sds = scs + MP;

  const int64_t macro_total = (n + ALS_SLAB_ROWS - 1) / ALS_SLAB_ROWS;
  const int64_t macro_per = (macro_total + gridDim.x - 1) / gridDim.x;
  const int64_t mac_s = (int64_t)blockIdx.x * macro_per;
  const int64_t mac_e = min64(macro_total, mac_s + macro_per);
  if (mac_s >= mac_e) return;  // whole block, before any barrier
  const int64_t full_e = min64(mac_e, n / ALS_SLAB_ROWS);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rw = lane & 15;   // row of a tile
  const int kog = lane >> 4;  // k-group of a k-step; entries 4 kog .. of C; lane of the quad

  // ---- once per block: tables and V to LDS, the Z image cleared ----
  for (int i = threadIdx.x; i < MP; i += AL_THREADS) {
    const int c = min(i, m - 1);  // a padding column stands on a real one
    colp[i] = (uint64_t)(uintptr_t)cols[c];
    outp[i] = (i < m && outs) ? (uint64_t)(uintptr_t)outs[i] : 0ull;
    mhs[i] = mean_hi[c];
    mls[i] = mean_lo[c];
    scs[i] = scale[c];
    sds[i] = sd[c];
  }
  for (int i = threadIdx.x; i < m * KR; i += AL_THREADS) Vs[(i / KR) * VST + i % KR] = V[i];
  for (int i = threadIdx.x; i < 3 * ZPLANE / 8; i += AL_THREADS)
    reinterpret_cast<nat_u4 *>(zs)[i] = nat_u4{0u, 0u, 0u, 0u};
  block_barrier();

  // ---- x staging: thread t takes the 4-row segment t & 15 of the slab and
  // the column pair t >> 4 of every k-step ----
  const int seg = threadIdx.x & 15;
  const int pq = threadIdx.x >> 4;
  auto stage = [&](int it, const float (&a)[4], const float (&b)[4]) {
    const int col = it * 32 + pq * 2;
    short *const dst =
        zs + ((((pq >> 2) + it * 4) * AL_ZSTRIDE + seg * 4 + (seg >> 2)) * 8 + (pq & 3) * 2);
    const float ha = mhs[col], la = mls[col], sa = scs[col];
    const float hb = mhs[col + 1], lb = mls[col + 1], sb = scs[col + 1];
    const bool b_real = col + 1 < m;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const bool na = isnan(a[rr]), nb = !b_real || isnan(b[rr]);
      const float za = na ? 0.f : ((a[rr] - ha) - la) * sa;
      const float zb = nb ? 0.f : ((b[rr] - hb) - lb) * sb;
      const uint32_t hw = pack_bf16(za, zb);
      const uint32_t lw = pack_bf16(za - bf16_value(hw & 0xFFFFu), zb - bf16_value(hw >> 16));
      *reinterpret_cast<uint32_t *>(dst + rr * 8) = hw;
      *reinterpret_cast<uint32_t *>(dst + ZPLANE + rr * 8) = lw;
      *reinterpret_cast<uint32_t *>(dst + 2 * ZPLANE + rr * 8) =
          (na ? 0u : BF16_ONE) | (nb ? 0u : BF16_ONE << 16);
    }
  };
  auto stage_full = [&](int64_t slab) {
    const int64_t off = slab * ALS_SLAB_ROWS + seg * 4;
    nat_u4 pre[2 * AL_MAXKS];
#pragma unroll
    for (int i = 0; i < 2 * AL_MAXKS; ++i) {
      // a padding column is neither loaded nor staged
      const int col = (i >> 1) * 32 + pq * 2 + (i & 1);
      pre[i] = nat_u4{0u, 0u, 0u, 0u};
      if ((i >> 1) < KS && col < m)
        pre[i] = __builtin_nontemporal_load((gvecptr)((gcolptr)(uintptr_t)colp[col] + off));
    }
#pragma unroll
    for (int it = 0; it < AL_MAXKS; ++it) {
      if (it < KS && it * 32 + pq * 2 < m) {
        const nat_f4 va = __builtin_bit_cast(nat_f4, pre[2 * it]);
        const nat_f4 vb = __builtin_bit_cast(nat_f4, pre[2 * it + 1]);
        const float a[4] = {va.x, va.y, va.z, va.w};
        const float b[4] = {vb.x, vb.y, vb.z, vb.w};
        stage(it, a, b);
      }
    }
  };
  // the partial slab: rows at and past n count as null
  auto stage_partial = [&](int64_t slab) {
    const int64_t row = slab * ALS_SLAB_ROWS + seg * 4;
    const float nanv = __builtin_nanf("");
    for (int it = 0; it < KS; ++it) {
      const int col = it * 32 + pq * 2;
      if (col < m) {
        const gcolptr xa = (gcolptr)(uintptr_t)colp[col] + row;
        const gcolptr xb = (gcolptr)(uintptr_t)colp[col + 1] + row;
        float a[4], b[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          a[rr] = (row + rr < n) ? xa[rr] : nanv;
          b[rr] = (row + rr < n) ? xb[rr] : nanv;
        }
        stage(it, a, b);
      }
    }
  };

  // this lane's A fragments of (tile, k-step)
  auto load_a = [&](int i, bf16x8 &h, bf16x8 &l) {
    const int tile = i / KS, ks = i - tile * KS;
    const uint16_t *const src = img + ((int64_t)tile * 2 * KS + ks) * 512 + lane * 8;
    h = *reinterpret_cast<const bf16x8 *>(src);
    l = *reinterpret_cast<const bf16x8 *>(src + KS * 512);
  };

  const int row = wave * 16 + rw;  // the row of the slab this lane's quad solves
  for (int64_t slab = mac_s; slab < mac_e; ++slab) {
    // ---- 1. stage the slab ----
    if (slab < full_e)
      stage_full(slab);
    else
      stage_partial(slab);
    block_barrier();

    // ---- 2. normal equations: tile t on wave t & 3 ----
    for (int tile = wave; tile < TT; tile += 4) {
      const bool vtile = tile == TT - 1;
      f32x4 acc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      bf16x8 ah, al;
      load_a(tile * KS, ah, al);
      for (int ks = 0; ks < KS; ++ks) {
        bf16x8 nh, nl;
        load_a(tile * KS + (ks + 1 < KS ? ks + 1 : ks), nh, nl);
        const short *const zb = zs + ((kog + ks * 4) * AL_ZSTRIDE + rw) * 8;
        if (vtile) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bf16x8 zh = *reinterpret_cast<const bf16x8 *>(zb + q * 17 * 8);
            const bf16x8 zl = *reinterpret_cast<const bf16x8 *>(zb + q * 17 * 8 + ZPLANE);
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, zh, acc[q], 0, 0, 0);
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, zl, acc[q], 0, 0, 0);
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, zh, acc[q], 0, 0, 0);
          }
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bf16x8 mb = *reinterpret_cast<const bf16x8 *>(zb + q * 17 * 8 + 2 * ZPLANE);
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, mb, acc[q], 0, 0, 0);
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, mb, acc[q], 0, 0, 0);
          }
        }
        ah = nh, al = nl;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float *const p = Pp + (q * 16 + rw) * PS + tile * 16 + kog * 4;
        p[0] = acc[q].x, p[1] = acc[q].y, p[2] = acc[q].z, p[3] = acc[q].w;
      }
    }
    block_barrier();

    const int64_t row0 = slab * ALS_SLAB_ROWS;
    if (normal) {
      const int live = (int)min64(ALS_SLAB_ROWS, n - row0);
      for (int i = threadIdx.x; i < live * NT; i += AL_THREADS) {
        const int r = i / NT, e = i - r * NT;
        normal[row0 * NT + i] = Pp[r * PS + (e < T ? e : (TT - 1) * 16 + e - T)];
      }
    }

    // ---- 3. the wave's 16 rows, four lanes each ----
    float u[KR];
    {
      const float *const pr = Pp + row * PS;
      const float lam = reg * fmaxf(pr[T], 1.f);
      als_solve<KR>(pr, lam, kog, rw * 4, u);
    }
#pragma unroll
    for (int a = 0; a < KR; ++a)
      if ((a & 3) == kog) Ut[a * 68 + row] = u[a];

    // ---- 4. the null entries of the row: columns kog, kog + 4, ... ----
    const int64_t grow = row0 + row;
    if (outs && grow < n) {
      const short *const mrow = zs + 2 * ZPLANE + (row + (row >> 4)) * 8;
      for (int j = kog; j < m; j += 4) {
        const uint64_t o = outp[j];
        if (o != 0 && mrow[(j >> 3) * AL_ZSTRIDE * 8 + (j & 7)] == 0) {
          float dot = 0.f;
#pragma unroll
          for (int a = 0; a < KR; ++a) dot = fmaf(u[a], Vs[j * VST + a], dot);
          ((goutptr)(uintptr_t)o)[grow] = fmaf(dot, sds[j], mhs[j]);
        }
      }
    }
    block_barrier();  // Ut complete; the patch and the Z image are free

    // ---- 5. U: component t >> 4 (+ 16), rows 4 (t & 15) .. + 3; U's columns
    // are padded to whole slabs, rows at and past n get u = 0 ----
    if (U) {
      for (int a = pq; a < KR; a += 16) {
        const nat_f4 v = *reinterpret_cast<const nat_f4 *>(Ut + a * 68 + seg * 4);
        *reinterpret_cast<nat_f4 *>(U + a * ldu + row0 + seg * 4) = v;
      }
    }
  }
}

int als_cus() {
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

template <int KR>
int launch_als_row(const float *const *cols, int64_t n, int m, const float *mean_hi,
                   const float *mean_lo, const float *scale, const float *sd, const float *V,
                   const uint16_t *img, float reg, int blocks, float *const *outs, float *U,
                   int64_t ldu, float *normal, hipStream_t stream) {
  auto kern = als_row_kernel<KR>;
  const int ks = als_ks(m);
  const size_t lds = als_row_lds_bytes(ks, KR);
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)als_row_lds_bytes(AL_MAXKS, KR));
  if (err != hipSuccess) return (int)err;
  if (blocks <= 0) {
    // one wave of resident blocks, as K26
    int per_cu = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, reinterpret_cast<const void *>(kern), AL_THREADS, lds);
    if (per_cu <= 0) per_cu = 1;
    blocks = per_cu * als_cus();
  }
  const int64_t macro_total = (n + ALS_SLAB_ROWS - 1) / ALS_SLAB_ROWS;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(blocks, macro_total));
  hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(AL_THREADS), lds, stream, cols, n, m, ks,
                     mean_hi, mean_lo, scale, sd, V, img, reg, outs, U, ldu, normal);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// column half
// ---------------------------------------------------------------------------

constexpr int AC_KSTRIDE = 64 + 3;                   // slots of a frame plane
constexpr int AC_FPLANE = 2 * 4 * AC_KSTRIDE * 8;    // shorts per frame plane
constexpr int AC_USTRIDE = 64 + 4;                   // floats per component of the U slab

__host__ __device__ constexpr int als_col_estride(int kr) { return als_tiles(kr) * 16 + 3; }
__host__ __device__ constexpr size_t als_col_lds_bytes(int kr) {
  return (size_t)3 * AC_FPLANE * 2 + (size_t)2 * 2 * 4 * als_col_estride(kr) * 16 +
         (size_t)kr * AC_USTRIDE * 4 + (als_tiles(kr) - 1) * 16;
}
static_assert(als_col_lds_bytes(ALS_MAX_RANK) <= 80 * 1024, "two blocks fit a CU's LDS");

template <int KR>
__global__ __launch_bounds__(AL_THREADS) void als_col_kernel(
    const float *const *cols, int64_t n, int m, const float *mean_hi, const float *mean_lo,
    const float *scale, const float *U, int64_t ldu, int groups, int row_chunks,
    double *partials) {
  constexpr int T = als_tri(KR);
  constexpr int TT = als_tiles(KR);
  constexpr int ES = als_col_estride(KR);
  constexpr int EPLANE = 2 * 4 * ES * 8;  // shorts per entry plane
  extern __shared__ __attribute__((aligned(16))) short al_lds[];
  short *const fr = al_lds;                                        // M, Zh, Zl
  short *const en = fr + 3 * AC_FPLANE;                            // hi, lo
  float *const us = reinterpret_cast<float *>(en + 2 * EPLANE);    // [KR][AC_USTRIDE]
  uint8_t *const pair_tab = reinterpret_cast<uint8_t *>(us + KR * AC_USTRIDE);  // a | b << 4, e < T

  // chunk-major: neighbouring blocks read the same rows for different groups
  const int g = blockIdx.x % groups;
  const int chunk = blockIdx.x / groups;
  const int64_t macro_total = (n + ALS_SLAB_ROWS - 1) / ALS_SLAB_ROWS;
  const int64_t macro_per = (macro_total + row_chunks - 1) / row_chunks;
  const int64_t mac_s = (int64_t)chunk * macro_per;
  const int64_t mac_e = min64(macro_total, mac_s + macro_per);
  const int64_t full_e = min64(mac_e, n / ALS_SLAB_ROWS);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int mi = lane & 15;
  const int kog = lane >> 4;
  const int seg = threadIdx.x & 15;  // 4-row segment of the macro-slab
  const int cw = threadIdx.x >> 4;   // local column (+ 16 it); entry of a tile; U component

  for (int e = threadIdx.x; e < (TT - 1) * 16; e += AL_THREADS) {
    int a = 0, b = 0;
    if (e < T) unpack_pair(e, a, b);
    pair_tab[e] = (uint8_t)(a | (b << 4));
  }

  // slot offset (shorts) of rows 4 seg .. + 3 at slot 0 of a plane of stride S
  auto seg_off = [&](int S) { return (((seg >> 3) * 4 + ((seg & 7) >> 1)) * S) * 8 + (seg & 1) * 4; };
  short *const fdst = fr + seg_off(AC_KSTRIDE) + cw * 8;
  short *const edst = en + seg_off(ES) + cw * 8;

  gcolptr xp[4];
  float mh[4], ml[4], sc[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    // a padding column stands on a real one; the reduction never reads it
    const int c = min(g * 64 + it * 16 + cw, m - 1);
    xp[it] = (gcolptr)cols[c] + seg * 4;
    mh[it] = mean_hi[c];
    ml[it] = mean_lo[c];
    sc[it] = scale[c];
  }
  const gcolptr up = (gcolptr)U + (int64_t)cw * ldu + seg * 4;  // cw < KR only
  const bool w_live = (g * 4 + wave) * 16 < m;

  f32x4 acc[TT];
  double sum[TT][4];
#pragma unroll
  for (int i = 0; i < TT; ++i) {
    acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[i][r] = 0.0;
  }

  nat_f4 xr[4], ur;
  // rows at and past n count as null, with u = 0
  auto load = [&](int64_t s) {
    const int64_t off = s * ALS_SLAB_ROWS;
    if (s < full_e) {
#pragma unroll
      for (int it = 0; it < 4; ++it)
        xr[it] = __builtin_bit_cast(nat_f4, __builtin_nontemporal_load((gvecptr)(xp[it] + off)));
      if (cw < KR) ur = __builtin_bit_cast(nat_f4, *(gvecptr)(up + off));
    } else {
      const int64_t r = off + seg * 4;
      const float nanv = __builtin_nanf("");
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const gcolptr x = xp[it] + off;
        xr[it] = nat_f4{r + 0 < n ? x[0] : nanv, r + 1 < n ? x[1] : nanv, r + 2 < n ? x[2] : nanv,
                        r + 3 < n ? x[3] : nanv};
      }
      if (cw < KR) {
        const gcolptr x = up + off;
        ur = nat_f4{r + 0 < n ? x[0] : 0.f, r + 1 < n ? x[1] : 0.f, r + 2 < n ? x[2] : 0.f,
                    r + 3 < n ? x[3] : 0.f};
      }
    }
  };

  if (mac_s < mac_e) load(mac_s);
  for (int64_t s = mac_s; s < mac_e; ++s) {
    block_barrier();  // the previous macro-slab's LDS reads are complete
    // ---- frame planes and the U slab ----
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const float x[4] = {xr[it].x, xr[it].y, xr[it].z, xr[it].w};
      float z[4];
      uint32_t mk[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool nul = isnan(x[r]);
        z[r] = nul ? 0.f : ((x[r] - mh[it]) - ml[it]) * sc[it];
        mk[r] = nul ? 0u : BF16_ONE;
      }
      short *const d = fdst + it * 16 * 8;
      *reinterpret_cast<nat_u2 *>(d) = nat_u2{mk[0] | mk[1] << 16, mk[2] | mk[3] << 16};
      split4(z[0], z[1], z[2], z[3], d + AC_FPLANE, d + 2 * AC_FPLANE);
    }
    if (cw < KR) *reinterpret_cast<nat_f4 *>(us + cw * AC_USTRIDE + seg * 4) = ur;
    block_barrier();
    if (s + 1 < mac_e) load(s + 1);

    // ---- entry planes: products u_a u_b, then U itself ----
#pragma unroll
    for (int i = 0; i < TT; ++i) {
      nat_f4 v = nat_f4{0.f, 0.f, 0.f, 0.f};
      if (i < TT - 1) {
        if (i * 16 + cw < T) {
          const int ab = pair_tab[i * 16 + cw];
          const nat_f4 ua = *reinterpret_cast<const nat_f4 *>(us + (ab & 15) * AC_USTRIDE + seg * 4);
          const nat_f4 ub = *reinterpret_cast<const nat_f4 *>(us + (ab >> 4) * AC_USTRIDE + seg * 4);
          v = nat_f4{ua.x * ub.x, ua.y * ub.y, ua.z * ub.z, ua.w * ub.w};
        }
      } else if (cw < KR) {
        v = *reinterpret_cast<const nat_f4 *>(us + cw * AC_USTRIDE + seg * 4);
      }
      short *const d = edst + i * 16 * 8;
      split4(v.x, v.y, v.z, v.w, d, d + EPLANE);
    }
    block_barrier();

    // ---- products of the macro-slab, then the flush ----
    if (w_live) {
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const short *const bp = fr + ((st * 4 + kog) * AC_KSTRIDE + wave * 16 + mi) * 8;
        const short *const ap = en + ((st * 4 + kog) * ES + mi) * 8;
        const bf16x8 bm = *reinterpret_cast<const bf16x8 *>(bp);
        const bf16x8 bh = *reinterpret_cast<const bf16x8 *>(bp + AC_FPLANE);
        const bf16x8 bl = *reinterpret_cast<const bf16x8 *>(bp + 2 * AC_FPLANE);
#pragma unroll
        for (int i = 0; i < TT; ++i) {
          const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(ap + i * 16 * 8);
          const bf16x8 al = *reinterpret_cast<const bf16x8 *>(ap + i * 16 * 8 + EPLANE);
          if (i < TT - 1) {
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bm, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bm, acc[i], 0, 0, 0);
          } else {
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc[i], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < TT; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[i][r] += (double)acc[i][r];
        acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }

  // C layout: entry = (lane >> 4) * 4 + reg, column = lane & 15; a block that
  // owns no macro-slab writes zeros
  if (w_live) {
    double *const out = partials + (((int64_t)chunk * groups + g) * 4 + wave) * TT * 256 +
                        kog * 4 * 16 + mi;
#pragma unroll
    for (int i = 0; i < TT; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[i * 256 + r * 16] = sum[i][r];
    }
  }
}

// One thread per (column, entry): chunk sums in ascending order, fp64.
__global__ __launch_bounds__(AL_THREADS) void als_col_reduce_kernel(const double *partials,
                                                                    int row_chunks, int groups,
                                                                    int m, int KR, double *out) {
  const int T = als_tri(KR), TT = als_tiles(KR), NT = T + KR;
  const int t = blockIdx.x * AL_THREADS + threadIdx.x;
  if (t >= m * NT) return;
  const int j = t / NT, e = t - j * NT;
  const int tile = e < T ? e / 16 : TT - 1, ent = e < T ? e % 16 : e - T;
  const int64_t at = ((int64_t)((j / 64) * 4 + (j % 64) / 16) * TT + tile) * 256 + ent * 16 + j % 16;
  double s = 0.0;
  for (int ch = 0; ch < row_chunks; ++ch) s += partials[(int64_t)ch * groups * 4 * TT * 256 + at];
  out[t] = s;
}

template <int KR>
int launch_als_col(const float *const *cols, int64_t n, int m, const float *mean_hi,
                   const float *mean_lo, const float *scale, const float *U, int64_t ldu,
                   int row_chunks, double *partials, double *out, hipStream_t stream) {
  const int groups = als_groups(m);
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(als_col_kernel<KR>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)als_col_lds_bytes(KR));
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(als_col_kernel<KR>, dim3((uint32_t)groups * (uint32_t)row_chunks),
                     dim3(AL_THREADS), als_col_lds_bytes(KR), stream, cols, n, m, mean_hi, mean_lo, scale, U, ldu,
                     groups, row_chunks, partials);
  const int total = m * (als_tri(KR) + KR);
  hipLaunchKernelGGL(als_col_reduce_kernel, dim3((uint32_t)((total + AL_THREADS - 1) / AL_THREADS)),
                     dim3(AL_THREADS), 0, stream, partials, row_chunks, groups, m, KR, out);
  return (int)hipGetLastError();
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" int anovos_als_row_image(const float *V, int m, int kr, uint16_t *img,
                                    hipStream_t stream) {
  if (!als_shape_ok(m, kr)) return (int)hipErrorInvalidValue;
  const int total = als_tiles(kr) * als_ks(m) * 64;
  hipLaunchKernelGGL(als_row_image_kernel, dim3((uint32_t)((total + AL_THREADS - 1) / AL_THREADS)),
                     dim3(AL_THREADS), 0, stream, V, m, kr, als_ks(m), img);
  return (int)hipGetLastError();
}

extern "C" int anovos_als_row_solve(const void *const *cols, int64_t n, int m, int kr,
                                    const float *mean_hi, const float *mean_lo, const float *scale,
                                    const float *sd, const float *V, const uint16_t *img, float reg,
                                    int blocks, float *const *outs, float *U, int64_t ldu,
                                    float *normal, hipStream_t stream) {
  if (n < 1 || !als_shape_ok(m, kr) || !(reg > 0.f)) return (int)hipErrorInvalidValue;
  if (U && (ldu % ALS_SLAB_ROWS != 0 || ldu < n)) return (int)hipErrorInvalidValue;
  const float *const *c = (const float *const *)cols;
  switch (kr) {
    case 4: return launch_als_row<4>(c, n, m, mean_hi, mean_lo, scale, sd, V, img, reg, blocks, outs, U, ldu, normal, stream);
    case 8: return launch_als_row<8>(c, n, m, mean_hi, mean_lo, scale, sd, V, img, reg, blocks, outs, U, ldu, normal, stream);
    case 12: return launch_als_row<12>(c, n, m, mean_hi, mean_lo, scale, sd, V, img, reg, blocks, outs, U, ldu, normal, stream);
    case 16: return launch_als_row<16>(c, n, m, mean_hi, mean_lo, scale, sd, V, img, reg, blocks, outs, U, ldu, normal, stream);
  }
  return (int)hipErrorInvalidValue;
}

extern "C" int anovos_als_col_normal(const void *const *cols, int64_t n, int m, int kr,
                                     const float *mean_hi, const float *mean_lo, const float *scale,
                                     const float *U, int64_t ldu, int row_chunks, double *partials,
                                     double *out, hipStream_t stream) {
  if (n < 1 || !als_shape_ok(m, kr) || row_chunks < 1 || ldu % 4 != 0 || ldu < n)
    return (int)hipErrorInvalidValue;
  const float *const *c = (const float *const *)cols;
  switch (kr) {
    case 4: return launch_als_col<4>(c, n, m, mean_hi, mean_lo, scale, U, ldu, row_chunks, partials, out, stream);
    case 8: return launch_als_col<8>(c, n, m, mean_hi, mean_lo, scale, U, ldu, row_chunks, partials, out, stream);
    case 12: return launch_als_col<12>(c, n, m, mean_hi, mean_lo, scale, U, ldu, row_chunks, partials, out, stream);
    case 16: return launch_als_col<16>(c, n, m, mean_hi, mean_lo, scale, U, ldu, row_chunks, partials, out, stream);
  }
  return (int)hipErrorInvalidValue;
}

extern "C" int anovos_als_col_grid(int kr) {
  // one wave of resident blocks
  const void *f = kr == 4    ? reinterpret_cast<const void *>(als_col_kernel<4>)
                  : kr == 8  ? reinterpret_cast<const void *>(als_col_kernel<8>)
                  : kr == 12 ? reinterpret_cast<const void *>(als_col_kernel<12>)
                             : reinterpret_cast<const void *>(als_col_kernel<16>);
  int per_cu = 0;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, AL_THREADS, als_col_lds_bytes(kr));
  if (per_cu <= 0) per_cu = 1;
  return per_cu * als_cus();
}
