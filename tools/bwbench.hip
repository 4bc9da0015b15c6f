// Streaming-bandwidth microbenchmark for the engine's out-of-place
// column kernels (fillnan/axpb/bucketize/clamp shapes). Measures
// effective read+write TB/s for several loop shapes on gfx950 so the
// production kernels copy at the measured ceiling (~6.3 TB/s float4
// copy per MI355X_MICROARCH.md) instead of ~4.5.
//
// Build: hipcc --offload-arch=gfx950 -O3 tools/bwbench.hip -o gpurun_out/bwbench
// Run:   ./gpurun_out/bwbench

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdint>
#include <cstdlib>

#define CHECK(x)                                                              \
  do {                                                                        \
    hipError_t e = (x);                                                       \
    if (e != hipSuccess) {                                                    \
      printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__);         \
      return 1;                                                               \
    }                                                                         \
  } while (0)

constexpr int THREADS = 256;

// v1: the current production shape — per-block contiguous span, one
// float4 per lane per iteration
__global__ __launch_bounds__(THREADS) void k_copy_v1(const float *__restrict__ x,
                                                     float *__restrict__ out,
                                                     int64_t n, int nchunks) {
  const int chunk = blockIdx.x;
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  const float4 *xv = reinterpret_cast<const float4 *>(x + s);
  float4 *ov = reinterpret_cast<float4 *>(out + s);
  const int64_t nv = (e - s) / 4;
  for (int64_t i = threadIdx.x; i < nv; i += THREADS) ov[i] = xv[i];
}

// v2: two float4 in flight per lane (explicit 2x unroll)
__global__ __launch_bounds__(THREADS) void k_copy_v2(const float *__restrict__ x,
                                                     float *__restrict__ out,
                                                     int64_t n, int nchunks) {
  const int chunk = blockIdx.x;
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  const float4 *__restrict__ xv = reinterpret_cast<const float4 *>(x + s);
  float4 *__restrict__ ov = reinterpret_cast<float4 *>(out + s);
  const int64_t nv = (e - s) / 4;
  int64_t i = threadIdx.x;
  for (; i + THREADS < nv; i += 2 * THREADS) {
    float4 a = xv[i];
    float4 b = xv[i + THREADS];
    ov[i] = a;
    ov[i + THREADS] = b;
  }
  for (; i < nv; i += THREADS) ov[i] = xv[i];
}

// v4: four float4 in flight per lane
__global__ __launch_bounds__(THREADS) void k_copy_v4(const float *__restrict__ x,
                                                     float *__restrict__ out,
                                                     int64_t n, int nchunks) {
  const int chunk = blockIdx.x;
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  const float4 *__restrict__ xv = reinterpret_cast<const float4 *>(x + s);
  float4 *__restrict__ ov = reinterpret_cast<float4 *>(out + s);
  const int64_t nv = (e - s) / 4;
  int64_t i = threadIdx.x;
  for (; i + 3 * THREADS < nv; i += 4 * THREADS) {
    float4 a = xv[i];
    float4 b = xv[i + THREADS];
    float4 c = xv[i + 2 * THREADS];
    float4 d = xv[i + 3 * THREADS];
    ov[i] = a;
    ov[i + THREADS] = b;
    ov[i + 2 * THREADS] = c;
    ov[i + 3 * THREADS] = d;
  }
  for (; i < nv; i += THREADS) ov[i] = xv[i];
}

// v2nt: 2x unroll + non-temporal load/store (needs the native ext
// vector type, HIP_vector_type is not accepted by the builtin)
typedef float nat_f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(THREADS) void k_copy_v2nt(const float *__restrict__ x,
                                                       float *__restrict__ out,
                                                       int64_t n, int nchunks) {
  const int chunk = blockIdx.x;
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  const nat_f4 *__restrict__ xv = reinterpret_cast<const nat_f4 *>(x + s);
  nat_f4 *__restrict__ ov = reinterpret_cast<nat_f4 *>(out + s);
  const int64_t nv = (e - s) / 4;
  int64_t i = threadIdx.x;
  for (; i + THREADS < nv; i += 2 * THREADS) {
    nat_f4 a = __builtin_nontemporal_load(&xv[i]);
    nat_f4 b = __builtin_nontemporal_load(&xv[i + THREADS]);
    __builtin_nontemporal_store(a, &ov[i]);
    __builtin_nontemporal_store(b, &ov[i + THREADS]);
  }
  for (; i < nv; i += THREADS) {
    nat_f4 a = xv[i];
    ov[i] = a;
  }
}

// v2 with the fillnan select, to price the ALU work
__global__ __launch_bounds__(THREADS) void k_fill_v2(const float *__restrict__ x,
                                                     float *__restrict__ out,
                                                     int64_t n, int nchunks) {
  const int chunk = blockIdx.x;
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  const float4 *__restrict__ xv = reinterpret_cast<const float4 *>(x + s);
  float4 *__restrict__ ov = reinterpret_cast<float4 *>(out + s);
  const int64_t nv = (e - s) / 4;
  const float ff = 0.5f;
  int64_t i = threadIdx.x;
  for (; i + THREADS < nv; i += 2 * THREADS) {
    float4 a = xv[i];
    float4 b = xv[i + THREADS];
    a.x = isnan(a.x) ? ff : a.x; a.y = isnan(a.y) ? ff : a.y;
    a.z = isnan(a.z) ? ff : a.z; a.w = isnan(a.w) ? ff : a.w;
    b.x = isnan(b.x) ? ff : b.x; b.y = isnan(b.y) ? ff : b.y;
    b.z = isnan(b.z) ? ff : b.z; b.w = isnan(b.w) ? ff : b.w;
    ov[i] = a;
    ov[i + THREADS] = b;
  }
  for (; i < nv; i += THREADS) ov[i] = xv[i];
}

// v1 at 1024 threads per block
__global__ __launch_bounds__(1024) void k_copy_t1024(const float *__restrict__ x,
                                                     float *__restrict__ out,
                                                     int64_t n, int nchunks) {
  const int chunk = blockIdx.x;
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  const float4 *__restrict__ xv = reinterpret_cast<const float4 *>(x + s);
  float4 *__restrict__ ov = reinterpret_cast<float4 *>(out + s);
  const int64_t nv = (e - s) / 4;
  for (int64_t i = threadIdx.x; i < nv; i += 1024) ov[i] = xv[i];
}

// flat grid-stride (no chunk spans): float4 index = global thread stride
__global__ __launch_bounds__(THREADS) void k_copy_gridstride(const float *__restrict__ x,
                                                             float *__restrict__ out,
                                                             int64_t n, int nchunks) {
  const float4 *__restrict__ xv = reinterpret_cast<const float4 *>(x);
  float4 *__restrict__ ov = reinterpret_cast<float4 *>(out);
  const int64_t nv = n / 4;
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < nv; i += stride)
    ov[i] = xv[i];
}

// ------------------------------------------------------------------
// Product-shape variants of v2_nontemporal, one difference at a time.
// The engine's column kernels take a device table of column pointers and
// run ncols x nchunks blocks (col = blockIdx.x / nchunks); the copies above
// take their pointers as kernel arguments, which lets the compiler prove
// the global address space.
//   tbl_flat    (a) pointers fetched from the tables and left flat
//   tbl_global  (b) the same, cast once per block to address_space(1)
//   tbl_global over many separately allocated columns is (c)
//   tbl_glb_pre (d) as (b), loads of iteration k+1 issued before the
//               stores of iteration k
// ------------------------------------------------------------------
#define BW_GLOBAL __attribute__((address_space(1)))
typedef const nat_f4 BW_GLOBAL *gvec_in;
typedef nat_f4 BW_GLOBAL *gvec_out;

__global__ __launch_bounds__(THREADS) void k_tbl_flat(const float *const *cols,
                                                      float *const *outs,
                                                      const int64_t *lens, int nchunks) {
  const int col = blockIdx.x / nchunks;
  const int chunk = blockIdx.x % nchunks;
  const float *__restrict__ x = cols[col];
  float *__restrict__ out = outs[col];
  const int64_t n = lens[col];
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  const nat_f4 *__restrict__ xv = reinterpret_cast<const nat_f4 *>(x + s);
  nat_f4 *__restrict__ ov = reinterpret_cast<nat_f4 *>(out + s);
  const int64_t nv = (e - s) / 4;
  int64_t i = threadIdx.x;
  for (; i + THREADS < nv; i += 2 * THREADS) {
    nat_f4 a = __builtin_nontemporal_load(&xv[i]);
    nat_f4 b = __builtin_nontemporal_load(&xv[i + THREADS]);
    __builtin_nontemporal_store(a, &ov[i]);
    __builtin_nontemporal_store(b, &ov[i + THREADS]);
  }
  for (; i < nv; i += THREADS) {
    nat_f4 a = xv[i];
    ov[i] = a;
  }
}

__global__ __launch_bounds__(THREADS) void k_tbl_global(const float *const *cols,
                                                        float *const *outs,
                                                        const int64_t *lens, int nchunks) {
  const int col = blockIdx.x / nchunks;
  const int chunk = blockIdx.x % nchunks;
  const int64_t n = lens[col];
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  const gvec_in xv = (gvec_in)(cols[col] + s);
  const gvec_out ov = (gvec_out)(outs[col] + s);
  const int64_t nv = (e - s) / 4;
  int64_t i = threadIdx.x;
  for (; i + THREADS < nv; i += 2 * THREADS) {
    nat_f4 a = __builtin_nontemporal_load(&xv[i]);
    nat_f4 b = __builtin_nontemporal_load(&xv[i + THREADS]);
    __builtin_nontemporal_store(a, &ov[i]);
    __builtin_nontemporal_store(b, &ov[i + THREADS]);
  }
  for (; i < nv; i += THREADS) {
    nat_f4 a = xv[i];
    ov[i] = a;
  }
}

__global__ __launch_bounds__(THREADS) void k_tbl_glb_pre(const float *const *cols,
                                                         float *const *outs,
                                                         const int64_t *lens, int nchunks) {
  const int col = blockIdx.x / nchunks;
  const int chunk = blockIdx.x % nchunks;
  const int64_t n = lens[col];
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  const gvec_in xv = (gvec_in)(cols[col] + s);
  const gvec_out ov = (gvec_out)(outs[col] + s);
  const int64_t nv = (e - s) / 4;
  int64_t i = threadIdx.x;
  if (i + THREADS < nv) {
    nat_f4 a = __builtin_nontemporal_load(&xv[i]);
    nat_f4 b = __builtin_nontemporal_load(&xv[i + THREADS]);
    // invariant: a, b hold vectors i and i + THREADS, both < nv
    for (; i + 3 * THREADS < nv; i += 2 * THREADS) {
      nat_f4 a2 = __builtin_nontemporal_load(&xv[i + 2 * THREADS]);
      nat_f4 b2 = __builtin_nontemporal_load(&xv[i + 3 * THREADS]);
      __builtin_nontemporal_store(a, &ov[i]);
      __builtin_nontemporal_store(b, &ov[i + THREADS]);
      a = a2;
      b = b2;
    }
    __builtin_nontemporal_store(a, &ov[i]);
    __builtin_nontemporal_store(b, &ov[i + THREADS]);
    i += 2 * THREADS;
  }
  for (; i < nv; i += THREADS) {
    nat_f4 a = xv[i];
    ov[i] = a;
  }
}

// (b) with the blocks of one row range next to each other: chunk-major,
// col = blockIdx.x % ncols, so that the blocks in flight at one time stream
// the same rows of neighbouring columns
__global__ __launch_bounds__(THREADS) void k_tbl_global_cm(const float *const *cols,
                                                           float *const *outs,
                                                           const int64_t *lens, int nchunks) {
  const int ncols = gridDim.x / nchunks;
  const int col = blockIdx.x % ncols;
  const int chunk = blockIdx.x / ncols;
  const int64_t n = lens[col];
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  const gvec_in xv = (gvec_in)(cols[col] + s);
  const gvec_out ov = (gvec_out)(outs[col] + s);
  const int64_t nv = (e - s) / 4;
  int64_t i = threadIdx.x;
  for (; i + THREADS < nv; i += 2 * THREADS) {
    nat_f4 a = __builtin_nontemporal_load(&xv[i]);
    nat_f4 b = __builtin_nontemporal_load(&xv[i + THREADS]);
    __builtin_nontemporal_store(a, &ov[i]);
    __builtin_nontemporal_store(b, &ov[i + THREADS]);
  }
  for (; i < nv; i += THREADS) {
    nat_f4 a = xv[i];
    ov[i] = a;
  }
}

// (b) with the columns taken in groups of G: blocks run over the chunks of
// one group before the next group starts, and inside a chunk over the
// group's columns. G = 1 is the column-major order, G >= ncols the
// chunk-major one.
template <int G>
__global__ __launch_bounds__(THREADS) void k_tbl_global_grp(const float *const *cols,
                                                            float *const *outs,
                                                            const int64_t *lens, int nchunks) {
  const int ncols = gridDim.x / nchunks;
  const int grp = blockIdx.x / (G * nchunks);
  const int within = blockIdx.x % (G * nchunks);
  const int gcols = min(G, ncols - grp * G);
  const int col = grp * G + within % gcols;
  const int chunk = within / gcols;
  const int64_t n = lens[col];
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t s = (int64_t)chunk * per;
  const int64_t e = min(n, s + per);
  const gvec_in xv = (gvec_in)(cols[col] + s);
  const gvec_out ov = (gvec_out)(outs[col] + s);
  const int64_t nv = (e - s) / 4;
  int64_t i = threadIdx.x;
  for (; i + THREADS < nv; i += 2 * THREADS) {
    nat_f4 a = __builtin_nontemporal_load(&xv[i]);
    nat_f4 b = __builtin_nontemporal_load(&xv[i + THREADS]);
    __builtin_nontemporal_store(a, &ov[i]);
    __builtin_nontemporal_store(b, &ov[i + THREADS]);
  }
  for (; i < nv; i += THREADS) {
    nat_f4 a = xv[i];
    ov[i] = a;
  }
}

// Column-table launch: `ncols` columns of `n` floats each, ncols x nchunks
// blocks. Checks the copy of the first and last column once per kernel.
struct ColTables {
  const float *const *cols;
  float *const *outs;
  const int64_t *lens;
};

template <typename K>
double bench_tbl(K kern, const ColTables &t, int ncols, int64_t n, int nchunks,
                 const char *name) {
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  const dim3 grid((uint32_t)ncols * (uint32_t)nchunks);
  hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, 0, t.cols, t.outs, t.lens, nchunks);
  hipDeviceSynchronize();
  hipEventRecord(a);
  for (int r = 0; r < 5; ++r)
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, 0, t.cols, t.outs, t.lens, nchunks);
  hipEventRecord(b);
  hipDeviceSynchronize();
  float ms = 0;
  hipEventElapsedTime(&ms, a, b);
  double tbps = 2.0 * ncols * n * 4 * 5 / (ms / 1000.0) / 1e12;
  printf("%-22s %8.3f ms/iter  %6.2f TB/s  %s\n", name, ms / 5, tbps,
         hipGetLastError() == hipSuccess ? "" : "LAUNCH ERROR");
  hipEventDestroy(a);
  hipEventDestroy(b);
  return tbps;
}

// pick_chunks of the bindings (anovos_bindings.hip)
static int pick_chunks(int64_t n, int ncols) {
  int64_t by_size = (n + (1 << 16) - 1) >> 16;
  int64_t cap = 16384 / ncols > 1 ? 16384 / ncols : 1;
  int64_t c = by_size < cap ? by_size : cap;
  if (c < 1) c = 1;
  int64_t fl = 2048 / ncols > 1 ? 2048 / ncols : 1;
  if (by_size < fl) fl = by_size;
  if (fl < 1) fl = 1;
  return (int)(c > fl ? c : fl);
}

// (c): ncols separately allocated column pairs of `rows` floats against one
// buffer pair of the same total size cut into the same number of blocks.
static int run_columns(int ncols, int64_t rows) {
  const int nchunks = pick_chunks(rows, ncols);
  printf("--- %d columns x %lld rows, nchunks=%d (%d blocks) ---\n", ncols, (long long)rows,
         nchunks, ncols * nchunks);
  const float **hc = new const float *[ncols];
  float **ho = new float *[ncols];
  int64_t *hl = new int64_t[ncols];
  const float **dc;
  float **dout;
  int64_t *dl;
  CHECK(hipMalloc(&dc, ncols * sizeof(void *)));
  CHECK(hipMalloc(&dout, ncols * sizeof(void *)));
  CHECK(hipMalloc(&dl, ncols * sizeof(int64_t)));
  for (int c = 0; c < ncols; ++c) {
    float *x, *o;
    CHECK(hipMalloc(&x, rows * 4));
    CHECK(hipMalloc(&o, rows * 4));
    CHECK(hipMemset(x, 0x3f, rows * 4));
    hc[c] = x;
    ho[c] = o;
    hl[c] = rows;
  }
  CHECK(hipMemcpy(dc, hc, ncols * sizeof(void *), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dout, ho, ncols * sizeof(void *), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dl, hl, ncols * sizeof(int64_t), hipMemcpyHostToDevice));
  ColTables t{dc, dout, dl};
  bench_tbl(k_tbl_flat, t, ncols, rows, nchunks, "c_cols_flat");
  bench_tbl(k_tbl_global, t, ncols, rows, nchunks, "c_cols_global");
  bench_tbl(k_tbl_glb_pre, t, ncols, rows, nchunks, "c_cols_glb_pre");
  bench_tbl(k_tbl_global_cm, t, ncols, rows, nchunks, "c_cols_chunkmaj");
  bench_tbl(k_tbl_global_grp<2>, t, ncols, rows, nchunks, "c_cols_grp2");
  bench_tbl(k_tbl_global_grp<4>, t, ncols, rows, nchunks, "c_cols_grp4");
  bench_tbl(k_tbl_global_grp<8>, t, ncols, rows, nchunks, "c_cols_grp8");
  bench_tbl(k_tbl_global_grp<16>, t, ncols, rows, nchunks, "c_cols_grp16");
  bench_tbl(k_tbl_global_grp<32>, t, ncols, rows, nchunks, "c_cols_grp32");
  bench_tbl(k_tbl_global_grp<64>, t, ncols, rows, nchunks, "c_cols_grp64");
  bench_tbl(k_tbl_global, t, ncols, rows, nchunks, "c_cols_global(again)");
  // what the block count does to the same layout: chunks per column up to
  // the 64K-element floor of pick_chunks
  const int by_size = (int)((rows + (1 << 16) - 1) >> 16);
  for (int mult : {2, 4, 8, 16, 32}) {
    const int nc = nchunks * mult < by_size ? nchunks * mult : by_size;
    char name[64];
    snprintf(name, sizeof name, "c_cols_x%d(%d)", nc, (int)(rows / nc));
    bench_tbl(k_tbl_global, t, ncols, rows, nc, name);
    snprintf(name, sizeof name, "c_cm_x%d", nc);
    bench_tbl(k_tbl_global_cm, t, ncols, rows, nc, name);
    if (nc == by_size) break;
  }
  for (int c = 0; c < ncols; ++c) {
    CHECK(hipFree((void *)hc[c]));
    CHECK(hipFree(ho[c]));
  }
  // the same bytes as one buffer pair, the same number of blocks
  const int64_t total = rows * ncols;
  float *x, *o;
  CHECK(hipMalloc(&x, total * 4));
  CHECK(hipMalloc(&o, total * 4));
  CHECK(hipMemset(x, 0x3f, total * 4));
  hc[0] = x;
  ho[0] = o;
  hl[0] = total;
  CHECK(hipMemcpy(dc, hc, sizeof(void *), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dout, ho, sizeof(void *), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dl, hl, sizeof(int64_t), hipMemcpyHostToDevice));
  bench_tbl(k_tbl_flat, t, 1, total, ncols * nchunks, "c_one_flat");
  bench_tbl(k_tbl_global, t, 1, total, ncols * nchunks, "c_one_global");
  bench_tbl(k_tbl_glb_pre, t, 1, total, ncols * nchunks, "c_one_glb_pre");
  CHECK(hipFree(x));
  CHECK(hipFree(o));
  CHECK(hipFree(dc));
  CHECK(hipFree(dout));
  CHECK(hipFree(dl));
  delete[] hc;
  delete[] ho;
  delete[] hl;
  return 0;
}

template <typename K>
double bench(K kern, const float *x, float *out, int64_t n, int nchunks,
             int threads, const char *name) {
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  // warmup
  hipLaunchKernelGGL(kern, dim3(nchunks), dim3(threads), 0, 0, x, out, n, nchunks);
  hipDeviceSynchronize();
  hipEventRecord(a);
  for (int r = 0; r < 5; ++r)
    hipLaunchKernelGGL(kern, dim3(nchunks), dim3(threads), 0, 0, x, out, n, nchunks);
  hipEventRecord(b);
  hipDeviceSynchronize();
  float ms = 0;
  hipEventElapsedTime(&ms, a, b);
  double tbps = 2.0 * n * 4 * 5 / (ms / 1000.0) / 1e12;
  printf("%-16s %7.3f ms/iter  %6.2f TB/s\n", name, ms / 5, tbps);
  hipEventDestroy(a);
  hipEventDestroy(b);
  return tbps;
}

int main(int argc, char **argv) {
  // usage: bwbench [ncols rows]   (default 150 x 125M, the benchmark's f32 block)
  const int ncols = argc > 1 ? atoi(argv[1]) : 150;
  const int64_t rows = argc > 2 ? atoll(argv[2]) : 125000000LL;
  const int64_t n = 1LL << 30;  // 4 GB in, 4 GB out
  float *x, *out;
  CHECK(hipMalloc(&x, n * 4));
  CHECK(hipMalloc(&out, n * 4));
  CHECK(hipMemset(x, 0x3f, n * 4));
  const float **dc;
  float **dout;
  int64_t *dl;
  CHECK(hipMalloc(&dc, sizeof(void *)));
  CHECK(hipMalloc(&dout, sizeof(void *)));
  CHECK(hipMalloc(&dl, sizeof(int64_t)));
  CHECK(hipMemcpy(dc, &x, sizeof(void *), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dout, &out, sizeof(void *), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dl, &n, sizeof(int64_t), hipMemcpyHostToDevice));
  ColTables one{dc, dout, dl};
  for (int nchunks : {2048, 4096, 16384}) {
    printf("--- nchunks=%d ---\n", nchunks);
    bench(k_copy_v1, x, out, n, nchunks, THREADS, "v1_current");
    bench(k_copy_v2, x, out, n, nchunks, THREADS, "v2_unroll2");
    bench(k_copy_v4, x, out, n, nchunks, THREADS, "v4_unroll4");
    bench(k_copy_v2nt, x, out, n, nchunks, THREADS, "v2_nontemporal");
    bench(k_fill_v2, x, out, n, nchunks, THREADS, "fill_v2");
    bench(k_copy_t1024, x, out, n, nchunks, 1024, "v1_1024thr");
    bench(k_copy_gridstride, x, out, n, nchunks, THREADS, "gridstride");
    bench_tbl(k_tbl_flat, one, 1, n, nchunks, "a_tbl_flat");
    bench_tbl(k_tbl_global, one, 1, n, nchunks, "b_tbl_global");
    bench_tbl(k_tbl_glb_pre, one, 1, n, nchunks, "d_tbl_glb_pre");
  }
  CHECK(hipFree(x));
  CHECK(hipFree(out));
  CHECK(hipFree(dc));
  CHECK(hipFree(dout));
  CHECK(hipFree(dl));
  return run_columns(ncols, rows);
}
