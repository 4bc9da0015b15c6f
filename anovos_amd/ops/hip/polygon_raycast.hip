// K33: point-in-polygon membership by banded ray casting (gfx950).
//
// Operation. For P (lat, lon) column pairs and a set of rings, one f32 per
// row: NaN if lat or lon is NaN, else 1 if the point is inside ANY ring, else
// 0. Inside a ring is odd crossing parity of the ray towards +x; parity is
// taken per ring and OR-ed over rings. With x = lon, y = lat and an edge
// (px, py) -> (qx, qy), exactly the rule of geo_utils.point_in_polygon:
//
//   straddles = (py > y) != (qy > y)
//   crosses   = straddles && (x < px + (y - py) * (qx - px) / (qy - py))
//
// in fp64, in this order, IEEE division, nothing contracted into an FMA (the
// file is compiled with fp contract off), so the result has the bits of the
// torch expression. Horizontal edges never straddle; the host drops them.
//
// Table (ops/polygon.py edge_table builds the index, pip_table_kernel the
// image). The latitude extent [ymin, ymax] of the edges is cut into B uniform
// bands; band_off[B + 1] is a CSR index into a list of edge records in which
// an edge appears once for every band it overlaps, each band's records
// sorted by ring. A row reads only the records of band(y):
//
//   band(y) = f < B - 1 ? (int)f : B - 1,   f = floor((y - ymin) * scale)
//
// for ymin <= y <= ymax; every other row (NaN included) is outside and reads
// nothing. Correctness condition: an edge that straddles y is in the list of
// band(y). It holds because the host files an edge under band(min(py, qy))
// .. band(max(py, qy)) computed with THE SAME uncontracted fp64 expression -
// a subtract, a multiply by a positive constant, a floor, a clamp, each
// monotone - so min <= y < max puts band(y) inside that range. No widening
// by a band on either side is needed or done.
//
// A record is 48 bytes, three 16-byte slots, so that every read is aligned:
//   slot 0: py, qy             read for every record (one 128-bit read)
//   slot 1: px, qx - px        read under `straddles` only
//   slot 2: qy - py, ring id   the ring id (low 32 bits of an int64) is read
//                              for every record, qy - py under `straddles`
// The two differences are taken once when the image is built: a lone IEEE
// subtract has the same bits wherever it runs. The image is the records
// followed by band_off (int32, padded to 16 bytes): pip_table_bytes().
//
// Work split. Persistent 256-thread blocks walk (row tile, pair) items in a
// grid-stride loop, pairs innermost so that no division is needed; a tile is
// PIP_ROWS = 4 rows per lane at a stride of 256 rows, so every load and the
// f32 store of a wave are one contiguous run (columns and outputs need
// element alignment only). The 8 loads of the next item are issued before the
// edge loop of the current one. f32 and f64 columns are read as they are and
// widened in registers (template parameter).
//
// A lane keeps one parity bit per row and folds it into `inside` whenever
// the ring id changes and at the end. With B == 1 all rows share one list:
// the lane's four rows go through it together and every record read is one
// address per wave - the broadcast brute force that small polygons want.
// With B > 1 the four rows walk their own bands one after the other.
//
// Two placements of the image, the loop body templated on the address space:
//   LDS     the image fits PIP_LDS_BYTES: staged once per block with 16-byte
//           copies, read with ds_read_b128 / b64 / b32.
//   global  larger images (country outlines) stay where they are, a few MB
//           read through the vector cache with global_load_dwordx4.
// No matrix instructions: nothing here is a product.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "anovos_kernels.h"

#pragma clang fp contract(off)

namespace {

#define DEV_INLINE __device__ __forceinline__
#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

constexpr int PIP_THREADS = 256;
constexpr int PIP_ROWS = 4;
constexpr int PIP_TILE = PIP_THREADS * PIP_ROWS;

typedef double nat_d2 __attribute__((ext_vector_type(2)));

// The image seen as 16-byte slots, doubles and 32-bit words, in LDS or in
// global memory.
template <bool LDS>
struct Image;
template <>
struct Image<true> {
  typedef const nat_d2 LDS_AS *slots;
  typedef const double LDS_AS *doubles;
  typedef const int LDS_AS *words;
};
template <>
struct Image<false> {
  typedef const nat_d2 GLOBAL_AS *slots;
  typedef const double GLOBAL_AS *doubles;
  typedef const int GLOBAL_AS *words;
};

struct PipBands {
  double ymin, ymax, scale;
  int nbands;
};

// edges is fp64 [E, 5] = (px, py, qx, qy, ring); record k is edge
// band_edges[k]. One thread per record, and per word of the offset part.
__global__ void pip_table_kernel(const double *edges, const int *band_edges, const int *band_off,
                                 int nrec, int nbands, nat_d2 *image) {
  const int k = blockIdx.x * PIP_THREADS + threadIdx.x;
  if (k < nrec) {
    const double *e = edges + 5 * (int64_t)band_edges[k];
    const double px = e[0], py = e[1], qx = e[2], qy = e[3];
    image[3 * (int64_t)k] = nat_d2{py, qy};
    image[3 * (int64_t)k + 1] = nat_d2{px, qx - px};
    image[3 * (int64_t)k + 2] = nat_d2{qy - py, __longlong_as_double((long long)e[4])};
  }
  int *off = (int *)(image + 3 * (int64_t)nrec);
  if (k < (nbands + 1 + 3) / 4 * 4) off[k] = k <= nbands ? band_off[k] : 0;
}

template <bool LDS>
DEV_INLINE bool pip_crosses(typename Image<LDS>::slots img, int k, double py, double x, double y) {
  const nat_d2 b = img[3 * k + 1];
  const double dy = ((typename Image<LDS>::doubles)img)[6 * k + 4];
  return x < b.x + (y - py) * b.y / dy;
}

// One row against the records [k0, k1) of its band.
template <bool LDS>
DEV_INLINE bool pip_row(typename Image<LDS>::slots img, int k0, int k1, double x, double y) {
  const typename Image<LDS>::words words = (typename Image<LDS>::words)img;
  bool inside = false, parity = false;
  int ring = -1;
  for (int k = k0; k < k1; ++k) {
    const nat_d2 a = img[3 * k];
    const int r = words[12 * k + 10];
    if (r != ring) {
      inside |= parity;
      parity = false;
      ring = r;
    }
    if ((a.x > y) != (a.y > y)) parity ^= pip_crosses<LDS>(img, k, a.x, x, y);
  }
  return inside | parity;
}

// The lane's rows together against all records (B == 1): bit j of the result
// is row j. A row outside [ymin, ymax], or with a NaN, straddles nothing.
template <bool LDS>
DEV_INLINE unsigned pip_rows_all(typename Image<LDS>::slots img, int nrec, const double *x,
                                 const double *y) {
  const typename Image<LDS>::words words = (typename Image<LDS>::words)img;
  unsigned inside = 0, parity = 0;
  int ring = -1;
  for (int k = 0; k < nrec; ++k) {
    const nat_d2 a = img[3 * k];
    const int r = words[12 * k + 10];
    if (r != ring) {
      inside |= parity;
      parity = 0;
      ring = r;
    }
#pragma unroll
    for (int j = 0; j < PIP_ROWS; ++j)
      if ((a.x > y[j]) != (a.y > y[j]))
        parity ^= (unsigned)pip_crosses<LDS>(img, k, a.x, x[j], y[j]) << j;
  }
  return inside | parity;
}

template <typename T>
struct PipRows {
  T lat[PIP_ROWS], lon[PIP_ROWS];
};

// Rows t * PIP_TILE + j * PIP_THREADS + thread of pair p; NaN past the end.
template <typename T>
DEV_INLINE void pip_load(PipRows<T> &r, const void *const *lats, const void *const *lons,
                         const int64_t *lens, int p, int64_t t) {
  const T GLOBAL_AS *la = (const T GLOBAL_AS *)lats[p];
  const T GLOBAL_AS *lo = (const T GLOBAL_AS *)lons[p];
  const int64_t n = lens[p];
  const int64_t first = t * PIP_TILE + threadIdx.x;
#pragma unroll
  for (int j = 0; j < PIP_ROWS; ++j) {
    const int64_t i = first + j * PIP_THREADS;
    r.lat[j] = (T)NAN;
    r.lon[j] = (T)NAN;
    if (i < n) {
      r.lat[j] = __builtin_nontemporal_load(&la[i]);
      r.lon[j] = __builtin_nontemporal_load(&lo[i]);
    }
  }
}

template <typename T, bool LDS>
__global__ __launch_bounds__(PIP_THREADS) void pip_kernel(
    const void *const *lats, const void *const *lons, const int64_t *lens, int npairs,
    int64_t tiles, const nat_d2 *image, int nrec, PipBands bands, float *const *outs) {
  extern __shared__ nat_d2 pip_lds[];
  typename Image<LDS>::slots img;
  if (LDS) {
    const int slots = 3 * nrec + (bands.nbands + 1 + 3) / 4;
    for (int i = threadIdx.x; i < slots; i += PIP_THREADS) pip_lds[i] = image[i];
    __syncthreads();
    img = (typename Image<LDS>::slots)pip_lds;
  } else {
    img = (typename Image<LDS>::slots)image;
  }
  const typename Image<LDS>::words off = (typename Image<LDS>::words)(img + 3 * nrec);

  int64_t t = blockIdx.x;
  int p = 0;
  if (t >= tiles) return;
  PipRows<T> cur, nxt;
  pip_load(cur, lats, lons, lens, p, t);
  for (;;) {
    // the next item: pairs innermost, then the block's next tile
    int pn = p + 1;
    int64_t tn = t;
    if (pn == npairs) {
      pn = 0;
      tn += gridDim.x;
    }
    const bool more = tn < tiles;
    if (more) pip_load(nxt, lats, lons, lens, pn, tn);

    double x[PIP_ROWS], y[PIP_ROWS];
#pragma unroll
    for (int j = 0; j < PIP_ROWS; ++j) {
      x[j] = (double)cur.lon[j];
      y[j] = (double)cur.lat[j];
    }
    unsigned inside = 0;
    if (bands.nbands == 1) {
      inside = pip_rows_all<LDS>(img, nrec, x, y);
    } else {
#pragma unroll
      for (int j = 0; j < PIP_ROWS; ++j) {
        int k0 = 0, k1 = 0;
        if (y[j] >= bands.ymin && y[j] <= bands.ymax) {
          const double f = floor((y[j] - bands.ymin) * bands.scale);
          const int b = f < (double)(bands.nbands - 1) ? (int)f : bands.nbands - 1;
          k0 = off[b];
          k1 = off[b + 1];
        }
        inside |= (unsigned)pip_row<LDS>(img, k0, k1, x[j], y[j]) << j;
      }
    }

    float GLOBAL_AS *o = (float GLOBAL_AS *)outs[p];
    const int64_t n = lens[p];
    const int64_t first = t * PIP_TILE + threadIdx.x;
#pragma unroll
    for (int j = 0; j < PIP_ROWS; ++j) {
      const int64_t i = first + j * PIP_THREADS;
      const float v = (x[j] != x[j] || y[j] != y[j]) ? NAN : (float)((inside >> j) & 1u);
      if (i < n) __builtin_nontemporal_store(v, &o[i]);
    }
    if (!more) break;
    cur = nxt;
    p = pn;
    t = tn;
  }
}

int pip_cus() {
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

template <typename T, bool LDS>
int launch_pip(const void *const *lats, const void *const *lons, const int64_t *lens, int npairs,
               int64_t maxn, const void *image, int nrec, PipBands bands, int blocks,
               float *const *outs, hipStream_t stream) {
  auto kern = pip_kernel<T, LDS>;
  const size_t lds = LDS ? (size_t)pip_table_bytes(nrec, bands.nbands) : 0;
  if (blocks <= 0) {
    // one wave of resident blocks, as K31
    int per_cu = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(kern),
                                                       PIP_THREADS, lds);
    if (per_cu <= 0) per_cu = 1;
    blocks = per_cu * pip_cus();
  }
  const int64_t tiles = (maxn + PIP_TILE - 1) / PIP_TILE;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(blocks, tiles));
  hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(PIP_THREADS), lds, stream, lats, lons, lens,
                     npairs, tiles, (const nat_d2 *)image, nrec, bands, outs);
  return (int)hipGetLastError();
}

bool pip_shape_ok(int64_t nrec, int nbands) {
  return nrec >= 0 && nrec <= PIP_MAX_RECORDS && nbands >= 1 && nbands <= PIP_MAX_BANDS;
}

}  // namespace

extern "C" int anovos_pip_table(const double *edges, const int *band_off, const int *band_edges,
                                int64_t nrec, int nbands, void *image, hipStream_t stream) {
  if (!pip_shape_ok(nrec, nbands)) return (int)hipErrorInvalidValue;
  const int64_t threads = std::max<int64_t>(nrec, (nbands + 1 + 3) / 4 * 4);
  hipLaunchKernelGGL(pip_table_kernel, dim3((uint32_t)((threads + PIP_THREADS - 1) / PIP_THREADS)),
                     dim3(PIP_THREADS), 0, stream, edges, band_edges, band_off, (int)nrec, nbands,
                     (nat_d2 *)image);
  return (int)hipGetLastError();
}

extern "C" int anovos_points_in_polygons(const void *const *lats, const void *const *lons,
                                         const int64_t *lens, int npairs, int64_t maxn, int dtype,
                                         const void *image, int64_t nrec, int nbands, double ymin,
                                         double ymax, double scale, int use_lds, int blocks,
                                         float *const *outs, hipStream_t stream) {
  if (npairs < 1 || maxn < 1 || !pip_shape_ok(nrec, nbands)) return (int)hipErrorInvalidValue;
  if (use_lds && pip_table_bytes(nrec, nbands) > PIP_LDS_BYTES) return (int)hipErrorInvalidValue;
  const PipBands bands{ymin, ymax, scale, nbands};
  const int r = (int)nrec;
  if (dtype == 0)
    return use_lds ? launch_pip<float, true>(lats, lons, lens, npairs, maxn, image, r, bands, blocks, outs, stream)
                   : launch_pip<float, false>(lats, lons, lens, npairs, maxn, image, r, bands, blocks, outs, stream);
  if (dtype == 1)
    return use_lds ? launch_pip<double, true>(lats, lons, lens, npairs, maxn, image, r, bands, blocks, outs, stream)
                   : launch_pip<double, false>(lats, lons, lens, npairs, maxn, image, r, bands, blocks, outs, stream);
  return (int)hipErrorInvalidValue;
}
