// Launcher prototypes and host/device limits of the anovos_amd HIP kernels.
//
// Included by the bindings (anovos_bindings.hip) and by every file that
// defines a launcher (anovos_kernels.hip, corr_mfma.hip, pair_counts.hip,
// grouped_moments.hip, grades.hip, pairwise_gram.hip, row_quadform.hip):
// the launchers have C linkage, so a definition whose parameter list
// drifts from the prototype the bindings call through would link cleanly
// and pass garbage; with the prototype in scope it fails to compile
// ("conflicting types").

#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

// ---- limits the host planning code and the kernels must agree on ----

// K5 / K22: uint32 counters one block stages in LDS (64 KiB). A column of
// code_counts(_multi) with more slots, or a pair table with more cells,
// counts in global memory instead.
constexpr int CODE_LDS_SLOTS = 16384;
constexpr int PAIR_LDS_SLOTS = 16384;
// K22 work item: anchor column + up to PAIR_PMAX partners, as
// PAIR_ITEM_WORDS int64 words (layout in pair_counts.hip)
constexpr int PAIR_PMAX = 8;
constexpr int PAIR_ITEM_WORDS = 4 + 4 * PAIR_PMAX;
// K23 work item: one code column, a window of w slots and P value columns
// with w * P <= GRP_CELLS accumulator cells, P <= GRP_PMAX, as
// GRP_ITEM_WORDS int64 words (layout in grouped_moments.hip). Every thread
// of a block owns GRP_CELL_BYTES of LDS per cell (fp64 s1, fp64 s2, uint32
// row count): GRP_CELLS * GRP_THREADS * GRP_CELL_BYTES = 80 KiB, two
// blocks per CU.
constexpr int GRP_CELLS = 16;
constexpr int GRP_PMAX = 8;
constexpr int GRP_THREADS = 256;
constexpr int GRP_CELL_BYTES = 20;
constexpr int GRP_ITEM_WORDS = 5 + 2 * GRP_PMAX;
// K3 grouped refinement histograms: sub-bins per bracket, brackets per
// column and launch (RB_MAXB * RB_BINS uint32 counters in static LDS)
constexpr int RB_BINS = 512;
constexpr int RB_MAXB = 16;
// K9: slots per column of the label-conditioned counts (2 * slots uint32
// counters in LDS; slot numbers up to 8192 are exact in fp32)
constexpr int LABEL_MAX_SLOTS = 8192;
// K6 with counts: cutoffs per column (doubles + uint32 counters in LDS)
constexpr int BKT_COUNTS_MAX_NCUT = 4096;
// K24: cells of a column's rank grid (at most GRADE_MAX_CELLS - 1 cutoffs;
// cutoffs, counters and the grade table of one column in LDS)
constexpr int GRADE_MAX_CELLS = 4096;
// K3q: bins (or dense integer counts) of one column whose CDF the
// quantile-query kernels hold in LDS as uint64
constexpr int QQ_MAX_BINS = 4096;
// K25: 16-column tiles per column group (a work item is a pair of groups),
// rows of the macro-slab a block stages per round, fp32 partials one block
// writes (tile pairs x 6 products x 256), and the rows one block may own:
// its fp32 count accumulators are exact below 2^24
constexpr int PAIRGRAM_GROUP_TILES = 4;
constexpr int PAIRGRAM_SLAB_ROWS = 64;
constexpr int PAIRGRAM_ITEM_FLOATS = PAIRGRAM_GROUP_TILES * PAIRGRAM_GROUP_TILES * 6 * 256;
constexpr int64_t PAIRGRAM_MAX_BLOCK_ROWS = (int64_t)1 << 24;
// K26: most columns of a row quadratic form, rows of the slab a block
// stages per round, and the LDS of one block (all of a CU's): the Z slab
// (two bf16 planes, one 16-byte slot per column octet and row,
// ROWQUAD_Z_SLOTS slots per octet) beside the window of W's rows that stays
// resident (two bf16 planes of k_pad columns). Columns pad to 32 (an MFMA
// k-step), W's rows to 16 (a tile). The window plan depends only on k: at
// k_pad = 160 all 160 rows fit (43 520 + 102 400 B), at k_pad = 256 80 do.
constexpr int ROWQUAD_MAX_COLS = 256;
constexpr int ROWQUAD_SLAB_ROWS = 64;
constexpr int ROWQUAD_Z_SLOTS = 68;
constexpr int ROWQUAD_LDS_BYTES = 160 * 1024;
__host__ __device__ constexpr int rowquad_kpad(int k) { return (k + 31) / 32 * 32; }
__host__ __device__ constexpr int rowquad_rpad(int r) { return (r + 15) / 16 * 16; }
__host__ __device__ constexpr int rowquad_z_bytes(int k_pad) {
  return 2 * (k_pad / 8) * ROWQUAD_Z_SLOTS * 16;
}
__host__ __device__ constexpr int rowquad_w_row_bytes(int k_pad) { return 2 * (k_pad / 8) * 16; }
// rows of W (a multiple of 16) one launch keeps in LDS
__host__ __device__ constexpr int rowquad_window_rows(int k) {
  return (ROWQUAD_LDS_BYTES - rowquad_z_bytes(rowquad_kpad(k))) /
         rowquad_w_row_bytes(rowquad_kpad(k)) / 16 * 16;
}
static_assert(rowquad_window_rows(160) >= 160, "the 150-column benchmark frame takes one launch");
static_assert(rowquad_window_rows(ROWQUAD_MAX_COLS) >= 16, "a window holds at least one tile");
// Null lane masks (K1/K2+K4 and K5 emit, K10m reads): 64-bit words one
// chunk of `per` rows owns. A group of four words covers the 256 rows of
// one wave iteration of a 4-wide loop; one more group holds the <= 3 rows
// of the scalar tail. A column's mask has nchunks * this many words.
__host__ __device__ constexpr int64_t null_mask_chunk_words(int64_t per) {
  return 4 * ((((per >> 2) + 63) >> 6) + 1);
}

// ---- launchers: return a hipError_t as int, 0 on success ----
// dtype: 0 = float32 columns, 1 = float64 (K10 also 2 = int32 codes)

extern "C" {
int anovos_moments(const void *const *cols, const int64_t *lens,
                   const double *shifts, int ncols, int nchunks, int dtype,
                   double *partials, double *out, hipStream_t stream);
int anovos_hist(const void *const *cols, const int64_t *lens, int ncols,
                const double *lo, const double *hi, int nbins, int nchunks,
                int dtype, uint64_t *out, hipStream_t stream);
int anovos_bracket_hist(const void *const *cols, const int64_t *lens,
                        const int64_t *colidx, int nbrackets, const double *lo,
                        const double *hi, int nbins, int nchunks, int dtype,
                        uint64_t *out, hipStream_t stream);
int anovos_bucketize(const void *const *cols, const int64_t *lens, int ncols,
                     const double *cutflat, const int64_t *cutoff_off,
                     const int *cutoff_len, int max_ncut, int nchunks, int dtype,
                     int32_t *const *outs, hipStream_t stream);
int anovos_code_counts(const int32_t *codes, int64_t n, int size, int nchunks,
                       uint64_t *out, hipStream_t stream);
int anovos_hll(const void *x, int64_t n, int p, int nchunks, int dtype,
               int32_t *regs, hipStream_t stream);
int anovos_row_null(const void *const *cols, int ncols, int64_t n, int dtype,
                    int32_t *out, hipStream_t stream);
int anovos_hll_multi(const void *const *cols, const int64_t *lens, int ncols,
                     int p, int nchunks, int dtype, int32_t *regs,
                     hipStream_t stream);
int anovos_axpb(const void *const *cols, const int64_t *lens, int ncols,
                const double *a, const double *b, int nchunks, int dtype,
                float *const *outs, hipStream_t stream);
int anovos_fillnan(const void *const *cols, const int64_t *lens, int ncols,
                   const double *fill, int nchunks, int dtype,
                   void *const *outs, hipStream_t stream);
int anovos_bracket_hist_grouped(const void *const *cols, const int64_t *lens,
                                const int *bstart, int ncols, const double *lo,
                                const double *hi, const double *p1lo,
                                const double *p1scale, int p1bins, int nchunks,
                                int dtype, uint64_t *out, hipStream_t stream);
int anovos_bucketize_float(const void *const *cols, const int64_t *lens, int ncols,
                           const double *cutflat, const int64_t *cutoff_off,
                           const int *cutoff_len, int max_ncut, int nchunks, int dtype,
                           float *const *outs, hipStream_t stream);
int anovos_bucketize_float_counts(const void *const *cols, const int64_t *lens, int ncols,
                                  const double *cutflat, const int64_t *cutoff_off,
                                  const int *cutoff_len, int max_ncut, int nchunks, int dtype,
                                  float *const *outs, uint64_t *counts, const int64_t *count_off,
                                  hipStream_t stream);
int anovos_lut_apply_f32(const int32_t *const *cols, const int64_t *lens, int ncols,
                         const float *lutflat, const int64_t *lut_off, int nchunks,
                         float *const *outs, hipStream_t stream);
int anovos_lut_apply_i32(const int32_t *const *cols, const int64_t *lens, int ncols,
                         const int32_t *lutflat, const int64_t *lut_off, int nchunks,
                         int32_t *const *outs, hipStream_t stream);
int anovos_fill_code(const int32_t *const *cols, const int64_t *lens, int ncols,
                     const int32_t *fill, int nchunks, int32_t *const *outs,
                     hipStream_t stream);
int anovos_code_counts_multi(const int32_t *const *cols, const int64_t *lens,
                             const int64_t *offs, const int *sizes, int ncols,
                             int lds_slots, int nchunks, uint64_t *out,
                             uint64_t *const *masks, hipStream_t stream);
int anovos_outlier_clamp(const void *const *cols, const int64_t *lens,
                         int ncols, const double *lo, const double *hi,
                         int nchunks, int mode, int dtype, void *const *outs,
                         uint64_t *counts, hipStream_t stream);
int anovos_moments_hll(const void *const *cols, const int64_t *lens,
                       const double *shifts, int ncols, int p, int nchunks,
                       int dtype, double *partials, double *mom_out,
                       int32_t *regs, uint64_t *const *masks, hipStream_t stream);
// masks (K5, K1/K2+K4 f32): null, or one pointer per column to
// nchunks * null_mask_chunk_words(ceil(len / nchunks)) words that receive
// the column's null lane masks; K5 takes a null entry for a column that
// counts in global memory. K10m adds the row null counts of columns that
// share the partition (n, nchunks, per) into out[n].
int anovos_row_null_masked(const uint64_t *const *masks, int ncols, int64_t n,
                           int nchunks, int64_t per, int32_t *out,
                           hipStream_t stream);
int anovos_bucketize_label_counts(const void *const *cols, const uint8_t *label,
                                  const int64_t *lens, const double *cutflat,
                                  const int64_t *cutoff_off, const int *cutoff_len,
                                  const int64_t *offs, const int *sizes, int ncols,
                                  int max_ncut, int max_slots, int nchunks,
                                  int dtype, uint64_t *out, hipStream_t stream);
int anovos_label_counts_multi(const void *const *cols, const uint8_t *label,
                              const int64_t *lens, const int64_t *offs,
                              const int *sizes, const int *dtypes, int ncols,
                              int max_slots, int nchunks, uint64_t *out,
                              hipStream_t stream);
// K3q: quantile queries on device-resident histograms, one block per
// column. hist is [ncols, nbins] (nbins <= QQ_MAX_BINS); lo / hi / n are
// per column, probs has P entries; vals and flags are [ncols, P], maxbin
// [ncols]. The dense-integer form reads the first R[c] (given as fp64) of
// the `rows` counts of column c.
int anovos_hist_quantile_query(const uint64_t *hist, const double *lo, const double *hi,
                               const double *n, const double *probs, double rel_err,
                               int ncols, int nbins, int P, double *vals, uint8_t *flags,
                               int64_t *maxbin, hipStream_t stream);
int anovos_inthist_quantile_query(const uint64_t *counts, int rows, const double *cmin,
                                  const double *n, const double *R, const double *probs,
                                  double rel_err, int ncols, int P, double *vals,
                                  hipStream_t stream);
// corr_mfma.hip
int anovos_centered_gram(const void *const *cols, int64_t n, int k,
                         const float *means, const int *pair_i,
                         const int *pair_j, int npairs, int row_chunks,
                         float *partials, float *gram, hipStream_t stream);
int anovos_centered_gram_sr(const void *const *cols, int64_t n, int k,
                            const float *means, const int *pair_i,
                            const int *pair_j, int npairs, int row_chunks,
                            float *partials, float *gram, hipStream_t stream);
int anovos_gram_sr_grid(int k);
// pair_counts.hip
int anovos_pair_code_counts(const int32_t *const *cols, const int64_t *items,
                            int nitems, int64_t n, int64_t per, int nchunks,
                            int lds_slots, uint64_t *out, hipStream_t stream);
// grouped_moments.hip
int anovos_grouped_moments(const int32_t *const *codes, const void *const *vals,
                           const double *shifts, const int64_t *items, int nitems,
                           int64_t n, int64_t per, int nchunks, int cells, int dtype,
                           double *partials, double *out, hipStream_t stream);
// grades.hip
int anovos_grade_counts(const void *const *cols, const int64_t *lens, int ncols,
                        const double *cutflat, const int64_t *cutoff_off,
                        const int *cutoff_len, int max_ncut, int nchunks, int dtype,
                        uint64_t *counts, const int64_t *count_off, hipStream_t stream);
int anovos_grade_apply(const void *const *cols, const int64_t *lens, int ncols,
                       const double *cutflat, const int64_t *cutoff_off,
                       const int *cutoff_len, const float *tabflat, const int64_t *tab_off,
                       float null_grade, int max_ncut, int nchunks, int dtype,
                       float *const *outs, hipStream_t stream);
// pairwise_gram.hip: out is fp64 [4, k, k] = (N, P, S, Q); items are pairs
// of column groups (item_gi[t] <= item_gj[t]); partials holds
// row_chunks * nitems * PAIRGRAM_ITEM_FLOATS floats
int anovos_pairwise_gram(const void *const *cols, int64_t n, int k, const float *means,
                         const int *item_gi, const int *item_gj, int nitems, int row_chunks,
                         float *partials, double *out, hipStream_t stream);
int anovos_pairwise_gram_grid();
// row_quadform.hip: wimg holds the two bf16 planes of W [r, k] as
// 2 * (k_pad / 8) * r_pad * 8 uint16 (anovos_row_quadform_split fills it,
// once per call); one launch takes the rows [r0, r0 + rw_pad) of it, both
// multiples of 16 with rw_pad <= rowquad_window_rows(k), and writes
// (accumulate = 0) or adds to (1) out[n]. blocks <= 0: one wave of resident
// blocks.
int anovos_row_quadform_split(const float *W, int r, int k, uint16_t *wimg, hipStream_t stream);
int anovos_row_quadform(const void *const *cols, int64_t n, int k, const float *shift,
                        const float *scale, const uint16_t *wimg, int r, int r0, int rw_pad,
                        int accumulate, int blocks, float *out, hipStream_t stream);
}
