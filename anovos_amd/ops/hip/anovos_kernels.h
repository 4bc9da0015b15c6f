// Launcher prototypes and host/device limits of the anovos_amd HIP kernels.
//
// Included by the bindings (anovos_bindings.hip) and by every file that
// defines a launcher (anovos_kernels.hip, corr_mfma.hip, pair_counts.hip,
// grouped_moments.hip, grades.hip, pairwise_gram.hip, row_quadform.hip,
// project_columns.hip, split_gram.hip, knn_impute.hip, mlp_encode.hip,
// chain_impute.hip, als_sweep.hip, polygon_raycast.hip):
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
// K27 shares K26's column limit, slab, LDS images and window plan. Most
// components of one launch: a lane keeps three output pointers, one per 64
// components (project_columns.hip). A window is at most min(r_pad,
// rowquad_window_rows(k)) <= 160 components.
constexpr int PROJ_MAX_WINDOW = 192;
// K28: tiles per column group and rows of a macro-slab as K25; fp64 partials
// one block writes (tile pairs x 256); and the rows whose products one fp32
// accumulator takes before it is added into its fp64 shadow - a multiple of
// the macro-slab. The kernel's per-entry error bound on sum |z_i| |z_j|,
//   3 * 2^-18 + (3 * SPLITGRAM_FLUSH_ROWS + 4) * 2^-24,
// depends on it (ops/corr.py SPLITGRAM_GAMMA repeats the figure).
constexpr int SPLITGRAM_GROUP_TILES = 4;
constexpr int SPLITGRAM_SLAB_ROWS = 64;
constexpr int SPLITGRAM_ITEM_DOUBLES = SPLITGRAM_GROUP_TILES * SPLITGRAM_GROUP_TILES * 256;
constexpr int SPLITGRAM_FLUSH_ROWS = 64;
// K29: KNN imputation apply (knn_impute.hip). Most columns of a model
// (m_pad = 32 * KS, KS <= 4), most neighbours, most donors (a donor index
// and the image offsets stay far below 2^31); rows of the slab a block owns
// at a time; donor tiles (16 donors each) of one stage of the LDS ring.
// KNN_CAND: entries of a lane's private candidate list. A lane sees the
// donors d with (d % 16) / 4 == lane / 16, a quarter of them, and a true
// neighbour is lost from its list only if KNN_CAND donors of the same
// quarter look nearer in the filter pass. With KNN_CAND = KNN_MAX_K + 8 that
// takes k + 8 donors that look nearer overall, so: the k true neighbours
// survive whenever they are among the k + 8 nearest of the filter pass, and
// the union of a row's four lists (4 * KNN_CAND = 64 >= k + 8) is what the
// exact re-rank orders.
constexpr int KNN_MAX_COLS = 128;
constexpr int KNN_MAX_K = 8;
constexpr int KNN_MAX_DONORS = 65536;
constexpr int KNN_SLAB_ROWS = 64;
constexpr int KNN_STAGE_TILES = 2;
constexpr int KNN_CAND = KNN_MAX_K + 8;
__host__ __device__ constexpr int knn_mpad(int m) { return (m + 31) / 32 * 32; }
// donor tiles of the image: padded to whole stages
__host__ __device__ constexpr int knn_tiles(int s) {
  return ((s + 15) / 16 + KNN_STAGE_TILES - 1) / KNN_STAGE_TILES * KNN_STAGE_TILES;
}
// uint16 entries of one donor tile of the image: 5 planes x KS k-steps x 64
// lanes x 8 columns
__host__ __device__ constexpr int knn_tile_shorts(int m) { return 5 * (knn_mpad(m) / 32) * 512; }
// K30: fused three-layer MLP encode (mlp_encode.hip). d <= MLP_MAX_COLS
// input columns pad to KS = mlp_ks(d) k-steps of 32; the layer widths are
// n1 <= 64 * KS, n2 <= 32 * KS, n3 <= 32 * KS (every autoencoder shape of
// d <= 160 columns: n1 = 2 d, n3 <= n2 <= d). n1 and n2 pad to 32 - two
// 16-component tiles make one k-step of the next layer - n3 to 16. The
// weight image is a sequence of ring stages of mlp_stage_shorts(d) uint16,
// one per tile of layers 1 and 3 and mlp_l2_stages() per tile of layer 2
// (whose k-steps number up to 2 * KS: a stage holds KS of them), followed
// by the biases as f32, 16 per tile.
constexpr int MLP_MAX_COLS = 160;
constexpr int MLP_SLAB_ROWS = ROWQUAD_SLAB_ROWS;
__host__ __device__ constexpr int mlp_ks(int d) { return (d + 31) / 32; }
__host__ __device__ constexpr int mlp_tiles12(int width) { return 2 * ((width + 31) / 32); }
__host__ __device__ constexpr int mlp_tiles3(int n3) { return (n3 + 15) / 16; }
__host__ __device__ constexpr int mlp_l2_stages(int d, int n1) {
  return (n1 + 31) / 32 > mlp_ks(d) ? 2 : 1;
}
__host__ __device__ constexpr int mlp_stages(int d, int n1, int n2, int n3) {
  return mlp_tiles12(n1) + mlp_tiles12(n2) * mlp_l2_stages(d, n1) + mlp_tiles3(n3);
}
// two planes x KS k-steps x 64 lanes x 8 inputs
__host__ __device__ constexpr int mlp_stage_shorts(int d) { return 2 * mlp_ks(d) * 512; }
__host__ __device__ constexpr int64_t mlp_image_shorts(int d, int n1, int n2, int n3) {
  return (int64_t)mlp_stages(d, n1, n2, n3) * mlp_stage_shorts(d) +
         2 * 16 * (mlp_tiles12(n1) + mlp_tiles12(n2) + mlp_tiles3(n3));
}
__host__ __device__ constexpr bool mlp_widths_ok(int d, int n1, int n2, int n3) {
  return d >= 1 && d <= MLP_MAX_COLS && n1 >= 1 && n1 <= 64 * mlp_ks(d) && n2 >= 1 &&
         n2 <= 32 * mlp_ks(d) && n3 >= 1 && n3 <= 32 * mlp_ks(d);
}
// K31: regression (IterativeImputer) apply as a row-local chain
// (chain_impute.hip). m columns pad to KS = chain_ks(m) k-steps of 32, the
// m_s steps of a round to chain_tiles(m_s) tiles of 16. The coefficient
// image is one stage of chain_stage_shorts(m) uint16 per (round, step tile),
// followed by the intercepts as f32, 16 per stage.
constexpr int CHAIN_MAX_COLS = 160;
constexpr int CHAIN_MAX_ROUNDS = 32;
constexpr int CHAIN_SLAB_ROWS = ROWQUAD_SLAB_ROWS;
__host__ __device__ constexpr int chain_ks(int m) { return (m + 31) / 32; }
__host__ __device__ constexpr int chain_tiles(int m_s) { return (m_s + 15) / 16; }
// two planes x KS k-steps x 64 lanes x 8 columns
__host__ __device__ constexpr int chain_stage_shorts(int m) { return 2 * chain_ks(m) * 512; }
__host__ __device__ constexpr int64_t chain_image_shorts(int m, int m_s, int R) {
  return (int64_t)R * chain_tiles(m_s) * (chain_stage_shorts(m) + 2 * 16);
}
__host__ __device__ constexpr bool chain_shape_ok(int m, int m_s, int R) {
  return m >= 2 && m <= CHAIN_MAX_COLS && m_s >= 1 && m_s <= m && R >= 1 && R <= CHAIN_MAX_ROUNDS;
}
// K32: the two halves of an ALS sweep (als_sweep.hip). The rank pads to
// KR = als_kr(rank) in {4, 8, 12, 16}; a symmetric KR x KR matrix travels as
// its als_tri(KR) lower entries, (a, b) with a >= b at a (a + 1) / 2 + b,
// followed by the KR entries of the right-hand side. Entries go to the MFMA
// in tiles of 16: the products (and one slot of ones, which counts the
// observed entries), then one tile for the right-hand side. The m columns
// pad to als_ks(m) k-steps of 32 (row half) and go in als_groups(m) groups
// of 64 (column half).
constexpr int ALS_MAX_RANK = 16;
constexpr int ALS_MAX_COLS = 160;
constexpr int ALS_SLAB_ROWS = ROWQUAD_SLAB_ROWS;
__host__ __device__ constexpr int als_kr(int rank) { return (rank + 3) / 4 * 4; }
__host__ __device__ constexpr int als_tri(int kr) { return kr * (kr + 1) / 2; }
__host__ __device__ constexpr int als_tiles(int kr) { return (als_tri(kr) + 1 + 15) / 16 + 1; }
__host__ __device__ constexpr int als_ks(int m) { return (m + 31) / 32; }
__host__ __device__ constexpr int als_groups(int m) { return (m + 63) / 64; }
// uint16 entries of the row half's image: tiles x two planes x KS k-steps x
// 64 lanes x 8 columns
__host__ __device__ constexpr int64_t als_row_image_shorts(int m, int kr) {
  return (int64_t)als_tiles(kr) * 2 * als_ks(m) * 512;
}
// doubles of the column half's partials per row chunk: groups x 4 waves x
// tiles x 256
__host__ __device__ constexpr int64_t als_col_chunk_doubles(int m, int kr) {
  return (int64_t)als_groups(m) * 4 * als_tiles(kr) * 256;
}
__host__ __device__ constexpr bool als_shape_ok(int m, int kr) {
  return m >= 1 && m <= ALS_MAX_COLS && kr >= 4 && kr <= ALS_MAX_RANK && kr % 4 == 0;
}
// K33: point-in-polygon membership (polygon_raycast.hip). The band-edge
// image is nrec records of PIP_RECORD_BYTES followed by the nbands + 1 int32
// band offsets, padded to 16 bytes. A block stages it in LDS when it fits
// PIP_LDS_BYTES: 40 KiB leaves room for four 256-thread blocks (16 waves) on
// a CU's 160 KiB, and the launch asks for the image's own size, so the small
// polygons of the streaming case run eight blocks per CU. Larger images are
// read from global memory.
constexpr int PIP_RECORD_BYTES = 48;
constexpr int PIP_LDS_BYTES = 40 * 1024;
constexpr int PIP_MAX_BANDS = 65536;
constexpr int64_t PIP_MAX_RECORDS = (int64_t)1 << 24;
__host__ __device__ constexpr int64_t pip_table_bytes(int64_t nrec, int nbands) {
  return nrec * PIP_RECORD_BYTES + (nbands + 1 + 3) / 4 * 16;
}
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
// split_gram.hip: out is fp64 [k, k]; mean_hi + mean_lo is the fp64 mean
// split into two floats; items as above; an fp32 accumulator is flushed
// into fp64 every flush_slabs macro-slabs; partials holds
// row_chunks * nitems * SPLITGRAM_ITEM_DOUBLES doubles. n >= 1.
int anovos_split_gram(const void *const *cols, int64_t n, int k, const float *mean_hi,
                      const float *mean_lo, const int *item_gi, const int *item_gj, int nitems,
                      int row_chunks, int flush_slabs, double *partials, double *out,
                      hipStream_t stream);
int anovos_split_gram_grid();
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
// project_columns.hip: the scores themselves. wimg as above; one launch
// writes the components [r0, min(r0 + rw_pad, r)) of every row into the
// columns outs[c] (r device pointers, each n floats, 16-byte aligned).
int anovos_project_columns(const void *const *cols, int64_t n, int k, const float *shift,
                           const float *scale, const uint16_t *wimg, int r, int r0, int rw_pad,
                           int blocks, float *const *outs, hipStream_t stream);
// knn_impute.hip: donors is f32 [s, m] row-major with NaN for null, mean_hi +
// mean_lo the per-column centre split into two floats (m entries). The
// image kernel fills img (knn_tiles(s) * knn_tile_shorts(m) uint16) for the
// target column; the apply kernel takes the r tasks rows[0 .. r) of that
// column (row indices into the n-row columns cols[0 .. m); an index outside
// [0, n) counts as a row of nulls) and writes est[r], idx[r, k], d2[r, k].
// cand_idx / cand_d2, if not null, take [r, 4 * KNN_CAND]: every lane's
// candidate list as the filter pass left it (donor -1 / +inf where empty).
// 1 <= m <= KNN_MAX_COLS, 1 <= s <= KNN_MAX_DONORS, 1 <= k <= KNN_MAX_K,
// r >= 1. blocks <= 0: one wave of resident blocks.
int anovos_knn_donor_image(const float *donors, int s, int m, int target, const float *mean_hi,
                           const float *mean_lo, uint16_t *img, hipStream_t stream);
int anovos_knn_impute(const void *const *cols, int64_t n, int m, const int64_t *rows, int64_t r,
                      const float *mean_hi, const float *mean_lo, const float *donors, int s,
                      int target, int k, const uint16_t *img, int blocks, float *est, int *idx,
                      float *d2, int *cand_idx, float *cand_d2, hipStream_t stream);
// mlp_encode.hip: W1 [n1, d], W2 [n2, n1], W3 [n3, n2] f32 row-major, b1 / b2
// / b3 their biases; widths within mlp_widths_ok. The image kernel fills img
// (mlp_image_shorts uint16, 16-byte aligned) once per call; the encode
// kernel writes y = W3 relu(W2 relu(W1 z + b1) + b2) + b3 of every row into
// the columns outs[c] (n3 device pointers, each n floats, 16-byte aligned).
// n >= 1. blocks <= 0: one wave of resident blocks.
int anovos_mlp_weight_image(const float *W1, const float *b1, const float *W2, const float *b2,
                            const float *W3, const float *b3, int d, int n1, int n2, int n3,
                            uint16_t *img, hipStream_t stream);
int anovos_mlp_encode(const void *const *cols, int64_t n, int d, const float *shift,
                      const float *scale, const uint16_t *img, int n1, int n2, int n3, int blocks,
                      float *const *outs, hipStream_t stream);
// chain_impute.hip: C is f32 [R, m_s, m] row-major (zero outside a step's
// neighbours and at its own target), beta f32 [R, m_s], order int32 [m_s]
// with distinct entries in [0, m), mean_hi + mean_lo the fp64 centre split
// into two floats, lo / hi f32 [m] clip bounds of the centred values (may be
// -inf / +inf); shapes within chain_shape_ok. The image kernel fills img
// (chain_image_shorts uint16, 16-byte aligned) once per call; the apply
// kernel writes z_j + mean_hi[j] to outs[j][i] for every null x_j[i] of a
// column j that is in order and has outs[j] != null (m device pointers, each
// n floats), and nothing else. n >= 1. blocks <= 0: one wave of resident
// blocks.
int anovos_chain_image(const float *C, const float *beta, int m, int m_s, int R, uint16_t *img,
                       hipStream_t stream);
int anovos_chain_impute(const void *const *cols, int64_t n, int m, int m_s, int R,
                        const float *mean_hi, const float *mean_lo, const int *order,
                        const float *C, const uint16_t *img, const float *lo, const float *hi,
                        int blocks, float *const *outs, hipStream_t stream);
// als_sweep.hip: kr in {4, 8, 12, 16}, 1 <= m <= ALS_MAX_COLS; mean_hi +
// mean_lo the fp64 centre split into two floats, scale = 1 / sd, all f32 [m].
// Row half: V is f32 [m, kr] (padding components zero); the image kernel
// fills img (als_row_image_shorts uint16, 16-byte aligned) once per call.
// Any of the three outputs may be null: outs (m device pointers, null or n
// floats each) takes fmaf(u . v_j, sd_j, mean_hi_j) at the null entries of
// column j and nothing else; U (kr columns of ldu floats, ldu a multiple of
// 64 and >= n, 16-byte aligned) takes the solutions, zero at the rows past
// n; normal f32 [n, als_tri(kr) + kr] the normal equations before the
// regulariser. n >= 1, reg > 0. blocks <= 0: one wave of resident blocks.
// Column half: U as above with ldu a multiple of 4; out is fp64 [m,
// als_tri(kr) + kr]; partials holds row_chunks * als_col_chunk_doubles.
int anovos_als_row_image(const float *V, int m, int kr, uint16_t *img, hipStream_t stream);
int anovos_als_row_solve(const void *const *cols, int64_t n, int m, int kr, const float *mean_hi,
                         const float *mean_lo, const float *scale, const float *sd, const float *V,
                         const uint16_t *img, float reg, int blocks, float *const *outs, float *U,
                         int64_t ldu, float *normal, hipStream_t stream);
int anovos_als_col_normal(const void *const *cols, int64_t n, int m, int kr, const float *mean_hi,
                          const float *mean_lo, const float *scale, const float *U, int64_t ldu,
                          int row_chunks, double *partials, double *out, hipStream_t stream);
int anovos_als_col_grid(int kr);
// polygon_raycast.hip: edges is fp64 [E, 5] = (px, py, qx, qy, ring) without
// horizontal edges, band_off int32 [nbands + 1] ascending from 0 to nrec,
// band_edges int32 [nrec] with entries in [0, E), every band's entries in
// ring order. The table kernel fills image (pip_table_bytes, 16-byte
// aligned) once per call. The membership kernel serves npairs (lat, lon)
// column pairs of one dtype, lens[p] rows each (maxn the longest, >= 1), and
// writes 1 / 0 / NaN to outs[p][0 .. lens[p]); band(y) is defined by ymin,
// ymax and scale = nbands / (ymax - ymin) as the file header states. use_lds
// needs pip_table_bytes <= PIP_LDS_BYTES. blocks <= 0: one wave of resident
// blocks.
int anovos_pip_table(const double *edges, const int *band_off, const int *band_edges,
                     int64_t nrec, int nbands, void *image, hipStream_t stream);
int anovos_points_in_polygons(const void *const *lats, const void *const *lons,
                              const int64_t *lens, int npairs, int64_t maxn, int dtype,
                              const void *image, int64_t nrec, int nbands, double ymin,
                              double ymax, double scale, int use_lds, int blocks,
                              float *const *outs, hipStream_t stream);
}
