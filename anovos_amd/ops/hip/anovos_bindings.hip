// Torch bindings for the anovos_amd MI355X kernels (anovos_kernels.hip,
// corr_mfma.hip, pair_counts.hip, grouped_moments.hip, grades.hip,
// pairwise_gram.hip, row_quadform.hip). Compiled by torch.utils.cpp_extension
// with hipcc for gfx950; streams come from the caller's current torch HIP
// stream so kernels compose with the engine's side-stream overlap
// (core/dist.py SideStream).
//
// Every binding has the same shape: gather_columns() validates the column
// list, the binding validates its other arguments, and only then is
// anything allocated, uploaded or launched. Mixed f32 / f64 lists run one
// launch per dtype (split_by_dtype) and scatter back by original position.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <vector>

#include "anovos_kernels.h"

namespace {

hipStream_t current_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_hip(int err, const char *what) {
  TORCH_CHECK(err == 0, what, " failed: ", hipGetErrorString((hipError_t)err));
}

int pick_chunks(int64_t n, int ncols) {
  // fill 256 CUs x 8 XCDs: target >= ~2048 workgroups, >= ~64K elems/chunk
  int64_t by_size = (n + (1 << 16) - 1) >> 16;
  int64_t cap = std::max<int64_t>(1, 16384 / std::max(1, ncols));
  int64_t c = std::min<int64_t>(std::max<int64_t>(by_size, 1), cap);
  int64_t floor_c = std::min<int64_t>(by_size, std::max<int64_t>(1, 2048 / std::max(1, ncols)));
  return (int)std::max<int64_t>(c, std::max<int64_t>(floor_c, 1));
}

torch::TensorOptions on(const torch::Device &dev, torch::ScalarType t) {
  return torch::TensorOptions().dtype(t).device(dev);
}

// Host array (int64 / int32 / double / float) -> device tensor: a
// non-blocking copy from a pageable tensor that owns its bytes. An empty
// array uploads as one zero, so data_ptr() is never null.
template <typename T>
torch::Tensor upload(const std::vector<T> &vals, const torch::Device &dev) {
  auto cpu = torch::zeros({(int64_t)std::max<size_t>(vals.size(), 1)},
                          torch::TensorOptions().dtype(c10::CppTypeToScalarType<T>::value));
  if (!vals.empty()) std::memcpy(cpu.template data_ptr<T>(), vals.data(), vals.size() * sizeof(T));
  return cpu.to(dev, /*non_blocking=*/true);
}

// An uploaded array of addresses, as the pointer table a launcher takes.
template <typename T>
T *const *ptr_table(const torch::Tensor &t) {
  return (T *const *)t.data_ptr<int64_t>();
}

template <typename T>
std::vector<T> pick(const std::vector<T> &vals, const std::vector<int64_t> &idx) {
  std::vector<T> out;
  for (int64_t i : idx) out.push_back(vals[i]);
  return out;
}

// Allowed column dtypes of a binding: bit (1 << dtype code), where the
// code is what the launchers take as `dtype`.
constexpr int F32 = 1, F64 = 2, I32 = 4;

// The columns of one binding call (or, after split_by_dtype, of one
// launch): every kernel reads a column as a dense array from data_ptr().
struct ColumnBatch {
  const char *name;
  torch::Device device;
  int dtype = -1;                  // common dtype code, -1 when mixed
  std::vector<int64_t> ptrs, lens;
  std::vector<int64_t> idx;        // position in the binding's column list
  std::vector<int> dtypes;         // 0 f32, 1 f64, 2 int32
  int64_t maxn = 0;

  int ncols() const { return (int)ptrs.size(); }
  void add(int64_t ptr, int64_t len, int64_t i, int d) {
    dtype = ptrs.empty() || dtype == d ? d : -1;
    ptrs.push_back(ptr);
    lens.push_back(len);
    idx.push_back(i);
    dtypes.push_back(d);
    maxn = std::max(maxn, len);
  }
};

// Refuses, before anything touches the device: an empty list, host
// tensors, a second device, strided views, dtypes outside `allowed` and,
// with equal_len, columns of differing length.
ColumnBatch gather_columns(const std::vector<torch::Tensor> &cols, const char *name, int allowed,
                           bool equal_len = false) {
  TORCH_CHECK(!cols.empty(), name, ": no columns");
  ColumnBatch b{name, cols[0].device()};
  TORCH_CHECK(b.device.is_cuda(), name, ": device columns required");
  for (size_t i = 0; i < cols.size(); ++i) {
    auto &t = cols[i];
    TORCH_CHECK(t.device() == b.device, name, ": columns must be on the same device");
    TORCH_CHECK(t.is_contiguous(), name, ": columns must be contiguous");
    auto st = t.scalar_type();
    int d = st == torch::kFloat32 ? 0 : st == torch::kFloat64 ? 1 : st == torch::kInt32 ? 2 : 3;
    TORCH_CHECK((allowed >> d) & 1, name, ": expected ",
                allowed == I32 ? "int32 code" : allowed == F32 ? "float32"
                : allowed == (F32 | F64) ? "float32/float64"
                : allowed == (F32 | I32) ? "float32/int32" : "float32/float64/int32",
                " columns, got ", st);
    TORCH_CHECK(!equal_len || t.numel() == cols[0].numel(), name,
                ": all columns must have equal length");
    b.add((int64_t)t.data_ptr(), t.numel(), (int64_t)i, d);
  }
  return b;
}

// The f32 columns, then the f64 columns (then int32): one launch each,
// empty groups left out. idx keeps the original positions.
std::vector<ColumnBatch> split_by_dtype(const ColumnBatch &all) {
  std::vector<ColumnBatch> out;
  for (int d = 0; d < 3; ++d) {
    ColumnBatch b{all.name, all.device};
    for (int j = 0; j < all.ncols(); ++j)
      if (all.dtypes[j] == d) b.add(all.ptrs[j], all.lens[j], all.idx[j], d);
    if (b.ncols()) out.push_back(std::move(b));
  }
  return out;
}

std::vector<int64_t> out_ptrs(const std::vector<torch::Tensor> &outs, const ColumnBatch &b) {
  std::vector<int64_t> p;
  for (int64_t i : b.idx) p.push_back((int64_t)outs[i].data_ptr());
  return p;
}

void check_count(size_t got, size_t want, const char *name, const char *what) {
  TORCH_CHECK(got == want, name, ": ", what, " has ", got, " entries, expected ", want);
}

// A per-column / per-bracket parameter array as fp64, on the host ...
std::vector<double> host_f64(const torch::Tensor &t, size_t count, const char *name,
                             const char *what) {
  check_count((size_t)t.numel(), count, name, what);
  auto c = t.to(torch::kFloat64).cpu().contiguous();
  return std::vector<double>(c.data_ptr<double>(), c.data_ptr<double>() + c.numel());
}

// ... or dense on the device.
torch::Tensor device_f64(const torch::Tensor &t, size_t count, const ColumnBatch &b,
                         const char *what) {
  check_count((size_t)t.numel(), count, b.name, what);
  return t.to(torch::kFloat64).to(b.device).contiguous();
}

// `label` / `out`: read or written through data_ptr() next to the columns.
void check_dense_on_device(const torch::Tensor &t, const ColumnBatch &b, const char *what,
                           torch::ScalarType st, int64_t numel) {
  TORCH_CHECK(t.device() == b.device && t.is_contiguous() && t.scalar_type() == st, b.name, ": ",
              what, " must be a contiguous ", st, " tensor on the columns' device");
  TORCH_CHECK(t.numel() == numel, b.name, ": column/", what, " length mismatch");
}

// Cutoffs of the columns of one launch, flattened: column j's are
// flat[offs[j] .. offs[j] + lens[j]); max_ncut >= 1 sizes the kernel's LDS.
struct CutoffTable {
  std::vector<double> flat;
  std::vector<int64_t> offs;
  std::vector<int> lens;
  int max_ncut = 1;
};

CutoffTable cutoff_table(const std::vector<torch::Tensor> &cutoffs, const std::vector<int64_t> &idx) {
  CutoffTable ct;
  for (int64_t i : idx) {
    auto cc = cutoffs[i].to(torch::kFloat64).cpu().contiguous();
    const double *cd = cc.data_ptr<double>();
    ct.offs.push_back((int64_t)ct.flat.size());
    ct.flat.insert(ct.flat.end(), cd, cd + cc.numel());
    ct.lens.push_back((int)cc.numel());
    ct.max_ncut = std::max(ct.max_ncut, (int)cc.numel());
  }
  return ct;
}

// Null lane masks of one binding call, by original column position: an
// int64 tensor of nchunks * null_mask_chunk_words(per) words and the
// partition {n, nchunks, per} it was made with; an undefined tensor and an
// empty partition for a column whose launch emits none.
struct NullMasks {
  std::vector<torch::Tensor> masks;
  std::vector<std::vector<int64_t>> parts;
  explicit NullMasks(size_t ncols) : masks(ncols), parts(ncols) {}

  // allocates column i's mask (left unwritten: the kernel writes every
  // word the reader looks at) and returns its address
  int64_t add(int64_t i, int64_t n, int nchunks, const torch::Device &dev) {
    const int64_t per = (n + nchunks - 1) / nchunks;
    masks[i] = torch::empty({nchunks * null_mask_chunk_words(per)}, on(dev, torch::kInt64));
    parts[i] = {n, (int64_t)nchunks, per};
    return (int64_t)masks[i].data_ptr();
  }
};

// K1/K2 (p < 0) and K1/K2+K4 fused (p >= 0: HLL registers from the same
// read; with `nm` the f32 launch also fills the columns' null lane masks).
std::tuple<torch::Tensor, torch::Tensor> moments_body(const std::vector<torch::Tensor> &cols,
                                                      const std::vector<double> &shifts,
                                                      int64_t p, const char *name,
                                                      NullMasks *nm = nullptr) {
  ColumnBatch all = gather_columns(cols, name, F32 | F64);
  if (!shifts.empty()) check_count(shifts.size(), cols.size(), name, "shifts");
  auto device = all.device;
  const bool hll = p >= 0;
  const int64_t m = hll ? (int64_t)1 << p : 0;
  auto mom = torch::zeros({all.ncols(), 9}, on(device, torch::kFloat64));
  torch::Tensor regs, reg_sub;
  if (hll) regs = torch::zeros({all.ncols(), m}, on(device, torch::kInt32));
  for (auto &b : split_by_dtype(all)) {
    int ncols = b.ncols();
    int nchunks = pick_chunks(b.maxn, ncols);
    auto dptr = upload(b.ptrs, device);
    auto dlen = upload(b.lens, device);
    auto dsh = upload(shifts.empty() ? std::vector<double>(ncols, 0.0) : pick(shifts, b.idx), device);
    auto partials = torch::empty({(int64_t)ncols * nchunks, 9}, on(device, torch::kFloat64));
    auto sub = torch::empty({ncols, 9}, on(device, torch::kFloat64));
    if (hll) {
      reg_sub = torch::zeros({ncols, m}, on(device, torch::kInt32));
      torch::Tensor dmask;
      if (nm && b.dtype == 0) {
        std::vector<int64_t> mptrs;
        for (int j = 0; j < ncols; ++j) mptrs.push_back(nm->add(b.idx[j], b.lens[j], nchunks, device));
        dmask = upload(mptrs, device);
      }
      check_hip(anovos_moments_hll(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(),
                                   dsh.data_ptr<double>(), ncols, (int)p, nchunks, b.dtype,
                                   partials.data_ptr<double>(), sub.data_ptr<double>(),
                                   reg_sub.data_ptr<int>(),
                                   dmask.defined() ? ptr_table<uint64_t>(dmask) : nullptr,
                                   current_stream()),
                "anovos_moments_hll");
    } else {
      check_hip(anovos_moments(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(),
                               dsh.data_ptr<double>(), ncols, nchunks, b.dtype,
                               partials.data_ptr<double>(), sub.data_ptr<double>(),
                               current_stream()),
                "anovos_moments");
    }
    auto didx = upload(b.idx, device);
    mom.index_copy_(0, didx, sub);
    if (hll) regs.index_copy_(0, didx, reg_sub);
  }
  return {mom, regs};
}

// K6 to float bin labels; with_counts adds int64 [ncols, max_ncut + 2] bin
// counts from the same pass (slot 0 nulls, slot b = bin label b), in the
// ORIGINAL column order, local to this rank, left on the device.
std::tuple<std::vector<torch::Tensor>, torch::Tensor> bucketize_float_body(
    const std::vector<torch::Tensor> &cols, const std::vector<torch::Tensor> &cutoffs,
    bool with_counts, const char *name) {
  ColumnBatch all = gather_columns(cols, name, F32 | F64);
  check_count(cutoffs.size(), cols.size(), name, "cutoffs");
  auto device = all.device;
  int64_t stride = 2;
  for (auto &c : cutoffs) {
    TORCH_CHECK(!with_counts || c.numel() <= BKT_COUNTS_MAX_NCUT, name,
                ": cutoff count out of LDS range");
    stride = std::max<int64_t>(stride, c.numel() + 2);
  }
  std::vector<torch::Tensor> outs;
  for (auto &t : cols) outs.push_back(torch::empty(t.sizes(), on(device, torch::kFloat32)));
  torch::Tensor counts;
  if (with_counts) counts = torch::zeros({all.ncols(), stride}, on(device, torch::kInt64));
  for (auto &b : split_by_dtype(all)) {
    CutoffTable ct = cutoff_table(cutoffs, b.idx);
    int nchunks = pick_chunks(b.maxn, b.ncols());
    auto dptr = upload(b.ptrs, device);
    auto dlen = upload(b.lens, device);
    auto dout = upload(out_ptrs(outs, b), device);
    auto doff = upload(ct.offs, device);
    auto dflat = upload(ct.flat, device);
    auto dclen = upload(ct.lens, device);
    if (with_counts) {
      std::vector<int64_t> coffs;
      for (int64_t i : b.idx) coffs.push_back(i * stride);
      auto dcoff = upload(coffs, device);
      check_hip(anovos_bucketize_float_counts(
                    ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(), b.ncols(),
                    dflat.data_ptr<double>(), doff.data_ptr<int64_t>(), dclen.data_ptr<int>(),
                    ct.max_ncut, nchunks, b.dtype, ptr_table<float>(dout),
                    (uint64_t *)counts.data_ptr<int64_t>(), dcoff.data_ptr<int64_t>(),
                    current_stream()),
                "anovos_bucketize_float_counts");
    } else {
      check_hip(anovos_bucketize_float(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(),
                                       b.ncols(), dflat.data_ptr<double>(),
                                       doff.data_ptr<int64_t>(), dclen.data_ptr<int>(),
                                       ct.max_ncut, nchunks, b.dtype, ptr_table<float>(dout),
                                       current_stream()),
                "anovos_bucketize_float");
    }
  }
  return {outs, counts};
}

// K12: out = lut[code], one LUT per column, T = float or int32_t.
template <typename T, typename Launcher>
std::vector<torch::Tensor> lut_apply_body(const std::vector<torch::Tensor> &cols,
                                          const std::vector<torch::Tensor> &luts,
                                          Launcher launch, const char *name) {
  ColumnBatch b = gather_columns(cols, name, I32);
  check_count(luts.size(), cols.size(), name, "luts");
  const auto st = c10::CppTypeToScalarType<T>::value;
  std::vector<int64_t> offs;
  std::vector<T> flat;
  for (auto &l : luts) {
    auto lc = l.to(st).cpu().contiguous();
    offs.push_back((int64_t)flat.size());
    flat.insert(flat.end(), lc.template data_ptr<T>(), lc.template data_ptr<T>() + lc.numel());
  }
  std::vector<torch::Tensor> outs;
  for (auto &t : cols) outs.push_back(torch::empty(t.sizes(), on(b.device, st)));
  int nchunks = pick_chunks(b.maxn, b.ncols());
  auto dptr = upload(b.ptrs, b.device);
  auto dlen = upload(b.lens, b.device);
  auto dout = upload(out_ptrs(outs, b), b.device);
  auto doff = upload(offs, b.device);
  auto dflat = upload(flat, b.device);
  check_hip(launch(ptr_table<const int32_t>(dptr), dlen.data_ptr<int64_t>(), b.ncols(),
                   dflat.template data_ptr<T>(), doff.data_ptr<int64_t>(), nchunks,
                   ptr_table<T>(dout), current_stream()),
            name);
  return outs;
}

}  // namespace

torch::Tensor column_moments(std::vector<torch::Tensor> cols, std::vector<double> shifts) {
  return std::get<0>(moments_body(cols, shifts, -1, "column_moments"));
}

// K1/K2+K4 fused: moments + HLL registers in one read.
// Returns (moments [ncols,9] f64, regs [ncols, 1<<p] i32); with null_masks
// also (masks, partitions) per column, None / [] for the f64 columns.
py::object moments_hll(std::vector<torch::Tensor> cols, int64_t p, std::vector<double> shifts,
                       bool null_masks) {
  TORCH_CHECK(p >= 0, "moments_hll: p must not be negative");
  if (!null_masks) return py::cast(moments_body(cols, shifts, p, "moments_hll"));
  NullMasks nm(cols.size());
  auto r = moments_body(cols, shifts, p, "moments_hll", &nm);
  return py::make_tuple(std::get<0>(r), std::get<1>(r), nm.masks, nm.parts);
}

torch::Tensor column_histograms(std::vector<torch::Tensor> cols, torch::Tensor lo,
                                torch::Tensor hi, int64_t nbins) {
  ColumnBatch all = gather_columns(cols, "column_histograms", F32 | F64);
  auto device = all.device;
  auto lo_d = device_f64(lo, cols.size(), all, "lo");
  auto hi_d = device_f64(hi, cols.size(), all, "hi");
  auto out = torch::zeros({all.ncols(), nbins}, on(device, torch::kInt64));
  for (auto &b : split_by_dtype(all)) {
    int nchunks = pick_chunks(b.maxn, b.ncols());
    auto dptr = upload(b.ptrs, device);
    auto dlen = upload(b.lens, device);
    auto didx = upload(b.idx, device);
    auto sub = torch::zeros({b.ncols(), nbins}, on(device, torch::kInt64));
    auto lo_sel = lo_d.index_select(0, didx);
    auto hi_sel = hi_d.index_select(0, didx);
    check_hip(anovos_hist(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(), b.ncols(),
                          lo_sel.data_ptr<double>(), hi_sel.data_ptr<double>(), (int)nbins,
                          nchunks, b.dtype, (uint64_t *)sub.data_ptr<int64_t>(),
                          current_stream()),
              "anovos_hist");
    out.index_copy_(0, didx, sub);
  }
  return out;
}

torch::Tensor bracket_histograms(std::vector<torch::Tensor> cols, torch::Tensor colidx,
                                 torch::Tensor lo, torch::Tensor hi, int64_t nbins) {
  ColumnBatch b = gather_columns(cols, "bracket_histograms", F32 | F64);
  TORCH_CHECK(b.dtype >= 0, "bracket_histograms: mixed dtypes unsupported");
  auto ci_h = colidx.to(torch::kInt64).cpu().contiguous();
  int nbrackets = (int)ci_h.numel();
  for (int i = 0; i < nbrackets; ++i) {
    int64_t c = ci_h.data_ptr<int64_t>()[i];
    TORCH_CHECK(c >= 0 && c < b.ncols(), "bracket_histograms: colidx entry ", c, " outside [0, ",
                b.ncols(), ")");
  }
  auto lo_d = device_f64(lo, nbrackets, b, "lo");
  auto hi_d = device_f64(hi, nbrackets, b, "hi");
  auto ci = ci_h.to(b.device);
  auto dptr = upload(b.ptrs, b.device);
  auto dlen = upload(b.lens, b.device);
  int nchunks = pick_chunks(b.maxn, nbrackets);
  auto out = torch::zeros({nbrackets, nbins}, on(b.device, torch::kInt64));
  check_hip(anovos_bracket_hist(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(),
                                ci.data_ptr<int64_t>(), nbrackets, lo_d.data_ptr<double>(),
                                hi_d.data_ptr<double>(), (int)nbins, nchunks, b.dtype,
                                (uint64_t *)out.data_ptr<int64_t>(), current_stream()),
            "anovos_bracket_hist");
  return out;
}

std::vector<torch::Tensor> bucketize_columns(std::vector<torch::Tensor> cols,
                                             std::vector<torch::Tensor> cutoffs) {
  ColumnBatch all = gather_columns(cols, "bucketize_columns", F32 | F64);
  check_count(cutoffs.size(), cols.size(), all.name, "cutoffs");
  auto device = all.device;
  std::vector<torch::Tensor> outs;
  for (auto &t : cols) outs.push_back(torch::empty_like(t, on(device, torch::kInt32)));
  for (auto &b : split_by_dtype(all)) {
    CutoffTable ct = cutoff_table(cutoffs, b.idx);
    int nchunks = pick_chunks(b.maxn, b.ncols());
    auto dptr = upload(b.ptrs, device);
    auto dlen = upload(b.lens, device);
    auto dout = upload(out_ptrs(outs, b), device);
    auto doff = upload(ct.offs, device);
    auto dflat = upload(ct.flat, device);
    auto dclen = upload(ct.lens, device);
    check_hip(anovos_bucketize(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(), b.ncols(),
                               dflat.data_ptr<double>(), doff.data_ptr<int64_t>(),
                               dclen.data_ptr<int>(), ct.max_ncut, nchunks, b.dtype,
                               ptr_table<int32_t>(dout), current_stream()),
              "anovos_bucketize");
  }
  return outs;
}

torch::Tensor code_counts(torch::Tensor codes, int64_t size) {
  ColumnBatch b = gather_columns({codes}, "code_counts", I32);
  TORCH_CHECK(size >= 0 && size < INT32_MAX, "code_counts: dictionary size out of range");
  auto out = torch::zeros({std::max<int64_t>(size, 1)}, on(b.device, torch::kInt64));
  if (size == 0 || codes.numel() == 0) return out.narrow(0, 0, size);
  int nchunks = pick_chunks(codes.numel(), 1);
  nchunks = std::min(nchunks, 8192);
  check_hip(anovos_code_counts(codes.data_ptr<int32_t>(), codes.numel(), (int)size, nchunks,
                               (uint64_t *)out.data_ptr<int64_t>(), current_stream()),
            "anovos_code_counts");
  return out;
}

torch::Tensor hll_registers(torch::Tensor x, int64_t p) {
  ColumnBatch b = gather_columns({x}, "hll_registers", F32 | F64);
  auto regs = torch::zeros({(int64_t)1 << p}, on(b.device, torch::kInt32));
  if (x.numel() == 0) return regs;
  int nchunks = std::min(pick_chunks(x.numel(), 1), 4096);
  check_hip(anovos_hll(x.data_ptr(), x.numel(), (int)p, nchunks, b.dtype,
                       regs.data_ptr<int32_t>(), current_stream()),
            "anovos_hll");
  return regs;
}

// K10: adds every row's null count into `out`; accepts float32/float64
// (NaN null) AND int32 dictionary codes (-1 null), one launch per dtype.
// K10m: adds the row null counts of the columns whose null lane masks are
// given into `out`; the masks share one partition {n, nchunks, per}.
void row_null_counts_masked(std::vector<torch::Tensor> masks, std::vector<int64_t> partition,
                            torch::Tensor out) {
  const char *name = "row_null_counts_masked";
  TORCH_CHECK(!masks.empty(), name, ": no columns");
  check_count(partition.size(), 3, name, "partition");
  const int64_t n = partition[0], nchunks = partition[1], per = partition[2];
  TORCH_CHECK(n >= 0 && nchunks >= 1 && nchunks <= INT32_MAX && per == (n + nchunks - 1) / nchunks,
              name, ": partition is not {n, nchunks, ceil(n / nchunks)}");
  auto device = masks[0].device();
  TORCH_CHECK(device.is_cuda(), name, ": device masks required");
  const int64_t words = nchunks * null_mask_chunk_words(per);
  std::vector<int64_t> ptrs;
  for (auto &t : masks) {
    TORCH_CHECK(t.device() == device && t.is_contiguous() && t.scalar_type() == torch::kInt64, name,
                ": masks must be contiguous int64 tensors on one device");
    TORCH_CHECK(t.numel() == words, name, ": a mask has ", t.numel(), " words, its partition needs ",
                words);
    // the kernel reads a group as one 32-byte-aligned vector
    TORCH_CHECK((int64_t)t.data_ptr() % 32 == 0, name, ": masks must be 32-byte aligned");
    ptrs.push_back((int64_t)t.data_ptr());
  }
  TORCH_CHECK(out.device() == device && out.is_contiguous() && out.scalar_type() == torch::kInt32,
              name, ": out must be a contiguous int32 tensor on the masks' device");
  TORCH_CHECK(out.numel() == n, name, ": mask/out length mismatch");
  auto dptr = upload(ptrs, device);
  check_hip(anovos_row_null_masked(ptr_table<const uint64_t>(dptr), (int)ptrs.size(), n,
                                   (int)nchunks, per, out.data_ptr<int32_t>(), current_stream()),
            "anovos_row_null_masked");
}

void row_null_counts_num(std::vector<torch::Tensor> cols, torch::Tensor out) {
  ColumnBatch all = gather_columns(cols, "row_null_counts_num", F32 | F64 | I32, /*equal_len=*/true);
  check_dense_on_device(out, all, "out", torch::kInt32, all.maxn);
  for (auto &b : split_by_dtype(all)) {
    auto dptr = upload(b.ptrs, b.device);
    check_hip(anovos_row_null(ptr_table<const void>(dptr), b.ncols(), out.numel(), b.dtype,
                              out.data_ptr<int32_t>(), current_stream()),
              "anovos_row_null");
  }
}

torch::Tensor hll_registers_multi(std::vector<torch::Tensor> cols, int64_t p) {
  ColumnBatch all = gather_columns(cols, "hll_registers_multi", F32 | F64);
  auto device = all.device;
  auto regs = torch::zeros({all.ncols(), (int64_t)1 << p}, on(device, torch::kInt32));
  for (auto &b : split_by_dtype(all)) {
    // contiguous sub-block trick: launch on a per-pass register buffer
    auto sub = torch::zeros({b.ncols(), (int64_t)1 << p}, on(device, torch::kInt32));
    auto dptr = upload(b.ptrs, device);
    auto dlen = upload(b.lens, device);
    int nchunks = std::max(1, std::min((int)((b.maxn + (1 << 20) - 1) >> 20), 4096 / b.ncols() + 1));
    check_hip(anovos_hll_multi(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(), b.ncols(),
                               (int)p, nchunks, b.dtype, sub.data_ptr<int32_t>(),
                               current_stream()),
              "anovos_hll_multi");
    regs.index_copy_(0, upload(b.idx, device), sub);
  }
  return regs;
}

std::vector<torch::Tensor> scale_columns(std::vector<torch::Tensor> cols, torch::Tensor a,
                                         torch::Tensor b) {
  ColumnBatch all = gather_columns(cols, "scale_columns", F32 | F64);
  auto av = host_f64(a, cols.size(), all.name, "a");
  auto bv = host_f64(b, cols.size(), all.name, "b");
  auto device = all.device;
  std::vector<torch::Tensor> outs;
  for (auto &t : cols) outs.push_back(torch::empty(t.sizes(), on(device, torch::kFloat32)));
  for (auto &g : split_by_dtype(all)) {
    int nchunks = pick_chunks(g.maxn, g.ncols());
    auto dptr = upload(g.ptrs, device);
    auto dlen = upload(g.lens, device);
    auto dout = upload(out_ptrs(outs, g), device);
    auto da = upload(pick(av, g.idx), device);
    auto db = upload(pick(bv, g.idx), device);
    check_hip(anovos_axpb(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(), g.ncols(),
                          da.data_ptr<double>(), db.data_ptr<double>(), nchunks, g.dtype,
                          ptr_table<float>(dout), current_stream()),
              "anovos_axpb");
  }
  return outs;
}

std::vector<torch::Tensor> fill_nan_columns(std::vector<torch::Tensor> cols, torch::Tensor fill) {
  ColumnBatch all = gather_columns(cols, "fill_nan_columns", F32 | F64);
  auto fv = host_f64(fill, cols.size(), all.name, "fill");
  auto device = all.device;
  std::vector<torch::Tensor> outs;
  for (auto &t : cols) outs.push_back(torch::empty_like(t));
  for (auto &b : split_by_dtype(all)) {
    int nchunks = pick_chunks(b.maxn, b.ncols());
    auto dptr = upload(b.ptrs, device);
    auto dlen = upload(b.lens, device);
    auto dout = upload(out_ptrs(outs, b), device);
    auto df = upload(pick(fv, b.idx), device);
    check_hip(anovos_fillnan(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(), b.ncols(),
                             df.data_ptr<double>(), nchunks, b.dtype, ptr_table<void>(dout),
                             current_stream()),
              "anovos_fillnan");
  }
  return outs;
}

// Fused categorical null-fill: out_i = (code == -1) ? fill_i : code.
std::vector<torch::Tensor> fill_code_columns(std::vector<torch::Tensor> cols,
                                             std::vector<int64_t> fills) {
  ColumnBatch b = gather_columns(cols, "fill_code_columns", I32);
  check_count(fills.size(), cols.size(), b.name, "fills");
  std::vector<torch::Tensor> outs;
  for (auto &t : cols) outs.push_back(torch::empty_like(t));
  int nchunks = pick_chunks(b.maxn, b.ncols());
  auto dptr = upload(b.ptrs, b.device);
  auto dlen = upload(b.lens, b.device);
  auto dout = upload(out_ptrs(outs, b), b.device);
  auto dfill = upload(std::vector<int32_t>(fills.begin(), fills.end()), b.device);
  check_hip(anovos_fill_code(ptr_table<const int32_t>(dptr), dlen.data_ptr<int64_t>(), b.ncols(),
                             dfill.data_ptr<int32_t>(), nchunks, ptr_table<int32_t>(dout),
                             current_stream()),
            "anovos_fill_code");
  return outs;
}

torch::Tensor bracket_histograms_grouped(std::vector<torch::Tensor> cols,
                                         torch::Tensor bracket_col,
                                         torch::Tensor lo, torch::Tensor hi,
                                         torch::Tensor p1lo, torch::Tensor p1scale,
                                         int64_t p1bins) {
  // brackets MUST be sorted by column index; returns [nbrackets, RB_BINS].
  ColumnBatch b = gather_columns(cols, "bracket_histograms_grouped", F32 | F64);
  auto bc = bracket_col.to(torch::kInt64).cpu().contiguous();
  const int64_t *bcol = bc.data_ptr<int64_t>();
  int ncols = b.ncols();
  int nb = (int)bc.numel();
  // dtype uniformity only matters for REFERENCED columns (the host
  // splits mixed-dtype bracket sets into per-dtype launches; columns
  // without brackets in this launch are never read)
  int dtype = -1;
  std::vector<int> bstart(ncols + 1, 0);
  for (int i = 0; i < nb; ++i) {
    TORCH_CHECK(bcol[i] >= 0 && bcol[i] < ncols, b.name, ": bad bracket col");
    if (i) TORCH_CHECK(bcol[i] >= bcol[i - 1], b.name, ": brackets must be sorted by column");
    if (dtype < 0) dtype = b.dtypes[bcol[i]];
    TORCH_CHECK(b.dtypes[bcol[i]] == dtype, "grouped brackets: mixed dtypes in one launch");
    bstart[bcol[i] + 1]++;
  }
  if (dtype < 0) dtype = b.dtypes[0];
  for (int c = 0; c < ncols; ++c) {
    TORCH_CHECK(bstart[c + 1] <= RB_MAXB, b.name, ": at most 16 brackets per column");
    bstart[c + 1] += bstart[c];
  }
  auto lo_d = device_f64(lo, nb, b, "lo");
  auto hi_d = device_f64(hi, nb, b, "hi");
  auto p1lo_d = device_f64(p1lo, ncols, b, "p1lo");
  auto p1scale_d = device_f64(p1scale, ncols, b, "p1scale");
  auto dptr = upload(b.ptrs, b.device);
  auto dlen = upload(b.lens, b.device);
  auto dbs = upload(bstart, b.device);
  int nchunks = pick_chunks(b.maxn, ncols);
  auto out = torch::zeros({nb, RB_BINS}, on(b.device, torch::kInt64));
  check_hip(anovos_bracket_hist_grouped(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(),
                                        dbs.data_ptr<int>(), ncols, lo_d.data_ptr<double>(),
                                        hi_d.data_ptr<double>(), p1lo_d.data_ptr<double>(),
                                        p1scale_d.data_ptr<double>(), (int)p1bins, nchunks, dtype,
                                        (uint64_t *)out.data_ptr<int64_t>(), current_stream()),
            "anovos_bracket_hist_grouped");
  return out;
}

std::vector<torch::Tensor> bucketize_columns_float(std::vector<torch::Tensor> cols,
                                                   std::vector<torch::Tensor> cutoffs) {
  return std::get<0>(bucketize_float_body(cols, cutoffs, false, "bucketize_columns_float"));
}

std::tuple<std::vector<torch::Tensor>, torch::Tensor> bucketize_columns_float_counts(
    std::vector<torch::Tensor> cols, std::vector<torch::Tensor> cutoffs) {
  return bucketize_float_body(cols, cutoffs, true, "bucketize_columns_float_counts");
}

std::vector<torch::Tensor> lut_apply_f32(std::vector<torch::Tensor> cols,
                                         std::vector<torch::Tensor> luts) {
  return lut_apply_body<float>(cols, luts, anovos_lut_apply_f32, "lut_apply_f32");
}

std::vector<torch::Tensor> lut_apply_i32(std::vector<torch::Tensor> cols,
                                         std::vector<torch::Tensor> luts) {
  return lut_apply_body<int32_t>(cols, luts, anovos_lut_apply_i32, "lut_apply_i32");
}

// K8: bf16 MFMA centered Gram — gram[i][j] = sum (x_i - mean_i)(x_j - mean_j)
torch::Tensor centered_gram_bf16(std::vector<torch::Tensor> cols, torch::Tensor means) {
  ColumnBatch b = gather_columns(cols, "centered_gram_bf16", F32, /*equal_len=*/true);
  check_count((size_t)means.numel(), cols.size(), b.name, "means");
  auto device = b.device;
  const int k = b.ncols();
  const int64_t n = b.maxn;
  auto means_d = means.to(device, torch::kFloat32).contiguous();
  const int kt = (k + 15) / 16;
  std::vector<int> pi_h, pj_h;
  for (int i = 0; i < kt; ++i)
    for (int j = i; j < kt; ++j) {
      pi_h.push_back(i);
      pj_h.push_back(j);
    }
  const int npairs = (int)pi_h.size();
  auto pi = upload(pi_h, device);
  auto pj = upload(pj_h, device);
  auto dptr = upload(b.ptrs, device);
  auto gram = torch::zeros({k, k}, on(device, torch::kFloat32));
  if (kt <= 13) {
    // single-read kernel: one block stages 128-row macro-slabs of ALL
    // columns through LDS; HBM traffic = n*k*4 bytes (vs ~kt x for
    // pair-parallel)
    const int64_t steps_total = (n + 31) / 32;
    // one full wave of resident blocks (occupancy x CUs), so every block
    // starts at once and owns one contiguous row range (see
    // anovos_gram_sr_grid); blocks past the last macro-slab add zeros
    int64_t target_chunks = anovos_gram_sr_grid(k);
    if (const char *e = getenv("ANOVOS_GRAM_CHUNKS")) target_chunks = atoll(e);
    int row_chunks = (int)std::min<int64_t>(target_chunks, std::max<int64_t>(1, steps_total));
    auto partials = torch::empty({(int64_t)row_chunks * npairs, 256}, on(device, torch::kFloat32));
    check_hip(anovos_centered_gram_sr(ptr_table<const void>(dptr), n, k, means_d.data_ptr<float>(),
                                      pi.data_ptr<int>(), pj.data_ptr<int>(), npairs, row_chunks,
                                      partials.data_ptr<float>(), gram.data_ptr<float>(),
                                      current_stream()),
              "anovos_centered_gram_sr");
    return gram;
  }
  // wide matrices: pair-parallel kernel (re-reads columns, but register
  // budget no longer admits the all-pairs accumulator set)
  int row_chunks = (int)std::min<int64_t>(std::max<int64_t>(1, 2048 / std::max(npairs, 1)),
                                          std::max<int64_t>(1, n >> 16));
  row_chunks = std::max(row_chunks, 1);
  auto partials = torch::empty({(int64_t)npairs * row_chunks, 256}, on(device, torch::kFloat32));
  check_hip(anovos_centered_gram(ptr_table<const void>(dptr), n, k, means_d.data_ptr<float>(),
                                 pi.data_ptr<int>(), pj.data_ptr<int>(), npairs, row_chunks,
                                 partials.data_ptr<float>(), gram.data_ptr<float>(),
                                 current_stream()),
            "anovos_centered_gram");
  return gram;
}

// K25: pairwise-complete Gram sums, fp64 [4, k, k] = (N, P, S, Q) with
// m = !isnan(x), z = m ? x - mean : 0: N = sum m_i m_j, P = sum z_i z_j,
// S[i][j] = sum z_i m_j, Q[i][j] = sum z_i^2 m_j (pairwise_gram.hip).
torch::Tensor pairwise_gram_bf16(std::vector<torch::Tensor> cols, torch::Tensor means) {
  ColumnBatch b = gather_columns(cols, "pairwise_gram_bf16", F32, /*equal_len=*/true);
  check_count((size_t)means.numel(), cols.size(), b.name, "means");
  TORCH_CHECK(means.device() == b.device, b.name, ": means must be on the columns' device");
  auto device = b.device;
  const int k = b.ncols();
  const int64_t n = b.maxn;
  auto means_d = means.to(torch::kFloat32).contiguous();
  const int groups = (k + 16 * PAIRGRAM_GROUP_TILES - 1) / (16 * PAIRGRAM_GROUP_TILES);
  std::vector<int> gi_h, gj_h;
  for (int i = 0; i < groups; ++i)
    for (int j = i; j < groups; ++j) {
      gi_h.push_back(i);
      gj_h.push_back(j);
    }
  const int64_t nitems = (int64_t)gi_h.size();
  // Row split: one wave of resident blocks over all items (see
  // anovos_gram_sr_grid), at least the split that keeps every block below
  // PAIRGRAM_MAX_BLOCK_ROWS rows (its fp32 counts are exact up to there; a
  // forced smaller split is raised to it), at most one macro-slab per block.
  const int64_t macro_total = (n + PAIRGRAM_SLAB_ROWS - 1) / PAIRGRAM_SLAB_ROWS;
  const int64_t macro_cap = PAIRGRAM_MAX_BLOCK_ROWS / PAIRGRAM_SLAB_ROWS - 1;
  const int64_t min_chunks = std::max<int64_t>(1, (macro_total + macro_cap - 1) / macro_cap);
  const int64_t capacity = std::max(1, anovos_pairwise_gram_grid());
  int64_t target_chunks = std::max<int64_t>(1, capacity / nitems);
  if (const char *e = getenv("ANOVOS_PAIRGRAM_CHUNKS")) target_chunks = atoll(e);
  const int row_chunks = (int)std::max<int64_t>(
      min_chunks, std::min<int64_t>(target_chunks, std::max<int64_t>(1, macro_total)));
  // Items per launch: what one wave of blocks holds, so that the partials
  // stay bounded however many groups k makes.
  const int64_t per_launch = std::max<int64_t>(1, std::min(nitems, capacity / row_chunks));
  auto gi = upload(gi_h, device);
  auto gj = upload(gj_h, device);
  auto dptr = upload(b.ptrs, device);
  auto out = torch::zeros({4, k, k}, on(device, torch::kFloat64));
  auto partials = torch::empty({(int64_t)row_chunks * per_launch, PAIRGRAM_ITEM_FLOATS},
                               on(device, torch::kFloat32));
  for (int64_t item0 = 0; item0 < nitems; item0 += per_launch) {
    const int cnt = (int)std::min(per_launch, nitems - item0);
    check_hip(anovos_pairwise_gram(ptr_table<const void>(dptr), n, k, means_d.data_ptr<float>(),
                                   gi.data_ptr<int>() + item0, gj.data_ptr<int>() + item0, cnt,
                                   row_chunks, partials.data_ptr<float>(),
                                   out.data_ptr<double>(), current_stream()),
              "anovos_pairwise_gram");
  }
  return out;
}

// K26: d2[n] = |W z|^2 per row, z_j = isnan(x_j) ? 0 : (x_j - shift_j) * scale_j,
// split-bf16 MFMA with fp32 accumulation (row_quadform.hip). W is [r, k],
// r <= k; where its two bf16 planes do not fit in LDS beside the slab, one
// launch per window of its rows, the later ones adding into d2.
torch::Tensor row_quadform_bf16x2(std::vector<torch::Tensor> cols, torch::Tensor shift,
                                  torch::Tensor scale, torch::Tensor W) {
  ColumnBatch b = gather_columns(cols, "row_quadform_bf16x2", F32, /*equal_len=*/true);
  check_count((size_t)shift.numel(), cols.size(), b.name, "shift");
  check_count((size_t)scale.numel(), cols.size(), b.name, "scale");
  TORCH_CHECK(W.dim() == 2 && W.is_floating_point(), b.name,
              ": W must be a 2-D floating-point tensor");
  const int64_t k = b.ncols();
  const int64_t r = W.size(0);
  TORCH_CHECK(W.size(1) == k, b.name, ": W has ", W.size(1), " columns, expected ", k);
  TORCH_CHECK(k <= ROWQUAD_MAX_COLS, b.name, ": ", k, " columns, at most ", ROWQUAD_MAX_COLS,
              " (ROWQUAD_MAX_COLS)");
  TORCH_CHECK(r >= 1 && r <= k, b.name, ": W has ", r, " rows, expected 1 .. ", k);
  TORCH_CHECK(shift.device() == b.device && scale.device() == b.device && W.device() == b.device,
              b.name, ": shift, scale and W must be on the columns' device");
  auto device = b.device;
  const int64_t n = b.maxn;
  auto out = torch::empty({n}, on(device, torch::kFloat32));
  if (n == 0) return out;
  auto shift_d = shift.to(torch::kFloat32).contiguous();
  auto scale_d = scale.to(torch::kFloat32).contiguous();
  auto W_d = W.to(torch::kFloat32).contiguous();
  const int r_pad = rowquad_rpad((int)r), k_pad = rowquad_kpad((int)k);
  auto wimg = torch::empty({2 * (int64_t)(k_pad / 8) * r_pad * 8}, on(device, torch::kInt16));
  auto dptr = upload(b.ptrs, device);
  int blocks = 0;  // one wave of resident blocks
  if (const char *e = getenv("ANOVOS_ROWQUAD_BLOCKS")) blocks = atoi(e);
  check_hip(anovos_row_quadform_split(W_d.data_ptr<float>(), (int)r, (int)k,
                                      (uint16_t *)wimg.data_ptr<int16_t>(), current_stream()),
            "anovos_row_quadform_split");
  const int window = rowquad_window_rows((int)k);
  for (int r0 = 0; r0 < r_pad; r0 += window)
    check_hip(anovos_row_quadform(ptr_table<const void>(dptr), n, (int)k,
                                  shift_d.data_ptr<float>(), scale_d.data_ptr<float>(),
                                  (const uint16_t *)wimg.data_ptr<int16_t>(), (int)r, r0,
                                  std::min(window, r_pad - r0), /*accumulate=*/r0 > 0, blocks,
                                  out.data_ptr<float>(), current_stream()),
              "anovos_row_quadform");
  return out;
}

// K5 fused: multi-column code counts (+ null slot per column).
// Returns flat int64 tensor of length sum(sizes_i + 1); with null_masks
// (flat, masks, partitions), where the columns that count in LDS get their
// null lane masks from the same read and the others None / [].
py::object code_counts_multi(std::vector<torch::Tensor> cols, std::vector<int64_t> sizes,
                             bool null_masks) {
  ColumnBatch b = gather_columns(cols, "code_counts_multi", I32);
  check_count(sizes.size(), cols.size(), b.name, "sizes");
  std::vector<int64_t> offs;
  int64_t off = 0;
  // the kernel stages a column's counters in LDS when its slots (codes +
  // null slot) number <= CODE_LDS_SLOTS and counts in global memory
  // otherwise, per column: size the LDS for the largest column that
  // stages, not for the largest column of the launch
  int lds_slots = 0;
  for (int64_t s : sizes) {
    TORCH_CHECK(s >= 0 && s < INT32_MAX, b.name, ": dictionary size out of range");
    offs.push_back(off);
    off += s + 1;
    if (s + 1 <= CODE_LDS_SLOTS) lds_slots = std::max(lds_slots, (int)s + 1);
  }
  int nchunks = pick_chunks(b.maxn, b.ncols());
  auto out = torch::zeros({off}, on(b.device, torch::kInt64));
  auto dptr = upload(b.ptrs, b.device);
  auto dlen = upload(b.lens, b.device);
  auto doff = upload(offs, b.device);
  auto dsz = upload(std::vector<int>(sizes.begin(), sizes.end()), b.device);
  NullMasks nm(cols.size());
  torch::Tensor dmask;
  if (null_masks) {
    std::vector<int64_t> mptrs;
    for (int j = 0; j < b.ncols(); ++j)
      mptrs.push_back(sizes[j] + 1 <= CODE_LDS_SLOTS ? nm.add(j, b.lens[j], nchunks, b.device) : 0);
    dmask = upload(mptrs, b.device);
  }
  check_hip(anovos_code_counts_multi(ptr_table<const int32_t>(dptr), dlen.data_ptr<int64_t>(),
                                     doff.data_ptr<int64_t>(), dsz.data_ptr<int>(), b.ncols(),
                                     lds_slots, nchunks, (uint64_t *)out.data_ptr<int64_t>(),
                                     null_masks ? ptr_table<uint64_t>(dmask) : nullptr,
                                     current_stream()),
            "anovos_code_counts_multi");
  if (!null_masks) return py::cast(out);
  return py::make_tuple(out, nm.masks, nm.parts);
}

// K22: contingency tables of column pairs. The kernel (pair_counts.hip)
// takes work items "anchor column + up to PAIR_PMAX partners".
namespace {

struct PairPlan {
  std::vector<int64_t> items;  // PAIR_ITEM_WORDS words per item
  std::vector<int64_t> offs;   // output offset of every pair's table
  int64_t total = 0;           // cells of all tables
  int nitems = 0;
  int lds_slots = 0;           // most counters any STAGED item needs
  int64_t col_reads = 0;       // column streams per row chunk: sum(1 + partners)
};

// Pairs are grouped by their first column (the anchor, in order of first
// appearance) and packed greedily in pair order: an item closes when it
// has PAIR_PMAX partners or the next table would not fit the LDS budget.
// A table with more cells than the budget is an item of its own that
// counts in global memory, so it never sizes the launch's LDS.
PairPlan plan_pair_items(const std::vector<int64_t> &sizes, const std::vector<int64_t> &pair_i,
                         const std::vector<int64_t> &pair_j) {
  const int64_t ncols = (int64_t)sizes.size();
  TORCH_CHECK(pair_i.size() == pair_j.size(), "pair_i/pair_j length mismatch");
  for (auto s : sizes) TORCH_CHECK(s >= 0 && s < INT32_MAX, "dictionary size out of range");
  PairPlan plan;
  std::vector<std::vector<int64_t>> by_anchor(ncols);
  std::vector<int64_t> order;
  for (size_t q = 0; q < pair_i.size(); ++q) {
    TORCH_CHECK(pair_i[q] >= 0 && pair_i[q] < ncols && pair_j[q] >= 0 && pair_j[q] < ncols,
                "pair index out of range");
    if (by_anchor[pair_i[q]].empty()) order.push_back(pair_i[q]);
    by_anchor[pair_i[q]].push_back((int64_t)q);
    plan.offs.push_back(plan.total);
    plan.total += (sizes[pair_i[q]] + 1) * (sizes[pair_j[q]] + 1);
  }
  auto open_item = [&](int64_t a) {
    plan.items.resize(plan.items.size() + PAIR_ITEM_WORDS, 0);
    int64_t *it = plan.items.data() + (int64_t)plan.nitems * PAIR_ITEM_WORDS;
    it[0] = a;
    it[1] = sizes[a];
    plan.nitems += 1;
    plan.col_reads += 1;
  };
  auto add_partner = [&](int64_t q, int64_t lds_off) {
    int64_t *it = plan.items.data() + (int64_t)(plan.nitems - 1) * PAIR_ITEM_WORDS;
    int64_t *pp = it + 4 + 4 * it[2];
    pp[0] = pair_j[q];
    pp[1] = sizes[pair_j[q]];
    pp[2] = lds_off;
    pp[3] = plan.offs[q];
    it[2] += 1;
    plan.col_reads += 1;
  };
  for (int64_t a : order) {
    int64_t used = 0;
    int nparts = 0;
    bool open = false;
    for (int64_t q : by_anchor[a]) {
      const int64_t cells = (sizes[a] + 1) * (sizes[pair_j[q]] + 1);
      if (cells > PAIR_LDS_SLOTS) {
        // word 3 stays 0: global-atomic item; the items are appended in
        // order, so it also closes the staged item that was open
        open_item(a);
        add_partner(q, 0);
        open = false;
        continue;
      }
      if (!open || nparts == PAIR_PMAX || used + cells > PAIR_LDS_SLOTS) {
        open_item(a);
        open = true;
        used = 0;
        nparts = 0;
      }
      add_partner(q, used);
      used += cells;
      nparts += 1;
      plan.items[(int64_t)(plan.nitems - 1) * PAIR_ITEM_WORDS + 3] = used;
      plan.lds_slots = std::max(plan.lds_slots, (int)used);
    }
  }
  return plan;
}

}  // namespace

// Flat int64 of the row-major tables [sizes[i]+1][sizes[j]+1] of the pairs
// (pair_i[p], pair_j[p]), in pair order; the null slot (any code outside
// [0, size)) is each table's last row / last column.
torch::Tensor pair_code_counts(std::vector<torch::Tensor> cols, std::vector<int64_t> sizes,
                               std::vector<int64_t> pair_i, std::vector<int64_t> pair_j) {
  ColumnBatch b = gather_columns(cols, "pair_code_counts", I32, /*equal_len=*/true);
  check_count(sizes.size(), cols.size(), b.name, "sizes");
  for (auto &t : cols) TORCH_CHECK(t.dim() == 1, "pair_code_counts: columns must be 1-D");
  const int64_t n = b.maxn;
  PairPlan plan = plan_pair_items(sizes, pair_i, pair_j);
  auto out = torch::zeros({plan.total}, on(b.device, torch::kInt64));
  if (n == 0 || plan.nitems == 0) return out;
  int nchunks = pick_chunks(n, plan.nitems);
  // chunk length a multiple of 4 rows: every chunk then starts at the same
  // offset inside a 16-byte line as the column itself
  const int64_t per = (((n + nchunks - 1) / nchunks) + 3) / 4 * 4;
  // a staged counter holds at most one block's rows
  TORCH_CHECK(per <= (int64_t)UINT32_MAX, "rows per block exceed the 32-bit LDS counters");
  TORCH_CHECK((int64_t)plan.nitems * nchunks <= (int64_t)INT32_MAX, "grid too large");
  auto dptr = upload(b.ptrs, b.device);
  auto ditems = upload(plan.items, b.device);
  check_hip(anovos_pair_code_counts(ptr_table<const int32_t>(dptr), ditems.data_ptr<int64_t>(),
                                    plan.nitems, n, per, nchunks, plan.lds_slots,
                                    (uint64_t *)out.data_ptr<int64_t>(), current_stream()),
            "anovos_pair_code_counts");
  return out;
}

// [work items, column streams per row chunk, LDS counters of the launch]
// for a pair list — what the benchmark needs to count the bytes read.
std::vector<int64_t> pair_code_counts_plan(std::vector<int64_t> sizes, std::vector<int64_t> pair_i,
                                           std::vector<int64_t> pair_j) {
  PairPlan plan = plan_pair_items(sizes, pair_i, pair_j);
  return {(int64_t)plan.nitems, plan.col_reads, (int64_t)plan.lds_slots};
}

// K23: (n, s1, s2) of value columns per slot of a code column. The kernel
// (grouped_moments.hip) takes work items "code column + slot window + up
// to GRP_PMAX value columns".
namespace {

struct GroupPlan {
  std::vector<int64_t> items;  // GRP_ITEM_WORDS words per item
  int nitems = 0;
  int cells = 0;               // most accumulator cells (w * P) of any item
  int64_t col_reads = 0;       // column streams per row chunk: sum(1 + P)
};

// Output offset of every pair's [size + 1][3] block, in pair order; the
// last entry is the total. Range-checks sizes and pair indices.
std::vector<int64_t> group_offsets(const std::vector<int64_t> &sizes, int64_t nvals,
                                   const std::vector<int64_t> &pair_c,
                                   const std::vector<int64_t> &pair_v) {
  const int64_t ncodes = (int64_t)sizes.size();
  TORCH_CHECK(pair_c.size() == pair_v.size(), "pair_c/pair_v length mismatch");
  for (auto s : sizes) TORCH_CHECK(s >= 0 && s < INT32_MAX, "dictionary size out of range");
  std::vector<int64_t> offs{0};
  for (size_t q = 0; q < pair_c.size(); ++q) {
    TORCH_CHECK(pair_c[q] >= 0 && pair_c[q] < ncodes && pair_v[q] >= 0 && pair_v[q] < nvals,
                "pair index out of range");
    offs.push_back(offs.back() + 3 * (sizes[pair_c[q]] + 1));
  }
  return offs;
}

// Items of the pairs whose value column is in `vpos` (value column ->
// position in the launch's value table, -1: another dtype's launch). Pairs
// are grouped by code column in order of first appearance. A dictionary
// whose slots fit GRP_CELLS packs min(GRP_PMAX, GRP_CELLS / slots) value
// columns per item in pair order; a larger one takes one item per window
// of GRP_CELLS slots and pair.
GroupPlan plan_group_items(const std::vector<int64_t> &sizes, const std::vector<int64_t> &vpos,
                           const std::vector<int64_t> &pair_c, const std::vector<int64_t> &pair_v,
                           const std::vector<int64_t> &offs) {
  GroupPlan plan;
  std::vector<std::vector<int64_t>> by_code(sizes.size());
  std::vector<int64_t> order;
  for (size_t q = 0; q < pair_c.size(); ++q) {
    if (vpos[pair_v[q]] < 0) continue;
    if (by_code[pair_c[q]].empty()) order.push_back(pair_c[q]);
    by_code[pair_c[q]].push_back((int64_t)q);
  }
  auto open_item = [&](int64_t c, int64_t g0, int64_t w) {
    plan.items.resize(plan.items.size() + GRP_ITEM_WORDS, 0);
    int64_t *it = plan.items.data() + (int64_t)plan.nitems * GRP_ITEM_WORDS;
    it[0] = c;
    it[1] = sizes[c];
    it[3] = g0;
    it[4] = w;
    plan.nitems += 1;
    plan.col_reads += 1;
  };
  auto add_value = [&](int64_t q) {
    int64_t *it = plan.items.data() + (int64_t)(plan.nitems - 1) * GRP_ITEM_WORDS;
    it[5 + 2 * it[2]] = vpos[pair_v[q]];
    it[6 + 2 * it[2]] = offs[q];
    it[2] += 1;
    plan.col_reads += 1;
    plan.cells = std::max(plan.cells, (int)(it[2] * it[4]));
  };
  for (int64_t c : order) {
    const int64_t slots = sizes[c] + 1;
    if (slots <= GRP_CELLS) {
      const int64_t pmax = std::min<int64_t>(GRP_PMAX, GRP_CELLS / slots);
      int64_t np = pmax;
      for (int64_t q : by_code[c]) {
        if (np == pmax) {
          open_item(c, 0, slots);
          np = 0;
        }
        add_value(q);
        np += 1;
      }
    } else {
      for (int64_t q : by_code[c])
        for (int64_t g0 = 0; g0 < slots; g0 += GRP_CELLS) {
          open_item(c, g0, std::min<int64_t>(GRP_CELLS, slots - g0));
          add_value(q);
        }
    }
    TORCH_CHECK((int64_t)plan.items.size() / GRP_ITEM_WORDS < (int64_t)INT32_MAX, "too many work items");
  }
  return plan;
}

}  // namespace

// Flat fp64 of the slot-major blocks [sizes[c] + 1][3] = (n, s1, s2) of the
// pairs (pair_c[q], pair_v[q]), in pair order: rows per slot, sum d and
// sum d^2 with d = (double)x - shifts[v] over the rows whose value is not
// NaN; the null slot (any code outside [0, size)) is each block's last row.
torch::Tensor grouped_moments(std::vector<torch::Tensor> codes, std::vector<int64_t> sizes,
                              std::vector<torch::Tensor> values, std::vector<double> shifts,
                              std::vector<int64_t> pair_c, std::vector<int64_t> pair_v) {
  ColumnBatch cb = gather_columns(codes, "grouped_moments", I32, /*equal_len=*/true);
  ColumnBatch vb = gather_columns(values, "grouped_moments", F32 | F64, /*equal_len=*/true);
  TORCH_CHECK(vb.device == cb.device, cb.name, ": columns must be on the same device");
  TORCH_CHECK(vb.maxn == cb.maxn, cb.name, ": all columns must have equal length");
  for (auto &t : codes) TORCH_CHECK(t.dim() == 1, cb.name, ": columns must be 1-D");
  for (auto &t : values) TORCH_CHECK(t.dim() == 1, cb.name, ": columns must be 1-D");
  check_count(sizes.size(), codes.size(), cb.name, "sizes");
  check_count(shifts.size(), values.size(), cb.name, "shifts");
  const int64_t n = cb.maxn;
  auto offs = group_offsets(sizes, vb.ncols(), pair_c, pair_v);
  auto device = cb.device;
  auto out = torch::zeros({offs.back()}, on(device, torch::kFloat64));
  if (n == 0 || pair_c.empty()) return out;
  auto dcodes = upload(cb.ptrs, device);
  for (auto &b : split_by_dtype(vb)) {
    std::vector<int64_t> vpos(vb.ncols(), -1);
    for (int j = 0; j < b.ncols(); ++j) vpos[b.idx[j]] = j;
    GroupPlan plan = plan_group_items(sizes, vpos, pair_c, pair_v, offs);
    if (plan.nitems == 0) continue;
    int nchunks = pick_chunks(n, plan.nitems);
    // chunk length a multiple of 4 rows: every chunk then starts at the same
    // offset inside a 16-byte line as the column itself
    const int64_t per = (((n + nchunks - 1) / nchunks) + 3) / 4 * 4;
    // a thread's row counter holds at most its share of one block's rows
    TORCH_CHECK(per / GRP_THREADS < (int64_t)UINT32_MAX, "rows per thread exceed the 32-bit LDS counters");
    TORCH_CHECK((int64_t)plan.nitems * nchunks <= (int64_t)INT32_MAX, "grid too large");
    auto dvals = upload(b.ptrs, device);
    auto dsh = upload(pick(shifts, b.idx), device);
    auto ditems = upload(plan.items, device);
    auto partials = torch::empty({(int64_t)plan.nitems * nchunks * GRP_CELLS * 3}, on(device, torch::kFloat64));
    check_hip(anovos_grouped_moments(ptr_table<const int32_t>(dcodes), ptr_table<const void>(dvals),
                                     dsh.data_ptr<double>(), ditems.data_ptr<int64_t>(), plan.nitems,
                                     n, per, nchunks, plan.cells, b.dtype,
                                     partials.data_ptr<double>(), out.data_ptr<double>(),
                                     current_stream()),
              "anovos_grouped_moments");
  }
  return out;
}

// [work items, column streams per row chunk, accumulator cells of the
// launch] for a pair list whose value columns share one dtype — what the
// benchmark needs to count the bytes read.
std::vector<int64_t> grouped_moments_plan(std::vector<int64_t> sizes, std::vector<int64_t> pair_c,
                                          std::vector<int64_t> pair_v) {
  int64_t nvals = 0;
  for (int64_t v : pair_v) nvals = std::max(nvals, v + 1);
  auto offs = group_offsets(sizes, nvals, pair_c, pair_v);
  std::vector<int64_t> vpos(nvals);
  for (int64_t j = 0; j < nvals; ++j) vpos[j] = j;
  GroupPlan plan = plan_group_items(sizes, vpos, pair_c, pair_v, offs);
  return {(int64_t)plan.nitems, plan.col_reads, (int64_t)plan.cells};
}

// K9 fused: label-conditioned histograms, ALL columns in one launch.
// Per column at out[off]: [slots] totals then [slots] event counts.
// Column dtype drives the slot mapping (f32 binned vs int32 codes).
torch::Tensor label_counts_multi(std::vector<torch::Tensor> cols, torch::Tensor label,
                                 std::vector<int64_t> sizes) {
  ColumnBatch b = gather_columns(cols, "label_counts_multi", F32 | I32, /*equal_len=*/true);
  check_count(sizes.size(), cols.size(), b.name, "sizes");
  check_dense_on_device(label, b, "label", torch::kUInt8, b.maxn);
  std::vector<int64_t> offs;
  std::vector<int> kinds;  // the kernel's own code: 0 f32 binned, 1 int32 codes
  int64_t off = 0;
  int max_slots = 0;
  for (int i = 0; i < b.ncols(); ++i) {
    TORCH_CHECK(sizes[i] >= 1 && sizes[i] <= LABEL_MAX_SLOTS, b.name, ": slot count out of LDS range");
    offs.push_back(off);
    off += 2 * sizes[i];
    kinds.push_back(b.dtypes[i] == 2 ? 1 : 0);
    max_slots = std::max(max_slots, (int)sizes[i]);
  }
  int nchunks = pick_chunks(b.maxn, b.ncols());
  auto out = torch::zeros({off}, on(b.device, torch::kInt64));
  auto dptr = upload(b.ptrs, b.device);
  auto dlen = upload(b.lens, b.device);
  auto doff = upload(offs, b.device);
  auto dsz = upload(std::vector<int>(sizes.begin(), sizes.end()), b.device);
  auto dkind = upload(kinds, b.device);
  check_hip(anovos_label_counts_multi(ptr_table<const void>(dptr), label.data_ptr<uint8_t>(),
                                      dlen.data_ptr<int64_t>(), doff.data_ptr<int64_t>(),
                                      dsz.data_ptr<int>(), dkind.data_ptr<int>(), b.ncols(),
                                      max_slots, nchunks, (uint64_t *)out.data_ptr<int64_t>(),
                                      current_stream()),
            "anovos_label_counts_multi");
  return out;
}

// K6+K9 fused: bucketize against per-column cutoffs + label-conditioned
// counts in one read of the RAW numeric columns (no binned
// materialization). Returns flat int64: per column [slots] totals then
// [slots] events at offsets in the ORIGINAL column order. The cutoffs are
// host lists (one tensor per column, flattened and uploaded), or with
// cut_matrix one contiguous fp64 [ncols, ncut] device tensor that the
// kernel reads where it lies: nothing is copied and nothing waits.
namespace {
torch::Tensor bucketize_label_counts_body(const std::vector<torch::Tensor> &cols,
                                          const std::vector<torch::Tensor> *cutoffs,
                                          const torch::Tensor *cut_matrix,
                                          const torch::Tensor &label,
                                          const std::vector<int64_t> &sizes, const char *name) {
  ColumnBatch all = gather_columns(cols, name, F32 | F64, /*equal_len=*/true);
  int64_t ncut = 0;
  if (cutoffs) {
    check_count(cutoffs->size(), cols.size(), all.name, "cutoffs");
  } else {
    TORCH_CHECK(cut_matrix->dim() == 2 && cut_matrix->size(0) == (int64_t)cols.size() &&
                    cut_matrix->size(1) >= 1 && cut_matrix->size(1) <= LABEL_MAX_SLOTS,
                all.name, ": cut_matrix must be [ncols, ncut] with 1 <= ncut <= ", LABEL_MAX_SLOTS);
    TORCH_CHECK(cut_matrix->device() == all.device && cut_matrix->is_contiguous() &&
                    cut_matrix->scalar_type() == torch::kFloat64,
                all.name, ": cut_matrix must be a contiguous float64 tensor on the columns' device");
    ncut = cut_matrix->size(1);
  }
  check_count(sizes.size(), cols.size(), all.name, "sizes");
  check_dense_on_device(label, all, "label", torch::kUInt8, all.maxn);
  auto device = all.device;
  std::vector<int64_t> out_offs;
  int64_t total = 0;
  for (int64_t s : sizes) {
    TORCH_CHECK(s >= 1 && s <= LABEL_MAX_SLOTS, all.name, ": slot count out of LDS range");
    out_offs.push_back(total);
    total += 2 * s;
  }
  auto out = torch::zeros({total}, on(device, torch::kInt64));
  for (auto &b : split_by_dtype(all)) {
    CutoffTable ct;
    torch::Tensor dflat;
    if (cutoffs) {
      ct = cutoff_table(*cutoffs, b.idx);
      dflat = upload(ct.flat, device);
    } else {
      for (int64_t i : b.idx) ct.offs.push_back(i * ncut);
      ct.lens.assign(b.idx.size(), (int)ncut);
      ct.max_ncut = (int)ncut;
      dflat = *cut_matrix;
    }
    auto sz = pick(sizes, b.idx);
    int max_slots = (int)std::max<int64_t>(1, *std::max_element(sz.begin(), sz.end()));
    int nchunks = pick_chunks(b.maxn, b.ncols());
    auto dptr = upload(b.ptrs, device);
    auto dlen = upload(b.lens, device);
    auto doff = upload(pick(out_offs, b.idx), device);
    auto dcoff = upload(ct.offs, device);
    auto dclen = upload(ct.lens, device);
    auto dsz = upload(std::vector<int>(sz.begin(), sz.end()), device);
    check_hip(anovos_bucketize_label_counts(
                  ptr_table<const void>(dptr), label.data_ptr<uint8_t>(), dlen.data_ptr<int64_t>(),
                  dflat.data_ptr<double>(), dcoff.data_ptr<int64_t>(), dclen.data_ptr<int>(),
                  doff.data_ptr<int64_t>(), dsz.data_ptr<int>(), b.ncols(), ct.max_ncut, max_slots,
                  nchunks, b.dtype, (uint64_t *)out.data_ptr<int64_t>(), current_stream()),
              "anovos_bucketize_label_counts");
  }
  return out;
}

// One per-column fp64 parameter of a quantile query: dense, on `dev`.
const double *query_param(const torch::Tensor &t, int64_t ncols, const torch::Device &dev,
                          const char *name, const char *what) {
  TORCH_CHECK(t.device() == dev && t.is_contiguous() && t.scalar_type() == torch::kFloat64 &&
                  t.numel() == ncols,
              name, ": ", what, " must be a contiguous float64 tensor of ", ncols,
              " entries on the histogram's device");
  return t.data_ptr<double>();
}

void check_query_matrix(const torch::Tensor &h, const std::vector<double> &probs, const char *name) {
  TORCH_CHECK(h.is_cuda() && h.dim() == 2 && h.is_contiguous() && h.scalar_type() == torch::kInt64,
              name, ": expected a contiguous int64 [ncols, nbins] device tensor");
  TORCH_CHECK(h.size(0) >= 1 && h.size(1) >= 1 && h.size(1) <= QQ_MAX_BINS, name,
              ": need at least one column and 1 .. ", QQ_MAX_BINS, " bins");
  TORCH_CHECK(!probs.empty(), name, ": no probabilities");
}
}  // namespace

torch::Tensor bucketize_label_counts(std::vector<torch::Tensor> cols,
                                     std::vector<torch::Tensor> cutoffs, torch::Tensor label,
                                     std::vector<int64_t> sizes) {
  return bucketize_label_counts_body(cols, &cutoffs, nullptr, label, sizes,
                                     "bucketize_label_counts");
}

torch::Tensor bucketize_label_counts_dev(std::vector<torch::Tensor> cols, torch::Tensor cut_matrix,
                                         torch::Tensor label, std::vector<int64_t> sizes) {
  return bucketize_label_counts_body(cols, nullptr, &cut_matrix, label, sizes,
                                     "bucketize_label_counts_dev");
}

// K3q: quantiles of [ncols, nbins] pass-1 histograms that are on the device.
// Returns (values f64 [ncols, P], refine flags u8 [ncols, P], largest bin
// count int64 [ncols]), all left on the device.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> hist_quantile_query(
    torch::Tensor hist, torch::Tensor lo, torch::Tensor hi, torch::Tensor n,
    std::vector<double> probs, double rel_err) {
  const char *name = "hist_quantile_query";
  check_query_matrix(hist, probs, name);
  const int64_t ncols = hist.size(0), P = (int64_t)probs.size();
  auto dev = hist.device();
  const double *plo = query_param(lo, ncols, dev, name, "lo");
  const double *phi = query_param(hi, ncols, dev, name, "hi");
  const double *pn = query_param(n, ncols, dev, name, "n");
  auto vals = torch::empty({ncols, P}, on(dev, torch::kFloat64));
  auto flags = torch::empty({ncols, P}, on(dev, torch::kUInt8));
  auto maxbin = torch::empty({ncols}, on(dev, torch::kInt64));
  auto dprobs = upload(probs, dev);
  check_hip(anovos_hist_quantile_query((const uint64_t *)hist.data_ptr<int64_t>(), plo, phi, pn,
                                       dprobs.data_ptr<double>(), rel_err, (int)ncols,
                                       (int)hist.size(1), (int)P, vals.data_ptr<double>(),
                                       flags.data_ptr<uint8_t>(), maxbin.data_ptr<int64_t>(),
                                       current_stream()),
            "anovos_hist_quantile_query");
  return {vals, flags, maxbin};
}

// K3q, dense integer counts: column c holds the counts of cmin[c] + 0 ..
// R[c] - 1 in the first R[c] entries of its row. Returns f64 [ncols, P].
torch::Tensor inthist_quantile_query(torch::Tensor counts, torch::Tensor cmin, torch::Tensor n,
                                     torch::Tensor R, std::vector<double> probs, double rel_err) {
  const char *name = "inthist_quantile_query";
  check_query_matrix(counts, probs, name);
  const int64_t ncols = counts.size(0), P = (int64_t)probs.size();
  auto dev = counts.device();
  const double *pmin = query_param(cmin, ncols, dev, name, "cmin");
  const double *pn = query_param(n, ncols, dev, name, "n");
  const double *pR = query_param(R, ncols, dev, name, "R");
  auto vals = torch::empty({ncols, P}, on(dev, torch::kFloat64));
  auto dprobs = upload(probs, dev);
  check_hip(anovos_inthist_quantile_query((const uint64_t *)counts.data_ptr<int64_t>(),
                                          (int)counts.size(1), pmin, pn, pR,
                                          dprobs.data_ptr<double>(), rel_err, (int)ncols, (int)P,
                                          vals.data_ptr<double>(), current_stream()),
            "anovos_inthist_quantile_query");
  return vals;
}

// K10/K11 fused: outlier counts + clamp/null treatment in one launch.
// mode: 0 count only, 1 clamp to bounds, 2 null-out. Returns
// (counts [k,2] int64, outs list — empty when mode==0).
std::tuple<torch::Tensor, std::vector<torch::Tensor>> outlier_clamp_columns(
    std::vector<torch::Tensor> cols, torch::Tensor lo, torch::Tensor hi, int64_t mode) {
  ColumnBatch all = gather_columns(cols, "outlier_clamp_columns", F32 | F64);
  auto device = all.device;
  auto lo_d = device_f64(lo, cols.size(), all, "lo");
  auto hi_d = device_f64(hi, cols.size(), all, "hi");
  auto counts = torch::zeros({all.ncols(), 2}, on(device, torch::kInt64));
  std::vector<torch::Tensor> outs;
  if (mode)
    for (auto &t : cols) outs.push_back(torch::empty_like(t));
  for (auto &b : split_by_dtype(all)) {
    int nchunks = pick_chunks(b.maxn, b.ncols());
    auto dptr = upload(b.ptrs, device);
    auto dlen = upload(b.lens, device);
    auto didx = upload(b.idx, device);
    auto lo_sel = lo_d.index_select(0, didx);
    auto hi_sel = hi_d.index_select(0, didx);
    auto sub = torch::zeros({b.ncols(), 2}, on(device, torch::kInt64));
    torch::Tensor dout;
    if (mode) dout = upload(out_ptrs(outs, b), device);
    check_hip(anovos_outlier_clamp(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(),
                                   b.ncols(), lo_sel.data_ptr<double>(), hi_sel.data_ptr<double>(),
                                   nchunks, (int)mode, b.dtype,
                                   mode ? ptr_table<void>(dout) : nullptr,
                                   (uint64_t *)sub.data_ptr<int64_t>(), current_stream()),
              "anovos_outlier_clamp");
    counts.index_copy_(0, didx, sub);
  }
  return {counts, outs};
}

namespace {

// K24 cutoffs: one list per column, at most GRADE_MAX_CELLS - 1 entries,
// strictly ascending, no NaN.
void check_grade_cutoffs(const std::vector<torch::Tensor> &cutoffs, size_t ncols, const char *name) {
  check_count(cutoffs.size(), ncols, name, "cutoffs");
  for (size_t i = 0; i < cutoffs.size(); ++i) {
    TORCH_CHECK(cutoffs[i].numel() <= GRADE_MAX_CELLS - 1, name, ": column ", i, " has ",
                cutoffs[i].numel(), " cutoffs, at most ", GRADE_MAX_CELLS - 1, " fit");
    auto cc = cutoffs[i].to(torch::kFloat64).cpu().contiguous();
    const double *c = cc.data_ptr<double>();
    for (int64_t j = 0; j < cc.numel(); ++j)
      TORCH_CHECK(c[j] == c[j] && (j == 0 || c[j] > c[j - 1]), name, ": cutoffs of column ", i,
                  " must be strictly ascending without NaN");
  }
}

}  // namespace

// K24 counting pass: int64 [ncols, max_ncut + 2] local counts in the
// original column order, slot 0 nulls, slot 1 + j cell j = #{c : c < x}.
torch::Tensor grade_counts(std::vector<torch::Tensor> cols, std::vector<torch::Tensor> cutoffs) {
  ColumnBatch all = gather_columns(cols, "grade_counts", F32 | F64);
  check_grade_cutoffs(cutoffs, cols.size(), all.name);
  auto device = all.device;
  int64_t stride = 2;
  for (auto &c : cutoffs) stride = std::max<int64_t>(stride, c.numel() + 2);
  auto counts = torch::zeros({all.ncols(), stride}, on(device, torch::kInt64));
  for (auto &b : split_by_dtype(all)) {
    CutoffTable ct = cutoff_table(cutoffs, b.idx);
    int nchunks = pick_chunks(b.maxn, b.ncols());
    auto dptr = upload(b.ptrs, device);
    auto dlen = upload(b.lens, device);
    auto doff = upload(ct.offs, device);
    auto dflat = upload(ct.flat, device);
    auto dclen = upload(ct.lens, device);
    std::vector<int64_t> coffs;
    for (int64_t i : b.idx) coffs.push_back(i * stride);
    auto dcoff = upload(coffs, device);
    check_hip(anovos_grade_counts(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(), b.ncols(),
                                  dflat.data_ptr<double>(), doff.data_ptr<int64_t>(),
                                  dclen.data_ptr<int>(), ct.max_ncut, nchunks, b.dtype,
                                  (uint64_t *)counts.data_ptr<int64_t>(),
                                  dcoff.data_ptr<int64_t>(), current_stream()),
              "anovos_grade_counts");
  }
  return counts;
}

// K24 transform pass: f32 tables[col][cell(x)], null_grade for NaN, into
// `outs` when given (dense f32 tensors of the columns' lengths on their
// device) or into new tensors.
std::vector<torch::Tensor> grade_apply(std::vector<torch::Tensor> cols,
                                       std::vector<torch::Tensor> cutoffs,
                                       std::vector<torch::Tensor> tables, double null_grade,
                                       std::optional<std::vector<torch::Tensor>> outs_in) {
  ColumnBatch all = gather_columns(cols, "grade_apply", F32 | F64);
  check_grade_cutoffs(cutoffs, cols.size(), all.name);
  check_count(tables.size(), cols.size(), all.name, "tables");
  for (size_t i = 0; i < tables.size(); ++i)
    TORCH_CHECK(tables[i].numel() == cutoffs[i].numel() + 1, all.name, ": table of column ", i,
                " has ", tables[i].numel(), " entries, expected ", cutoffs[i].numel() + 1);
  auto device = all.device;
  std::vector<torch::Tensor> outs;
  if (outs_in.has_value()) {
    outs = *outs_in;
    check_count(outs.size(), cols.size(), all.name, "outs");
    for (size_t i = 0; i < outs.size(); ++i)
      check_dense_on_device(outs[i], all, "outs", torch::kFloat32, cols[i].numel());
  } else {
    for (auto &t : cols) outs.push_back(torch::empty(t.sizes(), on(device, torch::kFloat32)));
  }
  for (auto &b : split_by_dtype(all)) {
    CutoffTable ct = cutoff_table(cutoffs, b.idx);
    std::vector<float> tflat;
    std::vector<int64_t> toffs;
    for (int64_t i : b.idx) {
      auto tc = tables[i].to(torch::kFloat32).cpu().contiguous();
      toffs.push_back((int64_t)tflat.size());
      tflat.insert(tflat.end(), tc.data_ptr<float>(), tc.data_ptr<float>() + tc.numel());
    }
    int nchunks = pick_chunks(b.maxn, b.ncols());
    auto dptr = upload(b.ptrs, device);
    auto dlen = upload(b.lens, device);
    auto dout = upload(out_ptrs(outs, b), device);
    auto doff = upload(ct.offs, device);
    auto dflat = upload(ct.flat, device);
    auto dclen = upload(ct.lens, device);
    auto dtoff = upload(toffs, device);
    auto dtflat = upload(tflat, device);
    check_hip(anovos_grade_apply(ptr_table<const void>(dptr), dlen.data_ptr<int64_t>(), b.ncols(),
                                 dflat.data_ptr<double>(), doff.data_ptr<int64_t>(),
                                 dclen.data_ptr<int>(), dtflat.data_ptr<float>(),
                                 dtoff.data_ptr<int64_t>(), (float)null_grade, ct.max_ncut,
                                 nchunks, b.dtype, ptr_table<float>(dout), current_stream()),
              "anovos_grade_apply");
  }
  return outs;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("grade_counts", &grade_counts, "rows per grid cell of each column, read-only (K24)");
  m.def("grade_apply", &grade_apply, "per-cell grade lookup to f32 columns (K24)",
        py::arg("cols"), py::arg("cutoffs"), py::arg("tables"), py::arg("null_grade"),
        py::arg("outs") = py::none());
  m.attr("GRADE_MAX_CELLS") = GRADE_MAX_CELLS;
  m.def("code_counts_multi",&code_counts_multi, "fused multi-column code counts + null slot (K5)",
        py::arg("cols"), py::arg("sizes"), py::arg("null_masks") = false);
  m.def("pair_code_counts", &pair_code_counts, "contingency tables of code-column pairs (K22)");
  m.def("pair_code_counts_plan", &pair_code_counts_plan,
        "[items, column streams, LDS counters] of a K22 pair list");
  m.def("grouped_moments", &grouped_moments, "(n, s1, s2) of value columns per code slot (K23)");
  m.def("grouped_moments_plan", &grouped_moments_plan,
        "[items, column streams, accumulator cells] of a K23 pair list");
  m.attr("GRP_CELLS") = GRP_CELLS;
  m.def("outlier_clamp_columns", &outlier_clamp_columns, "fused outlier count/clamp (K10/K11)");
  m.def("label_counts_multi", &label_counts_multi, "fused multi-column label-conditioned histograms (K9)");
  m.def("bucketize_label_counts", &bucketize_label_counts, "fused bucketize + label counts, no binned materialization (K6+K9)");
  m.def("bucketize_label_counts_dev", &bucketize_label_counts_dev,
        "bucketize_label_counts with the cutoffs as a device [ncols, ncut] matrix (K6+K9)");
  m.def("hist_quantile_query", &hist_quantile_query, "quantiles of device-resident histograms (K3q)");
  m.def("inthist_quantile_query", &inthist_quantile_query,
        "exact quantiles of device-resident dense integer counts (K3q)");
  m.def("moments_hll", &moments_hll, "fused moments + HLL registers (K1/K2+K4)",
        py::arg("cols"), py::arg("p"), py::arg("shifts") = std::vector<double>(),
        py::arg("null_masks") = false);
  m.def("centered_gram_bf16", &centered_gram_bf16, "bf16 MFMA centered Gram X^T X (K8)");
  m.def("pairwise_gram_bf16", &pairwise_gram_bf16,
        "bf16 MFMA pairwise-complete sums [4, k, k] = (N, P, S, Q) (K25)");
  m.def("row_quadform_bf16x2", &row_quadform_bf16x2,
        "per-row |W z|^2 of standardized columns, split-bf16 MFMA (K26)");
  m.def("bracket_histograms_grouped", &bracket_histograms_grouped, "grouped refinement histograms (K3)");
  m.def("bucketize_columns_float", &bucketize_columns_float, "bucketize to float bin labels (K6)");
  m.def("bucketize_columns_float_counts", &bucketize_columns_float_counts,
        "bucketize to float bin labels + per-column bin counts from the same pass (K6)");
  m.def("lut_apply_f32", &lut_apply_f32, "fused LUT gather -> float (K12)");
  m.def("lut_apply_i32", &lut_apply_i32, "fused LUT gather -> int32 (K12)");
  m.def("hll_registers_multi", &hll_registers_multi, "fused multi-column HLL (K4)");
  m.def("scale_columns", &scale_columns,
        "fused scaling (K11): out = (float)(((double)x - a) * b), f32 and f64 columns alike");
  m.def("fill_nan_columns", &fill_nan_columns, "fused NaN fill (K11)");
  m.def("fill_code_columns", &fill_code_columns, "fused categorical null fill (K11)");
  m.def("column_moments", &column_moments, "fused per-column moments (K1/K2)",
        py::arg("cols"), py::arg("shifts") = std::vector<double>());
  m.def("column_histograms", &column_histograms, "fused per-column histograms (K3/K6)");
  m.def("bracket_histograms", &bracket_histograms, "quantile-refinement histograms (K3)");
  m.def("bucketize_columns", &bucketize_columns, "branchless bucketize (K6)");
  m.def("code_counts", &code_counts, "dictionary code bincount (K5)");
  m.def("hll_registers", &hll_registers, "HyperLogLog registers (K4)");
  m.def("row_null_counts_num", &row_null_counts_num, "fused row null counts (K10)");
  m.def("row_null_counts_masked", &row_null_counts_masked,
        "row null counts from null lane masks (K10m)");
}
