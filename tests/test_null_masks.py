"""Null lane masks: emitted by the fused moments+HLL kernel (f32) and by
the multi-column code counts (int32), read by the masked row-null kernel.

The layout is rebuilt here from its description alone (`_pack`): a chunk
of `per` rows starting at s, vector index i = row offset // 4, group
i >> 6, four 64-bit words per group, bit i & 63 of word c = row s + 4 i + c
is null; the <= 3 tail rows of a chunk set bits 0..2 of word 0 of the next
group. Everything compared is an integer count or a bit pattern, so every
comparison is exact.

Shapes: one chunk up to 65 536 rows; 65 537 rows in 3 columns give 2
chunks of 32 769, 200 003 rows give 4 chunks of 50 001, so chunk starts
are odd. Nulls are planted at row 0, the last row, around every chunk
start, in every chunk's scalar tail and over one whole 256-row group."""

import numpy as np
import pandas as pd
import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

DEV = "cuda"
NAN = float("nan")
INF = float("inf")
CODE_LDS_SLOTS = 16384

SMALL = [1, 3, 4, 5, 255, 256, 257, 1023, 1025]
# n -> (nchunks, per) of a 3-column launch
MULTI = {65_537: (2, 32_769), 200_003: (4, 50_001)}
SHAPES = SMALL + list(MULTI)


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    e = backend.require_hip()
    assert e is not None, "HIP extension must be loadable on the GPU box"
    return e


# ------------------------------------------------------------ the layout
def _chunk_words(per):
    return 4 * ((((per // 4) + 63) // 64) + 1)  # vector groups of a full chunk + the tail group


def _word_and_bit(n, nchunks):
    """For every row: index of the mask word that holds its bit, and the bit."""
    per = -(-n // nchunks)
    wpc = _chunk_words(per)
    r = np.arange(n, dtype=np.int64)
    chunk = r // per
    s = chunk * per
    e = np.minimum(n, s + per)
    nv = (e - s) // 4
    j = r - s
    i = j // 4
    vec = j < 4 * nv
    word = np.where(vec, chunk * wpc + 4 * (i >> 6) + (j & 3), chunk * wpc + 4 * ((nv + 63) >> 6))
    bit = np.where(vec, i & 63, j - 4 * nv)
    return word, bit, nchunks * wpc, per


def _pack(nulls, nchunks):
    """(words, written): the mask of a bool row vector, and which words a
    producer has to write (those that hold the bit of some row)."""
    n = nulls.numel()
    word, bit, nwords, _ = _word_and_bit(n, nchunks)
    words = np.zeros(nwords, dtype=np.uint64)
    nz = nulls.numpy()
    np.add.at(words, word[nz], np.uint64(1) << bit[nz].astype(np.uint64))  # distinct bits: add = or
    written = np.zeros(nwords, dtype=bool)
    written[word] = True
    return words, written


def _check_mask(mask, part, nulls, nchunks):
    n = nulls.numel()
    per = -(-n // nchunks)
    assert tuple(part) == (n, nchunks, per)
    want, written = _pack(nulls, nchunks)
    got = mask.cpu().numpy().view(np.uint64)
    assert got.shape == want.shape
    assert np.array_equal(got[written], want[written])


# ------------------------------------------------------------ the data
def _planted(n, nchunks, g):
    """Bool [n]: row 0, the last row, s-1 / s / s+1 of every chunk start,
    every chunk's tail rows, one whole 256-row group, 1 % at random."""
    per = -(-n // nchunks)
    nulls = torch.rand(n, generator=g) < 0.01
    nulls[0] = True
    nulls[n - 1] = True
    for c in range(nchunks):
        s, e = c * per, min(n, (c + 1) * per)
        for r in (s - 1, s, s + 1):
            if 0 <= r < n:
                nulls[r] = True
        nulls[s + 4 * ((e - s) // 4) : e] = True
    if n >= 512:
        s = (nchunks - 1) * per  # the last chunk's group 1
        if n - s < 512:
            s = 0
        nulls[s + 256 : s + 512] = True
    return nulls


def _f32_cols(n, nchunks, seed):
    """[planted, all-null, null-free] f32 columns with +-inf among the
    values, and their null vectors."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-50, 50, (3, n), generator=g).to(torch.float32)
    x[torch.rand(3, n, generator=g) < 0.05] = INF
    x[torch.rand(3, n, generator=g) < 0.05] = -INF
    nulls = torch.stack([_planted(n, nchunks, g), torch.ones(n, dtype=torch.bool),
                         torch.zeros(n, dtype=torch.bool)])
    x[nulls] = NAN
    return x, nulls


SIZE = 7


def _i32_cols(n, nchunks, seed):
    """[planted, all-null, null-free] code columns of a 7-entry dictionary;
    codes -2 and 7 are outside it and are not nulls."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, SIZE, (3, n), generator=g).to(torch.int32)
    x[torch.rand(3, n, generator=g) < 0.05] = -2
    x[torch.rand(3, n, generator=g) < 0.05] = SIZE
    nulls = torch.stack([_planted(n, nchunks, g), torch.ones(n, dtype=torch.bool),
                         torch.zeros(n, dtype=torch.bool)])
    x[nulls] = -1
    return x, nulls


def _views(x, guard):
    """Rows of x as contiguous device views t[1:] of buffers with a guard
    value (a null) before the first and after the last element."""
    out = []
    for row in x:
        buf = torch.full((row.numel() + 2,), guard, dtype=row.dtype)
        buf[1:-1] = row
        v = buf.to(DEV)[1:-1]
        assert v.is_contiguous() and v.storage_offset() == 1
        out.append(v)
    return out


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape
    iv = {4: torch.int32, 8: torch.int64}[a.element_size()]
    assert torch.equal(a.view(iv), b.view(iv))


def _nchunks(n):
    return MULTI.get(n, (1, n))[0]


# ------------------------------------------------------------ kernels
@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("offset_views", [False, True])
@pytest.mark.parametrize("n", SHAPES)
def test_masks_counts_and_producers(ext, n, offset_views):
    """Masks have the described layout; the masked counts equal torch's
    and the column scan's, add into a non-zero `out`, and two launches
    with different partitions add into one `out`; moments, registers and
    code counts are bit-identical with masks on and off."""
    nchunks = _nchunks(n)
    xf, nf = _f32_cols(n, nchunks, 11 + n)
    xi, ni = _i32_cols(n, nchunks, 13 + n)
    if offset_views:
        cf, ci = _views(xf, NAN), _views(xi, -1)
    else:
        cf, ci = list(xf.to(DEV)), list(xi.to(DEV))
    sizes = [SIZE] * 3
    shifts = [0.0, 1.5, -2.0]

    mom0, regs0 = ext.moments_hll(cf, 12, shifts)
    mom1, regs1, fmasks, fparts = ext.moments_hll(cf, 12, shifts, null_masks=True)
    _same_bits(mom0, mom1)
    assert torch.equal(regs0, regs1)
    cnt0 = ext.code_counts_multi(ci, sizes)
    cnt1, imasks, iparts = ext.code_counts_multi(ci, sizes, null_masks=True)
    assert torch.equal(cnt0, cnt1)
    # the counts themselves, against torch (nulls and out-of-range codes share a slot)
    want = torch.stack([torch.cat([torch.bincount(r[(r >= 0) & (r < SIZE)].long(), minlength=SIZE),
                                   ((r < 0) | (r >= SIZE)).sum()[None]]) for r in xi]).reshape(-1)
    assert torch.equal(cnt1.cpu(), want)

    for k in range(3):
        _check_mask(fmasks[k], fparts[k], nf[k], nchunks)
        _check_mask(imasks[k], iparts[k], ni[k], nchunks)

    before = (torch.arange(n, dtype=torch.int32) % 7) + 1
    ref_f = torch.isnan(xf).sum(0).to(torch.int32)
    ref_i = (xi == -1).sum(0).to(torch.int32)
    assert torch.equal(ref_f, nf.sum(0).to(torch.int32)) and torch.equal(ref_i, ni.sum(0).to(torch.int32))

    out = before.clone().to(DEV)
    ext.row_null_counts_masked(fmasks, list(fparts[0]), out)
    assert torch.equal(out.cpu(), before + ref_f)
    ext.row_null_counts_masked(imasks, list(iparts[0]), out)
    assert torch.equal(out.cpu(), before + ref_f + ref_i)

    scan = before.clone().to(DEV)
    ext.row_null_counts_num(cf + ci, scan)
    assert torch.equal(out.cpu(), scan.cpu())

    # a second partition of the same rows: masks packed here with other
    # chunk counts (eleven columns: the unrolled loop and its remainder)
    for other in (3, 7):
        if other > n:
            continue
        g = torch.Generator().manual_seed(n + other)
        nulls = [_planted(n, other, g) for _ in range(11)]
        packed = [torch.from_numpy(_pack(v, other)[0].view(np.int64)).to(DEV) for v in nulls]
        ext.row_null_counts_masked(packed, [n, other, -(-n // other)], out)
        ref_f = ref_f + torch.stack(nulls).sum(0).to(torch.int32)
        assert torch.equal(out.cpu(), before + ref_f + ref_i)


@requires_gpu
@pytest.mark.gpu
def test_partitions_of_the_multi_chunk_shapes(ext):
    for n, (nchunks, per) in MULTI.items():
        x = torch.zeros(3, n, dtype=torch.float32, device=DEV)
        _, _, _, parts = ext.moments_hll(list(x), 12, [], null_masks=True)
        assert [tuple(p) for p in parts] == [(n, nchunks, per)] * 3
        assert (nchunks - 1) * per % 2 == 1  # an odd chunk start


@requires_gpu
@pytest.mark.gpu
def test_columns_without_a_mask(ext):
    """f64 columns and dictionaries above the LDS limit emit no mask; the
    other columns of the call do."""
    n = 1025
    g = torch.Generator().manual_seed(5)
    f32 = torch.randn(n, generator=g)
    f32[::9] = NAN
    cols = [f32.to(DEV), f32.double().to(DEV), f32.flip(0).to(DEV)]
    _, _, masks, parts = ext.moments_hll(cols, 12, [], null_masks=True)
    assert masks[1] is None and list(parts[1]) == []
    _check_mask(masks[0], parts[0], torch.isnan(f32), 1)
    _check_mask(masks[2], parts[2], torch.isnan(f32.flip(0)), 1)

    codes = torch.randint(-1, 5, (n,), generator=g).to(torch.int32)
    big = CODE_LDS_SLOTS  # + the null slot: one more than the LDS holds
    flat, masks, parts = ext.code_counts_multi([codes.to(DEV)] * 3, [5, big, big - 1], null_masks=True)
    assert masks[1] is None and list(parts[1]) == []
    _check_mask(masks[0], parts[0], codes == -1, 1)
    _check_mask(masks[2], parts[2], codes == -1, 1)
    assert torch.equal(flat, ext.code_counts_multi([codes.to(DEV)] * 3, [5, big, big - 1]))


@requires_gpu
@pytest.mark.gpu
def test_refusals(ext):
    out = torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="no columns"):
        ext.row_null_counts_masked([], [8, 1, 8], out)
    with pytest.raises(RuntimeError, match="no columns"):
        ext.moments_hll([], 12, [], null_masks=True)
    with pytest.raises(RuntimeError, match="no columns"):
        ext.code_counts_multi([], [], null_masks=True)
    mask = torch.zeros(_chunk_words(8), dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="partition"):
        ext.row_null_counts_masked([mask], [8, 1, 9], out)  # per is not ceil(n / nchunks)
    with pytest.raises(RuntimeError, match="partition"):
        ext.row_null_counts_masked([mask], [8, 0, 8], out)
    with pytest.raises(RuntimeError, match="words"):
        ext.row_null_counts_masked([mask[:4]], [8, 1, 8], out)  # too short for its partition
    with pytest.raises(RuntimeError, match="length mismatch"):
        ext.row_null_counts_masked([mask], [8, 1, 8], out[:7])
    odd = torch.zeros(_chunk_words(8) + 1, dtype=torch.int64, device=DEV)[1:]
    with pytest.raises(RuntimeError, match="aligned"):
        ext.row_null_counts_masked([odd], [8, 1, 8], out)  # 8 bytes off
    with pytest.raises(RuntimeError, match="int64"):
        ext.row_null_counts_masked([mask.to(torch.int32)], [8, 1, 8], out)
    assert int(out.sum()) == 0


# ------------------------------------------------------------ the frame
N_FRAME = 65_537  # two chunks


def _mixed_frame(dev):
    """f32, f64, small-dictionary and large-dictionary columns with planted
    nulls; some rows null in every column."""
    from anovos_amd.core.frame import AnovosFrame, Column

    n = N_FRAME
    g = torch.Generator().manual_seed(3)
    everywhere = torch.rand(n, generator=g) < 0.02
    cols = {}
    for i in range(4):
        x = torch.randint(0, 40, (n,), generator=g).to(torch.float32)
        x[_planted(n, 2, g) | everywhere] = NAN
        cols[f"f{i}"] = Column(f"f{i}", "float", x.to(dev))
    x = torch.randn(n, generator=g, dtype=torch.float64)
    x[_planted(n, 2, g) | everywhere] = NAN
    cols["d0"] = Column("d0", "double", x.to(dev))
    for i, size in enumerate([5, 9, CODE_LDS_SLOTS]):
        codes = torch.randint(0, size, (n,), generator=g).to(torch.int32)
        codes[_planted(n, 2, g) | everywhere] = -1
        cols[f"c{i}"] = Column(f"c{i}", "string", codes.to(dev), [f"v{j:05d}" for j in range(size)])
    return AnovosFrame(cols, dev)


NUM = ["f0", "f1", "f2", "f3", "d0"]
CAT = ["c0", "c1", "c2"]
MASKED = ["f0", "f1", "f2", "f3", "c0", "c1"]  # d0 is f64, c2 counts in global memory


def _warm(idf):
    from anovos_amd.ops import distinct as distinct_ops
    from anovos_amd.ops.groupby import cat_value_counts

    idf.clear_stats_cache()
    distinct_ops.approx_distinct(idf, NUM)
    cat_value_counts(idf, CAT)


def _reference_counts(idf):
    return sum(idf.col(c).null_mask().cpu().to(torch.int32) for c in NUM + CAT)


@requires_gpu
@pytest.mark.gpu
def test_row_null_counts_fallbacks(monkeypatch):
    """Warm masks, f64 and large-dictionary columns next to them, a cache
    filled for some columns only, a mask recorded with another partition,
    and the switch turned off all give the counts of the cold path."""
    from anovos_amd.ops import rowops

    idf = _mixed_frame(DEV)
    ref = _reference_counts(idf)
    idf.clear_stats_cache()
    cold = rowops.row_null_counts(idf, NUM + CAT).cpu()
    assert torch.equal(cold, ref)

    monkeypatch.delenv("ANOVOS_NULL_MASKS", raising=False)
    _warm(idf)
    key = rowops.NULL_MASK_KEY
    assert [c for c in NUM + CAT if key in idf.col(c).cache] == MASKED
    launches = []
    ext = rowops.backend.hip_ext()

    class Spy:
        def __getattr__(self, name):
            f = getattr(ext, name)
            if name.startswith("row_null_counts"):
                return lambda cols, *a: (launches.append((name, len(cols))), f(cols, *a))[1]
            return f

    monkeypatch.setattr(rowops.backend, "hip_ext", lambda: Spy())
    assert torch.equal(rowops.row_null_counts(idf, NUM + CAT).cpu(), ref)
    # f32 and code masks share (n, 2, per) here: one masked launch, and the
    # column scan for d0 and c2
    assert launches == [("row_null_counts_masked", 6), ("row_null_counts_num", 2)]

    # some columns only
    for c in ("f1", "c0"):
        del idf.col(c).cache[key]
    del launches[:]
    assert torch.equal(rowops.row_null_counts(idf, NUM + CAT).cpu(), ref)
    assert launches == [("row_null_counts_masked", 4), ("row_null_counts_num", 4)]

    # a mask of other rows: its n is not this shard's
    m, (n, nchunks, per) = idf.col("f0").cache[key]
    idf.col("f0").cache[key] = (m, (n - 1, nchunks, -(-(n - 1) // nchunks)))
    # ... and one made with another partition of the same rows: a group of its own
    nulls = idf.col("f2").null_mask().cpu()
    idf.col("f2").cache[key] = (torch.from_numpy(_pack(nulls, 5)[0].view(np.int64)).to(DEV),
                                (n, 5, -(-n // 5)))
    del launches[:]
    assert torch.equal(rowops.row_null_counts(idf, NUM + CAT).cpu(), ref)
    assert sorted(launches) == [("row_null_counts_masked", 1), ("row_null_counts_masked", 2),
                                ("row_null_counts_num", 5)]

    # the switch
    monkeypatch.setenv("ANOVOS_NULL_MASKS", "0")
    _warm(idf)
    assert not [c for c in NUM + CAT if key in idf.col(c).cache]
    del launches[:]
    assert torch.equal(rowops.row_null_counts(idf, NUM + CAT).cpu(), ref)
    assert launches == [("row_null_counts_num", 8)]


@requires_gpu
@pytest.mark.gpu
def test_statistics_do_not_depend_on_the_switch(monkeypatch):
    """What the two producers are called for is the same with masks on and off."""
    from anovos_amd.ops import distinct as distinct_ops
    from anovos_amd.ops.groupby import cat_value_counts

    idf = _mixed_frame(DEV)
    got = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("ANOVOS_NULL_MASKS", switch)
        idf.clear_stats_cache()
        distinct = distinct_ops.approx_distinct(idf, NUM)
        counts = cat_value_counts(idf, CAT)
        moments = {c: idf.col(c).cache["moments"] for c in NUM}
        got[switch] = (distinct, counts, moments, {c: idf.col(c).cache["nulls_local"] for c in CAT})
    assert got["1"][0] == got["0"][0]
    for c in CAT:
        assert torch.equal(got["1"][1][c], got["0"][1][c])
    for c in NUM:
        a, b = got["1"][2][c], got["0"][2][c]
        va = np.array([getattr(a, k) for k in a.__slots__], dtype=np.float64)
        vb = np.array([getattr(b, k) for k in b.__slots__], dtype=np.float64)
        assert np.array_equal(va.view(np.int64), vb.view(np.int64)), c
    assert got["1"][3] == got["0"][3]


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0.8, 1])
@pytest.mark.parametrize("treatment", [False, True])
def test_null_rows_detection_warm_equals_cold(ctx, monkeypatch, treatment, threshold):
    from anovos_amd.data_analyzer import quality_checker as qc
    from anovos_amd.ops import rowops

    monkeypatch.delenv("ANOVOS_NULL_MASKS", raising=False)
    idf = _mixed_frame(DEV)
    _warm(idf)
    assert rowops.NULL_MASK_KEY in idf.col("f0").cache
    odf_w, print_w = qc.nullRows_detection(ctx, idf, treatment=treatment, treatment_threshold=threshold)
    idf.clear_stats_cache()
    odf_c, print_c = qc.nullRows_detection(ctx, idf, treatment=treatment, treatment_threshold=threshold)
    pd.testing.assert_frame_equal(print_w, print_c)
    pd.testing.assert_frame_equal(print_w, _expected_null_rows(idf, treatment, threshold))
    assert odf_w.count() == odf_c.count()
    for c in NUM + CAT:
        _same_bits(odf_w.col(c).data, odf_c.col(c).data)
    if treatment:
        ncols = len(NUM + CAT)
        cnt = _reference_counts(idf)
        keep = ~(cnt == ncols if threshold == 1 else cnt > ncols * threshold)
        assert odf_w.count() == int(keep.sum())
        _same_bits(odf_w.col("f0").data, idf.col("f0").data.cpu()[keep])


# ------------------------------------------------------------ without a GPU
def _expected_null_rows(idf, treatment, threshold):
    """The table from its definition: one row per occurring null count,
    ascending, with the share of rows rounded to 4 places and the flag of
    the threshold rule."""
    cols = [c for c in idf.columns]
    cnt = sum(idf.col(c).null_mask().cpu().to(torch.int64) for c in cols).numpy()
    rows = []
    for nc in range(len(cols) + 1):
        k = int((cnt == nc).sum())
        if k:
            fl = int(nc == len(cols)) if threshold == 1 else int(nc > len(cols) * threshold)
            rows.append([nc, k, round(k / len(cnt), 4), fl])
    return pd.DataFrame(rows, columns=["null_cols_count", "row_count", "row_pct",
                                       "treated" if treatment else "flagged"])


@pytest.mark.parametrize("threshold", [0.0, 0.5, 0.8, 1])
@pytest.mark.parametrize("treatment", [False, True])
def test_null_rows_detection_on_the_cpu(ctx, treatment, threshold):
    from anovos_amd.data_analyzer import quality_checker as qc

    idf = _mixed_frame("cpu")
    odf, table = qc.nullRows_detection(ctx, idf, treatment=treatment, treatment_threshold=threshold)
    pd.testing.assert_frame_equal(table, _expected_null_rows(idf, treatment, threshold))
    ncols = len(idf.columns)
    cnt = _reference_counts(idf)
    flagged = cnt == ncols if threshold == 1 else cnt > ncols * threshold
    assert 0 < int(flagged.sum()) < N_FRAME
    if treatment:
        assert odf.count() == int((~flagged).sum())
        _same_bits(odf.col("d0").data, idf.col("d0").data[~flagged])
    else:
        assert odf is idf


def test_cpu_row_null_counts_ignore_the_cache(monkeypatch):
    """The CPU path counts from the columns, whatever the cache holds."""
    from anovos_amd.ops import rowops

    idf = _mixed_frame("cpu")
    ref = _reference_counts(idf)
    idf.col("f0").cache[rowops.NULL_MASK_KEY] = (torch.zeros(8, dtype=torch.int64), (N_FRAME, 1, N_FRAME))
    assert torch.equal(rowops.row_null_counts(idf, NUM + CAT), ref)
