"""Exact tests of the pair-count kernel (K22, ops/hip/pair_counts.hip).

Every input is built on the CPU from a seeded generator and every result
is compared, with exact integer equality, against a torch.bincount
reference written here: slot v for a code 0 <= v < size, the null slot
`size` for anything else, table (i, j) row-major [size_i + 1][size_j + 1],
tables concatenated in pair order.

Shapes follow the binding: rows split into chunks of about 65 536 (one
block each per work item), 16-byte vector loads with a scalar head and
tail, at most 16 384 LDS counters per work item, at most 8 partner
columns per anchor column."""

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

DEV = "cuda"
INT32_MAX = 2**31 - 1
LDS_SLOTS = 16384


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    e = backend.require_hip()
    assert e is not None, "HIP extension must be loadable on the GPU box"
    return e


def _slots(codes, size):
    c = codes.to(torch.int64)
    return torch.where((c >= 0) & (c < size), c, torch.full_like(c, size))


def _ref_tables(cols, sizes, pair_i, pair_j):
    """One int64 [size_i + 1, size_j + 1] table per pair."""
    out = []
    for i, j in zip(pair_i, pair_j):
        key = _slots(cols[i], sizes[i]) * (sizes[j] + 1) + _slots(cols[j], sizes[j])
        cells = (sizes[i] + 1) * (sizes[j] + 1)
        out.append(torch.bincount(key, minlength=cells).reshape(sizes[i] + 1, sizes[j] + 1))
    return out


def _codes(n, size, g):
    """Codes in [-1, size]: every valid code, NULL_CODE and `size` itself
    (the first code past the dictionary)."""
    return torch.randint(-1, size + 1, (n,), generator=g).to(torch.int32)


def _check(ext, cols, sizes, pair_i, pair_j, dev_cols=None):
    """Run the binding and compare table by table at the offsets the
    contract gives (cumulative cells in pair order)."""
    dev_cols = dev_cols if dev_cols is not None else [c.to(DEV) for c in cols]
    got = ext.pair_code_counts(dev_cols, sizes, pair_i, pair_j).cpu()
    want = _ref_tables(cols, sizes, pair_i, pair_j)
    assert got.dtype == torch.int64 and got.dim() == 1
    assert got.numel() == sum(t.numel() for t in want)
    off = 0
    for q, t in enumerate(want):
        g = got[off : off + t.numel()].reshape(t.shape)
        assert torch.equal(g, t), f"pair {q} = ({pair_i[q]}, {pair_j[q]}) at offset {off}"
        off += t.numel()
    return got


# 0: no launch; 1, 3: below one vector; 4, 5: one vector (+ tail); 255..257
# around one vector per thread of a wave group; 1023: four vectors short of
# a full block trip; 65 537: first length with two chunks; 131 079: three
# chunks of 43 696 rows (rounded up to a multiple of 4) with a short last one
LENGTHS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 65_537, 131_079]


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(ext, n):
    g = torch.Generator().manual_seed(1000 + n)
    sizes = [3, 5, 2]
    cols = [_codes(n, s, g) for s in sizes]
    got = _check(ext, cols, sizes, [0, 0, 1], [1, 2, 2])
    # every row lands in exactly one cell of every table
    assert int(got[: 4 * 6].sum()) == n and int(got[4 * 6 : 4 * 6 + 4 * 3].sum()) == n


@requires_gpu
@pytest.mark.gpu
def test_lds_limit_staged_and_global_items_in_one_launch(ext):
    """Tables of 16 383 and exactly 16 384 cells stage in LDS, 16 512 cells
    count in global memory, next to a small pair — one launch. The LDS of
    the launch must be sized by the largest table that stages (16 384
    counters), not by the largest table of the launch."""
    g = torch.Generator().manual_seed(7)
    n = 70_001  # two chunks
    sizes = [126, 128, 127, 127, 3, 5]
    cols = [_codes(n, s, g) for s in sizes]
    pair_i = [0, 2, 2, 4]
    pair_j = [1, 3, 1, 5]
    cells = [(sizes[i] + 1) * (sizes[j] + 1) for i, j in zip(pair_i, pair_j)]
    assert cells == [LDS_SLOTS - 1, LDS_SLOTS, 16_512, 24]
    _check(ext, cols, sizes, pair_i, pair_j)
    items, _reads, lds = ext.pair_code_counts_plan(sizes, pair_i, pair_j)
    assert items == 4 and lds == LDS_SLOTS


@requires_gpu
@pytest.mark.gpu
def test_packing_and_offsets(ext):
    g = torch.Generator().manual_seed(11)
    n = 70_003
    # column 0 is the anchor (10 categories); 1..8 small partners; 9 too
    # large for LDS (11 * 2001 cells); 10..12 fit LDS one at a time but
    # not together (11 * 701 = 7711 cells each)
    sizes = [10, 1, 2, 3, 4, 5, 6, 7, 8, 2000, 700, 700, 700]
    cols = [_codes(n, s, g) for s in sizes]
    dev_cols = [c.to(DEV) for c in cols]

    eight = list(range(1, 9))
    _check(ext, cols, sizes, [0] * 8, eight, dev_cols)
    items, reads, _ = ext.pair_code_counts_plan(sizes, [0] * 8, eight)
    assert (items, reads) == (1, 9)  # anchor once + eight partners

    # the oversized partner in the middle of the list
    pj = [1, 2, 3, 4, 9, 5, 6, 7, 8]
    _check(ext, cols, sizes, [0] * len(pj), pj, dev_cols)

    # more than eight partners, and partners that overflow the LDS budget
    pj = list(range(1, 13))
    _check(ext, cols, sizes, [0] * len(pj), pj, dev_cols)
    items, reads, lds = ext.pair_code_counts_plan(sizes, [0] * len(pj), pj)
    assert reads == items + len(pj) and lds <= LDS_SLOTS

    # several anchors interleaved in the pair list
    pi = [3, 0, 5, 0, 3, 12, 5, 0]
    pj = [4, 10, 6, 11, 5, 0, 9, 12]
    _check(ext, cols, sizes, pi, pj, dev_cols)


@requires_gpu
@pytest.mark.gpu
def test_slots(ext):
    """Empty and one-entry dictionaries; every code outside [0, size)
    lands in the null slot; a pair (i, i); the same pair twice."""
    sizes = [0, 1, 4]
    c0 = torch.tensor([-1, 0, 5, INT32_MAX, -7, 0, 1, -1, 3], dtype=torch.int32)
    c1 = torch.tensor([0, 1, -1, -7, INT32_MAX, 0, 0, 1, 0], dtype=torch.int32)
    c2 = torch.tensor([4, 3, -1, 0, INT32_MAX, -7, 2, 4, 1], dtype=torch.int32)
    cols = [c0, c1, c2]
    pair_i = [0, 0, 1, 2, 1, 1, 2]
    pair_j = [1, 0, 2, 2, 2, 1, 0]
    got = _check(ext, cols, sizes, pair_i, pair_j)
    n = c0.numel()
    # table (0, 0): one cell, every row
    assert got[2:3].tolist() == [n]
    # table (2, 2) is diagonal: codes 4, INT32_MAX, -7, -1 are all null
    t22 = got[2 + 1 + 10 : 2 + 1 + 10 + 25].reshape(5, 5)
    assert torch.equal(t22, torch.diag(torch.tensor([1, 1, 1, 1, 5])))
    # the pair listed twice gives the same table twice
    assert torch.equal(got[3:13], got[38:48])


@requires_gpu
@pytest.mark.gpu
def test_contention_one_cell(ext):
    n = 200_000
    sizes = [6, 9]
    cols = [torch.full((n,), 4, dtype=torch.int32), torch.full((n,), 7, dtype=torch.int32)]
    got = _check(ext, cols, sizes, [0], [1]).reshape(7, 10)
    assert int(got[4, 7]) == n and int(got.sum()) == n


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [(1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 2, 3), (0, 3, 0)])
def test_offset_views(ext, offsets):
    """Columns are base[o:o+n]: 4-byte aligned only. The elements outside
    the window hold code 0, the window never does, so an out-of-window
    read shows up in row 0 / column 0 of a table."""
    g = torch.Generator().manual_seed(23 + sum(offsets))
    n = 70_003
    sizes = [3, 5, 2]
    cols, dev_cols = [], []
    for s, o in zip(sizes, offsets):
        c = torch.randint(1, s + 2, (n,), generator=g).to(torch.int32)  # 1..size + 1 (size and size + 1 are null)
        base = torch.zeros(n + o + 5, dtype=torch.int32)
        base[o : o + n] = c
        v = base.to(DEV)[o : o + n]
        assert v.is_contiguous() and v.storage_offset() == o
        cols.append(c)
        dev_cols.append(v)
    got = _check(ext, cols, sizes, [0, 0, 1], [1, 2, 2], dev_cols)
    t01 = got[:24].reshape(4, 6)
    assert int(t01[0].sum()) == 0 and int(t01[:, 0].sum()) == 0 and int(t01.sum()) == n


@requires_gpu
@pytest.mark.gpu
def test_refusals(ext):
    n = 64
    a = torch.zeros(n, dtype=torch.int32, device=DEV)
    b = torch.zeros(n, dtype=torch.int32, device=DEV)
    strided = torch.zeros(2 * n, dtype=torch.int32, device=DEV)[::2]
    assert not strided.is_contiguous()
    with pytest.raises(RuntimeError):
        ext.pair_code_counts([a, strided], [2, 2], [0], [1])
    with pytest.raises(RuntimeError):
        ext.pair_code_counts([a, b.to(torch.int64)], [2, 2], [0], [1])
    with pytest.raises(RuntimeError):
        ext.pair_code_counts([a, b[: n - 1]], [2, 2], [0], [1])
    with pytest.raises(RuntimeError):
        ext.pair_code_counts([a, b], [2, 2], [0], [2])  # pair index == ncols
    with pytest.raises(RuntimeError):
        ext.pair_code_counts([a, b], [2, 2], [-1], [1])
    with pytest.raises(RuntimeError):
        ext.pair_code_counts([], [], [], [])
    with pytest.raises(RuntimeError):
        ext.pair_code_counts([a, b], [2], [0], [1])  # sizes / cols mismatch
    with pytest.raises(RuntimeError):
        ext.pair_code_counts([a, b], [2, 2], [0, 0], [1])  # pair_i / pair_j mismatch
    # a good call still works after the refusals
    got = ext.pair_code_counts([a, b], [2, 2], [0], [1]).cpu()
    assert got.tolist() == [n, 0, 0, 0, 0, 0, 0, 0, 0]
