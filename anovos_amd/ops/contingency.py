"""Contingency tables of categorical column pairs (kernel K22).

A categorical column is a tensor of int32 dictionary codes, so the table
of a column pair is a two-dimensional bincount over (slot_i, slot_j),
where a code outside [0, dictionary size) — NULL_CODE included — takes
the null slot after the last category. Integer tables merge across ranks
with one all-reduce.

- HIP path: ops/hip/pair_counts.hip packs an anchor column with several
  partner columns per work item, so k columns cost far fewer than
  2 * k(k-1)/2 column reads, and stages the counters in LDS.
- CPU path (also the reference inside the tests): torch.bincount over
  slot_i * s_j + slot_j.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from anovos_amd.core import dist
from anovos_amd.ops import backend
from anovos_amd.ops.groupby import align_dictionaries

# tables of one launch: bounds the flat int64 buffer that is allocated,
# all-reduced and copied to the host at once (50 columns with dictionaries
# of thousands would otherwise ask for tens of GB)
LAUNCH_TABLE_BYTES = 256 << 20


def _slots(codes: torch.Tensor, size: int) -> torch.Tensor:
    c = codes.to(torch.int64)
    return torch.where((c >= 0) & (c < size), c, torch.full_like(c, size))


def _launches(cells: Sequence[int], budget_bytes: int) -> List[Tuple[int, int]]:
    """[start, stop) ranges of consecutive pairs whose tables together stay
    within the budget; a table larger than the budget goes alone."""
    out, start, used = [], 0, 0
    for q, c in enumerate(cells):
        if q > start and used + 8 * c > budget_bytes:
            out.append((start, q))
            start, used = q, 0
        used += 8 * c
    if len(cells) > start:
        out.append((start, len(cells)))
    return out


def pair_contingency_tables(
    idf, cols: List[str], pairs: Optional[List[Tuple[str, str]]] = None
) -> Dict[Tuple[str, str], np.ndarray]:
    """Global contingency table of every pair: {(ci, cj): int64 array
    [len(dict_i) + 1, len(dict_j) + 1]} in dictionary order, nulls as the
    last row / last column. pairs=None means every (cols[a], cols[b]) with
    a < b. Collective: every rank calls it with the same cols and pairs."""
    cols = list(cols)
    for c in cols:
        if idf.col(c).kind != "categorical":
            raise TypeError(f"pair_contingency_tables needs categorical columns, got '{c}'")
    if pairs is None:
        pairs = [(cols[a], cols[b]) for a in range(len(cols)) for b in range(a + 1, len(cols))]
    pairs = [tuple(p) for p in pairs]
    # the slot layout keys off dictionary sizes: they must be rank-identical
    align_dictionaries(idf, cols)
    pos = {c: k for k, c in enumerate(cols)}
    sizes = [len(idf.col(c).dictionary or []) for c in cols]
    pi = [pos[a] for a, _ in pairs]
    pj = [pos[b] for _, b in pairs]
    cells = [(sizes[a] + 1) * (sizes[b] + 1) for a, b in zip(pi, pj)]
    data = [idf.col(c).data for c in cols]
    dev = data[0].device if data else idf.device

    use_gpu = bool(data) and all(t.is_cuda for t in data) and backend.use_hip(data[0])
    if use_gpu:
        ext = backend.hip_ext()
        data = [t.contiguous() if t.dtype == torch.int32 else t.to(torch.int32).contiguous() for t in data]

    out: Dict[Tuple[str, str], np.ndarray] = {}
    for start, stop in _launches(cells, LAUNCH_TABLE_BYTES):
        if use_gpu:
            flat = ext.pair_code_counts(data, sizes, pi[start:stop], pj[start:stop])
        else:
            slot = {}
            parts = []
            for a, b in zip(pi[start:stop], pj[start:stop]):
                for k in (a, b):
                    if k not in slot:
                        slot[k] = _slots(data[k], sizes[k])
                key = slot[a] * (sizes[b] + 1) + slot[b]
                parts.append(torch.bincount(key, minlength=(sizes[a] + 1) * (sizes[b] + 1)))
            flat = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=dev)
        host = dist.all_reduce_(flat, "sum").cpu().numpy()  # one collective, one copy per launch
        off = 0
        for q in range(start, stop):
            a, b = pi[q], pj[q]
            out[pairs[q]] = host[off : off + cells[q]].reshape(sizes[a] + 1, sizes[b] + 1)
            off += cells[q]
    return out
