#!/usr/bin/env python3
"""Idle intervals of the analyzer phase from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- \
        python bench.py --rows 50000000 --steps 2 --warmup 1
    python tools/trace_gaps.py DIR/NAME_kernel_trace.csv

Per pipeline step (one bucketize_label_counts dispatch each) it prints
  gram->bkt : end of the last Gram kernel to the start of
              bucketize_label_counts_kernel, and the time other kernels ran
              inside that interval;
  hist->next: end of the step's second hist_kernel to the start of the next
              kernel of the project (torch's small elementwise / copy
              kernels in between are listed as busy time);
and the per-dispatch times of the kernels the quantile and IV/IG sections use.
"""
import csv
import sys
from collections import defaultdict

OURS = ("_kernel<", "_kernel(")


def short(name):
    name = name.replace("void ", "")
    return name.split("(")[0].split("<")[0]


def main(path):
    rows = list(csv.DictReader(open(path)))
    ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in rows))
    ours = lambda n: not n.startswith("at::") and not n.startswith("__amd") and "rocprim" not in n
    bkt = [i for i, e in enumerate(ev) if e[2] == "bucketize_label_counts_kernel"]
    durs = defaultdict(list)
    for s, e, n in ev:
        if n in ("hist_kernel", "bucketize_label_counts_kernel", "label_counts_multi_kernel",
                 "hist_quantile_query_kernel", "inthist_quantile_query_kernel"):
            durs[n].append((e - s) / 1e3)
    prev = 0
    for step, ib in enumerate(bkt):
        seg = ev[prev:ib + 1]
        grams = [k for k, e in enumerate(seg) if e[2].startswith("gram_")]
        if grams:
            g_end = seg[grams[-1]][1]
            between = seg[grams[-1] + 1:-1]
            busy = sum(e - s for s, e, _ in between)
            print(f"step {step}: gram->bkt   gap {(seg[-1][0] - g_end) / 1e6:8.3f} ms, "
                  f"{len(between)} kernels busy {busy / 1e6:.3f} ms")
        hists = [k for k, e in enumerate(seg) if e[2] == "hist_kernel"]
        if len(hists) >= 2:
            print(f"step {step}: hist->hist  gap {(seg[hists[1]][0] - seg[hists[0]][1]) / 1e6:8.3f} ms "
                  f"(dense integer counts answered, pass-1 launch prepared)")
            h_end = seg[hists[1]][1]
            rest = seg[hists[1] + 1:]
            nxt_any = rest[0]
            k_ours = next(k for k, e in enumerate(rest) if ours(e[2]) and "quantile_query" not in e[2])
            busy = sum(e - s for s, e, _ in rest[:k_ours])
            print(f"step {step}: hist->next  gap {(rest[k_ours][0] - h_end) / 1e6:8.3f} ms to {rest[k_ours][2]}, "
                  f"{k_ours} kernels busy {busy / 1e6:.3f} ms; first kernel of any kind after "
                  f"{(nxt_any[0] - h_end) / 1e6:.3f} ms ({nxt_any[2][:40]})")
        prev = ib + 1
    for n, d in durs.items():
        print(f"{n}: " + " ".join(f"{x:.1f}" for x in d) + " us")


if __name__ == "__main__":
    main(sys.argv[1])
