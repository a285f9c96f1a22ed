"""Same-process timing of the document-masked attention kernels against the
unmasked ones, forward and backward, at b2 h32 d128 and s in {4096, 8192}.

Cases per sequence length:
  unmasked-ws     _C.attn_fwd / _C.attn_bwd with the dS workspace (s=4096)
  unmasked-free   the same, workspace limit 0 (the masked backward's sibling)
  doc-one         masked kernels, one document per row: the price of the
                  mask on rows that do not need it (compare unmasked-free)
  doc-2048/512/128  masked kernels, fixed document lengths: the gain from
                  skipping tiles outside a workgroup's documents
  doc-mixed       masked kernels, one row of mixed document lengths

Machines differ by 5-10 %, so all cases are alternated inside ONE process:
--repeats rounds over every case, each timing --iters calls with device
events; medians and the max-min spread over the rounds are reported. The
spread of unmasked-free is the run-to-run noise to hold doc-one against.

Run on GPU: python tools/bench_attention_docmask.py [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import _C, ops

B, H, KVH, D = 2, 32, 32, 128
SEQS = [4096, 8192]
# document lengths of the mixed row, repeated until the row is full
MIXED = [1500, 300, 40, 2200, 128, 700, 1, 3000, 64, 259]


def event_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def starts_fixed(s, length):
    pos = torch.arange(s, dtype=torch.int32)
    return (pos // length * length).expand(B, s)


def starts_mixed(s):
    start = torch.zeros(s, dtype=torch.int32)
    a, i = 0, 0
    while a < s:
        start[a:] = a
        a += MIXED[i % len(MIXED)]
        i += 1
    return start.expand(B, s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seqs", default=",".join(map(str, SEQS)))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    torch.manual_seed(0)
    entry = _C.attn_bwd_ws_limit()
    results = []
    for s in map(int, args.seqs.split(",")):
        q = torch.randn(B, s, H, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(B, s, KVH, D, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(B, s, KVH, D, device="cuda", dtype=torch.bfloat16)
        do = torch.randn_like(q)

        cases = {}      # name -> (limit, fwd, bwd, visible fraction)
        o, lse = _C.attn_fwd(q, k, v)
        plain = (lambda: _C.attn_fwd(q, k, v),
                 lambda o=o, lse=lse: _C.attn_bwd(do, q, k, v, o, lse, None))
        if s <= 4096:
            cases["unmasked-ws"] = (1 << 62, *plain, 1.0)
        cases["unmasked-free"] = (0, *plain, 1.0)
        layouts = [("doc-one", starts_fixed(s, s))]
        layouts += [(f"doc-{n}", starts_fixed(s, n)) for n in (2048, 512, 128)]
        layouts.append(("doc-mixed", starts_mixed(s)))
        full = s * (s + 1) / 2
        for name, start in layouts:
            m = ops.doc_mask_from_starts(start.contiguous().cuda())
            om, lsem = _C.attn_fwd_doc(q, k, v, m.start)
            pos = torch.arange(s, device="cuda")
            visible = float((pos - m.start[0] + 1).sum()) / full
            cases[name] = (
                entry,
                lambda m=m: _C.attn_fwd_doc(q, k, v, m.start),
                lambda m=m, om=om, lsem=lsem: _C.attn_bwd_doc(
                    do, q, k, v, om, lsem, None, m.start, m.end),
                visible)

        samples = {n: {"fwd": [], "bwd": []} for n in cases}
        for _ in range(args.repeats):
            for name, (limit, fwd, bwd, _) in cases.items():
                _C.attn_bwd_ws_limit(limit)
                samples[name]["fwd"].append(
                    event_ms(fwd, args.iters, args.warmup))
                samples[name]["bwd"].append(
                    event_ms(bwd, args.iters, args.warmup))
        _C.attn_bwd_ws_limit(entry)

        print(f"b{B} s{s} h{H} kvh{KVH} d{D}")
        for name, (_, _, _, visible) in cases.items():
            row = dict(s=s, case=name, visible_fraction=visible,
                       samples_ms=samples[name])
            line = f"    {name:14s} visible {visible:6.3f}"
            for ph in ("fwd", "bwd"):
                x = samples[name][ph]
                row[f"{ph}_median_ms"] = statistics.median(x)
                row[f"{ph}_spread_ms"] = max(x) - min(x)
                line += (f"  {ph} {row[f'{ph}_median_ms']:8.3f} ms "
                         f"(spread {row[f'{ph}_spread_ms']:.3f})")
            print(line)
            results.append(row)
        del cases, plain, q, k, v, do, o, lse
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
