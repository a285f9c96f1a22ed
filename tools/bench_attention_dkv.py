"""Same-process A/B of the attention-backward dk/dv kernel bodies
(FMS_AMD_ATTN_DKV / _C.attn_dkv_mode: "legacy" vs "keylane").

Machines differ by 5-10 %, so the two bodies are alternated inside ONE
process: --repeats rounds of (legacy, keylane) per shape and workspace
path, after one discarded warm-up round. Each round reports the
per-kernel device time of the dkv and dq kernels from torch.profiler and
the whole _C.attn_bwd (delta + dkv + dq) by device events. The spread is
max-min of the legacy repeats; the new body counts as faster only if its
median beats legacy's by more than twice that spread.

Paths: "ws" = default workspace limit (dkv publishes dS, the benchmark
path), "nows" = limit 0 (dkv keeps dS to itself, dq recomputes).

Run on GPU: python tools/bench_attention_dkv.py [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import _C

SHAPES = [("mha", (2, 4096, 32, 32, 128)), ("gqa", (2, 4096, 32, 8, 128))]
MODES = ["legacy", "keylane"]
# profiler-name substrings -> reported name (both dkv bodies share "dkv")
KERNELS = {"attn_bwd_dkv": "dkv", "attn_bwd_dq": "dq"}


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


def kernel_ms(fn, iters, warmup):
    """Per-kernel mean device time from torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        for sub, name in KERNELS.items():
            if sub in ev.key:
                t = getattr(ev, "device_time_total", None)
                if t is None:
                    t = ev.cuda_time_total
                out[name] = out.get(name, 0.0) + t / 1e3 / iters
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    torch.manual_seed(0)
    entry_mode = _C.attn_dkv_mode()
    entry_limit = _C.attn_bwd_ws_limit()
    paths = [("ws", entry_limit), ("nows", 0)]
    results = []
    for tag, (b, s, h, kvh, d) in SHAPES:
        q = torch.randn(b, s, h, d, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(b, s, kvh, d, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(b, s, kvh, d, device="cuda", dtype=torch.bfloat16)
        do = torch.randn_like(q)
        o, lse = _C.attn_fwd(q, k, v)
        bwd = lambda: _C.attn_bwd(do, q, k, v, o, lse, None)
        chain = 2 * b * h * s * s * d * 0.5   # one causal gemm chain
        for path, limit in paths:
            _C.attn_bwd_ws_limit(limit)
            # useful flops: dkv 4 chains; dq 1 (workspace) or 3 (recompute)
            flops = {"dkv": 4 * chain, "dq": (1 if path == "ws" else 3) * chain,
                     "attn_bwd": 5 * chain}
            samples = {m: {} for m in MODES}
            # round 0 is thrown away: it carries the first allocation of
            # the workspace and the profiler's start-up
            for rnd in range(args.repeats + 1):
                for m in MODES:
                    _C.attn_dkv_mode(m)
                    meas = kernel_ms(bwd, args.iters, args.warmup)
                    meas["attn_bwd"] = event_ms(bwd, args.iters, args.warmup)
                    if rnd == 0:
                        continue
                    for name, ms in meas.items():
                        samples[m].setdefault(name, []).append(ms)
            for name in ("dkv", "dq", "attn_bwd"):
                leg, new = samples["legacy"][name], samples["keylane"][name]
                spread = max(leg) - min(leg)
                ml, mn = statistics.median(leg), statistics.median(new)
                faster = (ml - mn) > 2 * spread
                row = dict(shape=tag, path=path, b=b, s=s, h=h, kvh=kvh, d=d,
                           what=name, legacy_ms=leg, keylane_ms=new,
                           legacy_median_ms=ml, keylane_median_ms=mn,
                           legacy_spread_ms=spread,
                           legacy_tfs=flops[name] / ml / 1e9,
                           keylane_tfs=flops[name] / mn / 1e9,
                           keylane_faster=faster)
                results.append(row)
                print(f"{tag} {path:4s} {name:8s} legacy {ml:7.3f} ms "
                      f"{row['legacy_tfs']:6.1f} TF/s (spread {spread:.3f}) | "
                      f"keylane {mn:7.3f} ms {row['keylane_tfs']:6.1f} TF/s | "
                      f"x{ml / mn:.3f} "
                      f"{'FASTER' if faster else 'within 2x spread'}")
                print(f"    legacy  {[round(x, 3) for x in leg]}")
                print(f"    keylane {[round(x, 3) for x in new]}")
    _C.attn_dkv_mode(entry_mode)
    _C.attn_bwd_ws_limit(entry_limit)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
