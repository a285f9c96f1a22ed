"""Same-process A/B of the causal-attention workgroup orders
(FMS_AMD_ATTN_SCHED / _C.attn_sched_mode: "legacy" vs "balanced").

Machines differ by 5-10 %, so the two orders are alternated inside ONE
process: --repeats rounds of (legacy, balanced), each round timing fwd
and bwd (delta + dkv + dq) with device events. The spread is max-min of
the legacy repeats; an order counts as faster only if its median beats
the other's by more than twice that spread.

--split additionally runs every round under torch.profiler and reports
the per-kernel device time (fwd, dkv, dq separately).

Run on GPU: python tools/bench_attention_sched.py [--split] [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import _C

SHAPES = [("mha", (2, 4096, 32, 32, 128)), ("gqa", (2, 4096, 32, 8, 128))]
MODES = ["legacy", "balanced"]
KERNELS = ["attn_fwd_kernel", "attn_bwd_dkv_kernel", "attn_bwd_dq_kernel"]


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
        for k in KERNELS:
            if k in ev.key:
                t = getattr(ev, "device_time_total", None)
                if t is None:
                    t = ev.cuda_time_total
                out[k] = out.get(k, 0.0) + t / 1e3 / iters
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    torch.manual_seed(0)
    entry = _C.attn_sched_mode()
    results = []
    for tag, (b, s, h, kvh, d) in SHAPES:
        q = torch.randn(b, s, h, d, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(b, s, kvh, d, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(b, s, kvh, d, device="cuda", dtype=torch.bfloat16)
        do = torch.randn_like(q)
        o, lse = _C.attn_fwd(q, k, v)
        fwd = lambda: _C.attn_fwd(q, k, v)
        bwd = lambda: _C.attn_bwd(do, q, k, v, o, lse, None)
        both = lambda: (fwd(), bwd())
        fwd_flops = 2 * 2 * b * h * s * s * d * 0.5   # QK^T + PV, causal
        # useful flops per kernel: fwd 2 chains, dkv 4, dq 1
        flops = {"fwd": fwd_flops, "bwd": fwd_flops * 2.5,
                 "attn_fwd_kernel": fwd_flops,
                 "attn_bwd_dkv_kernel": fwd_flops * 2.0,
                 "attn_bwd_dq_kernel": fwd_flops * 0.5}
        samples = {m: {} for m in MODES}
        for _ in range(args.repeats):
            for m in MODES:
                _C.attn_sched_mode(m)
                if args.split:
                    meas = kernel_ms(both, args.iters, args.warmup)
                else:
                    meas = {"fwd": event_ms(fwd, args.iters, args.warmup),
                            "bwd": event_ms(bwd, args.iters, args.warmup)}
                for name, ms in meas.items():
                    samples[m].setdefault(name, []).append(ms)
        for name in samples["legacy"]:
            leg, bal = samples["legacy"][name], samples["balanced"][name]
            spread = max(leg) - min(leg)
            ml, mb = statistics.median(leg), statistics.median(bal)
            faster = (ml - mb) > 2 * spread
            row = dict(shape=tag, b=b, s=s, h=h, kvh=kvh, d=d, what=name,
                       legacy_ms=leg, balanced_ms=bal, legacy_median_ms=ml,
                       balanced_median_ms=mb, legacy_spread_ms=spread,
                       legacy_tfs=flops[name] / ml / 1e9,
                       balanced_tfs=flops[name] / mb / 1e9,
                       balanced_faster=faster)
            results.append(row)
            print(f"{tag} {name:20s} legacy {ml:8.3f} ms {row['legacy_tfs']:6.1f} TF/s"
                  f" (spread {spread:.3f}) | balanced {mb:8.3f} ms "
                  f"{row['balanced_tfs']:6.1f} TF/s | x{ml / mb:.3f} "
                  f"{'FASTER' if faster else 'within 2x spread'}")
            print(f"    legacy   {[round(x, 3) for x in leg]}")
            print(f"    balanced {[round(x, 3) for x in bal]}")
    _C.attn_sched_mode(entry)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
