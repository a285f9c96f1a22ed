"""Same-process A/B of the two causal-attention backward paths: the dS
workspace path (dkv publishes dS, dq consumes it) against the
workspace-free path (dkv keeps dS, dq recomputes it), selected through
_C.attn_bwd_ws_limit (attn_ws.h).

Machines differ by 5-10 %, so the two paths are alternated inside ONE
process: --repeats rounds of (workspace, workspace-free), each timing the
whole _C.attn_bwd (delta + dkv + dq + output allocation) with device
events; medians and the max-min spread of the workspace repeats are
reported. The peak-memory rise of one backward is recorded per path.
A shape whose workspace does not fit in free device memory is timed
workspace-free only, and the output says so.

--split additionally reports per-kernel device time from torch.profiler.

Run on GPU: python tools/bench_attention_bwd_ws.py [--split] [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import _C

SHAPES = [("7b-mha", (2, 4096, 32, 32, 128)),
          ("7b-gqa", (2, 4096, 32, 8, 128)),
          ("16k-mha", (1, 16384, 32, 32, 128))]
PATHS = ["workspace", "free"]
KERNELS = ["attn_bwd_delta_kernel", "attn_bwd_dkv_kernel",
           "attn_bwd_dq_kernel", "attn_bwd_dq_recompute_kernel"]
GIB = 1 << 30


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


def peak_rise(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(t for t, _ in SHAPES))
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    torch.manual_seed(0)
    entry = _C.attn_bwd_ws_limit()
    limit = {"workspace": 1 << 62, "free": 0}
    results = []
    for tag, (b, s, h, kvh, d) in SHAPES:
        if tag not in args.shapes.split(","):
            continue
        q = torch.randn(b, s, h, d, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(b, s, kvh, d, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(b, s, kvh, d, device="cuda", dtype=torch.bfloat16)
        do = torch.randn_like(q)
        o, lse = _C.attn_fwd(q, k, v)
        bwd = lambda: _C.attn_bwd(do, q, k, v, o, lse, None)
        ws_bytes = b * h * s * s * 2
        torch.cuda.empty_cache()
        free_bytes, _ = torch.cuda.mem_get_info()
        paths = PATHS if ws_bytes + GIB < free_bytes else ["free"]
        # useful flops, causal: dv, dk, dq + one S and one dP chain
        flops = 2.5 * 2 * 2 * b * h * s * s * d * 0.5
        samples = {p: {} for p in paths}
        peaks = {}
        for p in paths:
            _C.attn_bwd_ws_limit(limit[p])
            peaks[p] = peak_rise(bwd)
        for _ in range(args.repeats):
            for p in paths:
                _C.attn_bwd_ws_limit(limit[p])
                meas = {"bwd": event_ms(bwd, args.iters, args.warmup)}
                if args.split:
                    meas.update(kernel_ms(bwd, args.iters, args.warmup))
                for name, ms in meas.items():
                    samples[p].setdefault(name, []).append(ms)
        row = dict(shape=tag, b=b, s=s, h=h, kvh=kvh, d=d,
                   workspace_bytes=ws_bytes, paths=paths,
                   peak_rise_bytes=peaks, samples_ms=samples)
        med = {p: {n: statistics.median(x) for n, x in samples[p].items()}
               for p in paths}
        row["median_ms"] = med
        print(f"{tag} b{b} s{s} h{h} kvh{kvh} d{d}: workspace "
              f"{ws_bytes / GIB:.2f} GiB")
        if "workspace" not in paths:
            print("    workspace does not fit in free device memory: "
                  "workspace-free only")
        for p in paths:
            x = samples[p]["bwd"]
            print(f"    {p:9s} bwd {med[p]['bwd']:8.3f} ms "
                  f"{flops / med[p]['bwd'] / 1e9:6.1f} TF/s useful "
                  f"(spread {max(x) - min(x):.3f}) peak rise "
                  f"{peaks[p] / GIB:.3f} GiB  {[round(t, 3) for t in x]}")
            for n in KERNELS:
                if n in med[p]:
                    print(f"        {n:30s} {med[p][n]:8.3f} ms")
        if len(paths) == 2:
            row["free_over_workspace"] = med["free"]["bwd"] / med["workspace"]["bwd"]
            print(f"    workspace-free / workspace = "
                  f"x{row['free_over_workspace']:.3f}")
        results.append(row)
        del q, k, v, do, o, lse, bwd
    _C.attn_bwd_ws_limit(entry)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
