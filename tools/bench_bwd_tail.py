"""Same-process A/B of the backward's elementwise tail against an OLDER
build of the extension: --old-ext points at the _C shared object of the
commit to compare with (build that commit in a second checkout).

Machines differ by 5-10 %, so old and new are alternated inside ONE
process: --repeats rounds of (old, new) per part after one discarded
round; medians are reported, the spread is max-min of the old repeats,
and the new path counts as faster only if the median gap exceeds twice
that spread. Shapes are the 7B step's own (b2 s4096 h32 d128, 8192x4096).

Parts:
  norm      everything one RMSNorm backward costs per step. Old: the dx
            and dw kernels (with the fp32 zero-fill), the bf16 cast, the
            accumulate into the grad slice, the zero-fill of that slice
            and the residual-stream add dx + dres. New: one
            rmsnorm_bwd_into with dres as dextra.
  norm_k    the rmsnorm_bwd binding alone (kernels only), the new one at
            each --grids block count.
  attn      whole _C.attn_bwd (MHA, dv into the fused slice) plus the two
            rope_into calls of the fused qkv backward.
  delta     the delta kernel's own device time inside attn_bwd, from
            torch.profiler.
The norm parts rotate over --sets input sets so that no call finds its
inputs in the 256 MB last-level cache.

Run on GPU: python tools/bench_bwd_tail.py --old-ext OLD/_C*.so [--json OUT]"""

import argparse
import importlib.util
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import _C as NEW

BF = torch.bfloat16


def load_old(path):
    spec = importlib.util.spec_from_file_location("fms_fsdp_amd_old._C", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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


def kernel_ms(fn, iters, warmup, substr):
    """Mean device time per call of the kernels whose name has `substr`."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    tot = 0.0
    for ev in prof.key_averages():
        if substr in ev.key:
            t = getattr(ev, "device_time_total", None)
            tot += (ev.cuda_time_total if t is None else t) / 1e3 / iters
    return tot


def ab(name, variants, measure, repeats, results):
    """variants: ordered {label: fn}, the first is the old path."""
    samples = {k: [] for k in variants}
    for rnd in range(repeats + 1):      # round 0 discarded
        for label, fn in variants.items():
            ms = measure(fn)
            if rnd:
                samples[label].append(ms)
    labels = list(variants)
    old = samples[labels[0]]
    spread = max(old) - min(old)
    mo = statistics.median(old)
    for label in labels:
        s = samples[label]
        m = statistics.median(s)
        row = dict(part=name, variant=label, ms=s, median_ms=m,
                   spread_ms=max(s) - min(s))
        line = f"{name:8s} {label:10s} median {m * 1e3:9.1f} us  " \
               f"{[round(v * 1e3, 1) for v in s]}"
        if label != labels[0]:
            row.update(gap_ms=mo - m, old_spread_ms=spread,
                       faster=(mo - m) > 2 * spread)
            line += f"  gap {(mo - m) * 1e3:8.1f} us vs 2x old spread " \
                    f"{2 * spread * 1e3:.1f} us -> " \
                    f"{'FASTER' if row['faster'] else 'within 2x spread'}"
        results.append(row)
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old-ext", required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--grids", type=int, nargs="*", default=[512, 1024, 2048])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    OLD = load_old(args.old_ext)
    dev = "cuda"
    torch.manual_seed(0)
    results = []
    ev = lambda fn: event_ms(fn, args.iters, args.warmup)

    # ---------------- RMSNorm backward, 8192 x 4096 ----------------
    rows, H = 8192, 4096
    w = torch.randn(H, device=dev).to(BF)
    sets = []
    for _ in range(args.sets):
        x = torch.randn(rows, H, device=dev).to(BF)
        _, rinv = NEW.rmsnorm_fwd(x, w, 1e-6)
        sets.append((torch.randn(rows, H, device=dev).to(BF), x, rinv,
                     torch.randn(rows, H, device=dev).to(BF)))
    gslice = torch.zeros(H, device=dev, dtype=BF)
    turn = [0]

    def nxt():
        turn[0] += 1
        return sets[turn[0] % len(sets)]

    def norm_old():
        dy, x, rinv, dres = nxt()
        gslice.zero_()                       # zero_grad's share
        dx, dw = OLD.rmsnorm_bwd(dy, x, w, rinv, None)
        gslice.add_(dw.to(BF))               # cast + autograd accumulate
        return dx + dres                     # residual-stream grad add

    def norm_new():
        dy, x, rinv, dres = nxt()
        return NEW.rmsnorm_bwd_into(dy, x, w, rinv, dres, gslice, False)

    ab("norm", {"old": norm_old, "new": norm_new}, ev, args.repeats, results)

    def norm_k(ext, grid=None):
        def fn():
            dy, x, rinv, _ = nxt()
            return ext.rmsnorm_bwd(dy, x, w, rinv, None)

        def with_grid():
            prev = NEW.rmsnorm_bwd_grid(grid)
            try:
                return ev(fn)
            finally:
                NEW.rmsnorm_bwd_grid(prev)
        return with_grid if grid else (lambda: ev(fn))

    variants = {"old": norm_k(OLD)}
    for g in args.grids:
        variants[f"new_g{g}"] = norm_k(NEW, g)
    ab("norm_k", variants, lambda f: f(), args.repeats, results)
    del sets

    # ---------------- attention backward + inverse RoPE ----------------
    b, s, h, d = 2, 4096, 32, 128
    qkv = torch.randn(b, s, 3 * h * d, device=dev).to(BF)
    q = qkv[..., :h * d].view(b, s, h, d)
    k = qkv[..., h * d:2 * h * d].view(b, s, h, d)
    v = qkv[..., 2 * h * d:].view(b, s, h, d)
    pos = torch.arange(s, device=dev, dtype=torch.float32)
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, device=dev,
                                          dtype=torch.float32) / d))
    fr = torch.outer(pos, inv)
    cos, sin = fr.cos().contiguous(), fr.sin().contiguous()
    qr, kr = NEW.rope_fwd(q, k, cos, sin, False)
    o, lse = NEW.attn_fwd(qr, kr, v)
    do = torch.randn_like(o)
    dqkv = torch.empty_like(qkv)
    dq_sl = dqkv[..., :h * d].view(b, s, h, d)
    dk_sl = dqkv[..., h * d:2 * h * d].view(b, s, h, d)
    dv_sl = dqkv[..., 2 * h * d:].view(b, s, h, d)

    def attn(ext):
        def fn():
            dq, dk, _ = ext.attn_bwd(do, qr, kr, v, o, lse, dv_sl)
            ext.rope_into(dq, dq_sl, cos, sin, True)
            ext.rope_into(dk, dk_sl, cos, sin, True)
        return fn

    attn_iters = max(args.iters // 4, 3)
    ab("attn", {"old": attn(OLD), "new": attn(NEW)},
       lambda f: event_ms(f, attn_iters, 2), args.repeats, results)
    ab("delta", {"old": attn(OLD), "new": attn(NEW)},
       lambda f: kernel_ms(f, attn_iters, 2, "attn_bwd_delta"), args.repeats,
       results)

    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
