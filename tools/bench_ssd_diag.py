"""Same-process A/B of the fused intra-chunk SSD kernel (ops.ssd_diag,
ops/hip/ssd_diag.hip) against the three-launch route it replaces
(FMS_AMD_SSD_DIAG=gemm: scores einsum, ssd_scores_decay, bmm), at the
mamba_2.8b head geometry: b = 2 rows of 4096, P 64, d_state 128, one group,
chunk 128, H in {80, 128}. C and B are last-dim slices of a conv-output
sized buffer, as the model passes them.

(a) `fwd`: the no-grad forward. (b) `ckpt`: the checkpointed training
pattern, forward without a graph, forward again with one, backward. (c)
`bwd`: the backward alone (its forward runs outside the timed events). The
route `fused+bwd` is the fused forward with the fused backward of
ops/hip/ssd_diag_bwd.hip (ops.ssd_diag_backward("fused")); `fused` keeps the
three-launch route's backward. (d) --nhb: `_C.ssd_diag_bwd` alone over the
head blocks per group, 0 = the binding's plan.

The two routes alternate inside ONE process: --repeats rounds, each timing
--iters calls per route with device events; medians and max-min spreads are
reported. Every call takes the next of --sets operand sets, so the inputs
of a call (about 175 MB at H = 80) have left the 256 MB last-level cache
since their last use.

Run on GPU: python tools/bench_ssd_diag.py [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import ops

B, L, P, G, N_STATE, Q = 2, 4096, 64, 1, 128, 128
# route -> (FMS_AMD_SSD_DIAG, ops.ssd_diag_backward mode)
ROUTES = {"gemm": ("gemm", "gemm"), "fused": ("fused", "gemm"),
          "fused+bwd": ("fused", "fused")}
PATTERNS = {"fwd": ("gemm", "fused"), "ckpt": tuple(ROUTES),
            "bwd": ("fused", "fused+bwd")}


def event_ms(fn, iters, warmup):
    """ms per call; a call that returns its own (start, end) events is
    timed between them, every other call from its start to the next one's."""
    for _ in range(warmup):
        fn()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    own = [fn() for _ in range(iters)]
    end.record()
    torch.cuda.synchronize()
    if own[0] is not None:
        return sum(a.elapsed_time(b) for a, b in own) / iters
    return start.elapsed_time(end) / iters


def operand_set(H):
    rows, nrow = B * L, B * (L // Q) * H
    conv = torch.randn(rows, H * P + 2 * G * N_STATE, device="cuda",
                       dtype=torch.bfloat16)
    Bm = conv[:, H * P:H * P + G * N_STATE]
    Cm = conv[:, H * P + G * N_STATE:]
    dacs = -(torch.rand(nrow, Q, device="cuda") * 0.05).cumsum(-1)
    xdt = torch.randn(nrow, Q, P, device="cuda", dtype=torch.bfloat16)
    dy = torch.randn(nrow, Q, P, device="cuda", dtype=torch.bfloat16)
    return Cm, Bm, dacs, xdt, dy


def cases(H, nsets):
    sets = [operand_set(H) for _ in range(nsets)]
    turn = [0]

    def call(route, pattern):
        os.environ["FMS_AMD_SSD_DIAG"] = ROUTES[route][0]
        ops.ssd_diag_backward(ROUTES[route][1])
        Cm, Bm, dacs, xdt, dy = sets[turn[0] % nsets]
        turn[0] += 1
        dims = (H, G, P, N_STATE, Q)
        if pattern != "bwd":
            with torch.no_grad():
                ops.ssd_diag(Cm, Bm, dacs, xdt, *dims)
            if pattern == "fwd":
                return None
        leaves = [t.detach().requires_grad_() for t in (Cm, Bm, dacs, xdt)]
        y = ops.ssd_diag(*leaves, *dims)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        torch.autograd.grad(y, leaves, dy)
        ev[1].record()
        return ev if pattern == "bwd" else None

    return {pat: {r: (lambda r=r, pat=pat: call(r, pat)) for r in routes}
            for pat, routes in PATTERNS.items()}


def nhb_cases(H, nsets):
    """_C.ssd_diag_bwd alone, one callable per head-block count."""
    from fms_fsdp_amd import _C
    sets = [operand_set(H) for _ in range(nsets)]
    turn = [0]

    def call(nhb):
        Cm, Bm, dacs, xdt, dy = sets[turn[0] % nsets]
        turn[0] += 1
        _C.ssd_diag_bwd(dy, Cm, Bm, dacs, xdt, H, G, P, N_STATE, Q, nhb)

    counts = [n for n in (0, 1, 2, 4, 8, 16) if n <= H // G] + [H // G]
    return {n: (lambda n=n: call(n)) for n in counts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--heads", type=int, nargs="+", default=[80, 128])
    ap.add_argument("--nhb", action="store_true",
                    help="time the fused backward over head_blocks instead")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    prev_mode = ops.ssd_diag_backward()

    torch.manual_seed(0)
    results = []
    print(f"b{B} l{L} P{P} G{G} n{N_STATE} Q{Q}; ms per call, median of "
          f"{args.repeats} rounds x {args.iters} calls (spread = max - min)")
    if args.nhb:
        bench_nhb(args, results)
    else:
        bench_routes(args, results)
    ops.ssd_diag_backward(prev_mode)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


def bench_nhb(args, results):
    for H in args.heads:
        routes = nhb_cases(H, args.sets)
        samples = {n: [] for n in routes}
        for _ in range(args.repeats):
            for n, fn in routes.items():
                samples[n].append(event_ms(fn, args.iters, args.warmup))
        for n, x in samples.items():
            med, spread = statistics.median(x), max(x) - min(x)
            results.append(dict(H=H, pattern="nhb", head_blocks=n,
                                median_ms=med, spread_ms=spread, samples_ms=x))
            print(f"  H{H:<4d}nhb {n:<4d} {med:7.4f} ({spread:.4f})")
        torch.cuda.empty_cache()


def bench_routes(args, results):
    """vs_gemm is against a pattern's first route: the three-launch route,
    or in `bwd` its backward."""
    for H in args.heads:
        for pat, routes in cases(H, args.sets).items():
            samples = {r: [] for r in routes}
            for _ in range(args.repeats):
                for r, fn in routes.items():
                    samples[r].append(event_ms(fn, args.iters, args.warmup))
            base = statistics.median(samples[PATTERNS[pat][0]])
            line = f"  H{H:<4d}{pat:5s}"
            for r, x in samples.items():
                med, spread = statistics.median(x), max(x) - min(x)
                results.append(dict(H=H, pattern=pat, route=r, median_ms=med,
                                    spread_ms=spread, vs_gemm=med / base,
                                    samples_ms=x))
                line += f"  {r} {med:7.4f} ({spread:.4f})"
            print(line + f"  last/gemm {results[-1]['vs_gemm']:.3f}")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
