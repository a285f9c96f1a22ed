"""Same-process A/B of the fused intra-chunk SSD kernel (ops.ssd_diag,
ops/hip/ssd_diag.hip) against the three-launch route it replaces
(FMS_AMD_SSD_DIAG=gemm: scores einsum, ssd_scores_decay, bmm), at the
mamba_2.8b head geometry: b = 2 rows of 4096, P 64, d_state 128, one group,
chunk 128, H in {80, 128}. C and B are last-dim slices of a conv-output
sized buffer, as the model passes them.

(a) `fwd`: the no-grad forward. (b) `ckpt`: the checkpointed training
pattern, forward without a graph, forward again with one, backward.

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
ROUTES = ("gemm", "fused")


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
        os.environ["FMS_AMD_SSD_DIAG"] = route
        Cm, Bm, dacs, xdt, dy = sets[turn[0] % nsets]
        turn[0] += 1
        dims = (H, G, P, N_STATE, Q)
        with torch.no_grad():
            ops.ssd_diag(Cm, Bm, dacs, xdt, *dims)
        if pattern == "ckpt":
            leaves = [t.detach().requires_grad_()
                      for t in (Cm, Bm, dacs, xdt)]
            torch.autograd.grad(ops.ssd_diag(*leaves, *dims), leaves, dy)

    return {pat: {r: (lambda r=r, pat=pat: call(r, pat)) for r in ROUTES}
            for pat in ("fwd", "ckpt")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--heads", type=int, nargs="+", default=[80, 128])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    torch.manual_seed(0)
    results = []
    print(f"b{B} l{L} P{P} G{G} n{N_STATE} Q{Q}; ms per call, median of "
          f"{args.repeats} rounds x {args.iters} calls (spread = max - min)")
    for H in args.heads:
        for pat, routes in cases(H, args.sets).items():
            samples = {r: [] for r in routes}
            for _ in range(args.repeats):
                for r, fn in routes.items():
                    samples[r].append(event_ms(fn, args.iters, args.warmup))
            base = statistics.median(samples["gemm"])
            line = f"  H{H:<4d}{pat:5s}"
            for r, x in samples.items():
                med, spread = statistics.median(x), max(x) - min(x)
                results.append(dict(H=H, pattern=pat, route=r, median_ms=med,
                                    spread_ms=spread, vs_gemm=med / base,
                                    samples_ms=x))
                line += f"  {r} {med:7.4f} ({spread:.4f})"
            print(line + f"  fused/gemm {results[-1]['vs_gemm']:.3f}")
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
