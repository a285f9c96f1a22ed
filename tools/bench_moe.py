"""Same-process A/B of MoEMLP.forward (models/mixtral.py) under
ops.moe_mode("loop") (the per-expert loop: torch.where, gather, two
hipBLASLt GEMMs, ops.swiglu, index_add_) and ops.moe_mode("fused") (the
kernel chain of ops/hip/moe.hip), no-grad bf16 at the mixtral_8x7b layer
shape: emb 4096, hidden 14336, 8 experts, top-2.

The routes alternate inside ONE process: --repeats rounds, each timing
--iters calls per route with device events (the loop's host syncs fall
inside the window); medians and max-min spreads are reported. Every call
takes the next of --sets layers (2.8 GB of expert weights each) and the next
input, so no operand of a call is left in the 256 MB last-level cache from
its last use. `relerr` is the largest difference of the two routes' outputs
over the largest output.

Run on GPU: python tools/bench_moe.py [--tokens 1 8 64] [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import ops
from fms_fsdp_amd.models.mixtral import MixtralConfig, MoEMLP


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+",
                    default=[1, 8, 64, 2048, 16384])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--emb", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=14336)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_moe.py needs a GPU"

    torch.manual_seed(0)
    cfg = MixtralConfig(emb_dim=args.emb, hidden_dim=args.hidden)
    layers = []
    for _ in range(args.sets):
        with torch.device("cuda"):
            m = MoEMLP(cfg).to(torch.bfloat16)
        m.reset_parameters()
        layers.append(m.requires_grad_(False))
    before = ops.moe_mode()
    results = []
    print(f"emb {args.emb} hidden {args.hidden} experts {cfg.num_experts} "
          f"top-{cfg.top_k}; ms per call, median of {args.repeats} rounds x "
          f"{args.iters} calls (spread = max - min)")
    try:
        for T in args.tokens:
            xs = [torch.randn(1, T, args.emb, device="cuda",
                              dtype=torch.bfloat16)
                  for _ in range(max(args.sets, 3))]
            turn = [0]

            def call(mode):
                i = turn[0]
                turn[0] += 1
                ops.moe_mode(mode)
                with torch.no_grad():
                    return layers[i % args.sets](xs[i % len(xs)])

            turn[0] = 0
            a = call("loop").float()
            turn[0] = 0
            b = call("fused").float()
            rel = ((a - b).abs().max() / a.abs().max()).item()
            samples = {"loop": [], "fused": []}
            for _ in range(args.repeats):
                for mode in samples:
                    samples[mode].append(event_ms(lambda: call(mode),
                                                  args.iters, args.warmup))
            med = {r: statistics.median(x) for r, x in samples.items()}
            line = f"  T{T:<6d}"
            for r, x in samples.items():
                results.append(dict(T=T, route=r, median_ms=med[r],
                                    spread_ms=max(x) - min(x), samples_ms=x,
                                    relerr=rel))
                line += f"  {r} {med[r]:9.4f} ({max(x) - min(x):.4f})"
            print(line + f"  fused/loop {med['fused'] / med['loop']:.3f}"
                  f"  relerr {rel:.2e}", flush=True)
    finally:
        ops.moe_mode(before)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
