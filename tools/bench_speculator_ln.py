"""Same-process A/B of the MLPSpeculator's head step, torch chain against the
kernels of ops/hip/layernorm.hip.

Part 1, the op alone at (T, H): `torch` is the chain of MLPSpeculator.forward
    z = emb(tok); v = h * sw + z * ew; y = gelu(LayerNormParameterized(v))
and `fused` is ops.layernorm_act on the same tensors, timed forward and
forward + backward (grads of h, emb, ln.weight and ln.bias). GB/s is the
kernels' minimum traffic over the time: 6 B per element forward (x and the
embedding row in, y out), 16 B per element for forward + backward (the
backward reads dy, x and the embedding row and writes dx and dz: 10 B).
Part 2, one stage-1 step of an MLPSpeculator (forward, the per-head cross
entropies, backward) under both ops.speculator_mode values.

The routes alternate inside ONE process: --repeats rounds, each timing
--iters calls per route with device events; medians and max-min spreads are
reported. Every call takes the next of --sets input sets, so x (64 MB at
8192 x 4096) is not left in the 256 MB last-level cache from its last use.

Run on GPU: python tools/bench_speculator_ln.py [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch
import torch.nn.functional as F

from fms_fsdp_amd import ops
from fms_fsdp_amd.models.speculator import (LayerNormParameterized,
                                            MLPSpeculator)

BF = torch.bfloat16


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


def ab(routes, args):
    """{route: (median ms, spread ms)} of callables timed alternately."""
    samples = {r: [] for r in routes}
    for _ in range(args.repeats):
        for r, fn in routes.items():
            samples[r].append(event_ms(fn, args.iters, args.warmup))
    return {r: (statistics.median(x), max(x) - min(x))
            for r, x in samples.items()}


def bench_op(T, H, V, args, results):
    sw = 0.5 ** (0.5 / 3)
    ew = (1 - sw ** 2) ** 0.5
    with torch.device("cuda"):
        emb = torch.nn.Embedding(V, H).to(BF)
        ln = LayerNormParameterized(H).to(BF)
    act = torch.nn.GELU()
    hs = [torch.randn(T, H, device="cuda", dtype=BF).requires_grad_()
          for _ in range(args.sets)]
    toks = [torch.randint(0, V, (T,), device="cuda")
            for _ in range(args.sets)]
    dy = torch.randn(T, H, device="cuda", dtype=BF)
    params = [emb.weight, ln.weight, ln.bias]
    turn = [0]

    def torch_chain(h, tok):
        return act(ln(h * sw + emb(tok) * ew))

    def fused(h, tok):
        return ops.layernorm_act(h, ln.weight, ln.bias, ln.eps,
                                 emb=emb.weight, tok=tok, sx=sw, se=ew,
                                 gelu=True)

    def call(fn, backward):
        i = turn[0] % args.sets
        turn[0] += 1
        if not backward:
            with torch.no_grad():
                return fn(hs[i], toks[i])
        y = fn(hs[i], toks[i])
        torch.autograd.grad(y, [hs[i], *params], dy)
        return y

    assert ops.layernorm_act_has_kernel(hs[0], ln.weight, ln.bias,
                                        emb.weight, toks[0])
    a = call(torch_chain, False).float()
    turn[0] = 0
    b = call(fused, False).float()
    rel = ((a - b).abs().max() / a.abs().max()).item()
    for backward, bytes_per_el in ((False, 6), (True, 16)):
        med = ab({"torch": lambda: call(torch_chain, backward),
                  "fused": lambda: call(fused, backward)}, args)
        what = "fwd+bwd" if backward else "fwd"
        gbs = T * H * bytes_per_el / med["fused"][0] / 1e6
        print(f"  ({T}, {H}) {what:8s}"
              f" torch {med['torch'][0]:8.4f} ({med['torch'][1]:.4f})"
              f"  fused {med['fused'][0]:8.4f} ({med['fused'][1]:.4f})"
              f"  fused/torch {med['fused'][0] / med['torch'][0]:.3f}"
              f"  fused {gbs:7.1f} GB/s  relerr {rel:.2e}", flush=True)
        results.append(dict(T=T, H=H, what=what, relerr=rel, fused_gbs=gbs,
                            **{f"{r}_ms": m[0] for r, m in med.items()},
                            **{f"{r}_spread_ms": m[1]
                               for r, m in med.items()}))


def bench_step(args, results):
    b, s, n = args.batch, args.seq, args.n_predict
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = MLPSpeculator(args.emb, args.inner, args.vocab, n)
    m.reset_parameters()
    m = m.to(BF)
    states = [torch.randn(b, s, args.emb, device="cuda", dtype=BF)
              for _ in range(args.sets)]
    inp = torch.randint(0, args.vocab, (b, s + n + 1), device="cuda")
    turn = [0]

    def step(mode):
        ops.speculator_mode(mode)
        i = turn[0] % args.sets
        turn[0] += 1
        m.zero_grad(set_to_none=True)
        preds = m(states[i], inp[:, 1:s + n])
        loss = sum(F.cross_entropy(preds[k].reshape(-1, preds.size(3)),
                                   inp[:, k + 2: s + k + 2].reshape(-1))
                   for k in range(n))
        loss.backward()
        return loss

    before = ops.speculator_mode()
    try:
        la, lb = step("torch").item(), step("fused").item()
        med = ab({"torch": lambda: step("torch"),
                  "fused": lambda: step("fused")}, args)
    finally:
        ops.speculator_mode(before)
    print(f"  stage-1 step b{b} s{s} emb{args.emb} inner{args.inner} "
          f"vocab{args.vocab} n{n}:"
          f" torch {med['torch'][0]:8.3f} ({med['torch'][1]:.3f})"
          f"  fused {med['fused'][0]:8.3f} ({med['fused'][1]:.3f})"
          f"  fused/torch {med['fused'][0] / med['torch'][0]:.3f}"
          f"  loss {la:.4f} / {lb:.4f}", flush=True)
    results.append(dict(what="stage1_step", loss_torch=la, loss_fused=lb,
                        **{f"{r}_ms": v[0] for r, v in med.items()},
                        **{f"{r}_spread_ms": v[1] for r, v in med.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+",
                    default=[8192, 4096, 8192, 2048], help="T H pairs")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--emb", type=int, default=4096)
    ap.add_argument("--inner", type=int, default=4096)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--n-predict", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_speculator_ln.py needs a GPU"
    torch.manual_seed(0)
    results = []
    print(f"ms per call, median of {args.repeats} rounds x {args.iters} "
          f"calls (spread = max - min)")
    for T, H in zip(args.shapes[::2], args.shapes[1::2]):
        bench_op(T, H, args.vocab, args, results)
    bench_step(args, results)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
