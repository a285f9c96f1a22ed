"""Same-process A/B of the MLP backward routes of `ops.swiglu_mlp`: the
composition (`swiglu_bwd`, then `_C.wgrad_tn` transposing dgu and the
saved h) against the fused route (`_C.swiglu_bwd_t` emitting dgu, dgu^T
and h^T in one pass, `_C.wgrad_tn_pre`).

Method of tools/bench_wgrad.py: one process, the variants alternated, one
discarded round plus --repeats, medians with max-min spread; a route
counts as faster only if its median gap exceeds twice the spread of the
old one. Every call takes the next of --sets operand sets, so nothing is
served from the 256 MB last-level cache.

Kernel level, rows x H = --tokens x --hidden:
  swiglu_bwd    the old kernel alone, with its TB/s (10 B per element of h)
  tr_dgu, tr_h  the two transposes it feeds, alone
  split         swiglu_bwd + tr_dgu + tr_h (22 B per element)
  fused         swiglu_bwd_t (16 B per element)
and the expected saving, 6 B per element over the measured rate of
swiglu_bwd, next to the measured one.

Op level: the backward of `ops.swiglu_mlp` (two dgrads, the swiglu
backward, two wgrads) under FMS_AMD_MLP_BWD=split and fused, device time
between events around `backward()` alone.

--tunableop FILE runs with TunableOp on and FILE as its table (a pattern
like tunableop_results%d.csv), tuning off.

Run on GPU: python tools/bench_mlp_bwd.py [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--emb", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=11008)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--tunableop", default=None)
    ap.add_argument("--json", default=None)
    return ap.parse_args()


args = parse()
if args.tunableop:      # before torch reads the environment
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = args.tunableop

import torch  # noqa: E402

from fms_fsdp_amd import _C, ops  # noqa: E402

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


def backward_ms(fn, iters, warmup):
    """fn() -> (y, dy); device time of y.backward(dy) alone."""
    for _ in range(warmup):
        y, dy = fn()
        y.backward(dy)
    pairs = []
    for _ in range(iters):
        y, dy = fn()
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        y.backward(dy)
        end.record()
        pairs.append((start, end))
    torch.cuda.synchronize()
    return sum(s.elapsed_time(e) for s, e in pairs) / iters


def ab(variants, measure, repeats):
    """variants: ordered {label: fn} -> {label: (median, samples)}"""
    samples = {k: [] for k in variants}
    for rnd in range(repeats + 1):      # round 0 discarded
        for label, fn in variants.items():
            ms = measure(fn)
            if rnd:
                samples[label].append(ms)
    return {k: (statistics.median(s), s) for k, s in samples.items()}


def report(res, results, level, nbytes=None):
    for label, (med, s) in res.items():
        row = dict(level=level, variant=label, median_ms=med, ms=s,
                   spread_ms=max(s) - min(s))
        line = f"{level:6s} {label:11s} median {med * 1e3:8.1f} us  spread " \
               f"{row['spread_ms'] * 1e3:6.1f}  " \
               f"{[round(v * 1e3, 1) for v in s]}"
        if nbytes and label in nbytes:
            row["tb_per_s"] = nbytes[label] / med / 1e9
            line += f"  {row['tb_per_s']:.2f} TB/s"
        results.append(row)
        print(line, flush=True)


def kernel_level(results):
    rows, H = args.tokens, args.hidden
    sets = []
    for _ in range(args.sets):
        gu = torch.randn(rows, 2 * H, device="cuda").to(BF)
        dh = torch.randn(rows, H, device="cuda").to(BF)
        sets.append((dh, gu, _C.swiglu_bwd(dh, gu), _C.swiglu_fwd(gu)))
    turn = [0]

    def nxt():
        turn[0] += 1
        return sets[turn[0] % len(sets)]

    def swiglu_bwd():
        dh, gu, _, _ = nxt()
        _C.swiglu_bwd(dh, gu)

    def tr_dgu():
        _C.transpose_bf16(nxt()[2])

    def tr_h():
        _C.transpose_bf16(nxt()[3])

    def split():
        dh, gu, _, h = nxt()
        _C.transpose_bf16(_C.swiglu_bwd(dh, gu))
        _C.transpose_bf16(h)

    def fused():
        dh, gu, _, _ = nxt()
        _C.swiglu_bwd_t(dh, gu)

    variants = {"swiglu_bwd": swiglu_bwd, "tr_dgu": tr_dgu, "tr_h": tr_h,
                "split": split, "fused": fused}
    res = ab(variants, lambda f: event_ms(f, args.iters, args.warmup),
             args.repeats)
    n = rows * H
    report(res, results, "kernel",
           {"swiglu_bwd": 10 * n, "tr_dgu": 8 * n, "tr_h": 4 * n,
            "split": 22 * n, "fused": 16 * n})
    rate = 10 * n / res["swiglu_bwd"][0]            # bytes per ms
    expected = 6 * n / rate
    measured = res["split"][0] - res["fused"][0]
    spread = max(res["split"][1]) - min(res["split"][1])
    print(f"kernel saving per layer: expected {expected * 1e3:.1f} us (6 B "
          f"per element at swiglu_bwd's rate), measured "
          f"{measured * 1e3:.1f} us, split spread {spread * 1e3:.1f} us -> "
          f"{'FASTER' if measured > 2 * spread else 'not faster'}",
          flush=True)
    results.append(dict(level="kernel", variant="saving",
                        expected_ms=expected, measured_ms=measured,
                        split_spread_ms=spread,
                        faster=measured > 2 * spread))
    dh, gu, dgu, h = sets[0]
    got = _C.swiglu_bwd_t(dh, gu)
    same = (torch.equal(got[0], dgu)
            and torch.equal(got[1], _C.transpose_bf16(dgu))
            and torch.equal(got[2], _C.transpose_bf16(h)))
    print(f"swiglu_bwd_t equals swiglu_bwd/swiglu_fwd + transposes: {same}",
          flush=True)
    results.append(dict(level="kernel", variant="bit_equal", value=same))


def op_level(results):
    tokens, emb, H = args.tokens, args.emb, args.hidden
    dev = "cuda"
    ws = []
    for shape in ((2 * H, emb), (emb, H)):
        w = (torch.randn(shape, device=dev) * 0.02).to(BF).requires_grad_()
        w._flat_grad_view = torch.zeros(shape, device=dev, dtype=BF)
        w._wgrad_fresh = True
        ws.append(w)
    sets = [(torch.randn(2, tokens // 2, emb, device=dev).to(BF)
             .requires_grad_(),
             torch.randn(2, tokens // 2, emb, device=dev).to(BF)
             .requires_grad_(),
             torch.randn(2, tokens // 2, emb, device=dev).to(BF))
            for _ in range(args.sets)]
    turn = [0]

    def route(name):
        def fn():
            turn[0] += 1
            x, res, dy = sets[turn[0] % len(sets)]
            x.grad = res.grad = None
            if name == "split":
                os.environ["FMS_AMD_MLP_BWD"] = "split"
            else:
                os.environ.pop("FMS_AMD_MLP_BWD", None)
            return ops.swiglu_mlp(x, ws[0], ws[1], res), dy
        return fn

    res = ab({"split": route("split"), "fused": route("fused")},
             lambda f: backward_ms(f, args.iters, args.warmup), args.repeats)
    report(res, results, "op")
    gap = res["split"][0] - res["fused"][0]
    spread = max(res["split"][1]) - min(res["split"][1])
    print(f"MLP backward per layer: fused saves {gap * 1e3:.1f} us, split "
          f"spread {spread * 1e3:.1f} us -> "
          f"{'FASTER' if gap > 2 * spread else 'not faster'}", flush=True)
    results.append(dict(level="op", variant="saving", measured_ms=gap,
                        split_spread_ms=spread, faster=gap > 2 * spread))
    # both routes from one input onto poisoned, fresh grad views
    out = {}
    for name in ("split", "fused"):
        for w in ws:
            w._flat_grad_view.fill_(float("nan"))
            w._wgrad_fresh = True
        y, dy = route(name)()
        y.backward(dy)
        x, r, _ = sets[turn[0] % len(sets)]
        out[name] = [y.detach(), x.grad, r.grad] + \
            [w._flat_grad_view.clone() for w in ws]
        turn[0] -= 1
    same = all(torch.equal(a, b) for a, b in zip(out["split"], out["fused"]))
    print(f"fused y, dx, dres and both wgrads bit-equal to split: {same}",
          flush=True)
    results.append(dict(level="op", variant="bit_equal", value=same))


def main():
    torch.manual_seed(0)
    results = []
    for level in (kernel_level, op_level):
        level(results)
        torch.cuda.empty_cache()
        if args.json:
            with open(args.json, "w") as f:
                json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
