"""Same-process A/B of the dgrad routes of `_DirectWgradLinearFn`: the old
`dy @ W` (BLAS class NN: W strided along the reduction) against
`_C.dgrad_tn`, which transposes W with transpose.hip into a transient copy
and runs `dy @ WT^T`, the forward's class TN.

Method of tools/bench_wgrad.py: one process, the variants alternated, one
discarded round plus --repeats, medians, --iters calls per sample; the
spread is max-min of the NN repeats, and the new route counts as faster
only if its median gap to NN exceeds twice that spread. Every call takes
the next of --sets input sets, so no call finds its operands in the 256 MB
last-level cache.

Per projection of the Llama2-7B block and per --tokens value it reports
  nn          the old route (GEMM alone: it has nothing else)
  tn_gemm     the TN GEMM alone on a weight transposed beforehand
  tn_default  the same with TunableOp off (hipBLASLt's own choice)
  fwd_twin    the projection's forward GEMM x @ W^T, the TN shape with the
              same m*n*k, for comparison in the same loop
  tr_w        the weight transpose alone, with its read+write TB/s
  dgrad_tn    the whole native op: transpose + GEMM
At the end: four `_C.dgrad_tn` calls from the same inputs must give
bit-equal dx, and the share of dx elements that differ between the two
routes is printed, with the worst difference in bf16 roundings.

--tunableop FILE runs with TunableOp on and FILE as its table, a pattern
like results%d.csv with %d the device ordinal; --tune also tunes the keys
the table lacks and writes them back when the process ends, so start from
a copy of the committed table.

Run on GPU: python tools/bench_dgrad.py [--tokens 8192 ...] [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="*", default=[8192])
    ap.add_argument("--projs", nargs="*", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--tunableop", default=None)
    ap.add_argument("--tune", action="store_true")
    ap.add_argument("--tune-ms", type=int, default=10,
                    help="tuning time per candidate algorithm")
    ap.add_argument("--json", default=None)
    return ap.parse_args()


args = parse()
if args.tunableop:      # before torch reads the environment
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "1" if args.tune else "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = args.tunableop

import torch  # noqa: E402

from fms_fsdp_amd import _C  # noqa: E402

BF = torch.bfloat16
# (out, in) of the 7B block's four projections
PROJS = {"qkv": (12288, 4096), "proj": (4096, 4096), "wg1": (22016, 4096),
         "w2": (4096, 11008)}


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


def ab(variants, measure, repeats):
    """variants: ordered {label: fn}, the first is the old route.
    -> {label: (median, samples)}"""
    samples = {k: [] for k in variants}
    for rnd in range(repeats + 1):      # round 0 discarded
        for label, fn in variants.items():
            ms = measure(fn)
            if rnd:
                samples[label].append(ms)
    return {k: (statistics.median(s), s) for k, s in samples.items()}


def tunable_off(fn):
    def run():
        on = torch.cuda.tunable.is_enabled()
        torch.cuda.tunable.enable(False)
        try:
            fn()
        finally:
            torch.cuda.tunable.enable(on)
    return run


def bench_proj(name, tokens, out, inn, results):
    dev = "cuda"
    sets = []
    for _ in range(args.sets):
        dy = torch.randn(tokens, out, device=dev).to(BF)
        w = (torch.randn(out, inn, device=dev) * 0.02).to(BF)
        x = torch.randn(tokens, inn, device=dev).to(BF)
        sets.append((dy, w, w.t().contiguous(), x))
    turn = [0]

    def nxt():
        turn[0] += 1
        return sets[turn[0] % len(sets)]

    def nn():
        dy, w, _, _ = nxt()
        torch.mm(dy, w)

    def tn_gemm():
        dy, _, wT, _ = nxt()
        torch.mm(dy, wT.t())

    def fwd_twin():     # the forward GEMM of this projection: same m*n*k
        _, w, _, x = nxt()
        torch.mm(x, w.t())

    def tr_w():
        _C.transpose_bf16(nxt()[1])

    def whole():
        dy, w, _, _ = nxt()
        _C.dgrad_tn(dy, w)

    variants = {"nn": nn, "tn_gemm": tn_gemm,
                "tn_default": tunable_off(tn_gemm), "fwd_twin": fwd_twin,
                "tr_w": tr_w, "dgrad_tn": whole}
    for fn in variants.values():     # tunes the missing keys, if asked to
        fn()
    torch.cuda.synchronize()
    res = ab(variants, lambda f: event_ms(f, args.iters, args.warmup),
             args.repeats)

    nn_med, nn_s = res["nn"]
    spread = max(nn_s) - min(nn_s)
    tr_bytes = 2 * 2 * out * inn
    gap = nn_med - res["dgrad_tn"][0]
    print(f"--- {name} tokens {tokens} out {out} in {inn}: NN spread "
          f"{spread * 1e3:.1f} us; whole op gap {gap * 1e3:+.1f} us "
          f"({'route' if gap > 2 * spread else 'keep NN'})", flush=True)
    for label, (med, s) in res.items():
        row = dict(proj=name, tokens=tokens, out=out, inn=inn, variant=label,
                   median_ms=med, ms=s, spread_ms=max(s) - min(s))
        line = f"{name:5s} {tokens:5d} {label:11s} median {med * 1e3:8.1f} us" \
               f"  {[round(v * 1e3, 1) for v in s]}"
        if label == "tr_w":
            row["tb_per_s"] = tr_bytes / med / 1e9
            line += f"  {row['tb_per_s']:.2f} TB/s"
        elif label != "nn":
            row.update(gap_ms=nn_med - med, nn_spread_ms=spread,
                       faster=(nn_med - med) > 2 * spread)
            line += f"  gap {(nn_med - med) * 1e3:+8.1f} us -> " \
                    f"{'FASTER' if row['faster'] else 'not faster'}"
        results.append(row)
        print(line, flush=True)

    # determinism of the whole op: four calls, same inputs
    dy, w, _, _ = sets[0]
    outs = [_C.dgrad_tn(dy, w) for _ in range(4)]
    same = all(torch.equal(outs[0], o) for o in outs[1:])
    print(f"{name:5s} {tokens:5d} dgrad_tn x4 bit-equal: {same}", flush=True)
    results.append(dict(proj=name, tokens=tokens, variant="determinism",
                        bit_equal=same))

    # the two routes against each other: both round an fp32 sum to bf16,
    # in another summation order, so elements may differ by one rounding
    old = torch.mm(dy, w).float()
    diff = (outs[0].float() - old).abs()
    differ = (diff > 0).float().mean().item()
    # in units of one bf16 rounding (2^-8 relative) of the old element, or
    # of dx's rms where the element is a smaller, cancelled sum
    scale = torch.maximum(old.abs(), old.pow(2).mean().sqrt())
    worst = (diff / (scale * 2.0 ** -8)).max().item()
    print(f"{name:5s} {tokens:5d} dgrad_tn vs nn: {differ * 100:.4f} % of "
          f"elements differ, worst by {worst:.2f} bf16 roundings",
          flush=True)
    results.append(dict(proj=name, tokens=tokens, variant="agreement",
                        differ_share=differ, worst_roundings=worst))


def main():
    torch.manual_seed(0)
    if args.tunableop and args.tune:
        torch.cuda.tunable.set_max_tuning_duration(args.tune_ms)
    results = []
    for tokens in args.tokens:
        for name in (args.projs or PROJS):
            out, inn = PROJS[name]
            bench_proj(name, tokens, out, inn, results)
            if args.json:
                with open(args.json, "w") as f:
                    json.dump(results, f, indent=1)
    if args.tunableop:
        for row in torch.cuda.tunable.get_results():
            if row[1].startswith("tn_"):
                print("tunableop", ",".join(str(v) for v in row), flush=True)


if __name__ == "__main__":
    main()
