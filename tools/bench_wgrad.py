"""Same-process A/B of the wgrad routes of `_DirectWgradLinearFn`: the
old `addmm(dy^T, x)` (BLAS class NT) against `_C.wgrad_tn`, which
transposes the operands with transpose.hip and runs the same product in
another class (mode 3 = TN, 1 = NN with only dy transposed, 2 = TT with
only x transposed).

Method of tools/bench_bwd_tail.py: one process, the variants alternated,
one discarded round plus --repeats, medians; the spread is max-min of the
NT repeats, and a route counts as faster only if its median gap to NT
exceeds twice that spread. Every call takes the next of --sets input
sets, so nothing is served from the 256 MB last-level cache.

Per projection of the Llama2-7B block and per --tokens value it reports
  nt            the old route (GEMM alone: it has nothing else)
  tn/nn/tt_gemm the GEMM of each class on operands transposed beforehand
  tn_default    the TN GEMM with TunableOp off (hipBLASLt's own choice)
  tr_dy, tr_x   each transpose alone, with its read+write TB/s
  wgrad_tn{3,1,2}  the whole native op: transposes + GEMM
and the gate figure NT - TN - (transpose bytes / 4.5 TB/s). At the end:
four `_C.wgrad_tn` calls from the same inputs must leave bit-equal grads.

--tunableop FILE runs with TunableOp on and FILE as its table, a pattern
like results%d.csv with %d the device ordinal; --tune also tunes the
keys the table lacks and writes them back when the process ends, so
start from a copy of the committed table.

Run on GPU: python tools/bench_wgrad.py [--tokens 8192 ...] [--json OUT]"""

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
    ap.add_argument("--one-operand-at", type=int, default=8192,
                    help="tokens value at which NN and TT are timed too")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--tunableop", default=None)
    ap.add_argument("--tune", action="store_true")
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
ASSUMED_TBS = 4.5


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
        x = torch.randn(tokens, inn, device=dev).to(BF)
        sets.append((dy, x, dy.t().contiguous(), x.t().contiguous()))
    g = torch.zeros(out, inn, device=dev, dtype=BF)
    turn = [0]

    def nxt():
        turn[0] += 1
        return sets[turn[0] % len(sets)]

    def nt():
        dy, x, _, _ = nxt()
        torch.addmm(g, dy.t(), x, beta=0, out=g)

    def tn_gemm():
        _, _, dyT, xT = nxt()
        torch.addmm(g, dyT, xT.t(), beta=0, out=g)

    def nn_gemm():
        _, x, dyT, _ = nxt()
        torch.addmm(g, dyT, x, beta=0, out=g)

    def tt_gemm():
        dy, _, _, xT = nxt()
        torch.addmm(g, dy.t(), xT.t(), beta=0, out=g)

    def tr_dy():
        _C.transpose_bf16(nxt()[0])

    def tr_x():
        _C.transpose_bf16(nxt()[1])

    def whole(mode):
        def fn():
            dy, x, _, _ = nxt()
            _C.wgrad_tn(dy, x, g, False, mode)
        return fn

    variants = {"nt": nt, "tn_gemm": tn_gemm,
                "tn_default": tunable_off(tn_gemm), "tr_dy": tr_dy,
                "tr_x": tr_x, "wgrad_tn3": whole(3)}
    if tokens == args.one_operand_at:
        variants.update(nn_gemm=nn_gemm, tt_gemm=tt_gemm,
                        wgrad_tn1=whole(1), wgrad_tn2=whole(2))
    for fn in variants.values():     # tunes the missing keys, if asked to
        fn()
    torch.cuda.synchronize()
    res = ab(variants, lambda f: event_ms(f, args.iters, args.warmup),
             args.repeats)

    nt_med, nt_s = res["nt"]
    spread = max(nt_s) - min(nt_s)
    tr_bytes = {"tr_dy": 2 * 2 * tokens * out, "tr_x": 2 * 2 * tokens * inn}
    assumed_tr = (tr_bytes["tr_dy"] + tr_bytes["tr_x"]) / (ASSUMED_TBS * 1e9)
    gate = nt_med - res["tn_gemm"][0] - assumed_tr
    print(f"--- {name} tokens {tokens} out {out} in {inn}: NT spread "
          f"{spread * 1e3:.1f} us; gate NT-TN-bytes/{ASSUMED_TBS}TB/s = "
          f"{gate * 1e3:+.1f} us ({'pass' if gate > 2 * spread else 'no'})",
          flush=True)
    for label, (med, s) in res.items():
        row = dict(proj=name, tokens=tokens, out=out, inn=inn, variant=label,
                   median_ms=med, ms=s, spread_ms=max(s) - min(s))
        line = f"{name:5s} {tokens:5d} {label:11s} median {med * 1e3:8.1f} us" \
               f"  {[round(v * 1e3, 1) for v in s]}"
        if label in tr_bytes:
            row["tb_per_s"] = tr_bytes[label] / med / 1e9
            line += f"  {row['tb_per_s']:.2f} TB/s"
        elif label != "nt":
            row.update(gap_ms=nt_med - med, nt_spread_ms=spread,
                       faster=(nt_med - med) > 2 * spread)
            line += f"  gap {(nt_med - med) * 1e3:+8.1f} us -> " \
                    f"{'FASTER' if row['faster'] else 'not faster'}"
        results.append(row)
        print(line, flush=True)
    results.append(dict(proj=name, tokens=tokens, variant="gate",
                        gate_ms=gate, nt_spread_ms=spread,
                        passes=gate > 2 * spread))

    # determinism of the whole op: four calls, same inputs
    dy, x, _, _ = sets[0]
    outs = []
    for _ in range(4):
        gi = torch.full((out, inn), float("nan"), device=dev, dtype=BF)
        _C.wgrad_tn(dy, x, gi, False, 3)
        outs.append(gi)
    same = all(torch.equal(outs[0], o) for o in outs[1:])
    print(f"{name:5s} {tokens:5d} wgrad_tn3 x4 bit-equal: {same}", flush=True)
    results.append(dict(proj=name, tokens=tokens, variant="determinism",
                        bit_equal=same))


def main():
    torch.manual_seed(0)
    results = []
    for tokens in args.tokens:
        for name in (args.projs or PROJS):
            out, inn = PROJS[name]
            bench_proj(name, tokens, out, inn, results)
            if args.json:
                with open(args.json, "w") as f:
                    json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
