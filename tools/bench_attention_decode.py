"""Same-process A/B of one layer's KV-cache decode step: the former route
(FMS_AMD_DECODE=sdpa: split, rope, two torch.cat over the whole history,
torch SDPA) against the kernels (kv_append + attn_decode over the
preallocated cache), both through ops.attention_cached.

Every step starts from a history of kv_len - 1 keys and appends one, so it
attends to kv_len keys. The step runs over a ring of per-layer caches whose
K/V bytes together exceed the last-level cache (--ring-mb), as the layers
of a model do, so no layer finds its history cached. The routes alternate
in --repeats rounds after one discarded round; the figure is the median,
the spread max-min of the former route's repeats.

Next to each time: the KV bytes a step has to read (2 * b * kv_len * kvh *
d * 2) and the rate they amount to, to hold against the device's measured
copy rate (6.29 TB/s on MI355X).

--splits sweeps _C.attn_decode alone over forced split counts (the table
behind attn_decode_plan.h); --e2e times Llama.generate on both routes.

Run on GPU: python tools/bench_attention_decode.py [--splits] [--e2e]
            [--json OUT]"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import _C, ops

BF = torch.bfloat16
# (tag, b, h, kvh, d, kv_len)
STAGE2 = [(tag, 96, h, kvh, 128, n)
          for tag, h, kvh in (("llama2-7b", 32, 32), ("llama3-8b", 32, 8),
                              ("starcoder", 48, 1))
          for n in (64, 192, 320)]
LONG = ("long-row", 1, 32, 8, 128, 16384)
ROUTES = ["sdpa", "kernels"]


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


def kv_bytes(b, kvh, d, n):
    return 2 * b * n * kvh * d * 2


def ring_size(b, kvh, d, n, ring_mb):
    return max(2, min(512, -(-(ring_mb << 20) // kv_bytes(b, kvh, d, n))))


def tables(pos, d):
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.outer(torch.tensor([float(pos)]), inv)
    return fr.cos().cuda(), fr.sin().cuda()


class Ring:
    """`layers` caches holding kv_len - 1 random keys, usable by both
    routes: the kernels see the preallocated rows, the former route the
    same rows as its cat-grown tensors."""

    def __init__(self, layers, b, h, kvh, d, n):
        self.n = n
        self.caches = []
        for _ in range(layers):
            c = ops.KVCache(b, n, kvh, d, BF, "cuda")
            c.k.normal_()
            c.v.normal_()
            self.caches.append(c)
        self.hist = [(c.k[:, :n - 1].contiguous(), c.v[:, :n - 1].contiguous())
                     for c in self.caches] if n > 1 else None
        self.qkv = torch.randn(b, 1, (h + 2 * kvh) * d, device="cuda",
                               dtype=BF)
        q, k, v = self.qkv.split([h * d, kvh * d, kvh * d], dim=-1)
        self.q, self.k, self.v = (q.view(b, 1, h, d), k.view(b, 1, kvh, d),
                                  v.view(b, 1, kvh, d))
        self.cos, self.sin = tables(n - 1, d)

    def drop_hist(self):
        self.hist = None

    def step_all(self, route):
        os.environ["FMS_AMD_DECODE"] = "sdpa" if route == "sdpa" else ""
        for i, c in enumerate(self.caches):
            c.len = self.n - 1
            if route == "sdpa":
                hk, hv = self.hist[i]
                c._cat = {"k": hk, "v": hv}
            ops.attention_cached(self.q, self.k, self.v, c, self.cos,
                                 self.sin)
            c._cat = {}


def bench_step(shape, args):
    tag, b, h, kvh, d, n = shape
    layers = ring_size(b, kvh, d, n, args.ring_mb)
    ring = Ring(layers, b, h, kvh, d, n)
    samples = {r: [] for r in ROUTES}
    with torch.no_grad():
        for rnd in range(args.repeats + 1):
            for r in ROUTES:
                ms = event_ms(lambda: ring.step_all(r),
                              max(2, args.calls // layers),
                              args.warmup) / layers
                if rnd:
                    samples[r].append(ms)
    old, new = samples["sdpa"], samples["kernels"]
    mo, mn = statistics.median(old), statistics.median(new)
    nbytes = kv_bytes(b, kvh, d, n)
    row = dict(shape=tag, b=b, h=h, kvh=kvh, d=d, kv_len=n, layers=layers,
               kv_bytes=nbytes, sdpa_us=[x * 1e3 for x in old],
               kernels_us=[x * 1e3 for x in new], sdpa_median_us=mo * 1e3,
               kernels_median_us=mn * 1e3,
               sdpa_spread_us=(max(old) - min(old)) * 1e3,
               sdpa_tbs=nbytes / mo / 1e9, kernels_tbs=nbytes / mn / 1e9,
               splits=_C.attn_decode_plan(
                   b, kvh, n,
                   torch.cuda.get_device_properties(0).multi_processor_count))
    print(f"{tag:10s} b{b} h{h} kvh{kvh} n{n:5d} ring{layers:3d} "
          f"{nbytes / 1e6:8.1f} MB | sdpa {mo * 1e3:8.1f} us "
          f"{row['sdpa_tbs']:5.2f} TB/s (spread {row['sdpa_spread_us']:.1f}) "
          f"| kernels {mn * 1e3:8.1f} us {row['kernels_tbs']:5.2f} TB/s "
          f"splits {row['splits']} | x{mo / mn:.2f}")
    return row


def bench_splits(shape, counts, args):
    """_C.attn_decode alone at forced split counts over a ring of caches."""
    tag, b, h, kvh, d, n = shape
    layers = ring_size(b, kvh, d, n, args.ring_mb)
    ring = Ring(layers, b, h, kvh, d, n)
    ring.drop_hist()
    q = torch.randn(b, 1, h, d, device="cuda", dtype=BF)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    plan = _C.attn_decode_plan(b, kvh, n, n_cu)
    rows = []
    for s in sorted(set(counts) | {plan}):
        def run():
            for c in ring.caches:
                _C.attn_decode(q, c.k, c.v, n, s)
        ms = statistics.median(
            event_ms(run, max(2, args.calls // layers), args.warmup) / layers
            for _ in range(args.repeats))
        nbytes = kv_bytes(b, kvh, d, n)
        rows.append(dict(shape=tag, b=b, h=h, kvh=kvh, d=d, kv_len=n,
                         splits=s, planned=(s == plan), us=ms * 1e3,
                         tbs=nbytes / ms / 1e9))
        print(f"{tag:10s} b{b} h{h} kvh{kvh} n{n:5d} attn_decode splits "
              f"{s:4d}{'*' if s == plan else ' '} {ms * 1e3:8.1f} us "
              f"{nbytes / ms / 1e9:5.2f} TB/s")
    return rows


def bench_e2e(args):
    """Llama.generate tokens/s, llama2_1.4b at the stage-2 defaults."""
    from fms_fsdp_amd.config import get_model_config, train_config
    from fms_fsdp_amd.models import Llama
    cfg = train_config()
    b, s0, new = (cfg.stage2_batch_size, cfg.stage2_prompt_length,
                  cfg.stage2_seq_length)
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = Llama(get_model_config("llama2_1.4b"))
        m.reset_parameters()
    m = m.bfloat16().eval()
    x = torch.randint(0, m.config.src_vocab_size, (b, s0), device="cuda")
    out = {}
    for rnd in range(args.e2e_repeats + 1):
        for r in ROUTES:
            os.environ["FMS_AMD_DECODE"] = "sdpa" if r == "sdpa" else ""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(x, new, do_sample=False)
            torch.cuda.synchronize()
            if rnd:
                out.setdefault(r, []).append(b * new /
                                             (time.perf_counter() - t0))
    row = dict(what="generate", model="llama2_1.4b", b=b, prompt=s0, new=new,
               sdpa_tok_s=out["sdpa"], kernels_tok_s=out["kernels"])
    print(f"generate llama2_1.4b b{b} prompt{s0} new{new}: sdpa "
          f"{statistics.median(out['sdpa']):.0f} tok/s | kernels "
          f"{statistics.median(out['kernels']):.0f} tok/s "
          f"(runs: {[round(v) for v in out['sdpa']]} / "
          f"{[round(v) for v in out['kernels']]})")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=400,
                    help="timed steps per measurement, over the whole ring")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ring-mb", type=int, default=1024)
    ap.add_argument("--splits", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-repeats", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    entry = os.environ.get("FMS_AMD_DECODE")
    torch.manual_seed(0)
    results = [bench_step(s, args) for s in STAGE2 + [LONG]]
    if args.splits:
        results += bench_splits(LONG, [1, 2, 4, 8, 16, 32, 64, 128], args)
        results += bench_splits(("mid-rows", 8, 32, 8, 128, 4096),
                                [1, 2, 4, 8, 16], args)
        results += bench_splits(STAGE2[-1], [1, 2, 5, 10], args)
    if args.e2e:
        results.append(bench_e2e(args))
    if entry is None:
        os.environ.pop("FMS_AMD_DECODE", None)
    else:
        os.environ["FMS_AMD_DECODE"] = entry
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
