"""Same-process A/B of one layer's multi-query step over the KV cache: s new
positions on a history of kv_len - s keys (a speculator's proposals being
verified, or one chunk of a chunked prefill).

"kernel" is ops.attention_cached as it stands (kv_append +
attn_decode_mq_kernel). "reference" is the route the same call took before
the kernel existed, spelled out: ops.kv_cache_append, then
reference.attention_cached over the cache rows (fp32 cast of the history,
an (s, n) mask, torch SDPA).

The step runs over a ring of per-layer caches whose K/V bytes together
exceed the last-level cache (--ring-mb), as the layers of a model do. The
routes alternate in --repeats rounds after one discarded round; the figure
is the median, the spread max-min of a route's repeats.

Next to each time: the K/V bytes the kernel's column blocks sweep and the
rate they amount to, and `vs_decode`, those bytes over the K/V bytes of s
separate attn_decode calls for the same positions. Nothing is asserted.

Run on GPU: python tools/bench_attention_verify.py [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import _C, ops
from fms_fsdp_amd.ops import reference

BF = torch.bfloat16
HEADS = (("llama2-7b", 32, 32), ("llama3-8b", 32, 8))
# (tag, b, s, h, kvh, d, kv_len)
VERIFY = [(tag, b, s, h, kvh, 128, n)
          for tag, h, kvh in HEADS for s in (4, 8) for n in (2048, 4096)
          for b in (1, 8, 96)]
CHUNK = [("chunk-" + tag, 1, 512, h, kvh, 128, 4096) for tag, h, kvh in HEADS]
ROUTES = ["reference", "kernel"]


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


def kv_traffic(b, s, h, kvh, d, n):
    """(K/V bytes the multi-query kernel sweeps, K/V bytes of s separate
    attn_decode calls): rows swept per (batch row, kv head) * row bytes."""
    G = h // kvh
    mq_rows = 0
    for cb in range(-(-s * G // 32)):
        qi_max = min((cb * 32 + 31) // G, s - 1)
        mq_rows += min(n, ((n - s + qi_max) // 32 + 1) * 32)
    dec_rows = -(-G // 32) * sum(n - s + qi + 1 for qi in range(s))
    row_bytes = 2 * b * kvh * d * 2
    return mq_rows * row_bytes, dec_rows * row_bytes


class Ring:
    """`layers` caches of capacity kv_len holding kv_len - s random keys."""

    def __init__(self, layers, b, s, h, kvh, d, n):
        self.n, self.s = n, s
        self.caches = []
        for _ in range(layers):
            c = ops.KVCache(b, n, kvh, d, BF, "cuda")
            c.k.normal_()
            c.v.normal_()
            self.caches.append(c)
        qkv = torch.randn(b, s, (h + 2 * kvh) * d, device="cuda", dtype=BF)
        q, k, v = qkv.split([h * d, kvh * d, kvh * d], dim=-1)
        self.q, self.k, self.v = (q.view(b, s, h, d), k.view(b, s, kvh, d),
                                  v.view(b, s, kvh, d))
        inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2,
                                              dtype=torch.float32) / d))
        fr = torch.outer(torch.arange(n - s, n, dtype=torch.float32), inv)
        self.cos, self.sin = fr.cos().cuda(), fr.sin().cuda()

    def step_all(self, route):
        for c in self.caches:
            c.len = self.n - self.s
            if route == "kernel":
                ops.attention_cached(self.q, self.k, self.v, c, self.cos,
                                     self.sin)
            else:
                qr = ops.kv_cache_append(c, self.q, self.k, self.v, self.cos,
                                         self.sin)
                reference.attention_cached(qr, c.k[:, :c.len], c.v[:, :c.len])


def bench(shape, args):
    tag, b, s, h, kvh, d, n = shape
    mq_bytes, dec_bytes = kv_traffic(b, s, h, kvh, d, n)
    cache_bytes = 2 * b * n * kvh * d * 2
    layers = max(2, min(512, -(-(args.ring_mb << 20) // cache_bytes)))
    ring = Ring(layers, b, s, h, kvh, d, n)
    samples = {r: [] for r in ROUTES}
    with torch.no_grad():
        for rnd in range(args.repeats + 1):
            for r in ROUTES:
                ms = event_ms(lambda: ring.step_all(r),
                              max(2, args.calls // layers),
                              args.warmup) / layers
                if rnd:
                    samples[r].append(ms)
    ref, new = samples["reference"], samples["kernel"]
    mr, mn = statistics.median(ref), statistics.median(new)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ncb = -(-s * (h // kvh) // 32)
    splits = min(_C.attn_decode_plan(b, kvh * ncb, n, n_cu),
                 (n - s) // 32 + 1)
    row = dict(shape=tag, b=b, s=s, h=h, kvh=kvh, d=d, kv_len=n,
               layers=layers, kv_bytes=mq_bytes, vs_decode=mq_bytes / dec_bytes,
               reference_us=[x * 1e3 for x in ref],
               kernel_us=[x * 1e3 for x in new],
               reference_median_us=mr * 1e3, kernel_median_us=mn * 1e3,
               reference_spread_us=(max(ref) - min(ref)) * 1e3,
               kernel_spread_us=(max(new) - min(new)) * 1e3,
               kernel_tbs=mq_bytes / mn / 1e9, splits=splits)
    print(f"{tag:15s} b{b:2d} s{s:3d} h{h} kvh{kvh:2d} n{n:5d} ring{layers:3d} "
          f"{mq_bytes / 1e6:8.1f} MB vs_decode {row['vs_decode']:.3f} | "
          f"reference {mr * 1e3:9.1f} us (spread "
          f"{row['reference_spread_us']:.1f}) | kernel {mn * 1e3:8.1f} us "
          f"(spread {row['kernel_spread_us']:.1f}) {row['kernel_tbs']:5.2f} "
          f"TB/s splits {splits} | x{mr / mn:.2f}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40,
                    help="timed steps per measurement, over the whole ring")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ring-mb", type=int, default=1024)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    results = []
    for shape in VERIFY + CHUNK:
        results.append(bench(shape, args))
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
