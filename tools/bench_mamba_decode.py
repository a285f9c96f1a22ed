"""Mamba2 recurrent decode on the GPU: the SSD step kernel alone and the
whole model's decode step.

ssd_step: _C.ssd_step at the head geometry of mamba_2.8b (H=80) and
mamba_9.8b (H=128), P=64, N=128, G=1, T=1, for b in {1, 8, 64}. A decode
step of a model walks one state per layer, so the call runs over a ring
of states (and of input buffers, column slices as the model hands them
over) whose bytes together exceed the last-level cache (--ring-mb): no
call finds its state cached. Reported per call: the median of --repeats
measurements in us, and the state traffic it amounts to (the fp32 state
read once and written once: 2 * b*H*P*N*4 bytes) in TB/s, to hold
against the device's streaming rate (adamw.hip: 6.3 TB/s measured on
MI355X). There is no former route to compare against.

--model NAME (repeatable; default mamba_2.8b): whole-model decode, ms per
token at b in {1, 8, 64} after a 128-token prompt, teacher-forced with
random tokens so that no host sync sits inside the timed window.

Run on GPU: python tools/bench_mamba_decode.py [--model mamba_9.8b]
            [--no-model] [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import _C

BF = torch.bfloat16
P, N, G = 64, 128, 1
GEOMS = [("mamba_2.8b", 80), ("mamba_9.8b", 128)]
BATCHES = (1, 8, 64)


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


def state_bytes(b, H):
    return 2 * b * H * P * N * 4


class Layer:
    """One layer's state and one decode token's inputs, laid out as the
    model does: z | xBC | dt in one in_proj row, x | B | C in one conv
    row."""

    def __init__(self, b, H):
        d_inner, gn = H * P, G * N
        self.state = torch.randn(b, H, P, N, device="cuda")
        zxbcdt = torch.randn(b, 1, 2 * d_inner + 2 * gn + H, device="cuda",
                             dtype=BF)
        self.z = zxbcdt[..., :d_inner]
        self.dt = zxbcdt[..., 2 * d_inner + 2 * gn:]
        xbc = torch.randn(b, 1, d_inner + 2 * gn, device="cuda", dtype=BF)
        self.x, self.B, self.C = xbc.split([d_inner, gn, gn], dim=-1)


def bench_step(tag, H, b, args):
    layers = max(2, min(1024, -(-(args.ring_mb << 20) // (state_bytes(b, H)
                                                          // 2))))
    ring = [Layer(b, H) for _ in range(layers)]
    dt_bias = torch.rand(H, device="cuda") - 4.0    # dt ~ 1e-2, slow decay
    A_log = torch.log(torch.empty(H, device="cuda").uniform_(1, 16))
    D = torch.ones(H, device="cuda")

    def run():
        for l in ring:
            _C.ssd_step(l.state, l.x, l.dt, l.B, l.C, l.z, dt_bias, A_log, D,
                        H, G, P, N)

    iters = max(2, args.calls // layers)
    us = [event_ms(run, iters, args.warmup) / layers * 1e3
          for _ in range(args.repeats + 1)][1:]
    med = statistics.median(us)
    nbytes = state_bytes(b, H)
    row = dict(what="ssd_step", geometry=tag, b=b, H=H, P=P, N=N, T=1,
               ring=layers, state_bytes=nbytes, us=us, median_us=med,
               spread_us=max(us) - min(us), tbs=nbytes / med / 1e6)
    print(f"ssd_step {tag:10s} b{b:3d} H{H:3d} ring{layers:5d} "
          f"{nbytes / 1e6:7.1f} MB | {med:8.1f} us (spread "
          f"{row['spread_us']:.1f}) {row['tbs']:5.2f} TB/s")
    return row


def bench_model(name, args):
    from fms_fsdp_amd.config import get_model_config
    from fms_fsdp_amd.models.mamba import MambaConfig, MambaLMHeadModel
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = MambaLMHeadModel(MambaConfig.from_dict(get_model_config(name)))
        m.reset_parameters()
    m = m.bfloat16().eval()
    rows = []
    prompt, new = 128, args.tokens
    for b in BATCHES:
        toks = torch.randint(0, m.config.vocab_size, (b, prompt + 2 * new),
                             device="cuda")
        ms = []
        with torch.no_grad():
            for rnd in range(args.model_repeats + 1):
                caches = m.allocate_cache(b, prompt + 2 * new, BF, "cuda")
                m(toks[:, :prompt], caches=caches)
                pos = [prompt]

                def step():
                    m(toks[:, pos[0]:pos[0] + 1], caches=caches)
                    pos[0] += 1
                t = event_ms(step, new, 2)
                if rnd:
                    ms.append(t)
        med = statistics.median(ms)
        rows.append(dict(what="decode", model=name, b=b, prompt=prompt,
                         tokens=new, ms_per_token=ms, median_ms=med,
                         tok_s=b / med * 1e3))
        print(f"decode {name} b{b:3d} prompt{prompt}: {med:7.3f} ms/token "
              f"({b / med * 1e3:8.0f} tok/s; runs "
              f"{[round(v, 3) for v in ms]})")
    del m
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000,
                    help="timed calls per measurement, over the whole ring")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ring-mb", type=int, default=1024)
    ap.add_argument("--model", action="append", default=None)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--model-repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.manual_seed(0)
    results = [bench_step(tag, H, b, args) for tag, H in GEOMS
               for b in BATCHES]
    if not args.no_model:
        for name in args.model or ["mamba_2.8b"]:
            results += bench_model(name, args)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
