"""Same-process timing of the document-masked SSD and conv kernels against
their unmasked siblings, per kernel and for one Mamba2Mixer forward +
backward, at the mamba_2.8b shape (d_model 2560, 80 heads of 64, one
group, d_state 128, chunk 128, conv width 4) with b = 2 rows of 4096.

Cases: `unmasked` (the kernels every run without doc_mask takes) and the
masked kernels with 1, 8 and 64 documents per row. Document k >= 1 starts
at k * (4096 / n) + 37, so every boundary falls inside a chunk and inside
a conv strip.

These kernels are memory-bound and the mask adds one 4-byte load per row
or strip element, so masked ~ unmasked is the expectation; the spread of
`unmasked` over the rounds is the noise to hold a difference against.
All cases are alternated inside ONE process: --repeats rounds over every
case, each timing --iters calls with device events; medians and max-min
spreads are reported.

Run on GPU: python tools/bench_ssd_docmask.py [--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import _C, ops
from fms_fsdp_amd.models.mamba import Mamba2Mixer, MambaConfig

B, L = 2, 4096
H, P, G, N_STATE, Q, W = 80, 64, 1, 128, 128, 4
DOCS = (1, 8, 64)


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


def doc_mask(n):
    start = torch.zeros(L, dtype=torch.int64)
    for k in range(1, n):
        s = k * (L // n) + 37
        start[s:] = s
    return ops.doc_mask_from_starts(start.expand(B, L).contiguous().cuda())


def kernel_cases(masks):
    """name -> {case -> callable}; case None is the unmasked kernel."""
    dev, bf = "cuda", torch.bfloat16
    rows, nrow = B * L, B * (L // Q) * H
    C = H * P + 2 * G * N_STATE
    r = lambda *s: torch.randn(*s, device=dev, dtype=bf)
    x, z, g1, g2 = r(rows, H * P), r(rows, H * P), r(rows, H * P), r(rows, H * P)
    yd, yo, dout = r(rows, H * P), r(rows, H * P), r(rows, H * P)
    dtf = torch.rand(nrow, Q, device=dev)
    dacs = -(torch.rand(nrow, Q, device=dev) * 0.05).cumsum(-1)
    scores = r(B * (L // Q) * G, Q, Q)
    gs = r(nrow, Q, Q)
    D = torch.randn(H, device=dev)
    xc, dyc = r(B, L, C), r(B, L, C)
    wc, bc = r(C, W) * 0.5, torch.randn(C, device=dev)

    def pick(plain, doc, tail=lambda m: (m.start, L)):
        out = {None: plain}
        for n, m in masks.items():
            out[n] = (lambda m=m: doc(*tail(m)))
        return out

    return {
        "ssd_xdt_fwd": pick(
            lambda: _C.ssd_xdt_fwd(x, dtf, dacs, H, P, Q),
            lambda *t: _C.ssd_xdt_fwd_doc(x, dtf, dacs, H, P, Q, *t)),
        "ssd_xdt_bwd": pick(
            lambda: _C.ssd_xdt_bwd(g1, g2, x, dtf, dacs, H, P, Q),
            lambda *t: _C.ssd_xdt_bwd_doc(g1, g2, x, dtf, dacs, H, P, Q, *t)),
        "ssd_sl_fwd": pick(
            lambda: _C.ssd_sl_fwd(dacs, scores, H, G),
            lambda *t: _C.ssd_sl_fwd_doc(dacs, scores, H, G, *t)),
        "ssd_sl_bwd": pick(
            lambda: _C.ssd_sl_bwd(gs, scores, dacs, H, G),
            lambda *t: _C.ssd_sl_bwd_doc(gs, scores, dacs, H, G, *t)),
        "ssd_ygate_fwd": pick(
            lambda: _C.ssd_ygate_fwd(yd, yo, dacs, x, D, z, H, G, P, Q),
            lambda *t: _C.ssd_ygate_fwd_doc(yd, yo, dacs, x, D, z, H, G, P,
                                            Q, *t)),
        "ssd_ygate_bwd": pick(
            lambda: _C.ssd_ygate_bwd(dout, yd, yo, dacs, x, D, z, H, G, P, Q),
            lambda *t: _C.ssd_ygate_bwd_doc(dout, yd, yo, dacs, x, D, z, H,
                                            G, P, Q, *t)),
        "cconv_fwd": pick(
            lambda: _C.cconv_fwd(xc, wc, bc),
            lambda *t: _C.cconv_fwd_doc(xc, wc, bc, *t),
            tail=lambda m: (m.start,)),
        "cconv_bwd": pick(
            lambda: _C.cconv_bwd(dyc, xc, wc, bc),
            lambda *t: _C.cconv_bwd_doc(dyc, xc, wc, bc, *t),
            tail=lambda m: (m.start, m.end)),
    }


def mixer_cases(masks):
    torch.manual_seed(0)
    cfg = MambaConfig(d_model=2560, n_layer=1, vocab_size=512,
                      d_state=N_STATE, headdim=P, expand=2, ngroups=G,
                      chunk_size=Q, d_conv=W)
    mixer = Mamba2Mixer(cfg, 0)
    mixer.reset_parameters()
    mixer = mixer.cuda().bfloat16()
    u = torch.randn(B, L, 2560, device="cuda", dtype=torch.bfloat16) * 0.5

    def step(m):
        for p in mixer.parameters():
            p.grad = None
        ui = u.clone().requires_grad_()
        mixer(ui, doc_mask=m).float().pow(2).mean().backward()

    out = {None: lambda: step(None)}
    for n, m in masks.items():
        out[n] = (lambda m=m: step(m))
    return {"Mamba2Mixer fwd+bwd": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    torch.manual_seed(0)
    masks = {n: doc_mask(n) for n in DOCS}
    results = []
    print(f"b{B} l{L} H{H} P{P} G{G} n{N_STATE} Q{Q} W{W}; ms, median of "
          f"{args.repeats} rounds x {args.iters} calls (spread = max - min)")
    for build in (kernel_cases, mixer_cases):
        for name, cases in build(masks).items():
            samples = {c: [] for c in cases}
            for _ in range(args.repeats):
                for c, fn in cases.items():
                    samples[c].append(event_ms(fn, args.iters, args.warmup))
            base = statistics.median(samples[None])
            line = f"  {name:20s}"
            for c, x in samples.items():
                med, spread = statistics.median(x), max(x) - min(x)
                label = "unmasked" if c is None else f"doc-{c}"
                results.append(dict(kernel=name, case=label, median_ms=med,
                                    spread_ms=spread, vs_unmasked=med / base,
                                    samples_ms=x))
                line += f"  {label} {med:7.4f} ({spread:.4f})"
                if c is not None:
                    line += f" x{med / base:.3f}"
            print(line)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
