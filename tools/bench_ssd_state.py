"""Same-process A/B of the inter-chunk state kernels (ops/hip/ssd_state.hip)
at the mamba_2.8b / mamba_9.8b head geometry: b = 2 rows of 4096, P 64,
d_state 128, one group, chunk 128, H in {80, 128}.

(1) `chain`: the gemm chain of Mamba2Mixer._scan_fused (states einsum, the
(nc x nc) decay matrix, prev einsum) against ops.ssd_chunk_state +
ops.ssd_state_pass; `fwd` is the no-grad forward, `fwd+bwd` the forward
with a graph and its backward. B is a last-dim slice of a conv-output sized
buffer, as the model passes it.
(2) `cont`: a 4096-token continuation of a Mamba2Mixer over a cache in use,
every token through ops.ssd_state_update (FMS_AMD_MAMBA_PREFILL=step)
against the chunked scan from the cached state.
(3) `cs_bwd`: the backward of ops.ssd_chunk_state alone (its graph is built
outside the timed region), under ops.ssd_chunk_state_backward("gemm") (the
two einsums) and ("fused") (ops/hip/ssd_state_bwd.hip with the sum of its
head-block partials and the cast).
(4) `yoff`: ops.ssd_yoff under ops.ssd_yoff_mode("gemm") (the einsum of
Mamba2Mixer._scan_fused on hipBLASLt) and ("fused") (ops/hip/ssd_yoff.hip);
`fwd` is the no-grad forward, `fwd+bwd` the forward with a graph and its
backward (for "fused" with the sum of the dC partials and the cast). C is a
last-dim slice of a conv-output sized buffer.

The routes alternate inside ONE process: --repeats rounds, each timing
--iters calls per route with device events; medians and max-min spreads are
reported. Every call takes the next of --sets operand sets, so the inputs
of a call have left the 256 MB last-level cache since their last use.

Run on GPU: python tools/bench_ssd_state.py [--cases chain cs_bwd cont yoff]
[--json OUT]"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from fms_fsdp_amd import ops
from fms_fsdp_amd.models.mamba import Mamba2Mixer, MambaConfig, segsum

B, L, P, G, N_STATE, Q = 2, 4096, 64, 1, 128, 128
NC = L // Q


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


def chain_gemm(Bm, xdtd, dacs, H):
    rep = H // G
    states = torch.einsum(
        "bckgn,bcgrkp->bcgrnp", Bm.reshape(B, NC, Q, G, N_STATE),
        xdtd.view(B, NC, G, rep, Q, P)).reshape(B, NC, H, N_STATE, P)
    W = torch.exp(segsum(dacs.view(B, NC, H, Q)[..., -1].permute(0, 2, 1)))
    Wsh = torch.cat([torch.zeros_like(W[:, :, :1]), W[:, :, :-1]],
                    dim=2).to(torch.bfloat16)
    return torch.einsum("bhzc,bchnp->bzhnp", Wsh, states)


def chain_fused(Bm, xdtd, dacs, H):
    states = ops.ssd_chunk_state(Bm, xdtd, H, G, P, N_STATE, Q)
    return ops.ssd_state_pass(states, dacs, B, H, P, N_STATE, Q)


def operand_sets(H, nsets):
    def operand_set():
        conv = torch.randn(B * L, H * P + 2 * G * N_STATE, device="cuda",
                           dtype=torch.bfloat16)
        nrow = B * NC * H
        return (conv[:, H * P:H * P + G * N_STATE],
                torch.randn(nrow, Q, P, device="cuda", dtype=torch.bfloat16),
                -(torch.rand(nrow, Q, device="cuda") * 0.05).cumsum(-1),
                torch.randn(B, NC, H, N_STATE, P, device="cuda",
                            dtype=torch.bfloat16))
    return [operand_set() for _ in range(nsets)]


def chain_cases(H, nsets):
    sets = operand_sets(H, nsets)
    turn = [0]

    def call(fn, grad):
        Bm, xdtd, dacs, dprev = sets[turn[0] % nsets]
        turn[0] += 1
        if not grad:
            with torch.no_grad():
                fn(Bm, xdtd, dacs, H)
            return
        leaves = [t.detach().requires_grad_() for t in (Bm, xdtd, dacs)]
        prev = fn(*leaves, H)
        torch.autograd.grad(prev, leaves, dprev.view_as(prev))

    return {pat: {r: (lambda fn=fn, grad=grad: call(fn, grad))
                  for r, fn in (("gemm", chain_gemm), ("fused", chain_fused))}
            for pat, grad in (("fwd", False), ("fwd+bwd", True))}


def cs_bwd_cases(H, nsets):
    sets = []
    for Bm, xdtd, _, dS in operand_sets(H, nsets):
        leaves = [Bm.detach().requires_grad_(), xdtd.requires_grad_()]
        S = ops.ssd_chunk_state(*leaves, H, G, P, N_STATE, Q)
        sets.append((S, leaves, dS.view_as(S)))
    turn = [0]

    def call(mode):
        S, leaves, dS = sets[turn[0] % nsets]
        turn[0] += 1
        prev = ops.ssd_chunk_state_backward(mode)
        torch.autograd.grad(S, leaves, dS, retain_graph=True)
        ops.ssd_chunk_state_backward(prev)

    return {"cs_bwd": {r: (lambda r=r: call(r)) for r in ("gemm", "fused")}}


def cont_cases(H, nsets):
    torch.manual_seed(0)
    cfg = MambaConfig(d_model=H * P // 2, n_layer=1, vocab_size=512,
                      d_state=N_STATE, headdim=P, ngroups=G, chunk_size=Q)
    mixer = Mamba2Mixer(cfg, 0)
    mixer.reset_parameters()
    mixer = mixer.to("cuda").bfloat16().eval()
    cache = ops.MambaCache(B, mixer.conv_dim, mixer.d_conv, H, P, N_STATE,
                           torch.bfloat16, "cuda")
    sets = [torch.randn(B, L, cfg.d_model, device="cuda",
                        dtype=torch.bfloat16) * 0.5 for _ in range(nsets)]
    with torch.no_grad():
        mixer(sets[0][:, :Q + 3], cache=cache)       # the cache is in use
    turn = [0]

    def call(route):
        os.environ["FMS_AMD_MAMBA_PREFILL"] = route
        u = sets[turn[0] % nsets]
        turn[0] += 1
        with torch.no_grad():
            mixer(u, cache=cache)

    return {"cont": {r: (lambda r=r: call(r)) for r in ("step", "chunked")}}


def yoff_cases(H, nsets):
    sets = []
    for Cm, dy, _, prev in operand_sets(H, nsets):
        # dyoff has the element count of an h-major activation
        sets.append((Cm, prev.view(B * NC * H, N_STATE, P), dy))
    turn = [0]

    def call(mode, grad):
        Cm, prev, dy = sets[turn[0] % nsets]
        turn[0] += 1
        old = ops.ssd_yoff_mode(mode)
        try:
            if grad:
                leaves = [Cm.detach().requires_grad_(),
                          prev.detach().requires_grad_()]
                y = ops.ssd_yoff(*leaves, H, G, P, N_STATE, Q, b=B)
                torch.autograd.grad(y, leaves, dy.view_as(y))
            else:
                with torch.no_grad():
                    ops.ssd_yoff(Cm, prev, H, G, P, N_STATE, Q, b=B)
        finally:
            ops.ssd_yoff_mode(old)

    return {"yoff " + pat: {r: (lambda r=r, grad=grad: call(r, grad))
                            for r in ("gemm", "fused")}
            for pat, grad in (("fwd", False), ("fwd+bwd", True))}


CASES = {"chain": chain_cases, "cs_bwd": cs_bwd_cases, "cont": cont_cases,
         "yoff": yoff_cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--heads", type=int, nargs="+", default=[80, 128])
    ap.add_argument("--cases", nargs="+", default=list(CASES),
                    choices=list(CASES))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    prefill = os.environ.get("FMS_AMD_MAMBA_PREFILL")
    results = []
    print(f"b{B} l{L} P{P} G{G} n{N_STATE} Q{Q}; ms per call, median of "
          f"{args.repeats} rounds x {args.iters} calls (spread = max - min)")
    for H in args.heads:
        for cases in (CASES[c] for c in args.cases):
            for pat, routes in cases(H, args.sets).items():
                samples = {r: [] for r in routes}
                for _ in range(args.repeats):
                    for r, fn in routes.items():
                        samples[r].append(event_ms(fn, args.iters,
                                                   args.warmup))
                line = f"  H{H:<4d}{pat:13s}"
                base = statistics.median(next(iter(samples.values())))
                for r, x in samples.items():
                    med, spread = statistics.median(x), max(x) - min(x)
                    results.append(dict(H=H, pattern=pat, route=r,
                                        median_ms=med, spread_ms=spread,
                                        vs_first=med / base, samples_ms=x))
                    line += f"  {r} {med:8.4f} ({spread:.4f})"
                print(line + f"  last/first {results[-1]['vs_first']:.3f}",
                      flush=True)
            torch.cuda.empty_cache()
    if prefill is None:
        os.environ.pop("FMS_AMD_MAMBA_PREFILL", None)
    else:
        os.environ["FMS_AMD_MAMBA_PREFILL"] = prefill
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
