"""Flagship training-step benchmark (driver contract — see repo brief).

Measures the BASELINE.json headline: Llama2-7B, HSDP, bf16, no activation
checkpointing, batch 2/GPU, seq 4096, synthetic data, random-init weights.
`value` is the WHOLE-JOB tokens/sec over all N GPUs; `vs_baseline` compares
the per-GPU rate to the reference's 4550 tok/s/GPU on 128x A100
(BASELINE.md). Weak scaling: per-GPU work fixed as N grows.

Usage:  python bench.py [--gpus N] [--steps K] [--warmup W] [--model llama2_7b]
                        [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints one JSON line;
--dump-outputs DIR also saves the last timed step's loss as DIR/loss.npy.
N>1 is launched by the driver via torch.distributed.run (one rank per GPU).
"""

import argparse
import json
import os
import time

import torch
import torch.distributed as dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", type=str, default="llama2_7b")
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--sharding", type=str, default="hsdp")
    ap.add_argument("--ac", type=str, default="0",
                    help="selective AC fraction (0 = off)")
    ap.add_argument("--hipgraph", action="store_true",
                    help="capture the whole training step in a hipGraph "
                         "(N=1; the step is 99.7%% GPU-busy eager, so this "
                         "trims only launch latency)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step returned to its caller (the training loss) "
                         "as DIR/loss.npy, float32")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements and checks beyond the "
                         "headline figure (none exist yet: a plain run "
                         "already does only setup, warmup and the timed "
                         "steps, so this changes nothing today)")
    args = ap.parse_args()

    from fms_fsdp_amd.config import get_model_config
    from fms_fsdp_amd.models import Llama, LlamaBlock
    from fms_fsdp_amd.parallel import ShardedModel, ShardedAdamW
    from fms_fsdp_amd.parallel.policies import apply_selective_ac
    from fms_fsdp_amd.utils.train import setup_environ_flags

    setup_environ_flags()
    # hipBLASLt algo table tuned on MI355X (committed in-tree); read-only
    tune_csv = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                            "tunableop_results0.csv")
    if os.path.exists(tune_csv) and "PYTORCH_TUNABLEOP_ENABLED" not in os.environ:
        os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
        os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
        os.environ["PYTORCH_TUNABLEOP_FILENAME"] = \
            tune_csv.replace("results0", "results%d")
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    use_cuda = torch.cuda.is_available()
    device = torch.device("cuda", local_rank) if use_cuda else torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(local_rank)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("nccl" if use_cuda else "gloo")

    torch.manual_seed(2023)
    mcfg = get_model_config(args.model)
    if args.model.startswith("mamba"):
        from fms_fsdp_amd.models.mamba import (MambaBlock, MambaConfig,
                                               MambaLMHeadModel)
        mc = MambaConfig.from_dict(mcfg)
        with torch.device(device):
            model = MambaLMHeadModel(mc)
            model.reset_parameters()
        block_cls = MambaBlock

        class _V:
            src_vocab_size = mc.vocab_size
        mcfg = _V()
    else:
        with torch.device(device):
            model = Llama(mcfg)
            model.reset_parameters()
        block_cls = LlamaBlock
    n_params = model.param_count()

    from fms_fsdp_amd.config import train_config
    from fms_fsdp_amd.parallel.policies import resolve_reshard_after_forward
    _rcfg = train_config()   # "auto" resolver, same path the entries use
    sm = ShardedModel(model, block_cls, sharding_strategy=args.sharding,
                      param_dtype=torch.bfloat16 if use_cuda else torch.float32,
                      reshard_after_forward=resolve_reshard_after_forward(
                          _rcfg, n_params),
                      prefetch_lookahead=1, device=device)
    if args.ac not in ("0", "0.0", 0):
        apply_selective_ac(sm, block_cls, args.ac)
    opt = ShardedAdamW(sm, lr=3e-4)

    bs, sl = args.batch_size, args.seq_len
    g = torch.Generator().manual_seed(1234 + rank)
    # distinct synthetic batch per step (no single-batch memorization:
    # the reported loss stays a meaningful ~log(V) even on 100-step
    # soak runs — 8 cycled batches were memorizable by mamba at 40 steps)
    nb = 64
    batches = [torch.randint(0, mcfg.src_vocab_size, (bs, sl + 1),
                             generator=g).to(device) for _ in range(nb)]
    it = [0]

    def eager_step(x, y):
        opt.zero_grad()
        loss = sm(x, labels=y)
        loss.backward()
        sm.clip_grad_norm_(1.0)
        opt.step()
        return loss

    if args.hipgraph and use_cuda and world == 1:
        # whole-step hipGraph capture: static input buffers, the eager
        # step replayed as one graph launch. AdamW's step-count/bias
        # correction become fixed at capture values — fine for a
        # steady-state throughput bench, NOT for real training (the
        # entries stay eager; the step is 99.7% GPU-busy eager anyway).
        sx = torch.zeros(bs, sl, dtype=torch.long, device=device)
        sy = torch.zeros(bs, sl, dtype=torch.long, device=device)
        sloss = torch.zeros((), device=device)
        for _ in range(2):   # warm up allocator state pre-capture
            inp = batches[it[0] % nb]; it[0] += 1
            eager_step(inp[:, :-1], inp[:, 1:].contiguous())
        graph = torch.cuda.CUDAGraph()
        inp = batches[it[0] % nb]; it[0] += 1
        sx.copy_(inp[:, :-1]); sy.copy_(inp[:, 1:])
        with torch.cuda.graph(graph):
            sloss.copy_(eager_step(sx, sy).detach())

        def step():
            inp = batches[it[0] % nb]
            it[0] += 1
            sx.copy_(inp[:, :-1], non_blocking=True)
            sy.copy_(inp[:, 1:], non_blocking=True)
            graph.replay()
            return sloss
    else:
        def step():
            inp = batches[it[0] % nb]
            it[0] += 1
            x, y = inp[:, :-1], inp[:, 1:].contiguous()
            return eager_step(x, y)

    for _ in range(args.warmup):
        step()

    if dist.is_initialized():
        dist.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.steps):
        loss = step()
    if use_cuda:
        torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
    elapsed = time.time() - t0

    # max over ranks
    et = torch.tensor([elapsed], device=device if use_cuda else "cpu")
    if dist.is_initialized():
        dist.all_reduce(et, op=dist.ReduceOp.MAX)
    elapsed = et.item()

    ms_per_step = elapsed / args.steps * 1000
    tokens_per_sec = world * bs * sl * args.steps / elapsed
    baseline_per_gpu = 4550.0  # 7B HSDP compile noAC bs2, A100
    vs_baseline = (tokens_per_sec / world) / baseline_per_gpu \
        if args.model == "llama2_7b" else None

    if args.dump_outputs and rank == 0:
        # inputs and init are seeded above, so two builds run with the same
        # arguments can be compared output for output
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "loss.npy"),
                loss.detach().float().cpu().numpy())

    if rank == 0:
        print(json.dumps({
            "metric": "tokens/sec (aggregate)",
            "value": round(tokens_per_sec, 1),
            "unit": "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(vs_baseline, 3) if vs_baseline else None,
            "dtype": "bf16" if use_cuda else "fp32",
            "data": "synthetic",
            "config": {"model": args.model, "global_batch": bs * world,
                       "seq_len": sl,
                       "parallelism": f"{args.sharding}{world}",
                       "tok_per_sec_per_gpu": round(tokens_per_sec / world, 1),
                       "final_loss": round(float(loss.detach()), 4)},
        }))

    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
