"""Headline benchmark: ResNet-50 DDP images/sec on 1/2/4/8 MI355X (BASELINE.json metric / config 2).

Model: ResNet-50 v1.5 random init, bf16 parameters + fp32 masters (fused SGD, momentum 0.9, wd 5e-5);
data: synthetic ImageNet-shape batches (224x224, 1000 classes) generated on device every step;
parallelism: one process per GPU, gradients all-reduced by the bucketed DDP over RCCL, overlapped with
backward.  Weak scaling: the per-GPU batch is fixed.
"""
from __future__ import annotations

import argparse
import contextlib
import os

import torch

from ..data.device import DeviceSyntheticImages
from ..models.resnet import resnet50
from ..ops import cross_entropy
from ..optim import SGD
from ..parallel.ddp import DistributedDataParallel
from .common import comm_record, emit, group_info, setup, teardown, timed

METRIC = "images/sec (whole node) ResNet-50 DDP at 1/2/4/8 MI355X; scaling efficiency"


PARAM_SAMPLE = 4096  # elements dumped per parameter tensor (all of a smaller one)


def build(batch: int, image: int, device, rank: int, dtype=torch.bfloat16, bucket_mb=None, keep=None):
    """``keep``: a dict that receives each step's logits as ``keep["logits"]`` (for ``--dump-outputs``)."""
    torch.manual_seed(0)
    model = resnet50(device=device, dtype=dtype)
    model = DistributedDataParallel(model, device_ids=[device.index] if device.type == "cuda" else None,
                                    bucket_cap_mb=bucket_mb)
    opt = SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-5)
    data = DeviceSyntheticImages(batch, image, 1000, device=device, dtype=dtype, seed=1234, rank=rank)

    def step():
        x, y = data.next()
        opt.zero_grad(set_to_none=True)
        out = model(x)
        loss = cross_entropy(out, y)
        loss.backward()
        opt.step()
        if keep is not None:
            keep["logits"] = out
        return loss

    return model, opt, step


def dump_outputs(outdir: str, loss, logits, model) -> None:
    """What the last timed step computed, as float32 ``.npy`` files: ``loss`` (scalar), ``logits``
    ([per-GPU batch, classes]) and ``params_sample``: the parameters after the step's update, a fixed
    seeded sample of at most PARAM_SAMPLE elements of each tensor, concatenated in registration order
    (weights and batches are seeded and a dumping run sums in a fixed order, see :func:`main`, so two runs
    and two builds compare file for file)."""
    import numpy as np

    os.makedirs(outdir, exist_ok=True)
    gen = torch.Generator().manual_seed(20240)
    pieces = []
    for p in model.parameters():
        flat = p.detach().reshape(-1)
        if flat.numel() > PARAM_SAMPLE:
            idx = torch.randint(0, flat.numel(), (PARAM_SAMPLE,), generator=gen)
            flat = flat[idx.to(flat.device)]
        pieces.append(flat.float().cpu())
    arrays = {"loss": loss.detach().float().cpu().reshape(1), "logits": logits.detach().float().cpu(),
              "params_sample": torch.cat(pieces)}
    for name, t in arrays.items():
        np.save(os.path.join(outdir, name + ".npy"), t.numpy())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    # per-GPU batch: 640 uses the 288 GB of an MI355X for throughput (bigger GEMM grids — the 14^2 / 7^2
    # convs' tile rounds quantise better: 640 * 196 / 256 = 490 tiles = 1.91 rounds of 256 CUs against
    # 1.53 at 512 — and less per-image launch / epilogue overhead); measured on one MI355X with the
    # current kernels (profiles/r2_resnet50_batch_sweep_v23.jsonl): 512 -> 10.94k, 576 -> 11.27k,
    # 640 -> 11.31k, 704 -> 11.07k, 768 -> 11.13k img/s (round-1 setting: --batch 256).
    ap.add_argument("--batch", type=int, default=int(os.environ.get("PDA_BENCH_BATCH", "640")),
                    help="per-GPU batch")
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--bucket-mb", type=float, default=None)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps rank 0 writes the last step's loss, logits and a sample of "
                         "the updated parameters to DIR/<name>.npy (float32); such a run sums in a fixed "
                         "order (PDA_DETERMINISTIC=1 unless the variable is already set), so the files "
                         "repeat from run to run and its speed is not the headline figure")
    ap.add_argument("--full", action="store_true",
                    help="also run the benchmark's secondary measurements; the headline run has none "
                         "(set-up, warm-up, the timed steps and the result line are all it does), so "
                         "this changes nothing today")
    a = ap.parse_args(argv)
    if a.dump_outputs:
        # The default kernels add BN statistics with atomics, and a random-init ResNet-50 amplifies that
        # last-bit noise to the first digits of the logits within a step (README, Quick start): a run whose
        # outputs are to be compared uses the fixed-order sums for all its steps, from before the first
        # one.  An exported PDA_DETERMINISTIC=0 keeps the default path (and its noise) in the dump.
        os.environ.setdefault("PDA_DETERMINISTIC", "1")
    # N=1 runs the DDP bucket all-reduces over a one-rank RCCL group (PDA_DDP_FORCE_COMM=0 turns it off)
    rank, world, local, device = setup(a.gpus, one_rank_group=True)
    if device.type == "cpu":  # plumbing-only run on a machine without a GPU
        a.batch, a.image = min(a.batch, 2), min(a.image, 64)
    # PDA_MAIN_PRIO=high: the whole step on a high-priority HIP stream (A/B knob for queue arbitration
    # against the low-priority weight-gradient side stream, ops/streams.py)
    ctx = contextlib.nullcontext()
    if device.type == "cuda" and os.environ.get("PDA_MAIN_PRIO") == "high":
        ctx = torch.cuda.stream(torch.cuda.Stream(device=device, priority=-1))
    with ctx:
        keep = {} if a.dump_outputs and rank == 0 else None
        model, _, step = build(a.batch, a.image, device, rank, bucket_mb=a.bucket_mb, keep=keep)
        losses = []
        before_timed = []

        def on_start():
            before_timed.append(len(losses))
            if hasattr(model, "comm_stats"):
                model.comm_stats(reset=True)

        secs = timed(lambda: losses.append(step()), a.steps, a.warmup, on_start=on_start)
        timed_steps_run = len(losses) - before_timed[0]  # counted, not echoed from --steps
        comm = comm_record(model, a.steps)
        if keep is not None:
            dump_outputs(a.dump_outputs, losses[-1], keep["logits"], model)
    # (after the timed window) a benchmark that diverged would be measuring garbage
    last = float(losses[-1].item())
    if last != last or abs(last) == float("inf"):
        raise SystemExit(f"non-finite training loss {last} in the benchmark run")
    ms = secs / a.steps * 1e3
    grp = group_info(device)
    world = grp["world"]
    imgs = a.batch * world * a.steps / secs
    emit({
        "metric": METRIC, "value": round(imgs, 2), "unit": "images/sec", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
        "timed_steps_run": timed_steps_run,
        "vs_baseline": None, "rccl_world": grp["rccl_world"], "backend": grp["backend"], "dtype": "bf16" if device.type == "cuda" else "bf16-cpu-plumbing",
        "data": "synthetic (on-device Philox, ImageNet shape 224x224x3, 1000 classes), random-init weights",
        "config": {"model": "resnet50", "global_batch": a.batch * world, "per_gpu_batch": a.batch,
                   "image_size": a.image, "seq_len": None, "parallelism": f"dp{world}",
                   "optimizer": "SGD(momentum=0.9, wd=5e-5), fp32 master weights"},
        "final_loss": round(last, 4),
        "fixed_order_sums": os.environ.get("PDA_DETERMINISTIC", "0") == "1",
        "comm": comm,
        "notes": "reference publishes no number for this metric (BASELINE.json published={}); per-GPU batch "
                 f"{a.batch} (640 = throughput-optimal on 288 GB HBM by a 512-768 sweep; --batch 256 gives "
                 "the round-1 setting); NB03 parity numbers are produced by pytorchdistributed_amd.bench.nb03",
    }, rank)
    teardown()


if __name__ == "__main__":
    main()
