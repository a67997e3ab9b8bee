"""Eager training step against torchseg_amd.step.ReplayedStep, per workload.

    python tools/bench_step.py --config bisenet|pspnet|dfn|psanet|fcn [--steps 30 --warmup 10 --reps 3] [--batch B --size S]

The builders of torchseg_amd/workloads behind the DDP wrapper with FusedSGD and PolyLR, at the per-rank shapes bench.py
uses (FCN: tools/bench_fcn.py's), synthetic input.  Two arms:
    eager   the hand-written loop (set lr, zero_grad, forward, backward, optimizer.step): what INTEGRATION.md gives a user
    replay  the same loop with `loss = step(*batch)` (ReplayedStep, warmup 3)
One process per arm, the arms alternate --reps times (eager, replay, eager, replay, ...), every process runs under its own
`timeout`, and the script stops at the first non-zero exit status.  Per process: ms/step between two HIP events around the
timed steps, the host's enqueue time per step (wall clock until the last step is queued, before any synchronisation),
torch.cuda.max_memory_allocated and max_memory_reserved over the timed steps (a graph's private pool is reserved once at
capture; what a replay uses inside it is not allocated again, so `allocated` of the replay arm counts only what lives
outside the pool).  The last lines are the per-arm summary (median, min - max over the repetitions).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FCN = dict(batch=4, size=512, classes=21)


def _build(config, dev, batch, size):
    """-> (wrapped model, optimizer, base lr, batch tuple)"""
    import torch
    import torch.nn as nn
    import bench
    from torchseg_amd.ddp import DistributedDataParallel
    from torchseg_amd.losses import ProbOhemCrossEntropy2d, SigmoidFocalLoss
    from torchseg_amd.syncbn import SyncBatchNorm
    if config == "fcn":
        from torchseg_amd.workloads import ensure_furnace_on_path
        ensure_furnace_on_path()
        from utils.init_func import group_weight
        from torchseg_amd.optim import FusedSGD
        from torchseg_amd.workloads.fcn import FCN as Net
        torch.manual_seed(304)
        model = Net(FCN["classes"], nn.CrossEntropyLoss(reduction='mean', ignore_index=255), norm_layer=SyncBatchNorm)
        base_lr = 1e-2
        groups = group_weight([], model, SyncBatchNorm, base_lr)
        model.to(dev)
        opt = FusedSGD(groups, lr=base_lr, momentum=0.9, weight_decay=1e-4)
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(batch, 3, size, size, generator=g, device=dev)
        y = torch.randint(0, FCN["classes"], (batch, size, size), generator=g, device=dev)
        y[:, :8] = 255
        data = (x, y.to(torch.uint8))
    else:
        model, opt, base_lr = bench.build_model(dev, batch, size, ProbOhemCrossEntropy2d, SyncBatchNorm, fused_sgd=True,
                                                config=config, focal_cls=SigmoidFocalLoss)
        data = bench.synthetic_batch(dev, batch, size, config=config,
                                     label_dtype=torch.uint8 if config in ("bisenet", "dfn") else torch.int64)
    model = DistributedDataParallel(model)
    model.train()
    return model, opt, base_lr, data


def child(a):
    import torch
    os.environ["TSG_DTYPE"] = "bf16"
    from torchseg_amd.tuning import use_shipped_miopen_db
    use_shipped_miopen_db(rank=0)
    torch.backends.cudnn.benchmark = False                         # immediate mode on the shipped find-db, as bench.py
    from torchseg_amd.workloads import ensure_furnace_on_path
    ensure_furnace_on_path()
    from engine.lr_policy import PolyLR
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    model, opt, base_lr, data = _build(a.config, dev, a.batch, a.size)
    pol = PolyLR(base_lr, 0.9, 80 * 1000)
    step = None
    if a.arm == "replay":
        from torchseg_amd.step import ReplayedStep
        step = ReplayedStep(model, opt, warmup=3, strict=True)

    def one(it):
        lr = pol.get_lr(it)
        for i, g in enumerate(opt.param_groups):                   # train.py:133-139
            g["lr"] = lr if i < 2 else lr * 10
        if step is not None:
            return step(*data)
        opt.zero_grad()
        loss = model(*data)
        loss.backward()
        opt.step()
        return loss

    for it in range(max(a.warmup, 5)):                             # replay arm: 3 eager steps, the capture, replays
        one(it)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for it in range(a.steps):
        loss = one(a.warmup + it)
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    out = dict(config=a.config, arm=a.arm, batch=a.batch, size=a.size, steps=a.steps,
               ms_per_step=round(e0.elapsed_time(e1) / a.steps, 3), host_enqueue_ms_per_step=round(host / a.steps * 1e3, 3),
               max_memory_allocated_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
               max_memory_reserved_mb=round(torch.cuda.max_memory_reserved() / 2 ** 20, 1),
               loss=round(float(loss.item()), 5))
    if step is not None:
        out.update(mode=step.mode, captures=step.captures, replays=step.replays)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="bisenet", choices=["bisenet", "pspnet", "dfn", "psanet", "fcn"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--timeout", type=int, default=300, help="seconds each process may take")
    ap.add_argument("--arm", default=None, choices=["eager", "replay"], help="run this arm in this process (what the parent starts)")
    a = ap.parse_args()
    if a.config == "fcn":
        shape = FCN
    else:
        import bench
        shape = bench.CONFIGS[a.config]
    a.batch = shape["batch"] if a.batch is None else a.batch
    a.size = shape["size"] if a.size is None else a.size
    if a.arm is not None:
        return child(a)
    rows = {"eager": [], "replay": []}
    for rep in range(a.reps):
        for arm in ("eager", "replay"):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--arm", arm,
                   "--config", a.config, "--steps", str(a.steps), "--warmup", str(a.warmup), "--batch", str(a.batch),
                   "--size", str(a.size)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stdout.write(r.stdout[-2000:])
                print("bench_step: %s arm, repetition %d: exit status %d; stopping" % (arm, rep, r.returncode), flush=True)
                sys.exit(r.returncode if r.returncode > 0 else 1)
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            rows[arm].append(json.loads(line))
    for arm in ("eager", "replay"):
        def col(k):
            v = [r[k] for r in rows[arm]]
            return "%.3f (%.3f - %.3f)" % (statistics.median(v), min(v), max(v))
        print("%-8s %-6s ms/step %s | host enqueue ms/step %s | peak allocated MB %s | peak reserved MB %s" % (
            a.config, arm, col("ms_per_step"), col("host_enqueue_ms_per_step"), col("max_memory_allocated_mb"),
            col("max_memory_reserved_mb")), flush=True)


if __name__ == "__main__":
    main()
