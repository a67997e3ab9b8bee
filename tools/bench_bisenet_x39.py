"""BiSeNet-X39 training-step timing (bench.py measures R18 only).

The X39 workload (torchseg_amd/workloads/bisenet_x39.py) behind the DDP wrapper with SyncBatchNorm, OHEM on all three
heads, FusedSGD and PolyLR (X39 train.py's parameter groups, all at the
config's lr); synthetic N(0,1) bf16-autocast input and uint8 labels; eager steps.  Prints one JSON line.

    python tools/bench_bisenet_x39.py [--steps 20 --warmup 10 --batch 16 --size 1024] [--dw-conv 0|1]

--dw-conv runs the measurement in a fresh child process with TSG_DW_CONV set accordingly (0: the depthwise layers on
the vendor library; 1: on tsg_dwconv3x3_*), for A/B pairs from one parent.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def measure(steps, warmup, batch, size):
    import torch
    import torch.nn as nn
    import bench
    from torchseg_amd.workloads import ensure_furnace_on_path
    ensure_furnace_on_path()
    from engine.lr_policy import PolyLR
    from utils.init_func import group_weight
    from torchseg_amd.ddp import DistributedDataParallel
    from torchseg_amd.losses import ProbOhemCrossEntropy2d
    from torchseg_amd.optim import FusedSGD
    from torchseg_amd.syncbn import SyncBatchNorm
    from torchseg_amd.workloads.bisenet_x39 import BiSeNetX39

    dev = torch.device("cuda:0")
    torch.manual_seed(12345)
    ohem = ProbOhemCrossEntropy2d(255, thresh=0.7, min_kept=batch * size * size // 16)
    model = BiSeNetX39(19, True, None, ohem, norm_layer=SyncBatchNorm)
    base_lr, wd = 1e-2, 5e-4                                     # X39 config.py:78-81
    groups = group_weight([], model.context_path, SyncBatchNorm, base_lr)
    for part in model.business_layer:                             # X39 train.py:69-83: every group at base_lr
        groups = group_weight(groups, part, SyncBatchNorm, base_lr)
    model = DistributedDataParallel(model.to(dev))
    opt = FusedSGD(groups, lr=base_lr, momentum=0.9, weight_decay=wd)
    pol = PolyLR(base_lr, 0.9, 80000)
    data = bench.synthetic_batch(dev, batch, size, label_dtype=torch.uint8)
    model.train()
    from torchseg_amd.dwconv import DepthwiseConv2d
    n_dw = sum(isinstance(m, DepthwiseConv2d) for m in model.module.modules())
    for it in range(warmup):
        bench.train_step(model, opt, data, pol, it, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(steps):
        loss = bench.train_step(model, opt, data, pol, warmup + it, 1)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return dict(model="BiSeNet-X39", batch=batch, size=size, steps=steps, warmup=warmup,
                dw_conv=os.environ.get("TSG_DW_CONV", "1"), depthwise_layers_on_ours=n_dw,
                ms_per_step=round(dt * 1e3, 3), img_per_s=round(batch / dt, 2), loss=round(float(loss.item()), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--dw-conv", type=int, choices=[0, 1], default=None)
    a = ap.parse_args()
    if a.dw_conv is not None:
        env = dict(os.environ, TSG_DW_CONV=str(a.dw_conv))
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--batch", str(a.batch), "--size", str(a.size)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-4000:])
        if r.returncode != 0:
            sys.stdout.write(r.stdout[-4000:])
            sys.exit(r.returncode if r.returncode > 0 else 1)
        sys.stdout.write(r.stdout.strip().splitlines()[-1] + "\n")
        return
    print(json.dumps(measure(a.steps, a.warmup, a.batch, a.size)))


if __name__ == "__main__":
    main()
