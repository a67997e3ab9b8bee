"""FCN-32s training-step timing (bench.py measures the BASELINE configs; FCN is not one of them).

The FCN workload (torchseg_amd/workloads/fcn.py, ResNet-101-v1c) behind the DDP wrapper with SyncBatchNorm,
nn.CrossEntropyLoss(ignore_index=255) on both heads (x32 and x16: the fused up-sampling criterion), FusedSGD over
train.py's parameter groups and PolyLR; synthetic N(0,1) bf16-autocast input, 21-class uint8 labels; eager steps.
Prints one JSON line.

    python tools/bench_fcn.py [--steps 20 --warmup 10 --batch 4 --size 512] [--deep-stem 0|1] [--stem-only]

--deep-stem runs the measurement in a fresh child process with TSG_DEEP_STEM_CONV set accordingly (0: the deep stem's
3 -> 64 3x3/2 image convolution on the vendor library; 1: on tsg_stem3_conv_*), for A/B pairs from one parent.
--stem-only times that convolution alone (forward + weight gradient, the image needs no gradient) as the step runs it:
bf16 autocast on a channels_last fp32 image; and reports it against its HBM floor (read x, write y; read x and dy).
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

NCLS = 21
HBM_TBPS = 6.3                 # achievable HBM bandwidth for the floor (MI355X: 8 TB/s peak, ~6.3 measured with a copy)


def _batch(dev, batch, size):
    import torch
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(batch, 3, size, size, generator=g, device=dev)
    y = torch.randint(0, NCLS, (batch, size, size), generator=g, device=dev)
    y[:, :8] = 255
    return x, y.to(torch.uint8)


def measure(steps, warmup, batch, size):
    import torch
    import torch.nn as nn
    import bench
    from torchseg_amd.workloads import ensure_furnace_on_path
    ensure_furnace_on_path()
    from engine.lr_policy import PolyLR
    from utils.init_func import group_weight
    from torchseg_amd.ddp import DistributedDataParallel
    from torchseg_amd.optim import FusedSGD
    from torchseg_amd.stemconv import DeepStemConv2d
    from torchseg_amd.syncbn import SyncBatchNorm
    from torchseg_amd.workloads.fcn import FCN

    dev = torch.device("cuda:0")
    torch.manual_seed(304)
    model = FCN(NCLS, nn.CrossEntropyLoss(reduction='mean', ignore_index=255), norm_layer=SyncBatchNorm)
    base_lr, wd = 1e-2, 1e-4                                     # fcn config.py:74-78
    groups = group_weight([], model, SyncBatchNorm, base_lr)    # fcn train.py:64-66
    model = DistributedDataParallel(model.to(dev))
    opt = FusedSGD(groups, lr=base_lr, momentum=0.9, weight_decay=wd)
    pol = PolyLR(base_lr, 0.9, 60 * 10582 // 32)
    data = _batch(dev, batch, size)
    model.train()
    n_stem = sum(isinstance(m, DeepStemConv2d) for m in model.module.modules())
    for it in range(warmup):
        bench.train_step(model, opt, data, pol, it, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(steps):
        loss = bench.train_step(model, opt, data, pol, warmup + it, 1)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return dict(model="FCN-32s-R101_v1c", batch=batch, size=size, steps=steps, warmup=warmup,
                deep_stem=os.environ.get("TSG_DEEP_STEM_CONV", "0"), deep_stem_layers_on_ours=n_stem,
                ms_per_step=round(dt * 1e3, 3), img_per_s=round(batch / dt, 2), loss=round(float(loss.item()), 5))


def measure_stem(steps, warmup, batch, size):
    """The deep stem's first convolution alone, forward + weight gradient, as the step runs it (bf16 autocast,
    channels_last fp32 image; its consumer reads y channels_last)."""
    import torch
    import torch.nn as nn
    from torchseg_amd.stemconv import install_deep_stem_conv
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    conv = nn.Conv2d(3, 64, 3, 2, 1, bias=False).to(dev)
    ours = os.environ.get("TSG_DEEP_STEM_CONV", "0") == "1"
    if ours:
        assert install_deep_stem_conv(conv) == 1
    x = torch.randn(batch, 3, size, size, device=dev).contiguous(memory_format=torch.channels_last)
    oh, ow = (size - 1) // 2 + 1, (size - 1) // 2 + 1
    dy = torch.randn(batch, 64, oh, ow, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)

    from torchseg_amd import stemconv

    def fwd():
        stemconv._cast_cache[0] = None              # a new image every step: ours casts it to bf16, as autocast does
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return conv(x)

    def step():
        conv.weight.grad = None
        fwd().backward(dy)

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps

    ms_fwd = timed(lambda: fwd())
    ms_step = timed(step)
    x_bytes = batch * 3 * size * size * 2                       # the bf16 image: what the kernel reads
    y_bytes = batch * oh * ow * 64 * 2
    floor_fwd = (x_bytes + y_bytes) / (HBM_TBPS * 1e12) * 1e3
    floor_step = 2 * floor_fwd
    return dict(what="deep-stem conv 3->64 3x3/2", batch=batch, size=size, deep_stem=("1" if ours else "0"),
                ms_fwd=round(ms_fwd, 4), ms_fwd_plus_wgrad=round(ms_step, 4), ms_wgrad=round(ms_step - ms_fwd, 4),
                hbm_floor_ms_fwd=round(floor_fwd, 4), hbm_floor_ms_fwd_plus_wgrad=round(floor_step, 4),
                floor_MB_fwd=round((x_bytes + y_bytes) / 1e6, 1), floor_MB_wgrad=round((x_bytes + y_bytes) / 1e6, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--deep-stem", type=int, choices=[0, 1], default=None)
    ap.add_argument("--stem-only", action="store_true")
    a = ap.parse_args()
    if a.deep_stem is not None:
        env = dict(os.environ, TSG_DEEP_STEM_CONV=str(a.deep_stem))
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--batch", str(a.batch), "--size", str(a.size)] + (["--stem-only"] if a.stem_only else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-4000:])
        if r.returncode != 0:
            sys.stdout.write(r.stdout[-4000:])
            sys.exit(r.returncode if r.returncode > 0 else 1)
        sys.stdout.write(r.stdout.strip().splitlines()[-1] + "\n")
        return
    fn = measure_stem if a.stem_only else measure
    print(json.dumps(fn(a.steps, a.warmup, a.batch, a.size)))


if __name__ == "__main__":
    main()
