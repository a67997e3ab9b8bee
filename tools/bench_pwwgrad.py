"""GPU microbench of the 1x1 convolutions' weight gradient (tsg_pw_wgrad, csrc/pwwgrad.hip) at every whole-map 1x1 layer
shape of the benched configurations: BiSeNet-R18 16 x 1024^2, PSPNet-R50 2 x 720^2, DFN-R101 2 x 1024^2, PSANet-R101
2 x 480^2 and FCN-R101 4 x 512^2.  The shapes are not written down here: each network is built the way bench.py /
tools/bench_fcn.py build it and ONE eager training step runs with pwconv.pointwise_wgrad wrapped, which records the
(B, C_in, C_out, H, W, stride) of every call and how often a step makes it.

Three arms per shape, bf16 channels_last operands, one process:
  hip      kernels.pw_wgrad: the new kernel INCLUDING its fold, workspace from the caching allocator per call
  today    pwconv.pointwise_wgrad with the switch off: chunked torch.bmm + ordered sum, INCLUDING the stride-2 gather
  vendor   aten.convolution_backward, weight gradient only (the vendor library with the shipped find-db)
HIP-event timing: 10 warm-up calls per arm, a calibration window, then 3 rounds in which the arms ALTERNATE, one window of
at least 0.25 s per arm and round; the median window is reported (min-max beside it).  Every call reuses the same
operands: cache-warm, back-to-back figures, like for like between the arms, below what a layer costs inside a step.
Also printed: the relative L2 distance of each arm's result from the float64 gradient of the same bf16 operands, and per
configuration the sum over its layers (count x median).

    python tools/bench_pwwgrad.py [OUT.txt] [--configs bisenet,pspnet,dfn,psanet,fcn]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn as nn

import bench
from torchseg_amd import kernels as K
from torchseg_amd import pwconv
from torchseg_amd.tuning import use_shipped_miopen_db

use_shipped_miopen_db(0)
dev = torch.device("cuda:0")
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = argv[0] if argv else None
configs = ["bisenet", "pspnet", "dfn", "psanet", "fcn"]
for i, a in enumerate(sys.argv):
    if a == "--configs":
        configs = sys.argv[i + 1].split(",")
NAMES = {"bisenet": "BiSeNet-R18 16 x 1024^2", "pspnet": "PSPNet-R50 2 x 720^2", "dfn": "DFN-R101 2 x 1024^2",
         "psanet": "PSANet-R101 2 x 480^2", "fcn": "FCN-R101 4 x 512^2"}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def step_shapes(config):
    """{(B, Cin, Cout, H, W, stride): calls per step} of pointwise_wgrad in one eager training step of the configuration"""
    from torchseg_amd.workloads import ensure_furnace_on_path
    ensure_furnace_on_path()
    from engine.lr_policy import PolyLR
    from utils.init_func import group_weight
    from torchseg_amd.ddp import DistributedDataParallel
    from torchseg_amd.losses import ProbOhemCrossEntropy2d, SigmoidFocalLoss
    from torchseg_amd.optim import FusedSGD
    from torchseg_amd.syncbn import SyncBatchNorm
    if config == "fcn":
        from torchseg_amd.workloads.fcn import FCN
        torch.manual_seed(304)
        model = FCN(21, nn.CrossEntropyLoss(reduction='mean', ignore_index=255), norm_layer=SyncBatchNorm)
        base_lr = 1e-2
        opt = FusedSGD(group_weight([], model, SyncBatchNorm, base_lr), lr=base_lr, momentum=0.9, weight_decay=1e-4)
        model.to(dev)
        g = torch.Generator(device=dev).manual_seed(0)
        y = torch.randint(0, 21, (4, 512, 512), generator=g, device=dev)
        y[:, :8] = 255
        data = (torch.randn(4, 3, 512, 512, generator=g, device=dev), y.to(torch.uint8))
    else:
        cfg = bench.CONFIGS[config]
        model, opt, base_lr = bench.build_model(dev, cfg["batch"], cfg["size"], ProbOhemCrossEntropy2d, SyncBatchNorm,
                                                fused_sgd=True, config=config, focal_cls=SigmoidFocalLoss)
        data = bench.synthetic_batch(dev, cfg["batch"], cfg["size"], config=config,
                                     label_dtype=torch.uint8 if config in ("bisenet", "dfn") else torch.int64)
    model = DistributedDataParallel(model)
    model.train()
    seen = {}
    orig = pwconv.pointwise_wgrad

    def spy(x, dy, stride, out=None):
        key = (x.shape[0], x.shape[1], dy.shape[1], x.shape[2], x.shape[3], int(stride))
        seen[key] = seen.get(key, 0) + 1
        return orig(x, dy, stride, out=out)

    pwconv.pointwise_wgrad = spy
    try:
        bench.train_step(model, opt, data, PolyLR(base_lr, 0.9, 80 * 1000), 0, 1)
        torch.cuda.synchronize()
    finally:
        pwconv.pointwise_wgrad = orig
    del model, opt, data
    torch.cuda.empty_cache()
    return seen


def window(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def time_arms(arms, rounds=3, seconds=0.25):
    """{name: (median, min, max) us}: the arms alternate, one window of >= `seconds` per arm and round"""
    n = {}
    for name, fn in arms.items():
        for _ in range(10):
            fn()
        n[name] = max(20, int(seconds * 1e6 / window(fn, 20)) + 1)
    ts = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            ts[name].append(window(fn, n[name]))
    return {name: (sorted(v)[len(v) // 2], min(v), max(v)) for name, v in ts.items()}


def bench_shape(key):
    B, Cin, Cout, H, W, st = key
    kp = K.provider()
    g = torch.Generator(device=dev).manual_seed(sum(key))
    OH, OW = (H - 1) // st + 1, (W - 1) // st + 1
    x = torch.randn(B, Cin, H, W, generator=g, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)
    dy = torch.randn(B, Cout, OH, OW, generator=g, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)
    wb = torch.zeros(Cout, Cin, 1, 1, device=dev, dtype=torch.bfloat16)
    arms = {}
    if kp.pw_wgrad_supported(x, dy, st):
        arms["hip"] = lambda: kp.pw_wgrad(x, dy, st)
    arms["today"] = lambda: pwconv.pointwise_wgrad(x, dy, st)
    arms["vendor"] = lambda: torch.ops.aten.convolution_backward(dy, x, wb, None, [st, st], [0, 0], [1, 1], False, [0, 0], 1,
                                                                 [False, True, False])[1]
    # float64 gradient of the same bf16 operands (GPU fp64 GEMM on the pixels the convolution read)
    xs = x[:, :, ::st, ::st].permute(0, 2, 3, 1).reshape(-1, Cin).double()
    ref = dy.permute(0, 2, 3, 1).reshape(-1, Cout).double().t().mm(xs)
    del xs
    rel = {name: ((fn().double().view(Cout, Cin) - ref).norm() / ref.norm()).item() for name, fn in arms.items()}
    del ref
    return time_arms(arms), rel


def main():
    old = pwconv._HIP_WGRAD
    pwconv._HIP_WGRAD = False            # "today" is the switch-off path; the new kernel is called through the provider
    try:
        per = {}
        for c in configs:
            per[c] = step_shapes(c)
        lib = K.provider().lib
        say("# us per call: median of 3 alternating windows of >= 0.25 s (min-max); cache-warm back-to-back calls; "
            "rel = |dw - dw64| / |dw64|; S = pixel slices")
        done = {}
        for c in configs:
            say("")
            say("%s: %d whole-map 1x1 weight gradients per step, %d distinct shapes" % (NAMES[c], sum(per[c].values()), len(per[c])))
            tot = {"hip": 0.0, "today": 0.0, "vendor": 0.0, "today (unsupported)": 0.0}
            for key in sorted(per[c], key=lambda k: (-k[3] * k[4], k[1], k[2], k[5])):
                if key not in done:
                    done[key] = bench_shape(key)
                t, rel = done[key]
                B, Cin, Cout, H, W, st = key
                S = lib.tsg_pw_wgrad_slices(Cin, Cout, B, H, W, st)
                gf = 2.0 * B * ((H - 1) // st + 1) * ((W - 1) // st + 1) * Cin * Cout / 1e9
                head = "  x%-2d %4d -> %4d @ %dx%dx%d s%d (%.2f GFLOP) S=%-3d" % (per[c][key], Cin, Cout, B, H, W, st, gf, S)
                cells = []
                for name in ("hip", "today", "vendor"):
                    if name in t:
                        cells.append("%s %6.1f (%.1f-%.1f) rel %.1e" % ((name,) + t[name] + (rel[name],)))
                        if "hip" in t:
                            tot[name] += per[c][key] * t[name][0]
                    else:
                        cells.append("%s unsupported" % name)
                if "hip" not in t:
                    tot["today (unsupported)"] += per[c][key] * t["today"][0]
                else:
                    best = min(("hip", "today", "vendor"), key=lambda nm: t[nm][0])
                    cells.append("best: %s" % best)
                say(head + " | " + " | ".join(cells))
            say("  per step over the supported layers: hip %.0f us, today %.0f us, vendor %.0f us; layers the kernel does not "
                "take (stay on today's path): %.0f us" % (tot["hip"], tot["today"], tot["vendor"], tot["today (unsupported)"]))
    finally:
        pwconv._HIP_WGRAD = old
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
