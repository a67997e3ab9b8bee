"""Inference measurements of BiSeNet-R18 (random weights, seed 0, eval mode, nn.BatchNorm2d):

  forward    1x3x768x1536 (the .speed config) and 1x3x1024x2048: the stock fp32 network, ours eager bf16
             (prepare_inference), ours graph bf16 (graph=True); compute_speed's protocol (synchronised host timing)
  tail       one 1024x1024 window of 19 x 128^2 bf16 logits into a 19 x 1024 x 2048 map: the unfused ATen chain
             (interpolate, log_softmax, [flip pass], exp, +=) against tsg_seg_tail_accum, with and without flip;
             device time from events over repeated launches, and bytes moved by the fused kernel (the logits read once,
             the window's part of the map read and written once) over that time
  sliding    Evaluator.sliding_eval of one 1024x2048 image (crop 1024, stride rate 2/3, flip), TSG_INFER 0 vs 1

    python tools/bench_infer.py [--quick]

--model x39: BiSeNet-X39 (workloads.bisenet_x39.BiSeNetX39, eval form) instead, forward table only, with the fused
separable units (prepare_inference(fuse_separable=), csrc/sepconv.hip) off and on:
  arms       stock fp32; ours eager bf16 off / on; ours graph bf16 off / on
  protocol   every arm runs in a fresh child process (model build, warm-up of each timed shape, then `iters` calls, each
             between its own pair of device events); the off / on children alternate `--reps` times (default 3) in one
             call.  Reported per arm and shape: the median over the children's medians (min-max over them), and the spread
             of each off arm against itself, (max - min) / median: a difference between off and on below that is noise.

    python tools/bench_infer.py --model x39 [--quick] [--reps 3]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "torchseg_amd", "furnace"))


def r18():
    from torchseg_amd.workloads.bisenet import BiSeNet
    torch.manual_seed(0)
    return BiSeNet(19, False, None, None, nn.BatchNorm2d).eval()


def x39():
    from torchseg_amd.workloads.bisenet_x39 import BiSeNetX39
    torch.manual_seed(0)
    return BiSeNetX39(19, False, None, None, pretrained_model=None, norm_layer=nn.BatchNorm2d).eval()


X39_RES = ((768, 1536), (1024, 2048))
X39_ARMS = ("stock_fp32", "eager_bf16_off", "eager_bf16_on", "graph_bf16_off", "graph_bf16_on")


def event_times(fn, iters, warmup):
    """ms of each of `iters` calls, every call between its own pair of device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def x39_arm(arm, iters, warmup):
    """one arm in this (child) process -> {"HxW": median ms, ...}"""
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    from torchseg_amd.sepconv import fused_calls
    dev = torch.device("cuda:0")
    net = x39().to(dev)
    if arm == "stock_fp32":
        def run(x):
            with torch.no_grad():
                return net(x)
    else:
        prep = prepare_inference(net, dtype=torch.bfloat16, graph=arm.startswith("graph"),
                                 fuse_separable=arm.endswith("_on"))
        assert prep.fused_separable == (51 if arm.endswith("_on") else 0)
        run = (lambda x: prep(x)) if prep.graph else (lambda x: materialize(prep(x)))
    out = {}
    for res in X39_RES:
        x = torch.randn(1, 3, *res, device=dev)
        out["%dx%d" % res] = float(np.median(event_times(lambda: run(x), iters, warmup)))
    if arm.endswith("_on"):
        assert fused_calls(prep.module) > 0
    return out


def x39_table(iters, warmup, reps):
    import subprocess

    def child(arm):
        cmd = [sys.executable, os.path.abspath(__file__), "--model", "x39", "--arm", arm, "--iters", str(iters),
               "--warmup", str(warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("arm %s failed (%d):\n%s\n%s" % (arm, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
        print("%s: %s" % (arm, r.stdout.strip().splitlines()[-1]), file=sys.stderr, flush=True)
        return json.loads(r.stdout.strip().splitlines()[-1])

    runs = {arm: [] for arm in X39_ARMS}
    runs["stock_fp32"].append(child("stock_fp32"))
    for _ in range(reps):                                   # off and on alternate
        for arm in ("graph_bf16_off", "graph_bf16_on", "eager_bf16_off", "eager_bf16_on"):
            runs[arm].append(child(arm))
    result = {"device": torch.cuda.get_device_name(0), "model": "BiSeNet-X39", "iters": iters, "warmup": warmup,
              "reps": reps, "runs_ms": runs}
    print("BiSeNet-X39 forward, batch 1, ms per call: median over %d child processes (min-max); %d timed calls per child, "
          "device events" % (reps, iters))
    print("%-16s %-28s %-28s" % ("arm", "1x3x768x1536", "1x3x1024x2048"))
    summary = {}
    for arm in X39_ARMS:
        cells = []
        for res in X39_RES:
            v = [r["%dx%d" % res] for r in runs[arm]]
            med = float(np.median(v))
            summary.setdefault(arm, {})["%dx%d" % res] = dict(median_ms=med, min_ms=min(v), max_ms=max(v),
                                                               spread=(max(v) - min(v)) / med)
            cells.append("%.3f (%.3f-%.3f)" % (med, min(v), max(v)))
        print("%-16s %-28s %-28s" % (arm, cells[0], cells[1]))
    for kind in ("graph", "eager"):
        for res in X39_RES:
            k = "%dx%d" % res
            off, on = summary[kind + "_bf16_off"][k], summary[kind + "_bf16_on"][k]
            gain = 1.0 - on["median_ms"] / off["median_ms"]
            print("%s %s: fused / unfused = %.3f (%+.1f %% time); spread of the off arm against itself %.1f %%: %s"
                  % (kind, k, on["median_ms"] / off["median_ms"], -100.0 * gain, 100.0 * off["spread"],
                     "beyond the spread" if abs(gain) > off["spread"] else "WITHIN the spread (no difference shown)"))
    result["summary"] = summary
    print(json.dumps(result))


def host_time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    spent = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        spent.append(time.perf_counter() - t0)
    return float(np.median(spent))


def event_time(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters / 1e3


def forward(res, iters, warmup):
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    dev = torch.device("cuda:0")
    x = torch.randn(1, 3, *res, device=dev)
    out = {}
    stock = r18().to(dev)
    with torch.no_grad():
        out["stock_fp32_ms"] = 1e3 * host_time(lambda: stock(x), iters, warmup)
    eager = prepare_inference(r18().to(dev), dtype=torch.bfloat16)
    out["ours_eager_bf16_ms"] = 1e3 * host_time(lambda: materialize(eager(x)), iters, warmup)
    graph = prepare_inference(r18().to(dev), dtype=torch.bfloat16, graph=True)
    out["ours_graph_bf16_ms"] = 1e3 * host_time(lambda: graph(x), iters, warmup)
    for k in list(out):
        out[k.replace("_ms", "_fps")] = 1e3 / out[k]
    return out


def tail(iters):
    from torchseg_amd import kernels as K
    kp = K.provider()
    dev = torch.device("cuda:0")
    z = torch.randn(1, 19, 128, 128, device=dev).to(torch.bfloat16)
    zf = torch.randn_like(z)
    data = torch.zeros(19, 1024, 2048, device=dev)
    geom = torch.tensor([[0, 683, 0, 0, 1024, 1024]], dtype=torch.int32, device=dev)
    region = (0, 1024, 683, 1707)
    res = {}
    for flip in (False, True):
        def aten():
            with torch.no_grad():
                s = F.log_softmax(F.interpolate(z, size=(1024, 1024), mode="bilinear", align_corners=True).float(), 1)
                if flip:
                    s = s + F.log_softmax(F.interpolate(zf, size=(1024, 1024), mode="bilinear",
                                                        align_corners=True).float(), 1).flip(-1)
                data[:, :, 683:1707] += torch.exp(s)[0]

        def fused():
            kp.seg_tail_accum(z, zf if flip else None, geom, data, 1024, 1024, accumulate=True, region=region)
        t_a, t_f = event_time(aten, iters), event_time(fused, iters)
        nbytes = 2 * 19 * 1024 * 1024 * 4 + z.numel() * z.element_size() * (2 if flip else 1)
        key = "flip" if flip else "noflip"
        res[key] = dict(aten_ms=1e3 * t_a, fused_ms=1e3 * t_f, speedup=t_a / t_f, fused_bytes=nbytes,
                        fused_TBps=nbytes / t_f / 1e12, share_of_8TBps=nbytes / t_f / 8e12)
    return res


def sliding(iters):
    from engine.evaluator import Evaluator
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    img = np.random.RandomState(0).randint(0, 256, (1024, 2048, 3)).astype(np.uint8)
    net = r18()
    res = {}
    for flag in ("0", "1"):
        os.environ["TSG_INFER"] = flag
        ev = Evaluator(None, 19, mean, std, copy.deepcopy(net), [1.0], True, [0])
        ev.val_func = ev.network
        res["TSG_INFER=%s_ms" % flag] = 1e3 * host_time(lambda: ev.sliding_eval(img, 1024, 2 / 3, device=0), iters, 2)
    os.environ["TSG_INFER"] = "0"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--model", choices=("r18", "x39"), default="r18")
    ap.add_argument("--reps", type=int, default=3, help="x39: how often the off / on children alternate")
    ap.add_argument("--arm", choices=X39_ARMS, default=None, help="x39: run this one arm here (what a child is started with)")
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.model == "x39":
        iters = a.iters or (10 if a.quick else 100)
        if a.arm is not None:
            print(json.dumps(x39_arm(a.arm, iters, a.warmup)))
        else:
            x39_table(iters, a.warmup, max(3, a.reps))
        return
    it = 5 if a.quick else 30
    result = {"device": torch.cuda.get_device_name(0), "dtype_env": os.environ.get("TSG_DTYPE", "bf16")}
    for res in ((768, 1536), (1024, 2048)):
        result["forward_%dx%d" % res] = forward(res, it, 10)
        print(json.dumps({"forward_%dx%d" % res: result["forward_%dx%d" % res]}), flush=True)
    result["tail_1024_window"] = tail(50)
    print(json.dumps({"tail_1024_window": result["tail_1024_window"]}), flush=True)
    result["sliding_eval_1024x2048_flip"] = sliding(3 if a.quick else 5)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
