"""Inference measurements of BiSeNet-R18 (random weights, seed 0, eval mode, nn.BatchNorm2d):

  forward    1x3x768x1536 (the .speed config) and 1x3x1024x2048: the stock fp32 network, ours eager bf16
             (prepare_inference), ours graph bf16 (graph=True); compute_speed's protocol (synchronised host timing)
  tail       one 1024x1024 window of 19 x 128^2 bf16 logits into a 19 x 1024 x 2048 map: the unfused ATen chain
             (interpolate, log_softmax, [flip pass], exp, +=) against tsg_seg_tail_accum, with and without flip;
             device time from events over repeated launches, and bytes moved by the fused kernel (the logits read once,
             the window's part of the map read and written once) over that time
  sliding    Evaluator.sliding_eval of one 1024x2048 image (crop 1024, stride rate 2/3, flip), TSG_INFER 0 vs 1

    python tools/bench_infer.py [--quick]
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
    a = ap.parse_args()
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
