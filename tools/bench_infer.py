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

--model r18 --convbn: the same arm scheme and protocol for BiSeNet-R18 with the fused 3x3 convolution + BatchNorm layers
(prepare_inference(fuse_convbn=), csrc/convbn.hip) off and on.  The off arm is the code path without the switch.

    python tools/bench_infer.py --model r18 --convbn [--quick] [--reps 3]

--model r18 --layers: per-layer figures of that kernel, CACHE-WARM MICRO-BENCHMARKS (one layer in a loop on the same
tensors: its operands stay in L2 / Infinity Cache, which is not where a layer finds them inside a network): the fused call
against tsg_conv3x3_gen_fwd + tsg_bn_apply_fwd (with the shortcut and ReLU) at the four backbone stage shapes of
BiSeNet-R18 for a 768 x 1536 image, off / on alternated `--reps` times, every timing a window of >= 0.25 s between two
device events.

    python tools/bench_infer.py --model r18 --layers [--reps 3]

--model r18|r50 --pwbn: the arm table for the fused 1x1 convolution + BatchNorm layers (prepare_inference(fuse_pointwise=),
csrc/pwbn.hip) off and on, with fuse_convbn=True in every one of our arms.  --model r50 is the ResNet-50 backbone alone
(base_model.resnet50(None, norm_layer=nn.BatchNorm2d)); a call computes its four stage outputs.

    python tools/bench_infer.py --model r50 --pwbn [--quick] [--reps 3]

--pwlayers: per-layer figures of that kernel, CACHE-WARM MICRO-BENCHMARKS as under --layers: the fused call against the
two launches of the unfused inference path (the vendor library's 1x1 convolution + tsg_bn_apply_fwd with the shortcut and
ReLU) at 1x1 layer shapes of ResNet-50 and BiSeNet-R18 for a 768 x 1536 image.

    python tools/bench_infer.py --pwlayers [--reps 3]

--model r50 --dilbn: the arm table for the fused DILATED 3x3 convolution + BatchNorm layers
(prepare_inference(fuse_dilated=), csrc/dilbn.hip) off and on, with fuse_convbn=True and fuse_pointwise=True in every one
of our arms.  The network is the dilated ResNet-50-v1c backbone of PSPNet / PSANet (deep stem of width 64, layer3 / layer4
at stride 1 and dilation 2 / 4); a call computes its four stage outputs.  The off arm is the code path without the switch.

    python tools/bench_infer.py --model r50 --dilbn [--quick] [--reps 3]

--dillayers: per-layer figures of that kernel, CACHE-WARM MICRO-BENCHMARKS as under --layers, at the three layer shapes of
the 96 x 192 map (256 -> 256 at dilation 2, 512 -> 512 at 2 and at 4): (a) the vendor library's convolution +
tsg_bn_apply_fwd, (b) tsg_conv3x3_dil_fwd + tsg_bn_apply_fwd, (c) the fused call, the three alternated.

    python tools/bench_infer.py --dillayers [--reps 3]

--model r18|r50 --s2bn: the arm table for the fused STRIDE-2 3x3 convolution + BatchNorm layers
(prepare_inference(fuse_strided=), csrc/s2bn.hip) off and on, with fuse_convbn=True and fuse_pointwise=True in every one of
our arms (5 layers in BiSeNet-R18, 3 in the ResNet-50 backbone).  The off arm is the code path without the switch.

    python tools/bench_infer.py --model r18 --s2bn [--quick] [--reps 3]

--s2layers: per-layer figures of that kernel, CACHE-WARM MICRO-BENCHMARKS as under --layers, at the stride-2 layer shapes of
BiSeNet-R18 and ResNet-50 for a 768 x 1536 image and the detail branch's two layers for 1024 x 2048: (a) the vendor
library's convolution + tsg_bn_apply_fwd (the inference path without the switch), (b) for 64 -> 64 tsg_conv3x3_c64_s2_fwd +
tsg_bn_apply_fwd, (c) the fused call, alternated.

    python tools/bench_infer.py --s2layers [--reps 3]

--model r18|r50 --stembn: the arm table for the fused image stems and deep stem (prepare_inference(fuse_stem=),
torchseg_amd/stembn.py) off and on, with every other fusion (fuse_convbn, fuse_dilated, fuse_strided, fuse_pointwise) on in
every one of our arms: 1 layer in BiSeNet-R18 (SpatialPath.conv_7x7), 3 in the dilated ResNet-50-v1c backbone (`--model
r50` is that backbone here, as under --dilbn).  The off arm is the code path without the switch.

    python tools/bench_infer.py --model r50 --stembn [--quick] [--reps 3]

--stemlayers: per-layer figures, CACHE-WARM MICRO-BENCHMARKS as under --layers, for the 384 x 768 and 512 x 1024 maps
(images of 768 x 1536 and 1024 x 2048).  The two image layers: (a) the vendor library's convolution + tsg_bn_apply_fwd
(3x3 only: the 7x7 never runs there), (b) tsg_stem3_conv_fwd / tsg_stem_conv_fwd + tsg_bn_apply_fwd, (c) the fused call.
The two inner deep-stem layers (64 -> 64, 64 -> 128): the vendor library's convolution + tsg_bn_apply_fwd against
tsg_conv3x3_bnact_fwd.

    python tools/bench_infer.py --stemlayers [--reps 3]

--model psp --ppmbn: the arm table of the WHOLE PSPNet-R50 (workloads.pspnet.PSPNet, 19 classes, eval form: backbone,
pyramid pooling head, classifier, the up-sampled log-probabilities materialised) with the concat-free pyramid pooling head
(prepare_inference(fuse_pyramid=), csrc/ppmbn.hip) off and on, every other fusion (fuse_convbn, fuse_dilated, fuse_strided,
fuse_pointwise, fuse_stem) on in every one of our arms.  The off arm is the code path without the switch.

    python tools/bench_infer.py --model psp --ppmbn [--quick] [--reps 3]

--ppmlayers: per-head figures, CACHE-WARM MICRO-BENCHMARKS as under --layers, at B = 1 on the 60 x 60, 96 x 192 and 128 x 256
maps with C = 2048, from the four pooled maps on: (s) the stock head as a network runs it (four bilinear up-samplings +
torch.cat + a 4096 -> 512 3x3 ConvBnRelu module behind prepare_inference(fuse_convbn=True), on whatever path its gate takes)
and (a) the same chain with tsg_conv3x3_bnact_fwd called on the concatenated tensor made channels_last (that convolution alone
beside it) against (b) tsg_ppm_taps_fwd + tsg_ppm_addend_fwd + tsg_conv3x3_bnact_add_fwd, and the three stages of (b) alone.

    python tools/bench_infer.py --ppmlayers [--reps 3]
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


def r50():
    from base_model.resnet import resnet50
    torch.manual_seed(0)
    return resnet50(None, norm_layer=nn.BatchNorm2d).eval()


def r50d():
    """the backbone of PSPNet / PSANet: ResNet-50-v1c (deep stem) with layer3 / layer4 at stride 1, dilation 2 / 4"""
    from functools import partial
    from base_model.resnet import resnet50
    from torchseg_amd.workloads.pspnet import _nostride_dilate
    torch.manual_seed(0)
    net = resnet50(None, norm_layer=nn.BatchNorm2d, deep_stem=True, stem_width=64)
    net.layer3.apply(partial(_nostride_dilate, dilate=2))
    net.layer4.apply(partial(_nostride_dilate, dilate=4))
    return net.eval()


def psp():
    """the whole PSPNet-R50: dilated ResNet-50-v1c backbone, pyramid pooling head, classifier"""
    from torchseg_amd.workloads.pspnet import PSPNet
    torch.manual_seed(0)
    return PSPNet(19, None, None, nn.BatchNorm2d, depth=50).eval()


def x39():
    from torchseg_amd.workloads.bisenet_x39 import BiSeNetX39
    torch.manual_seed(0)
    return BiSeNetX39(19, False, None, None, pretrained_model=None, norm_layer=nn.BatchNorm2d).eval()


ARM_RES = ((768, 1536), (1024, 2048))
ARMS = ("stock_fp32", "eager_bf16_off", "eager_bf16_on", "graph_bf16_off", "graph_bf16_on")


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


# table -> (builder, title, prepare_inference's switch, attribute with the installed count, that count, module of fused_calls,
#           what every one of our arms is prepared with besides)
EVERY_OTHER = {"fuse_convbn": True, "fuse_dilated": True, "fuse_strided": True, "fuse_pointwise": True}
ARM_MODELS = {"x39": (x39, "BiSeNet-X39", "fuse_separable", "fused_separable", 51, "sepconv", {}),
              "r18": (r18, "BiSeNet-R18", "fuse_convbn", "fused_convbn", 20, "convbn", {}),
              "r18+pwbn": (r18, "BiSeNet-R18, fuse_convbn=True", "fuse_pointwise", "fused_pointwise", 8, "pwbn",
                           {"fuse_convbn": True}),
              "r50+pwbn": (r50, "ResNet-50 backbone, fuse_convbn=True", "fuse_pointwise", "fused_pointwise", 36, "pwbn",
                           {"fuse_convbn": True}),
              "r50+dilbn": (r50d, "dilated ResNet-50-v1c backbone, fuse_convbn=True, fuse_pointwise=True", "fuse_dilated",
                            "fused_dilated", 8, "convbn:dil_fused_calls", {"fuse_convbn": True, "fuse_pointwise": True}),
              "r18+s2bn": (r18, "BiSeNet-R18, fuse_convbn=True, fuse_pointwise=True", "fuse_strided", "fused_strided", 5,
                           "convbn:s2_fused_calls", {"fuse_convbn": True, "fuse_pointwise": True}),
              "r50+s2bn": (r50, "ResNet-50 backbone, fuse_convbn=True, fuse_pointwise=True", "fuse_strided", "fused_strided", 3,
                           "convbn:s2_fused_calls", {"fuse_convbn": True, "fuse_pointwise": True}),
              "r18+stembn": (r18, "BiSeNet-R18, every other fusion on", "fuse_stem", "fused_stem", 1, "stembn", EVERY_OTHER),
              "r50+stembn": (r50d, "dilated ResNet-50-v1c backbone, every other fusion on", "fuse_stem", "fused_stem", 3,
                             "stembn", EVERY_OTHER),
              "psp+ppmbn": (psp, "PSPNet-R50 (the whole network), every other fusion on", "fuse_pyramid", "fused_pyramid", 1,
                            "ppmbn:pyramid_fused_calls", dict(EVERY_OTHER, fuse_stem=True))}


def arm_times(arm, iters, warmup, model="x39"):
    """one arm in this (child) process -> {"HxW": median ms, ...}"""
    import importlib
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    build, _, switch, counter, count, where, fixed = ARM_MODELS[model]
    where, _, counter_fn = where.partition(":")
    fused_calls = getattr(importlib.import_module("torchseg_amd." + where), counter_fn or "fused_calls")
    dev = torch.device("cuda:0")
    net = build().to(dev)
    if arm == "stock_fp32":
        def run(x):
            with torch.no_grad():
                return net(x)
    else:
        prep = prepare_inference(net, dtype=torch.bfloat16, graph=arm.startswith("graph"), **{switch: arm.endswith("_on")},
                                 **fixed)
        assert getattr(prep, counter) == (count if arm.endswith("_on") else 0)
        tensor_out = build not in (r50, r50d)             # the backbone returns its four stage outputs, all computed
        run = (lambda x: prep(x)) if prep.graph or not tensor_out else (lambda x: materialize(prep(x)))
    out = {}
    for res in ARM_RES:
        x = torch.randn(1, 3, *res, device=dev)
        out["%dx%d" % res] = float(np.median(event_times(lambda: run(x), iters, warmup)))
    if arm.endswith("_on"):
        assert fused_calls(prep.module) > 0
    return out


def arm_table(iters, warmup, reps, model="x39"):
    import subprocess
    title = ARM_MODELS[model][1]

    def child(arm):
        cmd = [sys.executable, os.path.abspath(__file__), "--model", model.split("+")[0], "--arm", arm, "--iters", str(iters),
               "--warmup", str(warmup)] + (["--" + model.split("+")[1]] if "+" in model else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("arm %s failed (%d):\n%s\n%s" % (arm, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
        print("%s: %s" % (arm, r.stdout.strip().splitlines()[-1]), file=sys.stderr, flush=True)
        return json.loads(r.stdout.strip().splitlines()[-1])

    runs = {arm: [] for arm in ARMS}
    runs["stock_fp32"].append(child("stock_fp32"))
    for _ in range(reps):                                   # off and on alternate
        for arm in ("graph_bf16_off", "graph_bf16_on", "eager_bf16_off", "eager_bf16_on"):
            runs[arm].append(child(arm))
    result = {"device": torch.cuda.get_device_name(0), "model": title, "iters": iters, "warmup": warmup,
              "reps": reps, "runs_ms": runs}
    print("%s forward, batch 1, ms per call: median over %d child processes (min-max); %d timed calls per child, "
          "device events" % (title, reps, iters))
    print("%-16s %-28s %-28s" % ("arm", "1x3x768x1536", "1x3x1024x2048"))
    summary = {}
    for arm in ARMS:
        cells = []
        for res in ARM_RES:
            v = [r["%dx%d" % res] for r in runs[arm]]
            med = float(np.median(v))
            summary.setdefault(arm, {})["%dx%d" % res] = dict(median_ms=med, min_ms=min(v), max_ms=max(v),
                                                               spread=(max(v) - min(v)) / med)
            cells.append("%.3f (%.3f-%.3f)" % (med, min(v), max(v)))
        print("%-16s %-28s %-28s" % (arm, cells[0], cells[1]))
    for kind in ("graph", "eager"):
        for res in ARM_RES:
            k = "%dx%d" % res
            off, on = summary[kind + "_bf16_off"][k], summary[kind + "_bf16_on"][k]
            gain = 1.0 - on["median_ms"] / off["median_ms"]
            print("%s %s: fused / unfused = %.3f (%+.1f %% time); spread of the off arm against itself %.1f %%: %s"
                  % (kind, k, on["median_ms"] / off["median_ms"], -100.0 * gain, 100.0 * off["spread"],
                     "beyond the spread" if abs(gain) > off["spread"] else "WITHIN the spread (no difference shown)"))
    result["summary"] = summary
    print(json.dumps(result))


R18_LAYERS = ((192, 384, 64), (96, 192, 128), (48, 96, 256), (24, 48, 512))      # (H, W, C) of layer1-4 at 768 x 1536


def window_ms(fn, min_s=0.25):
    """ms per call of fn over one window of at least `min_s` seconds between two device events"""
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    while True:
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 1e3 * min_s:
            return ms / n
        n = int(n * max(2.0, 1.2e3 * min_s / max(ms, 1e-3)))


GRAPH_CALLS = 20


def graphed(fn):
    """GRAPH_CALLS calls of fn captured in one graph -> its replay"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            fn()
    return g.replay


def r18_layers(reps):
    """the block tail conv3x3 -> BatchNorm -> + shortcut -> ReLU at BiSeNet-R18's four stage shapes: two launches against one"""
    from torchseg_amd import _lib as L, kernels as K
    kp = K.provider()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    CL = torch.channels_last
    rows = []
    print("CACHE-WARM MICRO-BENCHMARKS: one layer in a loop on the same tensors (%d calls per graph replay), us per call, median "
          "of %d windows of >= 0.25 s (min-max), unfused / fused alternated" % (GRAPH_CALLS, reps))
    print("%-22s %-30s %-30s %s" % ("layer (B x H x W x C)", "gen_fwd + bn_apply_fwd", "conv3x3_bnact_fwd", "fused / unfused"))
    for H, W, Cc in R18_LAYERS:
        x = torch.randn(1, Cc, H, W, generator=g).to(dev).bfloat16().contiguous(memory_format=CL)
        res = torch.randn(1, Cc, H, W, generator=g).to(dev).bfloat16().contiguous(memory_format=CL)
        w = (torch.randn(Cc, Cc, 3, 3, generator=g) * (2.0 / (9 * Cc)) ** 0.5).to(dev).contiguous(memory_format=CL)
        fp = torch.stack([0.5 + torch.rand(Cc, generator=g), torch.randn(Cc, generator=g), torch.zeros(Cc)]).to(dev)
        wf = kp.conv3x3_gen_prep_filter(w, 0, x)
        pack = kp.conv3x3_bnact_pack(w, None, fp)
        y = torch.empty_like(x)

        def unfused():
            t = kp.conv3x3_gen_fwd(x, wf, Cc)
            return kp.bn_apply_fwd(t, res, L.NHWC, 1, Cc, H * W, fp, True, out=y)

        def fused():
            return kp.conv3x3_bnact_fwd(x, pack, Cc, res, True)

        d = (unfused().float() - fused().float()).abs().max().item()
        gu, gf = graphed(unfused), graphed(fused)          # GRAPH_CALLS launches per replay: no host time between kernels
        tu, tf = [], []
        for _ in range(reps):
            tu.append(1e3 * window_ms(gu) / GRAPH_CALLS)
            tf.append(1e3 * window_ms(gf) / GRAPH_CALLS)
        mu, mf = float(np.median(tu)), float(np.median(tf))
        rows.append(dict(H=H, W=W, C=Cc, unfused_us=tu, fused_us=tf, max_abs_diff=d,
                         gen_variant=kp.conv3x3_gen_variant(1, H, W, Cc, Cc)))
        print("%-22s %-30s %-30s %.3f" % ("1x%dx%dx%d" % (H, W, Cc), "%.1f (%.1f-%.1f)" % (mu, min(tu), max(tu)),
                                          "%.1f (%.1f-%.1f)" % (mf, min(tf), max(tf)), mf / mu))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "layers": rows}))


# (H, W, C_in, C_out, stride, shortcut, ReLU) at 768 x 1536: ResNet-50's conv1 / conv3 / downsample of each stage, the dilated
# networks' 2048 -> 512 reduction on the 1/8 map, BiSeNet-R18's three shortcuts and ffm.conv_1x1
PW_LAYERS = ((192, 384, 64, 64, 1, False, True), (192, 384, 64, 256, 1, True, True), (192, 384, 256, 64, 1, False, True),
             (192, 384, 256, 512, 2, False, False), (96, 192, 512, 128, 1, False, True), (96, 192, 128, 512, 1, True, True),
             (96, 192, 512, 1024, 2, False, False), (48, 96, 1024, 256, 1, False, True), (48, 96, 256, 1024, 1, True, True),
             (48, 96, 1024, 2048, 2, False, False), (24, 48, 2048, 512, 1, False, True), (24, 48, 512, 2048, 1, True, True),
             (96, 192, 2048, 512, 1, False, True), (192, 384, 64, 128, 2, False, False), (96, 192, 128, 256, 2, False, False),
             (48, 96, 256, 512, 2, False, False), (96, 192, 256, 256, 1, False, True))


def pw_layers(reps):
    """conv1x1 -> BatchNorm (-> + shortcut) (-> ReLU): the vendor library's convolution + tsg_bn_apply_fwd against one launch"""
    from torchseg_amd import _lib as L, kernels as K
    kp = K.provider()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    CL = torch.channels_last
    rows = []
    print("CACHE-WARM MICRO-BENCHMARKS: one layer in a loop on the same tensors (%d calls per graph replay), us per call, median "
          "of %d windows of >= 0.25 s (min-max), unfused / fused alternated" % (GRAPH_CALLS, reps))
    print("%-34s %-30s %-30s %-10s %s" % ("layer (H x W, Cin -> Cout / s)", "conv2d + bn_apply_fwd", "conv1x1_bnact_fwd",
                                          "fused/unf.", "model TB/s of the fused call"))
    for H, W, Ci, Co, s, with_res, relu in PW_LAYERS:
        OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
        x = torch.randn(1, Ci, H, W, generator=g).to(dev).bfloat16().contiguous(memory_format=CL)
        res = torch.randn(1, Co, OH, OW, generator=g).to(dev).bfloat16().contiguous(memory_format=CL) if with_res else None
        w = (torch.randn(Co, Ci, 1, 1, generator=g) * (2.0 / Ci) ** 0.5).to(dev)
        wb = w.bfloat16().contiguous(memory_format=CL)
        fp = torch.stack([0.5 + torch.rand(Co, generator=g), torch.randn(Co, generator=g), torch.zeros(Co)]).to(dev)
        pack = kp.conv1x1_bnact_pack(w, None, fp)
        y = torch.empty((1, Co, OH, OW), dtype=torch.bfloat16, device=dev, memory_format=CL)

        def unfused():
            t = F.conv2d(x, wb, None, s)
            return kp.bn_apply_fwd(t, res, L.NHWC, 1, Co, OH * OW, fp, relu, out=y)

        def fused():
            return kp.conv1x1_bnact_fwd(x, pack, Co, s, res, relu)

        d = (unfused().float() - fused().float()).abs().max().item()
        gu, gf = graphed(unfused), graphed(fused)          # GRAPH_CALLS launches per replay: no host time between kernels
        tu, tf = [], []
        for _ in range(reps):
            tu.append(1e3 * window_ms(gu) / GRAPH_CALLS)
            tf.append(1e3 * window_ms(gf) / GRAPH_CALLS)
        mu, mf = float(np.median(tu)), float(np.median(tf))
        # the compulsory bytes of DESIGN.md 7's model: the pixels x reads, the residual, y and the filter, once each (the
        # Cout / 64 re-reads of x and the per-tile re-reads of the filter are meant to come from L2)
        nbytes = 2 * (OH * OW * Ci + OH * OW * Co * (2 if with_res else 1) + Ci * Co)
        rows.append(dict(H=H, W=W, Cin=Ci, Cout=Co, stride=s, residual=with_res, relu=relu, unfused_us=tu, fused_us=tf,
                         max_abs_diff=d, model_bytes=nbytes, plan=kp.conv1x1_bnact_plan(1, H, W, Ci, Co, s)))
        print("%-34s %-30s %-30s %-10.3f %.2f" % ("%dx%d, %d -> %d / %d%s" % (H, W, Ci, Co, s, " + res" if with_res else ""),
                                                  "%.1f (%.1f-%.1f)" % (mu, min(tu), max(tu)),
                                                  "%.1f (%.1f-%.1f)" % (mf, min(tf), max(tf)), mf / mu, nbytes / mf / 1e6))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "layers": rows}))


# (H, W, C, dilation): the middle convolutions of the layer3 / layer4 Bottlenecks of the dilated ResNet-50 / -101 on the 1/8 map
# of a 768 x 1536 image (5 / 22 layers, 1 layer, 2 layers)
DIL_LAYERS = ((96, 192, 256, 2), (96, 192, 512, 2), (96, 192, 512, 4))


def dil_layers(reps):
    """dilated conv3x3 -> BatchNorm -> ReLU: (a) the vendor library's convolution + tsg_bn_apply_fwd (the default inference
    path), (b) tsg_conv3x3_dil_fwd + tsg_bn_apply_fwd (TSG_CONV_DIL=1), (c) one launch"""
    from torchseg_amd import _lib as L, kernels as K
    kp = K.provider()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    CL = torch.channels_last
    rows = []
    print("CACHE-WARM MICRO-BENCHMARKS: one layer in a loop on the same tensors (%d calls per graph replay), us per call, median "
          "of %d windows of >= 0.25 s (min-max), the three variants alternated" % (GRAPH_CALLS, reps))
    print("%-26s %-26s %-26s %-26s %-8s %-8s %s" % ("layer (H x W, C -> C, d)", "(a) conv2d + bn_apply", "(b) dil_fwd + bn_apply",
                                                     "(c) conv3x3_dil_bnact_fwd", "c / a", "c / b", "model TB/s of (c)"))
    for H, W, Cc, d in DIL_LAYERS:
        x = torch.randn(1, Cc, H, W, generator=g).to(dev).bfloat16().contiguous(memory_format=CL)
        w = (torch.randn(Cc, Cc, 3, 3, generator=g) * (2.0 / (9 * Cc)) ** 0.5).to(dev).contiguous(memory_format=CL)
        wb = w.bfloat16().contiguous(memory_format=CL)
        fp = torch.stack([0.5 + torch.rand(Cc, generator=g), torch.randn(Cc, generator=g), torch.zeros(Cc)]).to(dev)
        wf = kp.conv3x3_dil_prep_filter(w, 0, x)
        pack = kp.conv3x3_bnact_pack(w, None, fp)
        y = torch.empty_like(x)

        def vendor():
            t = F.conv2d(x, wb, None, 1, d, d)
            return kp.bn_apply_fwd(t, None, L.NHWC, 1, Cc, H * W, fp, True, out=y)

        def ours():
            t = kp.conv3x3_dil_fwd(x, wf, Cc, d)
            return kp.bn_apply_fwd(t, None, L.NHWC, 1, Cc, H * W, fp, True, out=y)

        def fused():
            return kp.conv3x3_dil_bnact_fwd(x, pack, Cc, d, None, True)

        ref = fused().float()
        da, db = (vendor().float() - ref).abs().max().item(), (ours().float() - ref).abs().max().item()
        ga, gb, gc = graphed(vendor), graphed(ours), graphed(fused)     # GRAPH_CALLS launches per replay
        ta, tb, tc = [], [], []
        for _ in range(reps):
            ta.append(1e3 * window_ms(ga) / GRAPH_CALLS)
            tb.append(1e3 * window_ms(gb) / GRAPH_CALLS)
            tc.append(1e3 * window_ms(gc) / GRAPH_CALLS)
        ma, mb, mc = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
        # the compulsory bytes of DESIGN.md 7's model: x, y and the filter once each (the Cout / 64 re-reads of x, the halo
        # and the per-tile re-reads of the filter are meant to come from L2)
        nbytes = 2 * (H * W * Cc * 2 + 9 * Cc * Cc)
        rows.append(dict(H=H, W=W, C=Cc, dilation=d, vendor_us=ta, dil_fwd_us=tb, fused_us=tc, max_abs_diff_vendor=da,
                         max_abs_diff_dil_fwd=db, model_bytes=nbytes, plan=kp.conv3x3_dil_bnact_plan(1, H, W, Cc, Cc, d)))
        cell = lambda m, t: "%.1f (%.1f-%.1f)" % (m, min(t), max(t))
        print("%-26s %-26s %-26s %-26s %-8.3f %-8.3f %.2f" % ("%dx%d, %d -> %d, d %d" % (H, W, Cc, Cc, d), cell(ma, ta), cell(mb, tb),
                                                            cell(mc, tc), mc / ma, mc / mb, nbytes / mc / 1e6))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "layers": rows}))


# (H, W, C_in, C_out, image) of the INPUT: the detail branch's two layers and layer2 / 3 / 4's first conv1 of BiSeNet-R18, the
# first conv2 of layer2 / 3 / 4 of ResNet-50, for a 768 x 1536 image; the detail branch's two layers for 1024 x 2048
S2_LAYERS = ((384, 768, 64, 64, "768x1536"), (192, 384, 64, 64, "768x1536"), (192, 384, 64, 128, "768x1536"),
             (96, 192, 128, 256, "768x1536"), (48, 96, 256, 512, "768x1536"), (192, 384, 128, 128, "768x1536"),
             (96, 192, 256, 256, "768x1536"), (48, 96, 512, 512, "768x1536"), (512, 1024, 64, 64, "1024x2048"),
             (256, 512, 64, 64, "1024x2048"))


def s2_layers(reps):
    """stride-2 conv3x3 -> BatchNorm -> ReLU: (a) the vendor library's convolution + tsg_bn_apply_fwd (the inference path
    without the switch), (b) 64 -> 64 only: tsg_conv3x3_c64_s2_fwd + tsg_bn_apply_fwd, (c) one launch"""
    from torchseg_amd import _lib as L, kernels as K
    kp = K.provider()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    CL = torch.channels_last
    rows = []
    print("CACHE-WARM MICRO-BENCHMARKS: one layer in a loop on the same tensors (%d calls per graph replay), us per call, median "
          "of %d windows of >= 0.25 s (min-max), the variants alternated" % (GRAPH_CALLS, reps))
    print("%-36s %-26s %-26s %-26s %-8s %-8s %s" % ("layer (input H x W, Cin -> Cout; image)", "(a) conv2d + bn_apply",
                                                     "(b) c64_s2_fwd + bn_apply", "(c) conv3x3_s2_bnact_fwd", "c / a", "c / b",
                                                     "model TB/s of (c)"))
    for H, W, Ci, Co, image in S2_LAYERS:
        OH, OW = (H + 1) // 2, (W + 1) // 2
        x = torch.randn(1, Ci, H, W, generator=g).to(dev).bfloat16().contiguous(memory_format=CL)
        w = (torch.randn(Co, Ci, 3, 3, generator=g) * (2.0 / (9 * Ci)) ** 0.5).to(dev).contiguous(memory_format=CL)
        wb = w.bfloat16().contiguous(memory_format=CL)
        fp = torch.stack([0.5 + torch.rand(Co, generator=g), torch.randn(Co, generator=g), torch.zeros(Co)]).to(dev)
        pack = kp.conv3x3_bnact_pack(w, None, fp)
        y = torch.empty((1, Co, OH, OW), dtype=torch.bfloat16, device=dev, memory_format=CL)
        c64 = Ci == 64 and Co == 64

        def vendor():
            t = F.conv2d(x, wb, None, 2, 1)
            return kp.bn_apply_fwd(t, None, L.NHWC, 1, Co, OH * OW, fp, True, out=y)

        def ours():
            t = kp.conv3x3_c64_fwd(x, wb, stride=2)
            return kp.bn_apply_fwd(t, None, L.NHWC, 1, Co, OH * OW, fp, True, out=y)

        def fused():
            return kp.conv3x3_s2_bnact_fwd(x, pack, Co, None, True)

        ref = fused().float()
        da = (vendor().float() - ref).abs().max().item()
        db = (ours().float() - ref).abs().max().item() if c64 else None
        ga, gb, gc = graphed(vendor), graphed(ours) if c64 else None, graphed(fused)    # GRAPH_CALLS launches per replay
        ta, tb, tc = [], [], []
        for _ in range(reps):
            ta.append(1e3 * window_ms(ga) / GRAPH_CALLS)
            if c64:
                tb.append(1e3 * window_ms(gb) / GRAPH_CALLS)
            tc.append(1e3 * window_ms(gc) / GRAPH_CALLS)
        ma, mc = float(np.median(ta)), float(np.median(tc))
        mb = float(np.median(tb)) if c64 else None
        # the compulsory bytes of DESIGN.md 7's model: x, y and the filter once each (the Cout / 64 re-reads of x, the halo
        # and the per-tile re-reads of the filter are meant to come from L2)
        nbytes = 2 * (H * W * Ci + OH * OW * Co + 9 * Ci * Co)
        rows.append(dict(H=H, W=W, Cin=Ci, Cout=Co, image=image, vendor_us=ta, c64_s2_fwd_us=tb, fused_us=tc,
                         max_abs_diff_vendor=da, max_abs_diff_c64_s2_fwd=db, model_bytes=nbytes,
                         plan=kp.conv3x3_s2_bnact_plan(1, H, W, Ci, Co)))
        cell = lambda m, t: "%.1f (%.1f-%.1f)" % (m, min(t), max(t)) if t else "-"
        print("%-36s %-26s %-26s %-26s %-8.3f %-8s %.2f" % ("%dx%d, %d -> %d; %s" % (H, W, Ci, Co, image), cell(ma, ta), cell(mb, tb),
                                                             cell(mc, tc), mc / ma, "%.3f" % (mc / mb) if c64 else "-",
                                                             nbytes / mc / 1e6))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "layers": rows}))


STEM_MAPS = ((768, 1536), (1024, 2048))              # the IMAGE; the stem's maps are 384 x 768 and 512 x 1024


def stem_layers(reps):
    """the image layers: (a) the vendor convolution + tsg_bn_apply_fwd (3x3 only), (b) tsg_stem*_conv_fwd + tsg_bn_apply_fwd,
    (c) one launch; the two inner deep-stem layers: the vendor convolution + tsg_bn_apply_fwd against one launch"""
    from torchseg_amd import _lib as L, kernels as K
    kp = K.provider()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    CL = torch.channels_last
    rows = []
    cell = lambda t: "%.1f (%.1f-%.1f)" % (float(np.median(t)), min(t), max(t)) if t else "-"
    print("CACHE-WARM MICRO-BENCHMARKS: one layer in a loop on the same tensors (%d calls per graph replay), us per call, median "
          "of %d windows of >= 0.25 s (min-max), the variants alternated" % (GRAPH_CALLS, reps))
    print("%-40s %-26s %-26s %-26s %-8s %-8s %s" % ("layer (image H x W or input map, Cin -> Cout)", "(a) conv2d + bn_apply",
                                                     "(b) stem*_conv_fwd + bn_apply", "(c) fused", "c / a", "c / b",
                                                     "model TB/s of (c)"))
    for H, W in STEM_MAPS:
        OH, OW = H // 2, W // 2
        img = torch.randn(1, 3, H, W, generator=g).to(dev).bfloat16().contiguous()
        y = torch.empty((1, 64, OH, OW), dtype=torch.bfloat16, device=dev, memory_format=CL)
        fp = torch.stack([0.5 + torch.rand(64, generator=g), torch.randn(64, generator=g), torch.zeros(64)]).to(dev)
        for k in (3, 7):
            w = (torch.randn(64, 3, k, k, generator=g) * (2.0 / (3 * k * k)) ** 0.5).to(dev)
            wb = w.bfloat16()
            pack = kp.image_bnact_pack(w, fp)
            unfused = kp.stem3_conv_fwd if k == 3 else kp.stem_conv_fwd

            def vendor():
                t = F.conv2d(img, wb, None, 2, k // 2).contiguous(memory_format=CL)
                return kp.bn_apply_fwd(t, None, L.NHWC, 1, 64, OH * OW, fp, True, out=y)

            def ours():
                return kp.bn_apply_fwd(unfused(img, w), None, L.NHWC, 1, 64, OH * OW, fp, True, out=y)

            def fused():
                return kp.image_bnact_fwd(img, pack, k, True)

            ref = fused().float()
            db = (ours().float() - ref).abs().max().item()
            da = (vendor().float() - ref).abs().max().item() if k == 3 else None
            ga, gb, gc = graphed(vendor) if k == 3 else None, graphed(ours), graphed(fused)
            ta, tb, tc = [], [], []
            for _ in range(reps):
                if k == 3:
                    ta.append(1e3 * window_ms(ga) / GRAPH_CALLS)
                tb.append(1e3 * window_ms(gb) / GRAPH_CALLS)
                tc.append(1e3 * window_ms(gc) / GRAPH_CALLS)
            mb, mc = float(np.median(tb)), float(np.median(tc))
            nbytes = 2 * (3 * H * W + OH * OW * 64)            # the image once, y once
            rows.append(dict(layer="image %dx%d" % (k, k), H=H, W=W, vendor_us=ta, unfused_us=tb, fused_us=tc,
                             max_abs_diff_vendor=da, max_abs_diff_unfused=db, model_bytes=nbytes))
            print("%-40s %-26s %-26s %-26s %-8s %-8.3f %.2f" % ("image %dx%d, 3 -> 64 %dx%d / 2" % (H, W, k, k), cell(ta), cell(tb),
                                                                 cell(tc), "%.3f" % (mc / float(np.median(ta))) if ta else "-",
                                                                 mc / mb, nbytes / mc / 1e6))
        for Ci, Co in ((64, 64), (64, 128)):
            x = torch.randn(1, Ci, OH, OW, generator=g).to(dev).bfloat16().contiguous(memory_format=CL)
            w = (torch.randn(Co, Ci, 3, 3, generator=g) * (2.0 / (9 * Ci)) ** 0.5).to(dev).contiguous(memory_format=CL)
            wb = w.bfloat16().contiguous(memory_format=CL)
            fpi = torch.stack([0.5 + torch.rand(Co, generator=g), torch.randn(Co, generator=g), torch.zeros(Co)]).to(dev)
            pack = kp.conv3x3_bnact_pack(w, None, fpi)
            yi = torch.empty((1, Co, OH, OW), dtype=torch.bfloat16, device=dev, memory_format=CL)

            def vendor():
                return kp.bn_apply_fwd(F.conv2d(x, wb, None, 1, 1), None, L.NHWC, 1, Co, OH * OW, fpi, True, out=yi)

            def fused():
                return kp.conv3x3_bnact_fwd(x, pack, Co, None, True)

            da = (vendor().float() - fused().float()).abs().max().item()
            ga, gc = graphed(vendor), graphed(fused)
            ta, tc = [], []
            for _ in range(reps):
                ta.append(1e3 * window_ms(ga) / GRAPH_CALLS)
                tc.append(1e3 * window_ms(gc) / GRAPH_CALLS)
            mc = float(np.median(tc))
            nbytes = 2 * (OH * OW * (Ci + Co) + 9 * Ci * Co)
            rows.append(dict(layer="inner 3x3", H=OH, W=OW, Cin=Ci, Cout=Co, vendor_us=ta, fused_us=tc, max_abs_diff_vendor=da,
                             model_bytes=nbytes))
            print("%-40s %-26s %-26s %-26s %-8.3f %-8s %.2f" % ("map %dx%d, %d -> %d 3x3 / 1" % (OH, OW, Ci, Co), cell(ta), "-",
                                                                 cell(tc), mc / float(np.median(ta)), "-", nbytes / mc / 1e6))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "layers": rows}))


PPM_HEADS = ((60, 60), (96, 192), (128, 256))              # the 1/8 map of ADE's 480 x 480 crop, of 768 x 1536, of 1024 x 2048
PPM_SCALES = (1, 2, 3, 6)


def ppm_layers(reps):
    """PSPNet's head at B = 1, C = 2048, 4 x 512 pooled channels, 512 outputs, from the pooled maps on: (a) today's chain,
    four bilinear up-samplings + torch.cat + tsg_conv3x3_bnact_fwd over 4096 channels, against (b) the three launches of
    csrc/ppmbn.hip, and those three on their own; (s) is the stock head as a network runs it today: the same up-samplings and
    torch.cat, then a 4096 -> 512 3x3 ConvBnRelu module behind prepare_inference(fuse_convbn=True), which takes whatever
    path its gate gives it for the concatenated tensor (the row says how many of its calls were tsg_conv3x3_bnact_fwd)"""
    from seg_opr.seg_oprs import ConvBnRelu
    from torchseg_amd import convbn, kernels as K
    from torchseg_amd.infer import prepare_inference
    from torchseg_amd.upsample import install_aten_overrides
    install_aten_overrides()
    kp = K.provider()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    CL = torch.channels_last
    C, Cb, Cout, n = 2048, 512, 512, len(PPM_SCALES)
    maps = [(s, s) for s in PPM_SCALES]
    rows = []
    print("CACHE-WARM MICRO-BENCHMARKS: one head in a loop on the same tensors (%d calls per graph replay), us per call, median "
          "of %d windows of >= 0.25 s (min-max), the variants alternated" % (GRAPH_CALLS, reps))
    print("%-10s %-26s %-24s %-24s %-24s %-20s %-20s %-24s %-8s %-8s %s"
          % ("map", "(s) 4 up + cat + ConvBnRelu", "(a) 4 up + cat + conv4096", "conv4096 of (a) alone", "(b) taps+addend+conv_add",
             "ppm_taps_fwd", "ppm_addend_fwd", "conv3x3_bnact_add_fwd", "b / s", "b / a", "addend stages / conv_add"))
    torch.manual_seed(0)
    stock_head = prepare_inference(ConvBnRelu(C + n * Cb, Cout, 3, 1, 1, has_bias=False, norm_layer=nn.BatchNorm2d).to(dev),
                                   dtype=torch.bfloat16, fuse_convbn=True)
    for H, W in PPM_HEADS:
        x = torch.randn(1, C, H, W, generator=g).to(dev).bfloat16().contiguous(memory_format=CL)
        ps = [torch.randn(1, Cb, s, s, generator=g).to(dev).bfloat16().contiguous(memory_format=CL) for s in PPM_SCALES]
        w = (torch.randn(Cout, C + n * Cb, 3, 3, generator=g) * (2.0 / (9 * (C + n * Cb))) ** 0.5).to(dev)
        fp = torch.stack([0.5 + torch.rand(Cout, generator=g), torch.randn(Cout, generator=g), torch.zeros(Cout)]).to(dev)
        pack_all = kp.conv3x3_bnact_pack(w, None, fp)
        pack_x = kp.conv3x3_bnact_pack(w[:, :C], None, fp)
        wb = kp.ppm_pack_branches(w, C, n)
        T, E = kp.ppm_workspace(x, maps, Cb, Cout)
        xcat = torch.cat([x] + [F.interpolate(p, size=(H, W), mode="bilinear", align_corners=True) for p in ps], 1)
        xcat = xcat.contiguous(memory_format=CL)

        def stock():
            cat = torch.cat([x] + [F.interpolate(p, size=(H, W), mode="bilinear", align_corners=True) for p in ps], 1)
            return stock_head(cat)

        def today():
            cat = torch.cat([x] + [F.interpolate(p, size=(H, W), mode="bilinear", align_corners=True) for p in ps], 1)
            return kp.conv3x3_bnact_fwd(cat.contiguous(memory_format=CL), pack_all, Cout, None, True)

        def conv_all():
            return kp.conv3x3_bnact_fwd(xcat, pack_all, Cout, None, True)

        def taps():
            return kp.ppm_taps_fwd(ps, wb, T)

        def addend():
            return kp.ppm_addend_fwd(T, maps, E)

        def conv_add():
            return kp.conv3x3_bnact_add_fwd(x, pack_x, Cout, E, True)

        def ours():
            taps()
            addend()
            return conv_add()

        d = (today().float() - ours().float()).abs().max().item()
        cat = torch.cat([x] + [F.interpolate(p, size=(H, W), mode="bilinear", align_corners=True) for p in ps], 1)
        before = convbn.fused_calls(stock_head.module)
        stock()
        stock_fused = convbn.fused_calls(stock_head.module) - before      # 1: the module's call was tsg_conv3x3_bnact_fwd
        cat_is = dict(dtype=str(cat.dtype), channels_last=cat.is_contiguous(memory_format=CL), nchw=cat.is_contiguous(),
                      aligned16=cat.data_ptr() % 16 == 0)
        fns = (stock, today, conv_all, ours, taps, addend, conv_add)
        graphs = [graphed(f) for f in fns]                             # GRAPH_CALLS launches (or chains) per replay
        times = [[] for _ in fns]
        for _ in range(reps):
            for t, gr in zip(times, graphs):
                t.append(1e3 * window_ms(gr) / GRAPH_CALLS)
        med = [float(np.median(t)) for t in times]
        rows.append(dict(H=H, W=W, C=C, Cb=Cb, Cout=Cout, stock_us=times[0], today_us=times[1], conv4096_us=times[2],
                         ours_us=times[3], taps_us=times[4], addend_us=times[5], conv_add_us=times[6], max_abs_diff=d,
                         stock_module_fused_launches=stock_fused, cat_result=cat_is,
                         plan=kp.ppm_plan(1, H, W, maps, Cb, Cout), conv_plan=kp.conv3x3_bnact_add_plan(1, H, W, C, Cout)))
        cell = lambda m, t: "%.1f (%.1f-%.1f)" % (m, min(t), max(t))
        print("%-10s %-26s %-24s %-24s %-24s %-20s %-20s %-24s %-8.3f %-8.3f %.3f"
              % (("%dx%d" % (H, W),) + tuple(cell(m, t) for m, t in zip(med, times))
                 + (med[3] / med[0], med[3] / med[1], (med[4] + med[5]) / med[6])))
        print("           (s): torch.cat gave %s; %d of the ConvBnRelu module's calls was tsg_conv3x3_bnact_fwd" % (cat_is, stock_fused))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "heads": rows}))


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
    ap.add_argument("--model", choices=("r18", "x39", "r50", "psp"), default="r18")
    ap.add_argument("--reps", type=int, default=3, help="arm tables and --layers: how often off / on alternate")
    ap.add_argument("--arm", choices=ARMS, default=None, help="arm tables: run this one arm here (what a child is started with)")
    ap.add_argument("--convbn", action="store_true", help="r18: the arm table with the fused conv + BatchNorm layers off / on")
    ap.add_argument("--layers", action="store_true", help="r18: per-layer micro-benchmarks of the fused conv + BatchNorm kernel")
    ap.add_argument("--pwbn", action="store_true",
                    help="r18, r50: the arm table with fuse_convbn=True and the fused 1x1 conv + BatchNorm layers off / on")
    ap.add_argument("--pwlayers", action="store_true", help="per-layer micro-benchmarks of the fused 1x1 conv + BatchNorm kernel")
    ap.add_argument("--dilbn", action="store_true",
                    help="r50: the arm table of the DILATED ResNet-50-v1c backbone with fuse_convbn=True, fuse_pointwise=True and "
                         "the fused dilated 3x3 conv + BatchNorm layers off / on")
    ap.add_argument("--dillayers", action="store_true",
                    help="per-layer micro-benchmarks of the fused dilated 3x3 conv + BatchNorm kernel")
    ap.add_argument("--s2bn", action="store_true",
                    help="r18, r50: the arm table with fuse_convbn=True, fuse_pointwise=True and the fused stride-2 3x3 conv + "
                         "BatchNorm layers off / on")
    ap.add_argument("--s2layers", action="store_true",
                    help="per-layer micro-benchmarks of the fused stride-2 3x3 conv + BatchNorm kernel")
    ap.add_argument("--stembn", action="store_true",
                    help="r18, r50 (here the dilated ResNet-50-v1c backbone): the arm table with every other fusion on and the "
                         "fused image stems / deep stem off / on")
    ap.add_argument("--stemlayers", action="store_true",
                    help="per-layer micro-benchmarks of the fused image kernels and of the deep stem's inner layers")
    ap.add_argument("--ppmbn", action="store_true",
                    help="psp: the arm table of the whole PSPNet-R50 with every other fusion on and the concat-free pyramid "
                         "pooling head off / on")
    ap.add_argument("--ppmlayers", action="store_true",
                    help="per-head micro-benchmarks of the pyramid pooling head: today's chain against the three new launches")
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.ppmlayers:
        if sum((a.convbn, a.layers, a.pwbn, a.pwlayers, a.dilbn, a.dillayers, a.s2bn, a.s2layers, a.stembn, a.stemlayers, a.ppmbn)):
            ap.error("--ppmlayers is a measurement of its own: one per call")
        ppm_layers(max(3, a.reps))
        return
    if a.ppmbn != (a.model == "psp"):
        ap.error("--ppmbn belongs to --model psp, and --model psp has the --ppmbn arm table only")
    if a.ppmbn and sum((a.convbn, a.layers, a.pwbn, a.pwlayers, a.dilbn, a.dillayers, a.s2bn, a.s2layers, a.stembn, a.stemlayers)):
        ap.error("--ppmbn is a measurement of its own: one per call")
    if a.dilbn and a.model != "r50":
        ap.error("--dilbn belongs to --model r50 (the dilated ResNet-50-v1c backbone)")
    if sum((a.convbn, a.layers, a.pwbn, a.pwlayers, a.dilbn, a.dillayers, a.s2bn, a.s2layers, a.stembn, a.stemlayers)) > 1:
        ap.error("--convbn, --layers, --pwbn, --pwlayers, --dilbn, --dillayers, --s2bn, --s2layers, --stembn and --stemlayers "
                 "are separate measurements: one per call")
    if a.stemlayers:
        stem_layers(max(3, a.reps))
        return
    if a.stembn and a.model == "x39":
        ap.error("--stembn belongs to --model r18 or --model r50")
    if a.dillayers:
        dil_layers(max(3, a.reps))
        return
    if a.s2layers:
        s2_layers(max(3, a.reps))
        return
    if a.s2bn and a.model == "x39":
        ap.error("--s2bn belongs to --model r18 or --model r50")
    if a.model == "x39" and (a.convbn or a.layers):
        ap.error("--convbn and --layers belong to --model r18 (the x39 table is `--model x39` alone)")
    if a.convbn and a.layers:
        ap.error("--convbn and --layers are two measurements: one per call")
    if a.pwbn and a.model == "x39":
        ap.error("--pwbn belongs to --model r18 or --model r50")
    if a.model == "r50" and not (a.pwbn or a.pwlayers or a.dilbn or a.s2bn or a.stembn):
        ap.error("--model r50 has the --pwbn, --dilbn, --s2bn and --stembn arm tables (and --pwlayers, --dillayers, --s2layers, "
                 "--stemlayers) only")
    if sum((a.convbn, a.layers, a.pwbn, a.pwlayers)) > 1:
        ap.error("--convbn, --layers, --pwbn and --pwlayers are separate measurements: one per call")
    if a.pwlayers:
        pw_layers(max(3, a.reps))
        return
    if a.model == "r18" and a.layers:
        r18_layers(max(3, a.reps))
        return
    if a.model == "x39" or a.convbn or a.pwbn or a.dilbn or a.s2bn or a.stembn or a.ppmbn or a.arm is not None:
        iters = a.iters or (10 if a.quick else 100)
        table = a.model + ("+pwbn" if a.pwbn else "+dilbn" if a.dilbn else "+s2bn" if a.s2bn else "+stembn" if a.stembn else "+ppmbn" if a.ppmbn else "")
        if a.arm is not None:
            print(json.dumps(arm_times(a.arm, iters, a.warmup, table)))
        else:
            arm_table(iters, a.warmup, max(3, a.reps), table)
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
