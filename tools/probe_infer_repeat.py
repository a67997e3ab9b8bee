"""Which layers of the bf16 inference path do not repeat, and does torch.backends.cudnn.deterministic pin them?

A stride-2 BasicBlock, a Bottleneck and BiSeNet-R18 (1x3x64x128) behind prepare_inference, with the setting off and on: the
number of distinct outputs of three copies over repeated calls (eval, eval with gradients enabled, train mode), and, per
convolution / BatchNorm module, whether it repeats on a fixed input.  Recorded in profiles/convbn_vendor_repeat.txt.

    python tools/probe_infer_repeat.py
"""
import copy, hashlib, os, sys
import torch, torch.nn as nn
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "torchseg_amd", "furnace")); sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_convbn_cpu import _r18, _randomise_bn
from torchseg_amd.infer import prepare_inference
from torchseg_amd.fusion import materialize
dev = torch.device("cuda:0")
BF = torch.bfloat16
def h(t):
    return hashlib.md5(t.detach().float().cpu().numpy().tobytes()).hexdigest()[:8]
def scan(label, net, x, reps=5):
    """every conv / bn module: record its input once, re-run it `reps` times, count distinct results"""
    ins = {}
    hooks = [m.register_forward_hook(lambda m, a, o, n=n: (ins.setdefault(n, (m, a)), None)[1]) for n, m in net.module.named_modules()
             if isinstance(m, (nn.Conv2d, nn.modules.batchnorm._BatchNorm))]
    outs = {h(materialize(net(x))) for _ in range(reps)}
    for k in hooks: k.remove()
    print("%s: whole forward, %d calls -> %d distinct" % (label, reps, len(outs)))
    bad = []
    for n, (m, a) in ins.items():
        with torch.no_grad(), torch.autocast("cuda", dtype=BF):
            d = {h(m(*a)) for _ in range(reps)}
        if len(d) > 1:
            bad.append("%s %s in %s (%d distinct)" % (n, type(m).__name__, tuple(a[0].shape), len(d)))
    print("%s: modules that do not repeat on a fixed input: %s" % (label, bad or "none"))
for det in (False, True):
    torch.backends.cudnn.deterministic = det
    print("==== torch.backends.cudnn.deterministic = %s, benchmark = %s" % (det, torch.backends.cudnn.benchmark))
    from base_model.resnet import BasicBlock, Bottleneck, _shortcut
    torch.manual_seed(3)
    mods = {"basicblock-s2": (BasicBlock(64, 128, 2, nn.BatchNorm2d, downsample=_shortcut(64, 128, 2, nn.BatchNorm2d, 1e-5, 0.1)), 64),
            "bottleneck": (Bottleneck(256, 64, 1, nn.BatchNorm2d), 256)}
    for name, (m, cin) in mods.items():
        m = _randomise_bn(m, 7).eval()
        x = torch.randn(2, cin, 18, 40, generator=torch.Generator().manual_seed(8)).to(BF).to(dev).contiguous(memory_format=torch.channels_last)
        nets = [prepare_inference(copy.deepcopy(m).to(dev), dtype=BF, fuse_convbn=False) for _ in range(3)]
        print("%s: three copies x 4 calls, distinct outputs: %d" % (name, len({h(n(x)) for n in nets for _ in range(4)})))
        for train, grad in ((False, True), (True, False), (True, True)):
            outs = set()
            for n in nets:
                for _ in range(3):
                    n.module.train(train)
                    with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=BF):
                        outs.add(h(n.module(x)))
                    n.module.eval()
            print("%s train=%s grad=%s: three copies x 3 calls, distinct outputs: %d" % (name, train, grad, len(outs)))
        scan(name, nets[0], x)
    net = _r18(41).eval().to(dev)
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(42)).to(dev)
    nets = [prepare_inference(copy.deepcopy(net), dtype=BF, fuse_convbn=False) for _ in range(3)]
    print("r18 unfused: three copies x 4 calls, distinct outputs: %d" % len({h(materialize(n(x))) for n in nets for _ in range(4)}))
    scan("r18 unfused", nets[0], x)
    ons = [prepare_inference(copy.deepcopy(net), dtype=BF, fuse_convbn=True) for _ in range(3)]
    print("r18 fused: three copies x 4 calls, distinct outputs: %d" % len({h(materialize(n(x))) for n in ons for _ in range(4)}))
