"""GPU microbench of the dilated 3x3 convolutions (tsg_conv3x3_dil_fwd / _wrw, csrc/dilconv.hip) at the three shipped
layer shapes of the PSPNet / PSANet backbone (256 -> 256 d 2, 512 -> 512 d 2, 512 -> 512 d 4) at both per-rank map sizes
(2 x 90 x 90: PSPNet 720^2; 2 x 60 x 60: PSANet 480^2), bf16 channels_last: forward (+ statistics), data gradient and weight
gradient, ours against F.conv2d and its autograd on the vendor library with the shipped find-db, in one process.
HIP-event timing: 10 warm-up calls per shape and kernel, then 3 windows of at least 0.25 s each (the call count comes from
a calibration window); the median window is reported (min and max beside it).  Every call reuses the same operands, so
all figures are cache-warm, back-to-back figures: like for like between ours and the vendor kernels, above what a layer
reaches inside a step.  Also timed: tsg_bn_stats of the layer's output, the pass the statistics epilogue replaces.
Writes profiles/dilconv_layers.txt (or the file given as the first argument); profiles/dilconv_bench.txt quotes it."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from torchseg_amd import kernels as K
from torchseg_amd.tuning import use_shipped_miopen_db
use_shipped_miopen_db(0)
dev = torch.device("cuda:0")
kp = K.provider()
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              "profiles", "dilconv_layers.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timeit(fn, windows=3, seconds=0.25):
    for _ in range(10):
        fn()

    def window(n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n * 1e3
    n = max(50, int(seconds * 1e6 / window(50)) + 1)
    ts = sorted(window(n) for _ in range(windows))
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(t):
    return "%7.1f (%.1f-%.1f)" % t


say("# us per call: median of 3 windows of >= 0.25 s (min-max), cache-warm back-to-back calls; TF/s = 2 B Cin Cout 9 H W / median")
tot = {}
for H in (90, 60):
    for Cin, Cout, d, n in ((256, 256, 2, 5), (512, 512, 2, 1), (512, 512, 4, 2)):
        B = 2
        x = torch.randn(B, Cin, H, H, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)
        w = (torch.randn(Cout, Cin, 3, 3, device=dev) * (2.0 / (9 * Cin)) ** 0.5).contiguous(memory_format=torch.channels_last)
        wb = w.bfloat16().contiguous(memory_format=torch.channels_last)
        dy = torch.randn(B, Cout, H, H, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)
        wf, wt = kp.conv3x3_dil_prep_filter(w, 0, x), kp.conv3x3_dil_prep_filter(w, 1, dy)
        fl = 2.0 * B * Cin * Cout * 9 * H * H
        bw = lambda mask: torch.ops.aten.convolution_backward(dy, x, wb, None, [1, 1], [d, d], [d, d], False, [0, 0], 1, mask)
        t = {
            "fwd ours": timeit(lambda: kp.conv3x3_dil_fwd(x, wf, Cout, d)),
            "fwd ours+stats": timeit(lambda: kp.conv3x3_dil_fwd(x, wf, Cout, d, with_stats=True)),
            "fwd vendor": timeit(lambda: F.conv2d(x, wb, None, 1, d, d)),
            "dgrad ours": timeit(lambda: kp.conv3x3_dil_fwd(dy, wt, Cin, d)),
            "dgrad vendor": timeit(lambda: bw([True, False, False])),
            "wrw ours": timeit(lambda: kp.conv3x3_dil_wrw(x, dy, d)),
            "wrw vendor": timeit(lambda: bw([False, True, False])),
        }
        yy = kp.conv3x3_dil_fwd(x, wf, Cout, d)
        lay = K.bn_layout(yy)
        t_bn = timeit(lambda: kp.bn_stats(yy, *lay))
        dmax = (kp.conv3x3_dil_fwd(x, wf, Cout, d).float() - F.conv2d(x, wb, None, 1, d, d).float()).abs().max().item()
        say("%d->%d d%d @ %dx%dx%d (%.1f GFLOP, x%d per PSPNet-R50 step)  max|fwd ours - vendor| %.3g" %
            (Cin, Cout, d, B, H, H, fl / 1e9, n, dmax))
        for k, v in t.items():
            say("    %-15s %s us  %6.1f TF/s" % (k, fmt(v), fl / v[0] / 1e6))
        say("    %-15s %s us  (the pass 'fwd ours+stats' replaces)" % ("bn_stats of y", fmt(t_bn)))
        for k, v in t.items():
            tot[(H, k)] = tot.get((H, k), 0.0) + n * v[0]
for H in (90, 60):
    say("per PSPNet-R50 step at %d^2 (5 + 1 + 2 layers): forward ours+stats %.0f vs vendor %.0f us; data gradient ours %.0f vs "
        "vendor %.0f us; weight gradient ours %.0f vs vendor %.0f us" %
        (H, tot[(H, "fwd ours+stats")], tot[(H, "fwd vendor")], tot[(H, "dgrad ours")], tot[(H, "dgrad vendor")],
         tot[(H, "wrw ours")], tot[(H, "wrw vendor")]))
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
