"""GPU microbench of the wide classifier-head kernels (tsg_cls_head_wide_* on clw_fwd_k / clw_dgrad_k / clw_wgrad_k,
csrc/clswide.hip; TSG_CLS_HEAD_WIDE) against what the module runs without the switch on the same operands: the library
convolution under bf16 autocast on the channels_last map (BiasSplitConv2d: bias-free convolution, bias add, bias gradient
on the column-sum kernel) and the copies between channels_last and the planar layout of the criterion kernels
(`z.contiguous()` of losses.py forward, the planar -> channels_last copy of dz backward).
Shapes: the heads of bench.py's pspnet / psanet / fcn configs per rank, 2 x 512 x 90^2, 2 x 1024 x 90^2, 2 x 512 x 60^2,
2 x 1024 x 60^2 -> 150 and 16 x 512 x 16^2 -> 21.
HIP-event timing: 10 warm-up calls per entry, then 3 windows of at least 0.25 s each (the call count comes from a
calibration window); the median window is reported (min and max beside it).  Every call reuses the same operands:
cache-warm, back-to-back figures, like for like between the two forms.  Both sides allocate their outputs and include their
host cost: the baseline forward runs under no_grad, its backward is torch.autograd.grad through a retained graph.
Bytes and FLOPs come from the shapes; the HBM floor is bytes / 8 TB/s (the MI355X's specified peak).
Needs a GPU.  Writes profiles/clswide_bench.txt (or the file given as the first argument)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
if not torch.cuda.is_available():
    sys.exit("bench_clshead_wide.py: no GPU")
from torchseg_amd import kernels as K
from torchseg_amd.convbias import BiasSplitConv2d
dev = torch.device("cuda:0")
kp = K.provider()
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              "profiles", "clswide_bench.txt")
HBM = 8.0e12
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


say("# us per call: median of 3 windows of >= 0.25 s (min-max), cache-warm back-to-back calls on the same operands")
for B, C, S, N in ((2, 512, 90, 150), (2, 1024, 90, 150), (2, 512, 60, 150), (2, 1024, 60, 150), (16, 512, 16, 21)):
    g = torch.Generator().manual_seed(C + S)
    x = torch.randn(B, C, S, S, generator=g).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    dz = torch.randn(B, N, S, S, generator=g).to(dev).bfloat16().contiguous()
    torch.manual_seed(N)
    mod = BiasSplitConv2d(C, N, 1).to(dev)
    w, b = mod.weight.detach(), mod.bias.detach()
    assert kp.cls_head_wide_supported(x, w)
    P = B * S * S
    flop = 2.0 * P * C * N
    by_f = P * C * 2 + P * N * 2 + N * C * 4 + N * 4                 # x, z, W, bias
    by_b = 2 * (P * N * 2) + 2 * (P * C * 2) + 2 * N * C * 4 + N * 4   # dz twice, x, dx, W, dW, dbias
    wsb = kp.lib.tsg_cls_head_wide_wgrad_ws_bytes(B, S * S, C, N)

    def base_fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return mod(x).contiguous()

    xg = x.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        zg = mod(xg).contiguous()
    params = (xg, mod.weight, mod.bias)

    def base_bwd():
        return torch.autograd.grad(zg, params, dz, retain_graph=True)

    z = kp.cls_head_wide_fwd(x, w, b)
    zb = base_fwd()
    dx, dw, db = kp.cls_head_wide_bwd(dz, x, w, need_dx=True, need_db=True)
    gx, gw, gb = base_bwd()
    r = {
        "wide fwd": timeit(lambda: kp.cls_head_wide_fwd(x, w, b)),
        "wide bwd": timeit(lambda: kp.cls_head_wide_bwd(dz, x, w, need_dx=True, need_db=True)),
        "wide wgrad": timeit(lambda: kp.cls_head_wide_bwd(dz, x, w, need_dx=False, need_db=True)),
        "base fwd": timeit(base_fwd),
        "base bwd": timeit(base_bwd),
    }
    say("%d x %d x %d^2 -> %d bf16: %.2f GFLOP per direction; forward %.1f MB (HBM floor %.1f us), backward %.1f MB (%.1f us); "
        "weight-gradient partials %.2f MB written and read once"
        % (B, C, S, N, flop / 1e9, by_f / 1e6, by_f / HBM * 1e6, by_b / 1e6, by_b / HBM * 1e6, wsb / 1e6))
    say("    max |z wide - base| %.3g of %.3g; |dx| %.3g of %.3g; |dw| %.3g of %.3g; |db| %.3g of %.3g"
        % ((z.float() - zb.float()).abs().max().item(), zb.float().abs().max().item(),
           (dx.float() - gx.float()).abs().max().item(), gx.float().abs().max().item(),
           (dw - gw.float()).abs().max().item(), gw.float().abs().max().item(),
           (db - gb.float()).abs().max().item(), gb.float().abs().max().item()))
    for k, v in r.items():
        say("    %-11s %s us" % (k, fmt(v)))
    say("    wide / base: forward %.2f, backward (dgrad + wgrad + dbias) %.2f"
        % (r["wide fwd"][0] / r["base fwd"][0], r["wide bwd"][0] / r["base bwd"][0]))
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
