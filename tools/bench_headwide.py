"""GPU microbench of the fused upsample + cross-entropy head for 33..256 classes (tsg_ohem_up_fwd / _bwd on
ohem_upw_fwd_k / ohem_up_bwd_k<.., WIDE>, csrc/ohem.hip; TSG_FUSE_HEAD_WIDE) against the materialised chain it replaces on the same
operands: upsample_fwd + ohem_fwd + ohem_bwd + upsample_bwd.  Shapes: the ADE20K heads of bench.py, 2 x 150 x 90^2 -> 720^2
(PSPNet) and 2 x 150 x 60^2 -> 480^2 (PSANet), bf16 logits, uint8 and int64 labels, plain CE (thresh 1, min_kept 0: what
nn.CrossEntropyLoss of those networks is routed to).
HIP-event timing: 10 warm-up calls per entry, then 3 windows of at least 0.25 s each (the call count comes from a
calibration window); the median window is reported (min and max beside it).  Every call reuses the same operands: cache-warm,
back-to-back figures, like for like between the two forms, below what a head costs inside a step.  The provider methods
allocate their outputs, so both sides include the allocator.
Writes profiles/headwide_bench.txt (or the file given as the first argument)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torchseg_amd import kernels as K
dev = torch.device("cuda:0")
kp = K.provider()
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              "profiles", "headwide_bench.txt")
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
B, C = 2, 150
for IH, OH in ((90, 720), (60, 480)):
    g = torch.Generator().manual_seed(IH)
    lab_lo = torch.randint(0, C, (B, IH, IH), generator=g)
    z = (torch.randn(B, C, IH, IH, generator=g) + 4.0 * torch.nn.functional.one_hot(lab_lo, C).permute(0, 3, 1, 2).float())
    z = z.to(dev).bfloat16().contiguous()
    t = lab_lo.repeat_interleave(OH // IH, 1).repeat_interleave(OH // IH, 2)
    t[:, :8] = 255
    gs = torch.ones(1, device=dev)
    assert kp.ohem_up_wide_supported(z, OH, OH)
    for lname, ldt in (("uint8", torch.uint8), ("int64", torch.int64)):
        tl = t.to(ldt).to(dev)
        loss_f, nll_f, lse_f, sel_f = kp.ohem_up_fwd(z, tl, OH, OH, 255, 1.0, 0, None)
        full = kp.upsample_fwd(z, None, OH, OH)
        loss_m, nll_m, lse_m, sel_m = kp.ohem_fwd(full, tl, 255, 1.0, 0, None)
        dfull = kp.ohem_bwd(full, tl, 255, None, nll_m, lse_m, sel_m, gs)
        dz_f = kp.ohem_up_bwd(z, tl, OH, OH, 255, None, nll_f, lse_f, sel_f, gs)
        dz_m = kp.upsample_bwd(dfull, IH, IH)
        r = {
            "fused fwd": timeit(lambda: kp.ohem_up_fwd(z, tl, OH, OH, 255, 1.0, 0, None)),
            "fused bwd": timeit(lambda: kp.ohem_up_bwd(z, tl, OH, OH, 255, None, nll_f, lse_f, sel_f, gs)),
            "upsample_fwd": timeit(lambda: kp.upsample_fwd(z, None, OH, OH)),
            "ohem_fwd": timeit(lambda: kp.ohem_fwd(full, tl, 255, 1.0, 0, None)),
            "ohem_bwd": timeit(lambda: kp.ohem_bwd(full, tl, 255, None, nll_m, lse_m, sel_m, gs)),
            "upsample_bwd": timeit(lambda: kp.upsample_bwd(dfull, IH, IH)),
        }
        fused = r["fused fwd"][0] + r["fused bwd"][0]
        chain = r["upsample_fwd"][0] + r["ohem_fwd"][0] + r["ohem_bwd"][0] + r["upsample_bwd"][0]
        scale = dz_m.float().abs().max().item()
        say("%d x %d x %d^2 -> %d^2 bf16, %s labels: loss fused %.6f materialised %.6f; max |dz fused - materialised| %.3g of %.3g"
            % (B, C, IH, OH, lname, loss_f.item(), loss_m.item(), (dz_f.float() - dz_m.float()).abs().max().item(), scale))
        for k, v in r.items():
            say("    %-13s %s us" % (k, fmt(v)))
        say("    fused forward + backward %.1f us; materialised chain %.1f us; fused / chain = %.2f; full-resolution bytes not "
            "allocated: %.0f MB (logits) + %.0f MB (their gradient)"
            % (fused, chain, fused / chain, full.numel() * 2 / 1e6, dfull.numel() * 2 / 1e6))
        del full, dfull
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
