"""GPU parity of the wide classifier-convolution kernels (csrc/clswide.hip, through the C-ABI): nn.Conv2d(C_in, n, 1) + bias
of the pspnet / psanet (512 / 1024 -> 150) and fcn (512 -> 21) heads on a channels_last bf16 map, producing PLANAR logits.
Against oracle/conv_ref.py (fp64) and torch's fp64 autograd on the same bf16-rounded operands, with the bounds of
tests/test_clshead_gpu.py: forward and data gradient to one bf16 ulp plus a cancellation floor, weight / bias gradient to
fp32 accumulation accuracy; run-to-run bit-identical; poisoned, guard-banded buffers; the re-classed module inside
autocast; the PSPNet head statements with the fused wide criterion behind the wide classifier."""
import functools
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _guard
from oracle import conv_ref

pytestmark = pytest.mark.gpu

# (B, Cin, H, W, N, bias)
CASES = [
    (2, 512, 6, 6, 150, True),       # HW = 36: HW % 8 == 4; ragged class tile; a pixel group that spans both images
    (1, 1024, 10, 10, 150, True),    # the auxiliary head; P = 100, not a multiple of 32
    (3, 512, 4, 4, 21, True),        # FCN: the narrow class count at a wide C_in
    (2, 64, 8, 12, 33, False),       # smallest wide N and smallest C_in, no bias
    (1, 256, 5, 4, 256, True),       # maximum N; HW = 20
    (2, 192, 2, 2, 97, True),        # HW = 4; C_in not a power of two
    (1, 64, 90, 90, 150, True),      # the real 8100-pixel plane at a C_in that keeps the CPU oracle cheap
]


@functools.lru_cache(maxsize=None)
def _operands(case):
    """(x, w, bias, dz) fp32 on the CPU, and the fp64 results on the bf16-rounded operands: (z, dx, dw, db)"""
    B, Cin, H, W, N, has_bias = case
    g = torch.Generator().manual_seed(sum(case[:5]))
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(N, Cin, 1, 1, generator=g) * (1.0 / Cin) ** 0.5
    bias = torch.randn(N, generator=g) if has_bias else None
    dz = torch.randn(B, N, H, W, generator=g)
    xr = conv_ref.bf16_round(x).requires_grad_(True)
    wr = conv_ref.bf16_round(w).requires_grad_(True)
    br = bias.double().requires_grad_(True) if has_bias else None
    want = conv_ref.conv2d_ref(xr.detach(), wr.detach(), stride=1, pad=0)
    if has_bias:
        want = want + br.detach().view(1, -1, 1, 1)
    F.conv2d(xr, wr, br, 1, 0).backward(conv_ref.bf16_round(dz))
    return (x, w, bias, dz), (want, xr.grad, wr.grad, br.grad if has_bias else None)


def _device(case, cuda):
    (x, w, bias, dz), _ = _operands(case)
    xd = x.to(cuda).bfloat16().contiguous(memory_format=torch.channels_last)
    return xd, w.to(cuda), (bias.to(cuda) if bias is not None else None), dz.to(cuda).bfloat16().contiguous()


@pytest.mark.parametrize("case", CASES)
def test_cls_head_wide_kernels_vs_oracle(cuda, case):
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, Cin, H, W, N, has_bias = case
    _, (want, dx_ref, dw_ref, db_ref) = _operands(case)
    xd, wd, bd, dzd = _device(case, cuda)
    assert kp.cls_head_wide_supported(xd, wd)
    z = kp.cls_head_wide_fwd(xd, wd, bd)
    assert z.dtype == torch.bfloat16 and z.is_contiguous() and tuple(z.shape) == (B, N, H, W)
    assert torch.equal(z, kp.cls_head_wide_fwd(xd, wd, bd))
    err = (z.double().cpu() - want).abs()
    print("forward max err %.3e of %.3e" % (err.max().item(), want.abs().max().item()))
    assert bool((err <= want.abs() * 2.0 ** -8 + 1e-3 * want.abs().max()).all()), err.max().item()
    # backward
    dx, dw, db = kp.cls_head_wide_bwd(dzd, xd, wd, need_dx=True, need_db=has_bias)
    dx2, dw2, db2 = kp.cls_head_wide_bwd(dzd, xd, wd, need_dx=True, need_db=has_bias)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and (not has_bias or torch.equal(db, db2))
    assert dx.is_contiguous(memory_format=torch.channels_last) and dx.dtype == torch.bfloat16
    assert dw.shape == wd.shape and dw.dtype == torch.float32
    e = (dx.double().cpu() - dx_ref).abs()
    print("dgrad max err %.3e of %.3e" % (e.max().item(), dx_ref.abs().max().item()))
    assert bool((e <= dx_ref.abs() * 2.0 ** -8 + 1e-3 * dx_ref.abs().max()).all()), e.max().item()
    ew = (dw.double().cpu() - dw_ref).abs().max().item()
    print("wgrad max err %.3e of %.3e" % (ew, dw_ref.abs().max().item()))
    assert ew <= 1e-4 * dw_ref.abs().max().item() + 1e-6
    if has_bias:
        eb = (db.double().cpu() - db_ref).abs().max().item()
        print("dbias max err %.3e of %.3e" % (eb, db_ref.abs().max().item()))
        assert eb <= 1e-4 * db_ref.abs().max().item() + 1e-6
    else:
        assert db is None
    # without the data gradient the weight gradient is the same
    none, dw3, _ = kp.cls_head_wide_bwd(dzd, xd, wd, need_dx=False, need_db=False)
    assert none is None and torch.equal(dw3, dw)


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[5]])
def test_under_guard_bands(cuda, case):
    """plain, 0xFF- and 0xA5-poisoned calls are bit-equal and leave their guards alone: no output element is left unwritten,
    no operand is read past its end, and the workspace is used at exactly the size the query reports"""
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, Cin, H, W, N, has_bias = case
    xd, wd, bd, dzd = _device(case, cuda)
    wsb = kp.lib.tsg_cls_head_wide_wgrad_ws_bytes(B, H * W, Cin, N)
    assert wsb >= (N * Cin + B * N) * 4

    def fwd(x, w, b):
        return kp.cls_head_wide_fwd(x, w, b)

    def bwd(dz, x, w):
        return kp.cls_head_wide_bwd(dz, x, w, need_dx=True, need_db=True)

    _guard.three_calls(fwd, [xd, wd, bd])
    results = _guard.three_calls(bwd, [dzd, xd, wd])
    assert all(bool(torch.isfinite(t.float()).all()) for t in results[0])


class _Count:
    """counts provider calls (instance-level, removed on exit)"""

    def __init__(self, *names):
        from torchseg_amd import kernels as K
        self.kp, self.calls = K.provider(), {n: 0 for n in names}

    def __enter__(self):
        for n in self.calls:
            fn = getattr(self.kp, n)
            setattr(self.kp, n, (lambda name, f: lambda *a, **k: (self.calls.__setitem__(name, self.calls[name] + 1),
                                                                   f(*a, **k))[1])(n, fn))
        return self.calls

    def __exit__(self, *exc):
        for n in self.calls:
            delattr(self.kp, n)
        return False


def test_reclassed_head_inside_autocast(cuda):
    """pspnet network.py's last two statements of a head, Dropout2d(0.1) -> Conv2d(512, 150, 1), in train mode: planar bf16
    logits from one wide forward, gradients against fp64 (the dropout mask read off the dropout's output) within the bounds
    of test_clshead_gpu.py::test_reclassed_head_convolution_inside_autocast; eval + no_grad: the bits of a direct provider
    call; fp32 outside autocast: the ordinary path."""
    from torchseg_amd import kernels as K
    from torchseg_amd.clshead import ClsHeadWideConv2d, install_cls_head
    kp = K.provider()
    torch.manual_seed(1)
    head = nn.Sequential(nn.Dropout2d(0.1), nn.Conv2d(512, 150, 1)).to(cuda)
    keys = list(head.state_dict().keys())
    assert install_cls_head(head, wide=False) == 0 and type(head[1]) is nn.Conv2d
    assert install_cls_head(head, wide=True) == 1 and type(head[1]) is ClsHeadWideConv2d
    assert list(head.state_dict().keys()) == keys
    head.train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 512, 6, 10, generator=g)
    dz = torch.randn(2, 150, 6, 10, generator=g)
    xd = x.to(cuda).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dropped = []
    hook = head[0].register_forward_hook(lambda m, i, o: dropped.append(o.detach()))
    with _Count("cls_head_wide_fwd", "cls_head_wide_bwd", "cls_head_fwd") as calls:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            z = head(xd)
        assert z.is_contiguous() and z.dtype == torch.bfloat16 and tuple(z.shape) == (2, 150, 6, 10)
        z.backward(dz.to(cuda).bfloat16())
    hook.remove()
    assert calls == dict(cls_head_wide_fwd=1, cls_head_wide_bwd=1, cls_head_fwd=0), calls
    xc = dropped[0]
    assert xc.dtype == torch.bfloat16
    keep = (xc.float().abs().amax((2, 3), keepdim=True) > 0).double().cpu()        # Dropout2d zeroes whole channels
    assert 0.75 <= keep.mean().item() < 1.0
    xc = xc.double().cpu()
    xr = xc.clone().requires_grad_(True)
    wr = conv_ref.bf16_round(head[1].weight.detach().cpu().float()).requires_grad_(True)
    br = head[1].bias.detach().cpu().double().requires_grad_(True)
    F.conv2d(xr, wr, br).backward(conv_ref.bf16_round(dz))
    # through the dropout: the kept channels times the scale it applied (1 / 0.9 as the activation's dtype holds it),
    # read off its output; x.grad is then rounded twice (the data gradient, the product): 2^-8 of an element
    scale = xc.double().abs().sum().item() / (xd.detach().double().cpu() * keep).abs().sum().item()
    assert abs(scale - 1 / 0.9) <= 2.0 ** -8 * (1 / 0.9)
    xg = xr.grad * keep * scale
    ex = (xd.grad.double().cpu() - xg).abs().max().item()
    ew = (head[1].weight.grad.double().cpu() - wr.grad).abs().max().item()
    eb = (head[1].bias.grad.double().cpu() - br.grad).abs().max().item()
    print("x.grad %.3e of %.3e; weight.grad %.3e of %.3e; bias.grad %.3e of %.3e"
          % (ex, xg.abs().max().item(), ew, wr.grad.abs().max().item(), eb, br.grad.abs().max().item()))
    assert ex <= 2.0 ** -7 * xg.abs().max().item()
    assert ew <= 1e-4 * wr.grad.abs().max().item()
    assert eb <= 1e-4 * br.grad.abs().max().item()
    assert head[1].weight.grad.dtype == torch.float32 and head[1].bias.grad.dtype == torch.float32
    # evaluation: the bits of a direct provider call
    head.eval()
    xe = xd.detach()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ze = head(xe)
    assert torch.equal(ze, kp.cls_head_wide_fwd(xe, head[1].weight.detach(), head[1].bias.detach()))
    # fp32 activations outside autocast: the module's ordinary path
    with _Count("cls_head_wide_fwd") as calls:
        y32 = head[1](x.to(cuda))
    assert y32.dtype == torch.float32 and calls["cls_head_wide_fwd"] == 0
    assert (y32.double().cpu() - F.conv2d(x.double(), head[1].weight.detach().cpu().double(), br.detach())).abs().max().item() \
        <= 2e-2 * y32.abs().max().item()


class _Head(nn.Module):
    """pspnet network.py:46-56 in a test-authored module: 1x1 classifier, x8 bilinear, log_softmax, CrossEntropyLoss"""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(64, 150, 1)
        self.criterion = nn.CrossEntropyLoss(reduction='mean', ignore_index=255)

    def forward(self, x, label):
        fm = F.interpolate(self.conv(x), scale_factor=8, mode='bilinear', align_corners=True)
        return self.criterion(F.log_softmax(fm, dim=1), label)


def test_pspnet_statements_reach_the_wide_classifier_and_the_fused_wide_criterion(cuda, monkeypatch):
    """Both switches on: the classifier writes planar bf16 logits on the wide kernels, the up-sampling stays pending and the
    criterion runs on the fused wide kernels, which hand a planar bf16 logit gradient back to the wide backward.

    The fp64 reference runs the same statements on the bf16-rounded x and weight and rounds its logits to bf16 where the
    classifier stores them (straight through for the gradient).  Loss: 1e-4 * max(1, |ref|), the bound of
    tests/test_fused_head_wide_gpu.py for this chain.  That file's gradient bound for this chain, 2e-4 of the largest
    gradient, is stated for fp32 tensors; here the logit gradient and x.grad are bf16 tensors, whose rounding alone is
    2^-9 = 2e-3 of an element, so the gradient bounds are derived from the two roundings instead (and are far inside the
    0.1 of the largest gradient that file allows its bf16 comparison):
      x.grad[p, c]  <= 2^-9 sum_n |dz[n, p] W[n, c]|  (dz rounded to bf16)  + 2^-8 |ref|  (x.grad rounded)  + 1e-3 max |ref|
      dW[n, c]      <= 2^-9 sum_p |dz[n, p] x[p, c]|  + 1e-4 max |ref|      (fp32 accumulation: test_clshead_gpu.py)
      dbias[n]      <= 2^-9 sum_p |dz[n, p]|          + 1e-4 max |ref|"""
    from torchseg_amd import losses
    from torchseg_amd.clshead import ClsHeadWideConv2d, install_cls_head
    from torchseg_amd.fusion import FuseMode
    monkeypatch.setenv("TSG_CLS_HEAD_WIDE", "1")
    monkeypatch.setattr(losses, "FUSE_HEAD_WIDE", True)
    torch.manual_seed(8)
    head = _Head().to(cuda)
    assert install_cls_head(head) == 1 and type(head.conv) is ClsHeadWideConv2d
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 64, 6, 8, generator=g)
    label = torch.randint(0, 150, (2, 48, 64), generator=g)
    label[:, :5] = 255
    xf = x.to(cuda).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with _Count("cls_head_wide_fwd", "cls_head_wide_bwd", "ohem_up_fwd", "ohem_up_bwd", "upsample_fwd", "ohem_fwd") as calls:
        with FuseMode(head=True):
            out = head(xf, label.to(cuda))
        out.backward()
    assert calls == dict(cls_head_wide_fwd=1, cls_head_wide_bwd=1, ohem_up_fwd=1, ohem_up_bwd=1, upsample_fwd=0,
                         ohem_fwd=0), calls
    # fp64 reference
    xr = conv_ref.bf16_round(x).requires_grad_(True)
    wr = conv_ref.bf16_round(head.conv.weight.detach().cpu().float()).requires_grad_(True)
    br = head.conv.bias.detach().cpu().double().requires_grad_(True)
    z = F.conv2d(xr, wr, br)
    zq = z + (conv_ref.bf16_round(z.detach()) - z.detach())
    zq.retain_grad()
    ref = F.cross_entropy(F.interpolate(zq, scale_factor=8, mode='bilinear', align_corners=True), label, ignore_index=255)
    ref.backward()
    print("loss %.7f (fp64 %.7f)" % (out.item(), ref.item()))
    assert abs(out.item() - ref.item()) <= 1e-4 * max(1.0, abs(ref.item())), (out.item(), ref.item())
    dzr = zq.grad.abs()                                                            # [B, N, H, W]
    bx = 2.0 ** -9 * torch.einsum("bnhw,nc->bchw", dzr, wr.detach().abs()[:, :, 0, 0]) + 2.0 ** -8 * xr.grad.abs() \
        + 1e-3 * xr.grad.abs().max()
    ex = (xf.grad.double().cpu() - xr.grad).abs()
    bw = 2.0 ** -9 * torch.einsum("bnhw,bchw->nc", dzr, xr.detach().abs())[:, :, None, None] + 1e-4 * wr.grad.abs().max()
    ew = (head.conv.weight.grad.double().cpu() - wr.grad).abs()
    bb = 2.0 ** -9 * dzr.sum((0, 2, 3)) + 1e-4 * br.grad.abs().max()
    eb = (head.conv.bias.grad.double().cpu() - br.grad).abs()
    print("x.grad %.3e of %.3e; weight.grad %.3e of %.3e; bias.grad %.3e of %.3e"
          % (ex.max().item(), xr.grad.abs().max().item(), ew.max().item(), wr.grad.abs().max().item(), eb.max().item(),
             br.grad.abs().max().item()))
    assert bool((ex <= bx).all()), (ex / bx).max().item()
    assert bool((ew <= bw).all()), (ew / bw).max().item()
    assert bool((eb <= bb).all()), (eb / bb).max().item()
    assert ex.max().item() <= 0.1 * xr.grad.abs().max().item()
