"""GPU parity of the dilated 3x3 convolutions (csrc/dilconv.hip: tsg_conv3x3_dil_fwd / _wrw; torchseg_amd/dilconv.py).

Reference: float64 `F.conv2d(..., padding=d, dilation=d)` and its autograd on the CPU, on the bf16-rounded operands (the
pattern of test_conv3g_gpu.py::test_mode1_filter_is_the_data_gradient; oracle/conv_ref.py has no dilation argument).
Forward and data gradient are bf16: one bf16 ulp of the fp64 result (2^-8 relative) plus 1e-3 of the output scale for
cancellation, the bound of test_conv3g_gpu.py.  The weight gradient is fp32 with the accumulation scheme of
tsg_conv3x3_wrw (exact bf16 products, fp32 MFMA accumulation per block, fp64 fold of the block partials), only the
summation order and the tile split differ: its error (max-abs over max |ref|) may be at most 2x what tsg_conv3x3_wrw
makes at dilation 1 on the same x and dy.  (The plain kernel takes channel counts that are multiples of 64: for a shape
with a smaller C_in it is fed x zero-padded to 64 channels, which does not change the gradient of the real channels.)
H and W are deliberately not multiples of the tiles (8 x 32 forward, 4 x 32 weight gradient) or of the dilation; one map is
smaller than the dilation."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

# (B, Cin, Cout, H, W, d)
SHAPES = [(2, 256, 256, 90, 90, 2), (2, 512, 512, 90, 90, 4), (1, 512, 512, 60, 60, 4), (1, 16, 64, 5, 37, 2),
          (1, 32, 192, 1, 1, 2), (1, 64, 128, 3, 7, 4), (3, 128, 64, 19, 70, 2)]


def _r(t):
    return t.bfloat16().double()


def _nhwc(t, cuda):
    return t.to(cuda).bfloat16().contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """operands (CPU fp32) and the float64 references y, dx, dw, and the dilation-1 weight gradient of the same x, dy"""
    B, Cin, Cout, H, W, d = shape
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    dy = torch.randn(B, Cout, H, W, generator=g)
    xr, wr = _r(x).requires_grad_(True), _r(w).requires_grad_(True)
    y = F.conv2d(xr, wr, None, 1, d, d)
    y.backward(_r(dy))
    w1 = _r(w).requires_grad_(True)
    F.conv2d(_r(x), w1, None, 1, 1, 1).backward(_r(dy))
    return x, w, dy, y.detach(), xr.grad, wr.grad, w1.grad


def _check(y, y_ref):
    err = (y.double().cpu() - y_ref).abs()
    bound = y_ref.abs() * 2.0 ** -8 + 1e-3 * y_ref.abs().max()
    print("max err %.3e, max |ref| %.3e" % (err.max().item(), y_ref.abs().max().item()))
    assert bool((err <= bound).all()), (err.max().item(), y_ref.abs().max().item())


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_data_gradient_vs_float64(cuda, shape):
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, Cin, Cout, H, W, d = shape
    x, w, dy, y_ref, dx_ref, _, _ = _case(shape)
    xb, dyb = _nhwc(x, cuda), _nhwc(dy, cuda)
    wd = w.to(cuda).contiguous(memory_format=torch.channels_last)          # fp32 master, channels_last
    assert kp.conv3x3_dil_supported(xb, wd, 1, d, d, 1)
    y = kp.conv3x3_dil_fwd(xb, kp.conv3x3_dil_prep_filter(wd, 0, xb), Cout, d)
    assert tuple(y.shape) == (B, Cout, H, W) and y.is_contiguous(memory_format=torch.channels_last)
    _check(y, y_ref)
    dx = kp.conv3x3_dil_dgrad(dyb, wd, d)
    assert tuple(dx.shape) == (B, Cin, H, W) and dx.is_contiguous(memory_format=torch.channels_last)
    _check(dx, dx_ref)
    # a weight that is not channels_last is cast per call: the same filter, the same result
    assert torch.equal(y, kp.conv3x3_dil_fwd(xb, kp.conv3x3_dil_prep_filter(w.to(cuda), 0, xb), Cout, d))
    # the addend of the data gradient: bf16(bf16(conv) + addend), what the eager add computes
    g = torch.Generator().manual_seed(3)
    skip = _nhwc(torch.randn(B, Cin, H, W, generator=g), cuda)
    assert torch.equal(kp.conv3x3_dil_dgrad(dyb, wd, d, addend=skip), dx + skip)


@pytest.mark.parametrize("shape", [(2, 256, 256, 90, 90, 2), (1, 512, 512, 60, 60, 4), (3, 128, 64, 19, 70, 2),
                                   (1, 64, 128, 3, 7, 4)])
def test_statistics_epilogue_and_determinism(cuda, shape):
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, Cin, Cout, H, W, d = shape
    x, w = _case(shape)[:2]
    xb = _nhwc(x, cuda)
    wf = kp.conv3x3_dil_prep_filter(w.to(cuda).contiguous(memory_format=torch.channels_last), 0, xb)
    y, partial = kp.conv3x3_dil_fwd(xb, wf, Cout, d, with_stats=True)
    assert torch.equal(y, kp.conv3x3_dil_fwd(xb, wf, Cout, d))
    assert partial.shape[1:] == (2, Cout)
    sums = partial.double().sum(0).cpu()
    yf = y.double().cpu()
    ref = torch.stack([yf.sum((0, 2, 3)), (yf * yf).sum((0, 2, 3))])
    np.testing.assert_allclose(sums.numpy(), ref.numpy(), rtol=2e-5, atol=2e-3)
    y2, p2 = kp.conv3x3_dil_fwd(xb, wf, Cout, d, with_stats=True)
    assert torch.equal(y, y2) and torch.equal(partial, p2)
    layout, N, C, HW = K.bn_layout(y)
    p_ref, S = kp.bn_stats(y, layout, N, C, HW)
    np.testing.assert_allclose(sums.numpy(), p_ref[:S].double().sum(0).cpu().numpy(), rtol=2e-5, atol=2e-3)


@pytest.mark.parametrize("shape", SHAPES)
def test_weight_gradient_vs_float64_and_the_plain_kernel(cuda, shape):
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, Cin, Cout, H, W, d = shape
    x, w, dy, _, _, dw_ref, dw1_ref = _case(shape)
    xb, dyb = _nhwc(x, cuda), _nhwc(dy, cuda)
    dw = kp.conv3x3_dil_wrw(xb, dyb, d)
    assert tuple(dw.shape) == (Cout, Cin, 3, 3) and dw.dtype == torch.float32
    assert dw.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(dw, kp.conv3x3_dil_wrw(xb, dyb, d))                  # fixed summation order
    out = torch.full((Cout, Cin, 3, 3), float("nan"), device=cuda).contiguous(memory_format=torch.channels_last)
    assert kp.conv3x3_dil_wrw(xb, dyb, d, out=out) is out and torch.equal(out, dw)
    # the yardstick: the plain kernel at dilation 1 on the same x and dy
    pad = -Cin % 64
    x1 = _nhwc(F.pad(x, (0, 0, 0, 0, 0, pad)), cuda) if pad else xb
    dw1 = kp.conv3x3_wrw(x1, dyb)[:, :Cin]
    e1 = (dw1.double().cpu() - dw1_ref).abs().max().item() / dw1_ref.abs().max().item()
    e = (dw.double().cpu() - dw_ref).abs().max().item() / dw_ref.abs().max().item()
    print("wrw %s: dilated %.3e, plain kernel at dilation 1 %.3e (max-abs / max |ref|)" % (shape, e, e1))
    assert e <= 2.0 * e1, (e, e1)


def _pair(cuda, Cin, Cout, d, nhwc_weight=True):
    from torchseg_amd.dilconv import DilatedConv2d, install_dilated_conv
    torch.manual_seed(3)
    stock = nn.Conv2d(Cin, Cout, 3, 1, d, d, bias=False).to(cuda)
    if nhwc_weight:
        stock.weight.data = stock.weight.data.contiguous(memory_format=torch.channels_last)
    ours = nn.Conv2d(Cin, Cout, 3, 1, d, d, bias=False).to(cuda)
    ours.weight.data = stock.weight.data.clone(memory_format=torch.preserve_format)
    assert install_dilated_conv(ours) == 1 and type(ours) is DilatedConv2d
    return stock, ours


@pytest.mark.parametrize("Cin,Cout,d,nhwc_weight", [(256, 256, 2, True), (512, 512, 4, True), (64, 128, 2, False)])
def test_module_against_the_stock_layer(cuda, Cin, Cout, d, nhwc_weight):
    from torchseg_amd import kernels as K
    stock, ours = _pair(cuda, Cin, Cout, d, nhwc_weight)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, Cin, 30, 45, generator=g)
    dy = _nhwc(torch.randn(2, Cout, 30, 45, generator=g), cuda)
    res = []
    for conv in (stock, ours):
        xd = _nhwc(x, cuda).requires_grad_(True)
        counter = K.CallCounter(K.provider())
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = conv(xd)
            y.backward(dy)
            torch.cuda.synchronize()
        finally:
            counts = counter.stop()
        res.append((y.detach().float(), xd.grad.float(), conv.weight.grad))
        want = 0 if conv is stock else 1
        assert counts.get("conv3x3_dil_fwd", 0) == 2 * want and counts.get("conv3x3_dil_wrw", 0) == want, counts
    for a, b in zip(res[0], res[1]):
        torch.testing.assert_close(b.float(), a.float(), rtol=2e-2, atol=2e-2)
    gw = ours.weight.grad
    assert gw.dtype == torch.float32 and gw.stride() == ours.weight.stride()
    # an NCHW input takes the stock forward, and so does the parity mode (fp32 outside autocast)
    counter = K.CallCounter(K.provider())
    try:
        xn = x.to(cuda).bfloat16()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            yn = ours(xn)
        yf = ours(_nhwc(x, cuda).float())
    finally:
        counts = counter.stop()
    assert counts.get("conv3x3_dil_fwd", 0) == 0, counts
    assert yf.dtype == torch.float32
    torch.testing.assert_close(yn.float(), res[0][0], rtol=2e-2, atol=2e-2)


def test_syncbn_behind_the_layer_consumes_the_attached_partial(cuda):
    from torchseg_amd import kernels as K
    from torchseg_amd.stemconv import take_bn_partial
    from torchseg_amd.syncbn import SyncBatchNorm
    _, ours = _pair(cuda, 256, 256, 2)
    bn = SyncBatchNorm(256).to(cuda)
    ref_bn = nn.BatchNorm2d(256).to(cuda)
    net = nn.Sequential(ours, bn).train()
    g = torch.Generator().manual_seed(6)
    xd = _nhwc(torch.randn(2, 256, 23, 41, generator=g), cuda).requires_grad_(True)
    counter = K.CallCounter(K.provider())
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = ours(xd)
            part = take_bn_partial(y)
            z = bn(y)
        z.float().sum().backward()
        torch.cuda.synchronize()
    finally:
        counts = counter.stop()
    assert part is not None and part.shape[1:] == (2, 256)
    assert counts.get("bn_stats", 0) == 0, counts               # the statistics pass is the convolution's epilogue
    assert counts.get("conv3x3_dil_fwd", 0) == 2, counts
    with torch.autocast("cuda", dtype=torch.bfloat16):
        z_ref = ref_bn.train()(y.detach())
    torch.testing.assert_close(z.float(), z_ref.float(), rtol=2e-2, atol=2e-2)
    # in eval mode there is no statistics partial
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert take_bn_partial(net.eval()[0](xd.detach())) is None
    del net


def test_fwd_bwd_in_a_captured_graph_replays_like_eager(cuda):
    """Warm-up, eager reference, capture and replay on ONE stream (the discipline of
    test_dwconv_gpu.py::test_fwd_bwd_in_a_captured_graph_replays_like_eager): no parallel branches — under capture the
    weight gradient stays on the capturing stream."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _, ours = _pair(cuda, 128, 128, 2)
        g = torch.Generator().manual_seed(4)
        x = _nhwc(torch.randn(2, 128, 37, 50, generator=g), cuda).requires_grad_(True)
        gy = _nhwc(torch.randn(2, 128, 37, 50, generator=g), cuda)

        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
                y = ours(x)
            y.backward(gy)
            return y

        for _ in range(2):
            x.grad, ours.weight.grad = None, None
            step()
        x.grad, ours.weight.grad = None, None
        y_e = step()
        torch.cuda.current_stream().synchronize()
        want = (y_e.clone(), x.grad.clone(), ours.weight.grad.clone())
        x.grad, ours.weight.grad = None, None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            y_g = step()
        graph.replay()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(y_g, want[0]) and torch.equal(x.grad, want[1]) and torch.equal(ours.weight.grad, want[2])


def test_pspnet_step_runs_the_dilated_layers_on_our_kernels(cuda, monkeypatch):
    """One PSPNet-R50 training step at the shape of test_families_gpu.py (bench.CONFIGS["pspnet"]), bf16 compute (in the
    fp32 parity mode the layers belong to exactconv), against the same network on the CPU in fp32 with identical weights and
    inputs, with test_families_gpu.py's tolerances: the loss within 1e-4 max(1, |ref|) of the CPU loss; the gradients
    (heads / all parameters, relative L2 against the CPU) at most 2x as far as stock torch on the same device (+ 1e-3).

    What that gradient rule can and cannot see: the gradients of a randomly initialised 50-layer network under bf16 compute
    are 0.5 (heads) to 1.3 (all) away from the fp32 CPU gradients in relative L2 whoever runs the convolutions (measured for
    stock torch, TSG_CONV_DIL=0 and =1 alike, profiles/dilconv_bench.txt section 3), so the rule shows that the step is no
    further from the truth than the vendor path is, but a wrong gradient in a single layer would pass it.  That is checked
    separately, inside the same step: for the first and the last dilated layer the input x, the output gradient dy, the
    input gradient dx and the parameter's gradient are taken from the running step (tensor hooks), and dx and dw are
    compared with float64 autograd of F.conv2d on exactly those bf16 x, dy and the bf16-rounded weight.  dx is bf16:
    the bound of _check (2^-8 relative + 1e-3 of the scale).  dw is fp32 sums of N = B H W <= 16 200 exact bf16 products
    accumulated in fp32: a random walk of N roundings of 2^-24 relative to partial sums of the size of the result,
    sqrt(N) 2^-24 = 8e-6 of the gradient's scale, times 5 for the largest of 2.4 million entries, rounded up: 1e-4 of
    max |dw|.  A wrong tap, sign or channel gives an error of the order of max |dw| itself.

    With TSG_CONV_DIL=1 every dilated 3x3 layer makes one conv3x3_dil_fwd call in the forward pass, one for its data
    gradient, and one conv3x3_dil_wrw call; with 0 none."""
    import importlib.util
    from torchseg_amd import kernels as K
    from torchseg_amd.ddp import DistributedDataParallel
    from torchseg_amd.syncbn import SyncBatchNorm
    spec = importlib.util.spec_from_file_location("_tsg_families", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                "test_families_gpu.py"))
    fam = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fam)
    _batch, _build = fam._batch, fam._build
    torch.set_num_threads(min(os.cpu_count() or 1, 64))
    ref = _build("pspnet", nn.BatchNorm2d, False)
    batch = _batch("pspnet")
    dbatch = [t.to(cuda) for t in batch]
    loss_ref = ref(*batch)
    loss_ref.backward()
    n_dil = sum(1 for m in ref.modules() if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and max(m.dilation) > 1)
    assert n_dil >= 8

    def rel(model, keep):
        num = den = 0.0
        for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
            assert (p.grad is None) == (q.grad is None), n
            if q.grad is None or not keep(n):
                continue
            dd = p.grad.cpu().double() - q.grad.double()
            num += float((dd * dd).sum())
            den += float((q.grad.double() ** 2).sum())
        return (num / den) ** 0.5

    is_head = lambda n: not n.startswith("backbone.")
    stock = _build("pspnet", nn.BatchNorm2d, False)
    stock.load_state_dict(ref.state_dict())
    stock = stock.to(cuda)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss_stock = stock(*dbatch)
    loss_stock.backward()
    torch.cuda.synchronize()
    stock_fig = (abs(loss_stock.item() - loss_ref.item()), rel(stock, is_head), rel(stock, lambda n: True))
    del stock
    from torchseg_amd.dilconv import DilatedConv2d
    for flag in ("0", "1"):
        monkeypatch.setenv("TSG_CONV_DIL", flag)
        net = _build("pspnet", SyncBatchNorm, True)
        net.load_state_dict(ref.state_dict())
        net = DistributedDataParallel(net.to(cuda), compute_dtype=torch.bfloat16)
        dil = [m for m in net.module.modules() if type(m) is DilatedConv2d]
        assert len(dil) == (n_dil if flag == "1" else 0)
        cap, handles = {}, []
        for m in ([dil[0], dil[-1]] if dil else []):
            cap[m] = {}

            def pre(mod, args):
                cap[mod]["x"] = args[0].detach()
                args[0].register_hook(lambda g, mod=mod: cap[mod].__setitem__("dx", g.detach()))

            def post(mod, args, y):
                y.register_hook(lambda g, mod=mod: cap[mod].__setitem__("dy", g.detach()))
            handles += [m.register_forward_pre_hook(pre), m.register_forward_hook(post)]
        counter = K.CallCounter(K.provider())
        try:
            loss = net(*dbatch)
            n_fwd = counter.counts.get("conv3x3_dil_fwd", 0)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            counts = counter.stop()
            for h in handles:
                h.remove()
        fig = (abs(loss.item() - loss_ref.item()), rel(net.module, is_head), rel(net.module, lambda n: True))
        print("TSG_CONV_DIL=%s: loss %.6f (cpu %.6f, stock bf16 %.6f); grad rel-L2 vs cpu: heads %.2e (stock %.2e), all %.2e "
              "(stock %.2e); dil_fwd calls %d + %d, dil_wrw %d" % (flag, loss.item(), loss_ref.item(), loss_stock.item(), fig[1],
                                                                  stock_fig[1], fig[2], stock_fig[2], n_fwd,
                                                                  counts.get("conv3x3_dil_fwd", 0) - n_fwd,
                                                                  counts.get("conv3x3_dil_wrw", 0)))
        if flag == "0":
            assert counts.get("conv3x3_dil_fwd", 0) == 0 and counts.get("conv3x3_dil_wrw", 0) == 0, counts
            continue
        assert n_fwd == n_dil, (n_fwd, n_dil)
        assert counts.get("conv3x3_dil_fwd", 0) == 2 * n_dil and counts.get("conv3x3_dil_wrw", 0) == n_dil, counts
        # the layers' own gradients, from the operands the step gave them
        for m, c in cap.items():
            d = m.dilation[0]
            xr = _r(c["x"].cpu().float()).requires_grad_(True)
            wr = _r(m.weight.detach().cpu()).requires_grad_(True)
            F.conv2d(xr, wr, None, 1, d, d).backward(_r(c["dy"].cpu().float()))
            _check(c["dx"], xr.grad)
            e = (m.weight.grad.double().cpu() - wr.grad).abs().max().item() / wr.grad.abs().max().item()
            print("layer %d -> %d d %d in the step: dw max-abs error / max |ref| %.3e" % (m.in_channels, m.out_channels, d, e))
            assert e <= 1e-4, e
        assert fig[0] <= 1e-4 * max(1.0, abs(loss_ref.item())), (fig, stock_fig)
        assert fig[1] <= 2.0 * stock_fig[1] + 1e-3, (fig, stock_fig)
        assert fig[2] <= 2.0 * stock_fig[2] + 1e-3, (fig, stock_fig)
        del net
