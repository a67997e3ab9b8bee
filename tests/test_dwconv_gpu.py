"""GPU: the depthwise 3x3 kernels (csrc/dwconv.hip) against torch's CPU float64 grouped convolution on the same rounded
inputs, at the nine Xception39 shapes (batch 2, one at batch 16), odd sizes and sizes that are no multiple of any tile;
run-to-run identity of the weight gradient; DepthwiseConv2d against the stock module; one graph capture."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_bisenet_x39_cpu import SHAPES

pytestmark = pytest.mark.gpu

# (B, C, H, W, stride)
CASES = [(2, C, H, H, s) for C, H, s in SHAPES] + [(16, 64, 128, 128, 1), (2, 16, 33, 47, 2), (2, 24, 13, 29, 1),
                                                   (3, 8, 7, 5, 2), (1, 40, 1, 9, 2)]


def _ref(x, w, dy, stride):
    """float64 forward, data gradient and weight gradient, and the same of |x|, |w|, |dy| (the scale of the sums)"""
    C = x.shape[1]
    xd, wd, gd = x.double(), w.double(), dy.double()
    y = F.conv2d(xd, wd, None, stride, 1, 1, C)
    dx = torch.nn.grad.conv2d_input(xd.shape, wd, gd, stride, 1, 1, C)
    dw = torch.nn.grad.conv2d_weight(xd, wd.shape, gd, stride, 1, 1, C)
    ay = F.conv2d(xd.abs(), wd.abs(), None, stride, 1, 1, C)
    adx = torch.nn.grad.conv2d_input(xd.shape, wd.abs(), gd.abs(), stride, 1, 1, C)
    adw = torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, gd.abs(), stride, 1, 1, C)
    return (y, ay), (dx, adx), (dw, adw)


def _ulp(v, mant):
    """one unit in the last place of the float64 value v in a format with `mant` explicit mantissa bits"""
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-38)))
    return torch.pow(2.0, e - mant)


def _check(got, ref, mant, acc_eps, what):
    """|got - ref| <= 1 ulp of ref in the output format, + the accumulation's own rounding (acc_eps x sum of |terms|)"""
    want, scale = ref
    err = (got.double().cpu() - want).abs()
    tol = _ulp(want, mant) + acc_eps * scale
    bad = err > tol
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err - tol).max()))


def _inputs(B, C, H, W, stride, dtype, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(B, C, H, W, generator=g).to(dtype)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.3
    dy = torch.randn(B, C, OH, OW, generator=g).to(dtype)
    cl = torch.channels_last
    return x, w, dy, (x.to(dev).contiguous(memory_format=cl), w.to(dev), dy.to(dev).contiguous(memory_format=cl))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,C,H,W,stride", CASES)
def test_kernels_against_float64(cuda, B, C, H, W, stride, dtype):
    from torchseg_amd import kernels as K
    kp = K.provider()
    x, w, dy, (xd, wd, dyd) = _inputs(B, C, H, W, stride, dtype, cuda)
    assert kp.dwconv3x3_supported(xd, wd, stride, 1, 1, C)
    y = kp.dwconv3x3_fwd(xd, wd, stride)
    dx = kp.dwconv3x3_dgrad(dyd, wd, xd, stride)
    dw = kp.dwconv3x3_wgrad(xd, dyd, wd, stride)
    dw2 = kp.dwconv3x3_wgrad(xd, dyd, wd, stride)
    torch.cuda.synchronize()
    assert y.dtype == dtype and dx.dtype == dtype and dw.dtype == torch.float32
    assert y.is_contiguous(memory_format=torch.channels_last) and dx.shape == xd.shape
    assert torch.equal(dw, dw2)                      # bit-identical from launch to launch
    ry, rdx, rdw = _ref(x, w, dy, stride)
    if dtype == torch.bfloat16:                      # fp32 accumulation, one rounding to bf16
        _check(y, ry, 7, 9 * 2.0 ** -24, "y")
        _check(dx, rdx, 7, 9 * 2.0 ** -24, "dx")
        _check(dw, rdw, 23, 2.0 ** -18, "dw")       # fp32 lane sums over <= a few hundred pixels, fp64 fold
    else:                                            # exact products, fp64 accumulation, one rounding to fp32
        _check(y, ry, 23, 2.0 ** -48, "y")
        _check(dx, rdx, 23, 2.0 ** -48, "dx")
        _check(dw, rdw, 23, 2.0 ** -44, "dw")


def _pair(dev, C=32, stride=1):
    from torchseg_amd.dwconv import DepthwiseConv2d, install_depthwise_conv
    torch.manual_seed(3)
    stock = nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False).to(dev)
    ours = nn.Sequential(nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False)).to(dev)
    ours[0].load_state_dict(stock.state_dict())
    assert install_depthwise_conv(ours) == 1 and isinstance(ours[0], DepthwiseConv2d)
    return stock, ours[0]


def _counting(monkeypatch):
    from torchseg_amd import kernels as K
    kp = K.provider()
    calls = {"fwd": 0, "dgrad": 0, "wgrad": 0}
    for k in calls:
        orig = getattr(kp, "dwconv3x3_" + k)
        monkeypatch.setattr(kp, "dwconv3x3_" + k,
                            (lambda o, n: lambda *a: (calls.__setitem__(n, calls[n] + 1), o(*a))[1])(orig, k))
    return calls


@pytest.mark.parametrize("stride", [1, 2])
def test_module_under_autocast_against_stock(cuda, monkeypatch, stride):
    calls = _counting(monkeypatch)
    stock, ours = _pair(cuda, stride=stride)
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(2, 32, 40, 36, generator=g).to(cuda).bfloat16().contiguous(memory_format=torch.channels_last)
    prior = torch.randn(32, 1, 3, 3, generator=g).to(cuda)
    outs = []
    for m in (stock, ours):
        m.weight.grad = prior.clone()                # gradient accumulation into an existing .grad
        x = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x)
        gy = torch.ones_like(y).normal_(generator=torch.Generator(cuda).manual_seed(2))
        y.backward(gy)
        outs.append((y.float(), x.grad.float(), m.weight.grad.clone()))
    assert calls == {"fwd": 1, "dgrad": 1, "wgrad": 1}, calls
    (ys, dxs, dws), (yo, dxo, dwo) = outs
    assert yo.dtype == ys.dtype and outs[1][0].shape == ys.shape
    for a, b, what in ((yo, ys, "y"), (dxo, dxs, "dx"), (dwo - prior, dws - prior, "dw")):
        scale = b.abs().max().item()
        assert (a - b).abs().max().item() <= 2 ** -6 * scale, what      # bf16 operands on the stock side (autocast)


def test_nchw_input_takes_the_stock_forward(cuda, monkeypatch):
    calls = _counting(monkeypatch)
    stock, ours = _pair(cuda)
    x = torch.randn(2, 32, 16, 16, device=cuda)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        a, b = stock(x.bfloat16()), ours(x.bfloat16())           # contiguous (NCHW) input
    assert torch.equal(a, b)
    xf = x.contiguous(memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ours(xf)                                                   # fp32 under autocast: stock as well
    assert calls["fwd"] == 0
    ours(xf)                                                       # fp32 outside autocast: the parity kernels
    assert calls["fwd"] == 1


def test_fwd_bwd_in_a_captured_graph_replays_like_eager(cuda):
    """Warm-up, eager reference, capture and replay on ONE stream (bench.GraphedStep's discipline): autograd records the
    stream of each leaf's gradient accumulator when it is created, and a capture on another stream would have the engine
    join a stream that is not capturing."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stock, ours = _pair(cuda, C=64, stride=2)
        g = torch.Generator().manual_seed(4)
        x = torch.randn(2, 64, 48, 48, generator=g).to(cuda).bfloat16().contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        gy = torch.randn(2, 64, 24, 24, generator=g).to(cuda).bfloat16().contiguous(memory_format=torch.channels_last)

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
        want = (y_e.clone(), x.grad.clone(), ours.weight.grad.clone())
        x.grad, ours.weight.grad = None, None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            y_g = step()
        graph.replay()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(y_g, want[0]) and torch.equal(x.grad, want[1]) and torch.equal(ours.weight.grad, want[2])
