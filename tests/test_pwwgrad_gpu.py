"""The HIP weight gradient of the whole-map 1x1 convolutions (csrc/pwwgrad.hip; kernels.pw_wgrad; opt-in from
pwconv.pointwise_wgrad with TSG_PW_WGRAD_HIP=1): against the float64 gradient of the same bf16 operands, bit for bit from
run to run, inside poisoned guard-banded buffers, through a re-classed module, and under stream capture."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _guard

pytestmark = pytest.mark.gpu

# (B, C_in, C_out, H, W, stride)
CASES = [
    (1, 64, 64, 1, 1, 1),        # one pixel: everything is tail
    (2, 64, 128, 5, 7, 1),       # P = 70: not a multiple of the MFMA K step; spans two images
    (1, 128, 64, 9, 9, 2),       # stride 2, odd H and W: the last sampled row and column is the last of the map
    (2, 64, 64, 8, 6, 2),        # stride 2, even H and W: row 7 and column 5 must never be read
    (1, 192, 320, 6, 6, 1),      # channel counts that are not powers of two (64-wide tiles on both sides)
    (1, 2048, 512, 3, 3, 1),     # the widest channel pair of the R101 nets on a 9-pixel map
    (1, 512, 2048, 3, 3, 1),     # the same pair transposed
    (4, 64, 64, 64, 64, 1),      # one channel tile, 16 384 pixels: exercises the fold
    (2, 256, 64, 46, 45, 2),     # several slices with a ragged last one, at stride 2
]
SLICED, RAGGED = CASES[7], CASES[8]


def _out_hw(case):
    B, Cin, Cout, H, W, st = case
    return (H - 1) // st + 1, (W - 1) // st + 1


@functools.lru_cache(maxsize=None)
def _operands(case):
    """(x, dy) bf16 channels_last on the CPU and the fp64 weight gradient of those rounded operands (torch's fp64 conv2d
    autograd); computed once per case and shared, never modified"""
    B, Cin, Cout, H, W, st = case
    OH, OW = _out_hw(case)
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Cin, H, W, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    dy = torch.randn(B, Cout, OH, OW, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    w = torch.zeros(Cout, Cin, 1, 1, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, None, st, 0).backward(dy.double())
    return x, dy, w.grad.detach()


def _device(case, cuda):
    x, dy, _ = _operands(case)
    return (x.to(cuda).contiguous(memory_format=torch.channels_last), dy.to(cuda).contiguous(memory_format=torch.channels_last))


def _slices(case):
    from torchseg_amd import _lib
    B, Cin, Cout, H, W, st = case
    return _lib.lib().tsg_pw_wgrad_slices(Cin, Cout, B, H, W, st)


def test_cases_cover_the_fold_and_a_ragged_last_slice():
    """at least two cases run several slices, one of them with a last slice shorter than the others (all slices but the
    last hold the same number of 64-pixel chunks, so a chunk count S does not divide means a shorter last slice)"""
    from torchseg_amd import _lib
    lib = _lib.lib()
    assert sum(_slices(c) >= 2 for c in CASES) >= 2
    assert _slices(SLICED) >= 2
    S = _slices(RAGGED)
    B, Cin, Cout, H, W, st = RAGGED
    OH, OW = _out_hw(RAGGED)
    P = B * OH * OW
    assert S >= 2 and (-(-P // 64)) % S != 0 and P % 64 != 0
    assert lib.tsg_pw_wgrad_ws_bytes(Cin, Cout, B, H, W, st) == S * Cout * Cin * 4
    assert _slices(CASES[0]) == 1 and lib.tsg_pw_wgrad_ws_bytes(64, 64, 1, 1, 1, 1) == 0


@pytest.mark.parametrize("case", CASES)
def test_against_float64(cuda, case):
    from torchseg_amd import pwconv
    from torchseg_amd.kernels import provider
    kp = provider()
    x, dy = _device(case, cuda)
    _, _, ref = _operands(case)
    st = case[5]
    assert kp.pw_wgrad_supported(x, dy, st)
    dw = kp.pw_wgrad(x, dy, st)
    assert dw.shape == ref.shape and dw.dtype == torch.float32 and dw.is_contiguous()
    today = pwconv.pointwise_wgrad(x, dy, st) if not pwconv._HIP_WGRAD else None
    got = dw.double().cpu()
    err, bound = (got - ref).abs().max().item(), 1e-4 * ref.abs().max().item() + 1e-6
    rel = ((got - ref).norm() / ref.norm()).item()
    rel_today = ((today.double().cpu() - ref).norm() / ref.norm()).item() if today is not None else float("nan")
    print("pw_wgrad %s S=%d: max err %.3e (bound %.3e), rel L2 %.3e; pointwise_wgrad today rel L2 %.3e"
          % (case, _slices(case), err, bound, rel, rel_today))
    assert bool(torch.isfinite(dw).all())
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("case", CASES)
def test_bit_reproducible(cuda, case):
    from torchseg_amd.kernels import provider
    kp = provider()
    x, dy = _device(case, cuda)
    st = case[5]
    a = kp.pw_wgrad(x, dy, st)
    b = kp.pw_wgrad(x, dy, st)
    out = torch.full_like(a, float("nan"))
    assert kp.pw_wgrad(x, dy, st, out=out) is out
    # an unrelated kernel over 256 MB dirties L2 and the Infinity Cache
    junk = torch.empty(64 << 20, dtype=torch.float32, device=cuda)
    junk.fill_(1.0).mul_(3.0)
    c = kp.pw_wgrad(x, dy, st)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, out) and torch.equal(a, c)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    with pytest.raises(ValueError):
        kp.pw_wgrad(x, dy, st, out=torch.empty(a.shape[1], a.shape[0], 1, 1, device=cuda).permute(1, 0, 2, 3))


@pytest.mark.parametrize("case", CASES)
def test_guard_bands(cuda, case):
    from torchseg_amd.kernels import provider
    kp = provider()
    x, dy = _device(case, cuda)
    st = case[5]
    # plain, then operands and every provider allocation (result and workspace) inside arenas of 0xFF and of 0xA5: no guard
    # byte moves and the three results are bit-identical (a read past a tail or an unwritten output would show)
    results = _guard.three_calls(lambda xx, dd: kp.pw_wgrad(xx, dd, st), [x, dy])
    for r in results:
        assert bool(torch.isfinite(r).all())
    _, _, ref = _operands(case)
    assert (results[1].double().cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-6


def _module(cuda, cin, cout, stride, seed):
    from torchseg_amd.pwconv import PointwiseConv2d, install_pointwise_conv
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 1, stride, 0, bias=False).to(cuda).to(memory_format=torch.channels_last)
    assert install_pointwise_conv(torch.nn.Sequential(conv)) == 1 and isinstance(conv, PointwiseConv2d)
    return conv


@pytest.mark.parametrize("stride", [1, 2])
def test_module_level(cuda, stride, monkeypatch):
    from torchseg_amd import pwconv
    from torchseg_amd.kernels import provider
    kp = provider()
    # forward and stride-2 data gradient are the vendor library's, which at most small shapes does not reproduce ITSELF from
    # run to run (measured with the switch off: 256 -> 128 at 33 x 30, 32 x 32 and 16 x 16, 256 -> 512 at 8 x 8, 256 -> 64 at
    # 64 x 64 and 128 -> 256 at 32 x 32 all differ between two runs); 64 -> 128 at 24 x 40 does at both strides, and only
    # there can "the switch changes nothing but the weight gradient" be held to bit equality.  6 slices / 2 slices.
    B, cin, cout, H, W = 2, 64, 128, 24, 40
    conv = _module(cuda, cin, cout, stride, 11 + stride)
    g = torch.Generator().manual_seed(stride)
    x = torch.randn(B, cin, H, W, generator=g).to(cuda).contiguous(memory_format=torch.channels_last)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = torch.randn(B, cout, OH, OW, generator=g).to(cuda).bfloat16().contiguous(memory_format=torch.channels_last)
    calls = []
    orig = kp.pw_wgrad
    monkeypatch.setattr(kp, "pw_wgrad", lambda *a, **k: (calls.append(1), orig(*a, **k))[1], raising=False)

    def run(flag):
        monkeypatch.setattr(pwconv, "_HIP_WGRAD", flag)
        conv.weight.grad = None
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = conv(xi)
        assert y.dtype == torch.bfloat16
        y.backward(dy)
        torch.cuda.synchronize()
        return y.detach(), xi.grad, conv.weight.grad.clone()

    y0, dx0, dw0 = run(False)
    assert not calls                                     # never without the switch
    y1, dx1, dw1 = run(True)
    assert len(calls) == 1                               # once per layer with it
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    xb = x.bfloat16().contiguous(memory_format=torch.channels_last)
    direct = orig(xb, dy, stride)
    assert dw1.shape == conv.weight.shape and dw1.dtype == torch.float32
    assert torch.equal(dw1.view(torch.int32), direct.view(torch.int32))
    # and both paths compute the same gradient to fp32 accumulation error
    assert (dw1 - dw0).abs().max().item() <= 1e-4 * dw0.abs().max().item() + 1e-6


def test_stream_capture(cuda):
    from torchseg_amd.kernels import provider
    kp = provider()
    case = RAGGED
    assert _slices(case) >= 2
    st = case[5]
    x, dy = _device(case, cuda)
    xs, ds = torch.zeros_like(x), torch.zeros_like(dy)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        kp.pw_wgrad(xs, ds, st)                           # warm-up on the capturing stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):            # one kernel and its fold: a linear graph
        out = kp.pw_wgrad(xs, ds, st)
    g = torch.Generator().manual_seed(99)
    for rep in range(2):
        xn = torch.randn(x.shape, generator=g).to(cuda).bfloat16().contiguous(memory_format=torch.channels_last)
        dn = torch.randn(dy.shape, generator=g).to(cuda).bfloat16().contiguous(memory_format=torch.channels_last)
        xs.copy_(xn)
        ds.copy_(dn)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager = kp.pw_wgrad(xn, dn, st)
        torch.cuda.synchronize()
        assert bool(out.abs().max() > 0)
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)), rep
