"""GPU: the fused 1x1 convolution + BatchNorm (+ residual) (+ ReLU) of inference (csrc/pwbn.hip) against float64 on the
same rounded operands.

  1. exact data: every sum is exact in any order, the output must be BIT-equal to the float64 value rounded once;
  2. random data against float64 within the bound derived from the formats, per element (test_convbn_gpu._fused_tol with
     K = C_in), two calls bit-identical, operands untouched;
  3. operands and output inside poisoned guard bands (tests/_guard.py), three calls bit-identical, and the same result with
     x, residual and y at 16- and 48-byte offsets inside larger poisoned allocations;
  4. modules through prepare_inference(fuse_pointwise=True), with fuse_convbn off and on: the launch counts of both counters,
     the float64 composition with the bound carried through the stages, the untouched input, the stock path in train mode and
     with gradients enabled, and the pack cache;
  5. reproducibility as a property: an identity Bottleneck with both switches runs no vendor convolution, so five eager
     calls and the graph replay are bit-identical WITHOUT pinning the vendor library;
  6. ResNet-50 and BiSeNet-R18 with both switches: counts, the graph capture finding the packs ready, the pending tail and
     the Evaluator, and the distance from the fp32 parity run against the bf16 arm without the 1x1 fusion;
  7. the switch's default.

Shapes (B, H, W, C_in, C_out, stride), the smallest at which the tiling (64 output channels x 256 flat output pixels per
block step, chunks of 64 input channels, two filter buffers) can go wrong: test_pwbn_cpu.CASES."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import _guard
from test_convbn_cpu import _r18, _randomise_bn
from test_convbn_gpu import _Val, _assert_within, _fused_tol, _layer64
from test_pwbn_cpu import CASES, R18_INSTALLED, R18_ON_PATH, _r50

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

pytestmark = pytest.mark.gpu

COMBOS = [(False, True), (False, False), (True, True), (True, False)]      # (residual, relu)
CL = torch.channels_last
BF = torch.bfloat16
_ids = lambda c: "x".join(map(str, c))


@pytest.fixture(autouse=True)
def _restore_process_globals(monkeypatch):
    """prepare_inference switches syncbn.PREFER_CHANNELS_LAST_OUTPUT on for the process"""
    from torchseg_amd import syncbn
    monkeypatch.setattr(syncbn, "PREFER_CHANNELS_LAST_OUTPUT", syncbn.PREFER_CHANNELS_LAST_OUTPUT)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", torch.backends.cudnn.benchmark)


@pytest.fixture
def _pin_vendor_library(monkeypatch):
    """test_convbn_gpu._pin_vendor_library's setting: a bit-for-bit comparison of the STOCK path against itself needs the
    vendor library's deterministic kernels; the fused kernels do not read the setting."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


def _out_hw(case):
    B, H, W, Cin, Cout, s = case
    return (H - 1) // s + 1, (W - 1) // s + 1


def _operands(case, exact, seed=0):
    """CPU operands: x and residual already rounded to bf16, w fp32 [Cout,Cin,1,1] (bf16-representable when exact), fp32 a, b"""
    B, H, W, Cin, Cout, s = case
    OH, OW = _out_hw(case)
    g = torch.Generator().manual_seed(seed + 1000 * Cin + Cout + 7 * H + s)
    if exact:
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
        x = ri(-2, 2, B, Cin, H, W)
        w = ri(-1, 1, Cout, Cin, 1, 1)
        a = torch.pow(2.0, ri(-1, 1, Cout))
        b = ri(-16, 16, Cout) / 4
        res = ri(-4, 4, B, Cout, OH, OW)
    else:
        x = torch.randn(B, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 1, 1, generator=g) * (2.0 / Cin) ** 0.5
        a = 0.5 + torch.rand(Cout, generator=g)
        a = a * torch.where(torch.rand(Cout, generator=g) < 0.25, -1.0, 1.0)
        b = torch.randn(Cout, generator=g) * 0.5
        res = torch.randn(B, Cout, OH, OW, generator=g)
    return x.to(BF), w, a, b, res.to(BF)


_REF = {}


def _ref64(case, exact, seed=0):
    """(operands, u64, S): the float64 1x1 convolution of the bf16-rounded operands and the same sum of absolute values;
    computed once per case and shared"""
    key = (case, exact, seed)
    if key not in _REF:
        s = case[5]
        ops = _operands(case, exact, seed)
        x = ops[0].double()[:, :, ::s, ::s]
        w = ops[1].to(BF).double()[:, :, 0, 0]
        _REF[key] = (ops, torch.einsum("oc,bchw->bohw", w, x), torch.einsum("oc,bchw->bohw", w.abs(), x.abs()))
    return _REF[key]


def _epilogue64(u, a, b, res, relu):
    v = a.double().view(1, -1, 1, 1) * u + b.double().view(1, -1, 1, 1)
    if res is not None:
        v = v + res.double()
    return v.clamp_min(0.0) if relu else v


def _device_operands(ops, dev):
    x, w, a, b, res = ops
    fp = torch.stack([a, b, torch.zeros_like(a)]).to(dev)                 # rows 0, 1 of a fwd_pack [3][C_out]
    return x.to(dev).contiguous(memory_format=CL), w.to(dev), fp, res.to(dev).contiguous(memory_format=CL)


def _check(got, case, u, S, a, b, res, relu, what):
    y64 = _epilogue64(u, a, b, res, relu)
    aS = a.double().abs().view(1, -1, 1, 1) * S
    mag = aS + b.double().abs().view(1, -1, 1, 1) + (res.double().abs() if res is not None else 0.0)
    tol = _fused_tol(y64, aS, mag, case[3])
    err = (got.double().cpu() - y64).abs()
    bad = ~(err <= tol)
    print("pwbn %s: max err %.3e, max err / tol %.3f" % (what, float(err.max()), float((err / tol).max())))
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err - tol).max()))


def test_only_the_last_case_makes_a_block_walk_two_tiles(cuda):
    from torchseg_amd import kernels as K
    kp = K.provider()
    ntiles, nslots, noct, grid, lds = kp.conv1x1_bnact_plan(*CASES[-1])
    B, H, W, Cin, Cout, s = CASES[-1]
    assert Cout == 512 and B * H * W * Cout <= 10_000_000
    assert (ntiles, nslots, noct, grid) == (66, 64, 8, 512) and ntiles > nslots
    for case in CASES[:-1]:
        ntiles, nslots, _, _, _ = kp.conv1x1_bnact_plan(*case)
        assert ntiles <= nslots


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_exact_data_is_bit_equal_to_float64(cuda, case):
    """x in [-2, 2] integers, w in {-1, 0, 1}, a in {1/2, 1, 2}, b multiples of 1/4 in [-4, 4], residual integers in
    [-4, 4]: |u| <= 2 C_in <= 512 is an integer, a u + b + r a multiple of 1/4 below 2^12: exact in fp32 in any order; the
    only rounding is the last one."""
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout, s = case
    ops, u, _ = _ref64(case, True)
    x, w, a, b, res = ops
    xd, wd, fp, resd = _device_operands(ops, cuda)
    assert kp.conv1x1_bnact_supported(xd, Cout, s)
    pack = kp.conv1x1_bnact_pack(wd, None, fp)
    assert float(u.abs().max()) <= 2 * Cin <= 512 and float(u.abs().max()) * 2 + 8 < 2 ** 12
    for with_res, relu in COMBOS:
        y = kp.conv1x1_bnact_fwd(xd, pack, Cout, s, resd if with_res else None, relu)
        want = _epilogue64(u, a, b, res if with_res else None, relu)
        assert torch.equal(want, want.float().double())                 # the float64 value is an fp32 number
        want = want.float().to(BF)
        assert y.dtype == BF and y.shape == want.shape and y.is_contiguous(memory_format=CL)
        got = y.cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
            (case, with_res, relu, int((got != want).sum()), float((got.float() - want.float()).abs().max()))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_random_data_against_float64(cuda, case):
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout, s = case
    ops, u, S = _ref64(case, False)
    x, w, a, b, res = ops
    xd, wd, fp, resd = _device_operands(ops, cuda)
    pack = kp.conv1x1_bnact_pack(wd, None, fp)
    xk, rk = xd.clone(), resd.clone()
    for with_res, relu in COMBOS:
        r = resd if with_res else None
        y = kp.conv1x1_bnact_fwd(xd, pack, Cout, s, r, relu)
        y2 = kp.conv1x1_bnact_fwd(xd, pack, Cout, s, r, relu)
        torch.cuda.synchronize()
        assert y.dtype == BF and y.is_contiguous(memory_format=CL)
        assert torch.equal(_guard.raw_bytes(y), _guard.raw_bytes(y2))   # bit-identical from launch to launch
        _check(y, case, u, S, a, b, res if with_res else None, relu, (case, with_res, relu))
    assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(xk)) and torch.equal(_guard.raw_bytes(resd), _guard.raw_bytes(rk))
    # a foreign pack, and a residual of the wrong shape, dtype or layout, are refused by the provider
    from torchseg_amd._lib import TsgError
    with pytest.raises(TsgError):
        kp.conv1x1_bnact_fwd(xd, (pack[0][:-8], pack[1]), Cout, s, None, True)
    with pytest.raises(TsgError):
        kp.conv1x1_bnact_fwd(xd, pack, Cout, s, resd.float(), True)
    with pytest.raises(TsgError):
        kp.conv1x1_bnact_fwd(xd, pack, Cout, s, resd.contiguous(), True)
    with pytest.raises(TsgError):
        kp.conv1x1_bnact_fwd(xd, pack, Cout, s, resd[:, :, :-1], True)


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", [CASES[2], CASES[3]], ids=_ids)
def test_inside_guard_bands(cuda, case, with_res):
    """The ragged stride-1 and stride-2 cases.  Operands in guarded arenas, pack and output allocated through
    Guarded(fill) under both fills: no guard byte moves and the three results are bit-identical; then the raw entry point
    with x, residual and y at 16- and 48-byte offsets inside larger poisoned allocations: the same bits again, and not a
    byte around y has moved."""
    from torchseg_amd import _lib, kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout, s = case
    ops, u, S = _ref64(case, False, seed=3)
    x, w, a, b, res = ops
    xd, wd, fp, resd = _device_operands(ops, cuda)

    def layer(xx, ww, fwd_pack, rr):
        return kp.conv1x1_bnact_fwd(xx, kp.conv1x1_bnact_pack(ww, None, fwd_pack), Cout, s, rr, True)

    plain = _guard.three_calls(layer, [xd, wd, fp, resd if with_res else None])[0]
    _check(plain, case, u, S, a, b, res if with_res else None, True, (case, with_res))

    def inside(t, off, fill):
        """t's NHWC bytes at element offset `off` of a larger poisoned bf16 buffer -> (buffer, the view)"""
        n = t.numel()
        buf = torch.full((n + 2 * off + 64,), fill, dtype=torch.int16, device=cuda).view(BF)
        view = buf[off:off + n].view(t.shape[0], t.shape[2], t.shape[3], t.shape[1]).permute(0, 3, 1, 2)
        return buf, view

    wf, ab = kp.conv1x1_bnact_pack(wd, None, fp)
    bx, vx = inside(xd, 8, -1)
    vx.copy_(xd)
    br, vr = inside(resd, 24, -1)
    vr.copy_(resd)
    by, vy = inside(plain, 24, 0x5a5a)
    assert vx.data_ptr() % 32 == 16 and vr.data_ptr() % 64 == 48 and vy.data_ptr() % 16 == 0
    assert vx.is_contiguous(memory_format=CL)
    _lib.call(kp.lib.tsg_conv1x1_bnact_fwd, vx.data_ptr(), wf.data_ptr(), ab.data_ptr(), vr.data_ptr() if with_res else None,
              vy.data_ptr(), B, H, W, Cin, Cout, s, 1, _lib.stream_ptr(vx))
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(vy), _guard.raw_bytes(plain))
    raw = by.view(torch.int16)
    assert bool((raw[:24] == 0x5a5a).all()) and bool((raw[24 + plain.numel():] == 0x5a5a).all())
    assert bool((bx.view(torch.int16)[:8] == -1).all()) and bool((bx.view(torch.int16)[8 + xd.numel():] == -1).all())
    # a misaligned operand is refused before any launch
    for k in range(3):
        ptrs = [vx.data_ptr(), vr.data_ptr(), vy.data_ptr()]
        ptrs[k] += 2
        assert kp.lib.tsg_conv1x1_bnact_fwd(ptrs[0], wf.data_ptr(), ab.data_ptr(), ptrs[1], ptrs[2], B, H, W, Cin, Cout, s, 1,
                                            _lib.stream_ptr(vx)) == -4


# ---- module level ------------------------------------------------------------------------------------------------------
def _cbr(seed, relu=True):
    from seg_opr.seg_oprs import ConvBnRelu
    torch.manual_seed(seed)
    return ConvBnRelu(128, 192, 1, 1, 0, has_bias=relu, has_relu=relu)


def _bottleneck(seed, inplanes, stride, shortcut):
    from base_model.resnet import Bottleneck, _shortcut
    torch.manual_seed(seed)
    ds = _shortcut(inplanes, 256, stride, nn.BatchNorm2d, 1e-5, 0.1) if shortcut else None
    return Bottleneck(inplanes, 64, stride, nn.BatchNorm2d, downsample=ds)


def _basic(seed):
    from base_model.resnet import BasicBlock, _shortcut
    torch.manual_seed(seed)
    return BasicBlock(64, 128, 2, nn.BatchNorm2d, downsample=_shortcut(64, 128, 2, nn.BatchNorm2d, 1e-5, 0.1))


def _is_cbn_3x3(conv):
    return conv.kernel_size == (3, 3) and conv.stride == (1, 1)


def _cbr_ref(m, x, dev, cb):
    return _layer64(x, m.conv, m.bn, dev, relu=m.has_relu)


def _shortcut_ref(m, x, dev):
    return x if m.downsample is None else _layer64(x, m.downsample[0], m.downsample[1], dev, relu=False)


def _bottleneck_ref(m, x, dev, cb):
    out = _layer64(x, m.conv1, m.bn1, dev)
    out = _layer64(out, m.conv2, m.bn2, dev, fused=cb and _is_cbn_3x3(m.conv2))
    return _layer64(out, m.conv3, m.bn3, dev, res=_shortcut_ref(m, x, dev))


def _basic_ref(m, x, dev, cb):
    out = _layer64(x, m.conv1, m.bn1, dev, fused=cb and _is_cbn_3x3(m.conv1))
    return _layer64(out, m.conv2, m.bn2, dev, res=_shortcut_ref(m, x, dev), fused=cb)


# name: (builder, input channels, launches of ours per call, convbn's launches per call when it is installed,
#        float64 composition, the BatchNorm of one fused 1x1 layer)
MODULES = {"convbnrelu-bias": (lambda: _cbr(1), 128, 1, 0, _cbr_ref, lambda m: m.bn),
           "convbn-norelu": (lambda: _cbr(2, relu=False), 128, 1, 0, _cbr_ref, lambda m: m.bn),
           "bottleneck": (lambda: _bottleneck(3, 256, 1, False), 256, 2, 1, _bottleneck_ref, lambda m: m.bn3),
           "bottleneck-s2": (lambda: _bottleneck(4, 64, 2, True), 64, 3, 0, _bottleneck_ref, lambda m: m.bn1),
           "bottleneck-dilated": (lambda: _bottleneck(5, 64, 1, True), 64, 3, 1, _bottleneck_ref, lambda m: m.downsample[1]),
           "basicblock-s2": (lambda: _basic(6), 64, 1, 1, _basic_ref, lambda m: m.downsample[1])}


@pytest.mark.parametrize("cb", [False, True], ids=["pw", "pw+convbn"])
@pytest.mark.parametrize("name", list(MODULES))
def test_modules(cuda, name, cb, _pin_vendor_library):
    from torchseg_amd import convbn, pwbn
    from torchseg_amd.infer import prepare_inference
    build, Cin, launches, cbn_launches, ref, fused_bn = MODULES[name]
    cbn_launches = cbn_launches if cb else 0
    base = _randomise_bn(build(), 7).eval()
    on = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=cb, fuse_pointwise=True)
    off = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=cb, fuse_pointwise=False)
    assert on.fused_pointwise == launches and off.fused_pointwise == 0
    assert on.fused_convbn == off.fused_convbn == cbn_launches
    x = torch.randn(2, Cin, 18, 40, generator=torch.Generator().manual_seed(8)).to(BF)
    xd = x.to(cuda).contiguous(memory_format=CL)
    keep = xd.clone()

    y = on(xd)
    torch.cuda.synchronize()
    # the BasicBlock's shortcut: in eval mode without gradients the stock forward forms the residual through _identity
    # (conv_with_skip hands out no alias there), so it is ours with convbn's mixin and without
    assert pwbn.fused_calls(on.module) == launches and convbn.fused_calls(on.module) == cbn_launches
    assert y.dtype == BF and y.data_ptr() != xd.data_ptr()
    assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(keep))      # the input, which is the identity block's residual
    _assert_within(y, ref(on.module, _Val(x.double()), cuda, cb), "pwbn " + name)

    # train mode, and eval mode with gradients enabled: the replaced method, bit for bit (the vendor library pinned), called
    # exactly once with the module's own input, and no counter moves
    calls = []
    stock_cls = type(off.module)
    assert isinstance(on.module, stock_cls) and type(on.module) is not stock_cls
    stock_forward = stock_cls.forward

    def recording(self, *a, **k):
        calls.append((self, a[0] if a else None))
        return stock_forward(self, *a, **k)

    def run(m, xin, train, grad, dtype):
        m.train(train)
        with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=BF, enabled=dtype == BF):
            out = m(xin).detach().clone()
        m.eval()
        return out

    arms = {BF: (on, off, xd)}
    arms[torch.float32] = (prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_convbn=cb, fuse_pointwise=True),
                           prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_convbn=cb, fuse_pointwise=False),
                           x.float().to(cuda).contiguous(memory_format=CL))
    mismatch = []
    for dtype, (m_on, m_off, xin) in arms.items():
        modes = ((False, True), (True, False), (True, True)) + (((False, False),) if dtype == torch.float32 else ())
        for train, grad in modes:
            before = pwbn.fused_calls(m_on.module), convbn.fused_calls(m_on.module)
            stock_cls.forward = recording
            try:
                del calls[:]
                o_on = run(m_on.module, xin, train, grad, dtype)
                assert len(calls) == 1 and calls[0][0] is m_on.module and calls[0][1] is xin, (name, dtype, train, grad)
            finally:
                stock_cls.forward = stock_forward
            o_off = run(m_off.module, xin, train, grad, dtype)
            torch.cuda.synchronize()
            assert (pwbn.fused_calls(m_on.module), convbn.fused_calls(m_on.module)) == before, (name, dtype, train, grad)
            same = torch.equal(_guard.raw_bytes(o_on), _guard.raw_bytes(o_off))
            print("pwbn module %s %s train=%s grad=%s: re-classed and un-installed copy bit-equal: %s"
                  % (name, dtype, train, grad, same))
            if not same:
                mismatch.append((name, dtype, train, grad, float((o_on.float() - o_off.float()).abs().max())))
    assert not mismatch, mismatch
    assert pwbn.fused_calls(on.module) == launches
    for (k, p), (_, q) in zip(on.module.state_dict().items(), off.module.state_dict().items()):
        assert torch.equal(p, q), k                                         # the running statistics moved alike

    # the pack cache: an in-place write to running_var, then a whole state dict
    bn = fused_bn(on.module)
    before = on(xd).clone()
    with torch.no_grad():
        bn.running_var.mul_(4.0)
    after = on(xd).clone()
    torch.cuda.synchronize()
    assert pwbn.fused_calls(on.module) == 3 * launches and not torch.equal(before, after)
    _assert_within(after, ref(on.module, _Val(x.double()), cuda, cb), "pwbn " + name + " after running_var.mul_(4)")
    other = _randomise_bn(build(), 17).state_dict()
    on.module.load_state_dict(other)
    y3 = on(xd)
    torch.cuda.synchronize()
    assert pwbn.fused_calls(on.module) == 4 * launches
    _assert_within(y3, ref(on.module, _Val(x.double()), cuda, cb), "pwbn " + name + " after load_state_dict")
    # one fused layer's BatchNorm alone in train mode: that layer runs the replaced method, the running statistics move
    # inside a kernel (no tensor version counts it), and the next eval call must read the moved values
    bn = fused_bn(on.module)
    bn.train()
    on(xd)
    bn.eval()
    y4 = on(xd)
    torch.cuda.synchronize()
    assert pwbn.fused_calls(on.module) >= 5 * launches
    _assert_within(y4, ref(on.module, _Val(x.double()), cuda, cb), "pwbn " + name + " after a train-mode call of the BatchNorm alone")


def test_identity_bottleneck_is_reproducible_without_pinning_the_vendor_library(cuda):
    """conv1 and conv3 are ours (pwbn.hip), conv2 is ours (convbn.hip): no vendor convolution runs, so bit-reproducibility
    is a property of the block.  torch.backends.cudnn.deterministic is left alone."""
    from torchseg_amd import convbn, pwbn
    from torchseg_amd.infer import prepare_inference
    assert not torch.backends.cudnn.deterministic
    base = _randomise_bn(_bottleneck(31, 256, 1, False), 32).eval().to(cuda)
    eager = prepare_inference(copy.deepcopy(base), dtype=BF, fuse_convbn=True, fuse_pointwise=True)
    graph = prepare_inference(copy.deepcopy(base), dtype=BF, graph=True, fuse_convbn=True, fuse_pointwise=True)
    xs = [torch.randn(2, 256, 18, 40, generator=torch.Generator().manual_seed(s)).to(BF).to(cuda).contiguous(memory_format=CL)
          for s in (33, 34)]
    outs = [eager(xs[0]).clone() for _ in range(5)]
    torch.cuda.synchronize()
    assert all(torch.equal(_guard.raw_bytes(outs[0]), _guard.raw_bytes(o)) for o in outs[1:])
    assert (convbn.fused_calls(eager.module), pwbn.fused_calls(eager.module)) == (5, 10)     # all three convolutions
    replays = []
    for x in xs:
        a = eager(x).clone()
        b = graph(x).clone()
        torch.cuda.synchronize()
        assert torch.equal(_guard.raw_bytes(a), _guard.raw_bytes(b))
        replays.append(b)
    assert not torch.equal(replays[0], replays[1])
    assert convbn.fused_calls(graph.module) + pwbn.fused_calls(graph.module) == 2 * 3        # the warm-up and the capture


# ---- networks ----------------------------------------------------------------------------------------------------------
def _rel(o, p):
    return float((o.float() - p.float()).abs().max() / p.float().abs().max())


def _on_path(net, names):
    from torchseg_amd.pwbn import eligible_layers
    mods = dict(net.named_modules())
    return sum(len(eligible_layers(mods[n])[1]) for n in names)


def test_networks_against_the_fp32_parity_run(cuda):
    """Per backbone stage of ResNet-50 and for BiSeNet-R18's log-probabilities: with the 1x1 layers fused the bf16 network is
    at most 1.25 x as far from the fp32 parity run as the bf16 network with fuse_convbn alone (the factor
    tests/test_sepconv_gpu.py and tests/test_convbn_gpu.py use for the same comparison)."""
    from torchseg_amd import convbn, pwbn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    backbone = _r50(11).eval()
    full = _r18(13).eval()
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(14)).to(cuda)
    for label, base, n_pw, n_cbn in (("resnet50", backbone, 36, 13), ("bisenet-r18", full, len(R18_ON_PATH), 18)):
        arms = dict(parity=prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_convbn=True, fuse_pointwise=True),
                    without=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=True, fuse_pointwise=False),
                    fused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=True, fuse_pointwise=True))
        outs = {}
        for k, m in arms.items():
            o = m(x)
            o = [materialize(o)] if label == "bisenet-r18" else list(o)
            outs[k] = [t.clone() for t in o]
        torch.cuda.synchronize()
        assert pwbn.fused_calls(arms["fused"].module) == n_pw and convbn.fused_calls(arms["fused"].module) == n_cbn
        assert pwbn.fused_calls(arms["without"].module) == 0 and convbn.fused_calls(arms["without"].module) == n_cbn
        assert pwbn.fused_calls(arms["parity"].module) == 0             # fp32: the parity mode stays on the exact kernels
        dist = []
        for k, (pu, pf, pp) in enumerate(zip(outs["without"], outs["fused"], outs["parity"])):
            u, f = _rel(pu, pp), _rel(pf, pp)
            dist.append((u, f))
            what = "stage 1/%d" % (4 << k) if label == "resnet50" else "log-probabilities"
            print("pwbn parity [%s] %s: max |d| / max |fp32 parity|: bf16 fuse_convbn alone %.4e, with fuse_pointwise %.4e "
                  "(ratio %.3f)" % (label, what, u, f, f / u))
        for k, (u, f) in enumerate(dist):
            assert f <= 1.25 * u, (label, k, f, u)


@pytest.mark.parametrize("which", ["resnet50", "bisenet-r18"])
def test_networks_eager_graph_and_pending_tail(cuda, which):
    """The counts of the CPU test's lists, the graph capture finding the packs ready, and for BiSeNet-R18 the pending tail.
    Eager against replay is NOT compared bit for bit: the stems and stride-2 3x3 layers are still the vendor library's."""
    from torchseg_amd import convbn, pwbn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import pending_tail, prepare_inference
    if which == "resnet50":
        net = _r50(21).eval()
        installed, on_path, cbn_path = 36, 36, 13
        assert sum(len(pwbn.eligible_layers(m)[1]) for m in net.modules()) == installed
    else:
        net = _r18(21).eval()
        installed, on_path, cbn_path = len(R18_INSTALLED), _on_path(net, R18_ON_PATH), 18
        assert on_path == 4 and sorted(n for n, m in net.named_modules() if pwbn.eligible_layers(m)[0]) == sorted(R18_INSTALLED)
    net = net.to(cuda)
    eager = prepare_inference(copy.deepcopy(net), dtype=BF, fuse_convbn=True, fuse_pointwise=True)
    graph = prepare_inference(copy.deepcopy(net), dtype=BF, graph=True, fuse_convbn=True, fuse_pointwise=True)
    assert eager.fused_pointwise == installed and graph.fused_pointwise == installed
    replays = []
    for seed in (1, 2):
        x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(seed)).to(cuda)
        out = eager(x)
        if which == "bisenet-r18":
            tail = pending_tail(out)
            assert tail is not None and tuple(tail[1]) == (64, 128) and tail[0].shape[1] == 19     # still the pending head
            a = [materialize(out).clone()]
            b = [graph(x).clone()]
            assert a[0].shape == (1, 19, 64, 128)
        else:
            a = [t.clone() for t in out]
            b = [t.clone() for t in graph(x)]
            assert [t.shape[1] for t in a] == [256, 512, 1024, 2048]
        torch.cuda.synchronize()
        for s, t in zip(a, b):
            assert bool(torch.isfinite(s.float()).all()) and s.shape == t.shape
            d = float((s.float() - t.float()).abs().max())
            print("pwbn %s seed %d: max |eager - replay| %.3e of max |eager| %.3e" % (which, seed, d, float(s.float().abs().max())))
        replays.append(b[-1])
    assert not torch.equal(replays[0], replays[1])
    assert pwbn.fused_calls(eager.module) == 2 * on_path and convbn.fused_calls(eager.module) == 2 * cbn_path
    # the warm-up and the capture; the packs were ready for the capture
    assert pwbn.fused_calls(graph.module) == 2 * on_path and convbn.fused_calls(graph.module) == 2 * cbn_path


MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


def test_r18_evaluator_consumes_the_pending_tail(cuda, monkeypatch):
    """TSG_INFER=1 with TSG_CONVBN_FUSED=1 and TSG_PWBN_FUSED=1: sliding_eval takes the fused window tail (the pending value
    reaches the Evaluator), and the class map equals the one of the same evaluator on the eager path."""
    from engine.evaluator import Evaluator
    from torchseg_amd import convbn, pwbn
    net = _r18(31).eval()
    monkeypatch.delenv("TSG_DTYPE", raising=False)
    monkeypatch.setenv("TSG_INFER", "1")
    monkeypatch.setenv("TSG_CONVBN_FUSED", "1")
    monkeypatch.setenv("TSG_PWBN_FUSED", "1")
    img = np.random.RandomState(0).randint(0, 256, (96, 160, 3)).astype(np.uint8)
    ev = Evaluator(None, 19, MEAN, STD, copy.deepcopy(net), [1.0], False, [0])
    ev.val_func = ev.network
    taken = []
    stock = ev._fused_window_scores
    monkeypatch.setattr(ev, "_fused_window_scores", lambda *a, **k: taken.append(stock(*a, **k)) or taken[-1])
    pred = ev.sliding_eval(img, 96, 2 / 3, device=0)
    assert pred.shape == (96, 160) and pred.min() >= 0 and pred.max() < 19
    assert taken and all(t is not None for t in taken)
    assert ev._infer_net.fused_pointwise == len(R18_INSTALLED) and ev._infer_net.fused_convbn == 20
    assert pwbn.fused_calls(ev._infer_net.module) >= len(R18_ON_PATH) and convbn.fused_calls(ev._infer_net.module) >= 18
    monkeypatch.setattr(ev, "_fused_window_scores", lambda *a, **k: None)
    eager = ev.sliding_eval(img, 96, 2 / 3, device=0)
    assert np.array_equal(pred, eager), int((pred != eager).sum())


def test_switch_unset_installs_nothing(cuda, monkeypatch, _pin_vendor_library):
    """Unset, or off: nothing is re-classed and the output is the path's without the feature, bit for bit, in the fp32
    parity mode and in bf16 (the vendor library pinned to its deterministic kernels)."""
    from torchseg_amd import convbn, pwbn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    monkeypatch.delenv("TSG_DTYPE", raising=False)
    monkeypatch.delenv("TSG_CONVBN_FUSED", raising=False)
    monkeypatch.delenv("TSG_PWBN_FUSED", raising=False)
    net = _r18(41).eval().to(cuda)
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(42)).to(cuda)
    for dtype in (torch.float32, BF):
        unset = prepare_inference(copy.deepcopy(net), dtype=dtype)
        off = prepare_inference(copy.deepcopy(net), dtype=dtype, fuse_pointwise=False)
        for m in (unset, off):
            assert m.fused_pointwise == 0 and not any(isinstance(k, pwbn._FusedPointwise) for k in m.modules())
            assert all(type(k).__module__ != pwbn.__name__ for k in m.modules())
        a, b = materialize(unset(x)).clone(), materialize(off(x)).clone()
        torch.cuda.synchronize()
        print("pwbn switch unset, %s: max |unset - off| %.3e" % (dtype, float((a - b).abs().max())))
        assert torch.equal(a, b), dtype
    monkeypatch.setenv("TSG_PWBN_FUSED", "0")
    assert prepare_inference(copy.deepcopy(net)).fused_pointwise == 0
    monkeypatch.setenv("TSG_PWBN_FUSED", "1")
    on = prepare_inference(copy.deepcopy(net))
    assert on.fused_pointwise == len(R18_INSTALLED) and on.fused_convbn == 0
    materialize(on(x))
    assert pwbn.fused_calls(on.module) == len(R18_ON_PATH) and convbn.fused_calls(on.module) == 0
