"""GPU: the fused 3x3 convolution + BatchNorm (+ residual) (+ ReLU) of inference (csrc/convbn.hip) against torch's CPU
float64 convolutions on the same rounded operands.

  1. exact data: every sum is exact in any order, the output must be BIT-equal to the float64 value rounded once;
  2. random data against float64 within a bound derived from the formats, per element (see _fused_tol);
  3. operands and output inside poisoned guard bands (tests/_guard.py), three calls bit-identical, and the same result with
     x, residual and y at 16-byte-aligned offsets inside larger allocations;
  4. modules: a ConvBnRelu, a BasicBlock (identity and stride-2 / downsample forms) and a Bottleneck against the float64
     composition with the bound carried through the stages, the counters, the untouched operands, the stock path in
     train mode and with gradients enabled, and the pack cache;
  5. BiSeNet-R18 through prepare_inference(fuse_convbn=True): counts, eager against graph replay, the pending tail and the
     Evaluator, and the distance from the fp32 parity run against the unfused bf16 path's;
  6. the switch's default.

Shapes (B, H, W, C_in, C_out), the smallest at which the tiling can go wrong: a map smaller than one 8 x 32 tile with one
chunk of 16 input channels; an exact tile, two images, two chunks (both buffers of the double buffering); ragged in both
directions with an odd chunk count and two oc tiles; several tiles and three oc tiles; and 72 x 256 at C_out = 512, where the
kernel's own plan has 64 blocks per oc tile for 72 tiles, so that a block walks more than one tile."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _guard
from test_convbn_cpu import CASES, _r18, _randomise_bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

pytestmark = pytest.mark.gpu

COMBOS = [(False, True), (False, False), (True, True), (True, False)]      # (residual, relu)
CL = torch.channels_last
BF = torch.bfloat16
U32 = 2.0 ** -24                                                            # unit roundoff of fp32
_ids = lambda c: "x".join(map(str, c))


@pytest.fixture(autouse=True)
def _restore_process_globals(monkeypatch):
    """prepare_inference switches syncbn.PREFER_CHANNELS_LAST_OUTPUT on for the process"""
    from torchseg_amd import syncbn
    monkeypatch.setattr(syncbn, "PREFER_CHANNELS_LAST_OUTPUT", syncbn.PREFER_CHANNELS_LAST_OUTPUT)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", torch.backends.cudnn.benchmark)


# ---- the bound ---------------------------------------------------------------------------------------------------------
def _half_ulp_bf16(v):
    """half a unit in the last place of bf16 (7 explicit mantissa bits) at magnitude v (float64)"""
    return torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 8)


def _gamma(k):
    return k * U32 / (1 - k * U32)


def _fused_tol(y64, aS, mag, K, tol_in=0.0):
    """Bound of |kernel - y64| per element, y64 = relu?(a u + b + r) evaluated in float64 on the operands the kernel reads:
      e   = |a| gamma_K sum|w||x|        fp32 accumulation of K = 9 C_in exact products of bf16 values, in any order
          + 2.01 u (|a| sum|w||x| + |b| + |r|)   the rounding of the fma and of the addition, u = 2^-24 (the factor .01 covers
                                                   the second-order terms (1 + gamma_K)(1 + u) for K <= 10^4)
          + tol_in                                 what the caller knows about the error of the operands themselves
      tol = e + half a bf16 ulp at |y64| + e       the one rounding, at the largest magnitude the fp32 value can have
    (ReLU does not increase a difference.)"""
    e = _gamma(K) * aS + 2.01 * U32 * mag + tol_in
    return e + _half_ulp_bf16(y64.abs() + e)


def _operands(case, exact, seed=0):
    """CPU operands: x and residual already rounded to bf16, w fp32 (bf16-representable when exact), fp32 a, b"""
    B, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(seed + 1000 * Cin + Cout + 7 * H)
    if exact:
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
        x = ri(-2, 2, B, Cin, H, W)
        w = ri(-1, 1, Cout, Cin, 3, 3)
        a = torch.pow(2.0, ri(-1, 1, Cout))
        b = ri(-16, 16, Cout) / 4
        res = ri(-4, 4, B, Cout, H, W)
    else:
        x = torch.randn(B, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
        a = 0.5 + torch.rand(Cout, generator=g)
        a = a * torch.where(torch.rand(Cout, generator=g) < 0.25, -1.0, 1.0)
        b = torch.randn(Cout, generator=g) * 0.5
        res = torch.randn(B, Cout, H, W, generator=g)
    return x.to(BF), w, a, b, res.to(BF)


_REF = {}


def _ref64(case, exact, seed=0):
    """(operands, u64, S): the float64 convolution of the bf16-rounded operands and the same sum of absolute values;
    computed once per case and shared"""
    key = (case, exact, seed)
    if key not in _REF:
        ops = _operands(case, exact, seed)
        x, w = ops[0].double(), ops[1].to(BF).double()
        _REF[key] = (ops, F.conv2d(x, w, None, 1, 1), F.conv2d(x.abs(), w.abs(), None, 1, 1))
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
    tol = _fused_tol(y64, aS, mag, 9 * case[3])
    err = (got.double().cpu() - y64).abs()
    bad = ~(err <= tol)
    print("convbn %s: max err %.3e, max err / tol %.3f" % (what, float(err.max()), float((err / tol).max())))
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err - tol).max()))


def test_the_largest_case_makes_a_block_walk_two_tiles(cuda):
    from torchseg_amd import kernels as K
    kp = K.provider()
    ntiles, nslots, noct, grid, lds = kp.conv3x3_bnact_plan(*CASES[-1])
    assert (ntiles, nslots, noct, grid) == (72, 64, 8, 512) and ntiles > nslots
    for case in CASES[:-1]:
        ntiles, nslots, _, _, _ = kp.conv3x3_bnact_plan(*case)
        assert ntiles <= nslots


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_exact_data_is_bit_equal_to_float64(cuda, case):
    """x in [-2, 2] integers, w in {-1, 0, 1}, a in {1/2, 1, 2}, b multiples of 1/4 in [-4, 4], residual integers in
    [-4, 4]: |u| <= 2 * 9 * 64 is an integer, a u + b + r a multiple of 1/4 below 2^12: exact in fp32 in any order; the only
    rounding is the last one."""
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout = case
    ops, u, _ = _ref64(case, True)
    x, w, a, b, res = ops
    xd, wd, fp, resd = _device_operands(ops, cuda)
    assert kp.conv3x3_bnact_supported(xd, Cout)
    pack = kp.conv3x3_bnact_pack(wd, None, fp)
    assert float(u.abs().max()) * 2 + 8 < 2 ** 12
    for with_res, relu in COMBOS:
        y = kp.conv3x3_bnact_fwd(xd, pack, Cout, resd if with_res else None, relu)
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
    B, H, W, Cin, Cout = case
    ops, u, S = _ref64(case, False)
    x, w, a, b, res = ops
    xd, wd, fp, resd = _device_operands(ops, cuda)
    pack = kp.conv3x3_bnact_pack(wd, None, fp)
    xk, rk = xd.clone(), resd.clone()
    for with_res, relu in COMBOS:
        r = resd if with_res else None
        y = kp.conv3x3_bnact_fwd(xd, pack, Cout, r, relu)
        y2 = kp.conv3x3_bnact_fwd(xd, pack, Cout, r, relu)
        torch.cuda.synchronize()
        assert y.dtype == BF and y.is_contiguous(memory_format=CL)
        assert torch.equal(_guard.raw_bytes(y), _guard.raw_bytes(y2))   # bit-identical from launch to launch
        _check(y, case, u, S, a, b, res if with_res else None, relu, (case, with_res, relu))
    assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(xk)) and torch.equal(_guard.raw_bytes(resd), _guard.raw_bytes(rk))


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_inside_guard_bands(cuda, case, with_res):
    """Operands in guarded arenas, pack and output allocated through Guarded(fill) under both fills: no guard byte moves
    and the three results are bit-identical; then the raw entry point with x, residual and y at 16- and 48-byte offsets
    inside larger poisoned allocations: the same bits again, and not a byte around y has moved."""
    from torchseg_amd import _lib, kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout = case
    ops, u, S = _ref64(case, False, seed=3)
    x, w, a, b, res = ops
    xd, wd, fp, resd = _device_operands(ops, cuda)

    def layer(xx, ww, fwd_pack, rr):
        return kp.conv3x3_bnact_fwd(xx, kp.conv3x3_bnact_pack(ww, None, fwd_pack), Cout, rr, True)

    plain = _guard.three_calls(layer, [xd, wd, fp, resd if with_res else None])[0]
    _check(plain, case, u, S, a, b, res if with_res else None, True, (case, with_res))

    def inside(t, off, fill):
        """t's NHWC bytes at element offset `off` of a larger poisoned bf16 buffer -> (buffer, the view)"""
        n = t.numel()
        buf = torch.full((n + 2 * off + 64,), fill, dtype=torch.int16, device=cuda).view(BF)
        view = buf[off:off + n].view(t.shape[0], t.shape[2], t.shape[3], t.shape[1]).permute(0, 3, 1, 2)
        return buf, view

    wf, ab = kp.conv3x3_bnact_pack(wd, None, fp)
    bx, vx = inside(xd, 8, -1)
    vx.copy_(xd)
    br, vr = inside(resd, 24, -1)
    vr.copy_(resd)
    by, vy = inside(plain, 24, 0x5a5a)
    assert vx.data_ptr() % 32 == 16 and vy.data_ptr() % 16 == 0 and vx.is_contiguous(memory_format=CL)
    _lib.call(kp.lib.tsg_conv3x3_bnact_fwd, vx.data_ptr(), wf.data_ptr(), ab.data_ptr(), vr.data_ptr() if with_res else None,
              vy.data_ptr(), B, H, W, Cin, Cout, 1, _lib.stream_ptr(vx))
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(vy), _guard.raw_bytes(plain))
    raw = by.view(torch.int16)
    assert bool((raw[:24] == 0x5a5a).all()) and bool((raw[24 + plain.numel():] == 0x5a5a).all())
    # a misaligned operand is refused before any launch
    assert kp.lib.tsg_conv3x3_bnact_fwd(vx.data_ptr() + 2, wf.data_ptr(), ab.data_ptr(), None, vy.data_ptr(), B, H, W, Cin,
                                        Cout, 1, _lib.stream_ptr(vx)) == -4


# ---- module level ------------------------------------------------------------------------------------------------------
class _Val:
    """a float64 value on the CPU with a per-element bound of |device value - value|"""

    def __init__(self, v, tol=None):
        self.v, self.tol = v, torch.zeros_like(v) if tol is None else tol


def _bn_ab(bn, dev):
    """a, b of an eval-mode BatchNorm exactly as the device forms them (tsg_bn_affine of the fp32 tensors)"""
    from torchseg_amd import kernels as K
    with torch.autocast("cuda", enabled=False):
        mean = bn.running_mean.to(dev).float()
        invstd = torch.rsqrt(bn.running_var.to(dev).float() + bn.eps)
        fp = K.provider().bn_affine(mean, invstd, bn.weight.to(dev).float(), bn.bias.to(dev).float())
    torch.cuda.synchronize()
    return fp[0].cpu().double().view(1, -1, 1, 1), fp[1].cpu().double().view(1, -1, 1, 1)


def _layer64(x, conv, bn, dev, res=None, relu=True, fused=True):
    """conv -> bn (+ res) (-> relu) of _Vals.  fused: one rounding (_fused_tol).  Stock chain: the convolution's fp32 sum
    (any order: gamma_K) is rounded to bf16, then fma(a, t, b) + r in fp32 is rounded to bf16 (tsg_bn_apply_fwd)."""
    w = conv.weight.detach().cpu().to(BF).double()
    kw = dict(stride=conv.stride, padding=conv.padding, dilation=conv.dilation)
    K = conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1]
    u = F.conv2d(x.v, w, None, **kw)
    S = F.conv2d(x.v.abs() + x.tol, w.abs(), None, **kw)
    tol_u = F.conv2d(x.tol, w.abs(), None, **kw)
    a, b = _bn_ab(bn, dev)
    bias = conv.bias.detach().cpu().double().view(1, -1, 1, 1) if conv.bias is not None else None
    if bias is not None:
        u = u + bias                                      # the kernel folds it: b' = fl(b + a bias), two roundings of fp32
    r, tol_r = (res.v, res.tol) if res is not None else (0.0, 0.0)
    y = a * u + b + r
    y = y.clamp_min(0.0) if relu else y
    aS = a.abs() * S
    mag = aS + b.abs() + (a.abs() * bias.abs() if bias is not None else 0.0) + (res.v.abs() + res.tol if res is not None else 0.0)
    if fused:
        extra = a.abs() * tol_u + tol_r + (2 * U32 * (b.abs() + a.abs() * bias.abs()) if bias is not None else 0.0)
        return _Val(y, _fused_tol(y, aS, mag, K, extra))
    assert bias is None
    e_u = _gamma(K) * S + tol_u
    tol_t = e_u + _half_ulp_bf16(u.abs() + e_u)
    e = a.abs() * tol_t + 2.01 * U32 * (a.abs() * (u.abs() + tol_t) + b.abs() + (res.v.abs() + res.tol if res is not None else 0.0)) + tol_r
    return _Val(y, e + _half_ulp_bf16(y.abs() + e))


def _assert_within(got, val, what):
    err = (got.double().cpu() - val.v).abs()
    bad = ~(err <= val.tol)
    print("convbn module %s: max err %.3e, max err / bound %.3f" % (what, float(err.max()), float((err / val.tol).max())))
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err - val.tol).max()))


def _cbr(seed):
    from seg_opr.seg_oprs import ConvBnRelu
    torch.manual_seed(seed)
    return ConvBnRelu(48, 128, 3, 1, 1, has_bias=True)


def _basic(seed, stride):
    from base_model.resnet import BasicBlock, _shortcut
    torch.manual_seed(seed)
    if stride == 1:
        return BasicBlock(64, 64, 1, nn.BatchNorm2d)
    return BasicBlock(64, 128, 2, nn.BatchNorm2d, downsample=_shortcut(64, 128, 2, nn.BatchNorm2d, 1e-5, 0.1))


def _bottleneck(seed):
    from base_model.resnet import Bottleneck
    torch.manual_seed(seed)
    return Bottleneck(256, 64, 1, nn.BatchNorm2d)


def _cbr_ref(m, x, dev):
    return _layer64(x, m.conv, m.bn, dev)


def _basic_ref(m, x, dev):
    out = _layer64(x, m.conv1, m.bn1, dev, fused=m.conv1.stride == (1, 1))
    res = x if m.downsample is None else _layer64(x, m.downsample[0], m.downsample[1], dev, relu=False, fused=False)
    return _layer64(out, m.conv2, m.bn2, dev, res=res)


def _bottleneck_ref(m, x, dev):
    out = _layer64(x, m.conv1, m.bn1, dev, fused=False)
    out = _layer64(out, m.conv2, m.bn2, dev)
    return _layer64(out, m.conv3, m.bn3, dev, res=x, fused=False)


# (builder, input channels, launches per call, float64 composition)
MODULES = {"convbnrelu": (lambda: _cbr(1), 48, 1, _cbr_ref),
           "basicblock": (lambda: _basic(2, 1), 64, 2, _basic_ref),
           "basicblock-s2": (lambda: _basic(3, 2), 64, 1, _basic_ref),
           "bottleneck": (lambda: _bottleneck(4), 256, 1, _bottleneck_ref)}


@pytest.fixture
def _pin_vendor_library(monkeypatch):
    """The un-fused path of a network without weight gradients runs the vendor library's convolutions (WrwConv2d and
    PointwiseConv2d route to this package's kernels only with gradients enabled).  For shapes its tuned database does not
    hold, that library's pick can be a kernel whose partial sums meet in atomics: two copies of one module, or two calls,
    then differ in the last bits now and then.  torch.backends.cudnn.deterministic asks it for its deterministic kernels
    only, which is what a bit-for-bit comparison of the STOCK path against itself needs; the fused kernel does not read
    the setting."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


@pytest.mark.parametrize("name", list(MODULES))
def test_modules(cuda, name, _pin_vendor_library):
    from torchseg_amd.convbn import fused_calls
    from torchseg_amd.infer import prepare_inference
    build, Cin, launches, ref = MODULES[name]
    base = _randomise_bn(build(), 7).eval()
    on = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=True)
    off = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=False)
    assert on.fused_convbn == launches and off.fused_convbn == 0
    x = torch.randn(2, Cin, 18, 40, generator=torch.Generator().manual_seed(8)).to(BF)
    xd = x.to(cuda).contiguous(memory_format=CL)
    keep = xd.clone()

    y = on(xd)
    torch.cuda.synchronize()
    assert fused_calls(on.module) == launches and y.dtype == BF and y.data_ptr() != xd.data_ptr()
    assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(keep))      # the input, which is the identity block's residual
    _assert_within(y, ref(on.module, _Val(x.double()), cuda), name)
    # train mode, and eval mode with gradients enabled: the stock method, bit for bit, and the counter does not move.
    # Without weight gradients the stock convolutions of these modules are the vendor library's; this test runs with
    # torch.backends.cudnn.deterministic set (see _pin_vendor_library), under which two un-installed copies repeat.  On
    # top of the outputs: the re-classed module must have called the method it replaced exactly once, with its own input.
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
    arms[torch.float32] = (prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_convbn=True),
                           prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_convbn=False),
                           x.float().to(cuda).contiguous(memory_format=CL))
    mismatch = []
    for dtype, (m_on, m_off, xin) in arms.items():
        modes = ((False, True), (True, False), (True, True)) + (((False, False),) if dtype == torch.float32 else ())
        for train, grad in modes:
            before = fused_calls(m_on.module)
            stock_cls.forward = recording
            try:
                del calls[:]
                o_on = run(m_on.module, xin, train, grad, dtype)
                assert len(calls) == 1 and calls[0][0] is m_on.module and calls[0][1] is xin, (name, dtype, train, grad)
            finally:
                stock_cls.forward = stock_forward
            o_off = run(m_off.module, xin, train, grad, dtype)
            torch.cuda.synchronize()
            assert fused_calls(m_on.module) == before, (name, dtype, train, grad)
            same = torch.equal(_guard.raw_bytes(o_on), _guard.raw_bytes(o_off))
            print("convbn module %s %s train=%s grad=%s: re-classed and un-installed copy bit-equal: %s"
                  % (name, dtype, train, grad, same))
            if not same:
                mismatch.append((name, dtype, train, grad, float((o_on.float() - o_off.float()).abs().max())))
    assert not mismatch, mismatch
    assert fused_calls(on.module) == launches
    for (k, p), (_, q) in zip(on.module.state_dict().items(), off.module.state_dict().items()):
        assert torch.equal(p, q), k                                         # the running statistics moved alike

    # the pack cache: an in-place write to running_var, then a whole state dict
    bn = on.module.bn if name == "convbnrelu" else on.module.bn2            # the BatchNorm of a fused layer
    before = on(xd).clone()
    with torch.no_grad():
        bn.running_var.mul_(4.0)
    after = on(xd).clone()
    torch.cuda.synchronize()
    assert fused_calls(on.module) == 3 * launches and not torch.equal(before, after)
    _assert_within(after, ref(on.module, _Val(x.double()), cuda), name + " after running_var.mul_(4)")
    other = _randomise_bn(build(), 17).state_dict()
    on.module.load_state_dict(other)
    y3 = on(xd)
    torch.cuda.synchronize()
    assert fused_calls(on.module) == 4 * launches
    _assert_within(y3, ref(on.module, _Val(x.double()), cuda), name + " after load_state_dict")
    # the fused layer's BatchNorm alone in train mode: the call is the stock one, the running statistics move inside a
    # kernel (no tensor version counts it), and the next eval call must read the moved values
    bn = on.module.bn if name == "convbnrelu" else on.module.bn2
    bn.train()
    on(xd)
    bn.eval()
    assert fused_calls(on.module) == 4 * launches                           # the whole module ran the replaced method
    y4 = on(xd)
    torch.cuda.synchronize()
    assert fused_calls(on.module) == 5 * launches
    _assert_within(y4, ref(on.module, _Val(x.double()), cuda), name + " after a train-mode call of the BatchNorm alone")


# ---- BiSeNet-R18 -------------------------------------------------------------------------------------------------------
def _path_layers(net):
    """the fusable layers an inference forward of BiSeNet-R18 runs: everything but the two auxiliary heads"""
    from torchseg_amd.convbn import eligible_layers
    aux = {id(m) for h in list(net.heads)[:-1] for m in h.modules()}
    return sum(len(eligible_layers(m)[1]) for m in net.modules() if id(m) not in aux)


def _rel(o, p):
    return float((o.float() - p.float()).abs().max() / p.float().abs().max())


def test_r18_backbone_and_logits_against_the_fp32_parity_run(cuda):
    """Per backbone stage and for the final log-probabilities: the fused bf16 network is at most 1.25 x as far from the
    fp32 parity run as the unfused bf16 network (the factor tests/test_sepconv_gpu.py uses for the same comparison)."""
    from base_model.resnet import resnet18
    from torchseg_amd.convbn import eligible_layers, fused_calls
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    torch.manual_seed(11)
    backbone = _randomise_bn(resnet18(None, norm_layer=nn.BatchNorm2d), 12).eval()
    full = _r18(13).eval()
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(14)).to(cuda)
    for label, base, n in (("backbone", backbone, 13), ("network", full, 18)):
        arms = dict(parity=prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_convbn=True),
                    unfused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=False),
                    fused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=True))
        outs = {}
        for k, m in arms.items():
            o = m(x)
            o = [materialize(o)] if label == "network" else list(o)
            outs[k] = [t.clone() for t in o]
        torch.cuda.synchronize()
        assert fused_calls(arms["fused"].module) == n and fused_calls(arms["unfused"].module) == 0
        assert fused_calls(arms["parity"].module) == 0                  # fp32: the parity mode stays on the exact kernels
        for k, (pu, pf, pp) in enumerate(zip(outs["unfused"], outs["fused"], outs["parity"])):
            u, f = _rel(pu, pp), _rel(pf, pp)
            what = "stage 1/%d" % (4 << k) if label == "backbone" else "log-probabilities"
            print("convbn parity [%s] %s: max |d| / max |fp32 parity|: unfused bf16 %.4e, fused bf16 %.4e (ratio %.3f)"
                  % (label, what, u, f, f / u))
        for k, (pu, pf, pp) in enumerate(zip(outs["unfused"], outs["fused"], outs["parity"])):
            assert _rel(pf, pp) <= 1.25 * _rel(pu, pp), (label, k, _rel(pf, pp), _rel(pu, pp))


def test_r18_prepare_inference_eager_graph_and_pending_tail(cuda):
    from torchseg_amd.convbn import eligible_layers, fused_calls
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import pending_tail, prepare_inference
    net = _r18(21).eval()
    installed = sum(len(eligible_layers(m)[1]) for m in net.modules())
    on_path = _path_layers(net)
    assert (installed, on_path) == (20, 18)                   # the module tree holds two auxiliary heads inference never calls
    net = net.to(cuda)
    eager = prepare_inference(copy.deepcopy(net), dtype=BF, fuse_convbn=True)
    graph = prepare_inference(copy.deepcopy(net), dtype=BF, graph=True, fuse_convbn=True)
    assert eager.fused_convbn == installed and graph.fused_convbn == installed
    replays = []
    for seed in (1, 2):
        x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(seed)).to(cuda)
        out = eager(x)
        tail = pending_tail(out)
        assert tail is not None and tuple(tail[1]) == (64, 128) and tail[0].shape[1] == 19     # still the pending head
        a = materialize(out).clone()
        b = graph(x).clone()
        torch.cuda.synchronize()
        assert a.shape == (1, 19, 64, 128) and bool(torch.isfinite(a).all())
        assert torch.equal(a, b), (seed, float((a - b).abs().max()))
        replays.append(b)
    assert not torch.equal(replays[0], replays[1])
    assert fused_calls(eager.module) == 2 * on_path
    assert fused_calls(graph.module) == 2 * on_path           # the warm-up and the capture; the packs were ready for the capture


MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


def test_r18_evaluator_consumes_the_pending_tail(cuda, monkeypatch):
    """TSG_INFER=1 with TSG_CONVBN_FUSED=1: sliding_eval takes the fused window tail (the pending value reaches the
    Evaluator), and the class map equals the one of the same evaluator on the eager path (the materialised output)."""
    from engine.evaluator import Evaluator
    from torchseg_amd.convbn import fused_calls
    net = _r18(31).eval()
    monkeypatch.delenv("TSG_DTYPE", raising=False)
    monkeypatch.setenv("TSG_INFER", "1")
    monkeypatch.setenv("TSG_CONVBN_FUSED", "1")
    img = np.random.RandomState(0).randint(0, 256, (96, 160, 3)).astype(np.uint8)
    ev = Evaluator(None, 19, MEAN, STD, copy.deepcopy(net), [1.0], False, [0])
    ev.val_func = ev.network
    taken = []
    stock = ev._fused_window_scores
    monkeypatch.setattr(ev, "_fused_window_scores", lambda *a, **k: taken.append(stock(*a, **k)) or taken[-1])
    pred = ev.sliding_eval(img, 96, 2 / 3, device=0)
    assert pred.shape == (96, 160) and pred.min() >= 0 and pred.max() < 19
    assert taken and all(t is not None for t in taken)
    assert ev._infer_net.fused_convbn == 20 and fused_calls(ev._infer_net.module) >= 18
    monkeypatch.setattr(ev, "_fused_window_scores", lambda *a, **k: None)
    eager = ev.sliding_eval(img, 96, 2 / 3, device=0)
    assert np.array_equal(pred, eager), int((pred != eager).sum())


def test_switch_unset_installs_nothing(cuda, monkeypatch, _pin_vendor_library):
    """Unset, or off: nothing is re-classed and the output is the path's without the feature, bit for bit, in the fp32
    parity mode and in bf16 (the vendor library pinned to its deterministic kernels: see _pin_vendor_library)."""
    from torchseg_amd.convbn import _FusedConvBn, fused_calls
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    monkeypatch.delenv("TSG_DTYPE", raising=False)
    monkeypatch.delenv("TSG_CONVBN_FUSED", raising=False)
    net = _r18(41).eval().to(cuda)
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(42)).to(cuda)
    for dtype in (torch.float32, BF):
        unset = prepare_inference(copy.deepcopy(net), dtype=dtype)
        off = prepare_inference(copy.deepcopy(net), dtype=dtype, fuse_convbn=False)
        for m in (unset, off):
            assert m.fused_convbn == 0 and not any(isinstance(k, _FusedConvBn) for k in m.modules())
        a, b = materialize(unset(x)).clone(), materialize(off(x)).clone()
        torch.cuda.synchronize()
        print("convbn switch unset, %s: max |unset - off| %.3e" % (dtype, float((a - b).abs().max())))
        assert torch.equal(a, b), dtype
    assert prepare_inference(copy.deepcopy(net)).compute_dtype == BF                # the default is the bf16 path
    monkeypatch.setenv("TSG_CONVBN_FUSED", "1")
    on = prepare_inference(copy.deepcopy(net))
    assert on.fused_convbn == 20
    materialize(on(x))
    assert fused_calls(on.module) == 18
