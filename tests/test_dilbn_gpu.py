"""GPU: the fused dilated 3x3 convolution + BatchNorm (+ residual) (+ ReLU) of inference (csrc/dilbn.hip) against torch's
CPU float64 `F.conv2d(..., padding=d, dilation=d)` on the same bf16-rounded operands, d = 2 and 4.  The conventions, the
bound (_fused_tol: derived from the formats, K = 9 C_in) and the helpers are tests/test_convbn_gpu.py's.

  1. exact data: every sum is exact in fp32 in any order, the output must be BIT-equal to the float64 value rounded once;
  2. random data against float64 within _fused_tol, per element;
  3. operands and output inside poisoned guard bands (tests/_guard.py), three calls bit-identical, the same result with x,
     residual and y at 16-byte-aligned offsets inside larger allocations, x and the residual unchanged;
  4. modules: a dilated ConvBnRelu, a dilated Bottleneck with an identity shortcut and one with a `downsample`, against the
     float64 composition with the bound carried through the stages; the counters; the stock path in train mode and with
     gradients enabled; the pack cache; with pwbn's mixin as well, in both install orders; beside TSG_CONV_DIL=1;
  5. PSPNet-R50 (19 classes) through prepare_inference: counts, eager against graph replay, and the distance from the fp32
     parity run against the unfused bf16 path's, per backbone stage and for the log-probabilities;
  6. the switch's default.

Shapes (B, H, W, C_in, C_out), the smallest at which the tiling or the halo can go wrong: a 3 x 5 map, smaller than the halo
at d = 4, so that most taps of most pixels are padding; an exact tile, two images, two chunks (both halves of the double
buffer); ragged both ways with an odd chunk count and two oc tiles, the halo crossing a tile seam in both directions;
several tiles and three oc tiles; and 72 x 256 at C_out = 512, where the plan has 64 blocks per oc tile for 72 tiles, so that
a block walks two tiles."""
import copy
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _guard
from test_convbn_cpu import _randomise_bn
from test_convbn_gpu import (COMBOS, _Val, _assert_within, _device_operands, _epilogue64, _fused_tol, _layer64, _operands,
                             _rel)
from test_dilbn_cpu import GPU_CASES as CASES, LDS, _dilated_bottleneck, _dilated_cbr, _pspnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

pytestmark = pytest.mark.gpu

DILATIONS = [2, 4]
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
    """a bit-for-bit comparison of the STOCK path against itself needs the vendor library's deterministic kernels
    (tests/test_convbn_gpu.py::_pin_vendor_library); the fused kernel does not read the setting"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


_REF = {}


def _ref64(case, d, exact, seed=0):
    """(operands, u64, S): the float64 dilated convolution of the bf16-rounded operands and the same sum of absolute
    values; computed once per (case, dilation) and shared"""
    key = (case, d, exact, seed)
    if key not in _REF:
        ops = _operands(case, exact, seed + d)
        x, w = ops[0].double(), ops[1].to(BF).double()
        _REF[key] = (ops, F.conv2d(x, w, None, 1, d, d), F.conv2d(x.abs(), w.abs(), None, 1, d, d))
    return _REF[key]


def _check(got, case, u, S, a, b, res, relu, what):
    y64 = _epilogue64(u, a, b, res, relu)
    aS = a.double().abs().view(1, -1, 1, 1) * S
    mag = aS + b.double().abs().view(1, -1, 1, 1) + (res.double().abs() if res is not None else 0.0)
    tol = _fused_tol(y64, aS, mag, 9 * case[3])
    err = (got.double().cpu() - y64).abs()
    bad = ~(err <= tol)
    print("dilbn %s: max err %.3e, max err / tol %.3f" % (what, float(err.max()), float((err / tol).max())))
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err - tol).max()))


def test_the_largest_case_makes_a_block_walk_two_tiles(cuda):
    from torchseg_amd import kernels as K
    kp = K.provider()
    for d in DILATIONS:
        assert kp.conv3x3_dil_bnact_plan(*CASES[-1], d) == (72, 64, 8, 512, LDS[d])
        for case in CASES[:-1]:
            ntiles, nslots, _, _, _ = kp.conv3x3_dil_bnact_plan(*case, d)
            assert ntiles <= nslots


@pytest.mark.parametrize("d", DILATIONS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_exact_data_is_bit_equal_to_float64(cuda, case, d):
    """x in [-2, 2] integers, w in {-1, 0, 1}, a in {1/2, 1, 2}, b multiples of 1/4 in [-4, 4], residual integers in
    [-4, 4]: |u| <= 2 * 9 * 64 is an integer, a u + b + r a multiple of 1/4 below 2^12: exact in fp32 in any order; the only
    rounding is the last one."""
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout = case
    ops, u, _ = _ref64(case, d, True)
    x, w, a, b, res = ops
    xd, wd, fp, resd = _device_operands(ops, cuda)
    assert kp.conv3x3_dil_bnact_supported(xd, Cout, d)
    pack = kp.conv3x3_bnact_pack(wd, None, fp)                          # the plain layer's pack: no routine of its own
    assert float(u.abs().max()) * 2 + 8 < 2 ** 12
    for with_res, relu in COMBOS:
        y = kp.conv3x3_dil_bnact_fwd(xd, pack, Cout, d, resd if with_res else None, relu)
        want = _epilogue64(u, a, b, res if with_res else None, relu)
        assert torch.equal(want, want.float().double())                 # the float64 value is an fp32 number
        want = want.float().to(BF)
        assert y.dtype == BF and y.shape == want.shape and y.is_contiguous(memory_format=CL)
        got = y.cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
            (case, d, with_res, relu, int((got != want).sum()), float((got.float() - want.float()).abs().max()))


@pytest.mark.parametrize("d", DILATIONS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_random_data_against_float64(cuda, case, d):
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout = case
    ops, u, S = _ref64(case, d, False)
    x, w, a, b, res = ops
    xd, wd, fp, resd = _device_operands(ops, cuda)
    pack = kp.conv3x3_bnact_pack(wd, None, fp)
    xk, rk = xd.clone(), resd.clone()
    for with_res, relu in COMBOS:
        r = resd if with_res else None
        y = kp.conv3x3_dil_bnact_fwd(xd, pack, Cout, d, r, relu)
        y2 = kp.conv3x3_dil_bnact_fwd(xd, pack, Cout, d, r, relu)
        torch.cuda.synchronize()
        assert y.dtype == BF and y.is_contiguous(memory_format=CL)
        assert torch.equal(_guard.raw_bytes(y), _guard.raw_bytes(y2))   # bit-identical from launch to launch
        _check(y, case, u, S, a, b, res if with_res else None, relu, (case, d, with_res, relu))
    assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(xk)) and torch.equal(_guard.raw_bytes(resd), _guard.raw_bytes(rk))


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("d", DILATIONS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_inside_guard_bands(cuda, case, d, with_res):
    """Operands in guarded arenas, pack and output allocated through Guarded(fill) under both fills: no guard byte moves
    and the three results are bit-identical; then the raw entry point with x, residual and y at 16- and 48-byte offsets
    inside larger poisoned allocations: the same bits again, not a byte around y has moved, x and the residual are what
    they were."""
    from torchseg_amd import _lib, kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout = case
    ops, u, S = _ref64(case, d, False, seed=3)
    x, w, a, b, res = ops
    xd, wd, fp, resd = _device_operands(ops, cuda)

    def layer(xx, ww, fwd_pack, rr):
        return kp.conv3x3_dil_bnact_fwd(xx, kp.conv3x3_bnact_pack(ww, None, fwd_pack), Cout, d, rr, True)

    plain = _guard.three_calls(layer, [xd, wd, fp, resd if with_res else None])[0]
    _check(plain, case, u, S, a, b, res if with_res else None, True, (case, d, with_res))

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
    keep_x, keep_r = bx.clone(), br.clone()
    assert vx.data_ptr() % 32 == 16 and vy.data_ptr() % 16 == 0 and vx.is_contiguous(memory_format=CL)
    _lib.call(kp.lib.tsg_conv3x3_dil_bnact_fwd, vx.data_ptr(), wf.data_ptr(), ab.data_ptr(),
              vr.data_ptr() if with_res else None, vy.data_ptr(), B, H, W, Cin, Cout, d, 1, _lib.stream_ptr(vx))
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(vy), _guard.raw_bytes(plain))
    raw = by.view(torch.int16)
    assert bool((raw[:24] == 0x5a5a).all()) and bool((raw[24 + plain.numel():] == 0x5a5a).all())
    assert torch.equal(_guard.raw_bytes(bx), _guard.raw_bytes(keep_x)) and torch.equal(_guard.raw_bytes(br), _guard.raw_bytes(keep_r))
    # a misaligned operand and a dilation that is not ours are refused before any launch
    assert kp.lib.tsg_conv3x3_dil_bnact_fwd(vx.data_ptr() + 2, wf.data_ptr(), ab.data_ptr(), None, vy.data_ptr(), B, H, W, Cin,
                                            Cout, d, 1, _lib.stream_ptr(vx)) == -4
    assert kp.lib.tsg_conv3x3_dil_bnact_fwd(vx.data_ptr(), wf.data_ptr(), ab.data_ptr(), None, vy.data_ptr(), B, H, W, Cin,
                                            Cout, 3, 1, _lib.stream_ptr(vx)) == -3
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(vy), _guard.raw_bytes(plain))


# ---- module level ------------------------------------------------------------------------------------------------------
def _shortcut64(m, x, dev, fused):
    return x if m.downsample is None else _layer64(x, m.downsample[0], m.downsample[1], dev, relu=False, fused=fused)


def _cbr_ref(m, x, dev, pw):
    return _layer64(x, m.conv, m.bn, dev)


def _bottleneck_ref(m, x, dev, pw):
    """conv2 + bn2 + relu is the one fused layer; with pwbn's mixin (`pw`) the 1x1 layers and the shortcut are fused too"""
    out = _layer64(x, m.conv1, m.bn1, dev, fused=pw)
    out = _layer64(out, m.conv2, m.bn2, dev)
    return _layer64(out, m.conv3, m.bn3, dev, res=_shortcut64(m, x, dev, pw), fused=pw)


def _build(name, d, seed):
    torch.manual_seed(seed)
    return _dilated_cbr(d) if name == "convbnrelu" else _dilated_bottleneck(d, name == "bottleneck-downsample")


# name: (input channels, float64 composition, pwbn launches when its mixin is installed too)
MODULES = {"convbnrelu": (48, _cbr_ref, 0), "bottleneck": (256, _bottleneck_ref, 2), "bottleneck-downsample": (128, _bottleneck_ref, 3)}


def _input(Cin, cuda, seed=8):
    x = torch.randn(2, Cin, 18, 40, generator=torch.Generator().manual_seed(seed)).to(BF)
    return x, x.to(cuda).contiguous(memory_format=CL)


@pytest.mark.parametrize("d", DILATIONS)
@pytest.mark.parametrize("name", list(MODULES))
def test_modules(cuda, name, d, _pin_vendor_library):
    from torchseg_amd.convbn import dil_fused_calls, fused_calls
    from torchseg_amd.infer import prepare_inference
    Cin, ref, _ = MODULES[name]
    base = _randomise_bn(_build(name, d, 1), 7).eval()
    on = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_dilated=True)
    off = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_dilated=False)
    plain = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=True)       # the default selection: not ours
    assert on.fused_dilated == 1 and off.fused_dilated == 0 and on.fused_convbn == off.fused_convbn == 0
    assert plain.fused_convbn == 0 and plain.fused_dilated == 0
    x, xd = _input(Cin, cuda)
    keep = xd.clone()

    y = on(xd)
    torch.cuda.synchronize()
    assert dil_fused_calls(on.module) == 1 and fused_calls(on.module) == 1
    assert y.dtype == BF and y.data_ptr() != xd.data_ptr()
    assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(keep))      # the input, which is the identity block's residual
    _assert_within(y, ref(on.module, _Val(x.double()), cuda, False), "dilbn %s d%d" % (name, d))

    # train mode, and eval mode with gradients enabled (and every mode in fp32, the parity arm): the replaced method, bit for
    # bit (the vendor library pinned), called exactly once with the module's own input, and no counter moves
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
    arms[torch.float32] = (prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_dilated=True),
                           prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_dilated=False),
                           x.float().to(cuda).contiguous(memory_format=CL))
    assert arms[torch.float32][0].fused_dilated == 1
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
            print("dilbn module %s d%d %s train=%s grad=%s: re-classed and un-installed copy bit-equal: %s"
                  % (name, d, dtype, train, grad, same))
            if not same:
                mismatch.append((name, dtype, train, grad, float((o_on.float() - o_off.float()).abs().max())))
    assert not mismatch, mismatch
    assert dil_fused_calls(on.module) == 1 and dil_fused_calls(arms[torch.float32][0].module) == 0
    for (k, p), (_, q) in zip(on.module.state_dict().items(), off.module.state_dict().items()):
        assert torch.equal(p, q), k                                         # the running statistics moved alike

    # the pack cache: an in-place write to running_var, then a whole state dict
    bn = on.module.bn if name == "convbnrelu" else on.module.bn2            # the BatchNorm of the fused layer
    before = on(xd).clone()
    with torch.no_grad():
        bn.running_var.mul_(4.0)
    after = on(xd).clone()
    torch.cuda.synchronize()
    assert dil_fused_calls(on.module) == 3 and not torch.equal(before, after)
    _assert_within(after, ref(on.module, _Val(x.double()), cuda, False), name + " after running_var.mul_(4)")
    other = _randomise_bn(_build(name, d, 2), 17).state_dict()
    on.module.load_state_dict(other)
    y3 = on(xd)
    torch.cuda.synchronize()
    assert dil_fused_calls(on.module) == 4
    _assert_within(y3, ref(on.module, _Val(x.double()), cuda, False), name + " after load_state_dict")
    # the fused layer's BatchNorm alone in train mode: the call is the stock one, the running statistics move inside a
    # kernel (no tensor version counts it), and the next eval call must read the moved values
    bn.train()
    on(xd)
    bn.eval()
    assert dil_fused_calls(on.module) == 4                                  # the whole module ran the replaced method
    y4 = on(xd)
    torch.cuda.synchronize()
    assert dil_fused_calls(on.module) == 5 and fused_calls(on.module) == 5
    _assert_within(y4, ref(on.module, _Val(x.double()), cuda, False), name + " after a train-mode call of the BatchNorm alone")


@pytest.mark.parametrize("order", ["dilated-first", "pointwise-first"])
@pytest.mark.parametrize("d", DILATIONS)
@pytest.mark.parametrize("name", ["bottleneck", "bottleneck-downsample"])
def test_bottleneck_with_the_pointwise_mixin_is_three_fused_launches(cuda, name, d, order):
    """conv1 and conv3 (and a 1x1 shortcut) on csrc/pwbn.hip, conv2 on csrc/dilbn.hip, whichever installer ran first: pwbn's
    Bottleneck asks the class behind it through _cbn_gate / _cbn_ready / _cbn_run, and the pack carries the dilation."""
    from torchseg_amd import convbn, pwbn
    from torchseg_amd.infer import prepare_inference
    Cin, ref, pw_launches = MODULES[name]
    base = _randomise_bn(_build(name, d, 3), 9).eval()
    if order == "dilated-first":
        m = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_dilated=True, fuse_pointwise=True)
        assert m.fused_dilated == 1
    else:
        m = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_pointwise=True)
        assert m.fused_dilated == 0 and not isinstance(m.module, convbn._FusedConvBn)
        assert convbn.install_fused_convbn(m.module, dilated=True, plain=False) == 1
    assert m.fused_pointwise == pw_launches
    mro = type(m.module).__mro__
    assert issubclass(mro[1], pwbn._FusedPointwise) and isinstance(m.module, convbn._FusedConvBn)     # pwbn's mixin in front
    x, xd = _input(Cin, cuda, seed=10)
    keep = xd.clone()
    outs = [m(xd).clone() for _ in range(2)]
    torch.cuda.synchronize()
    assert pwbn.fused_calls(m.module) == 2 * pw_launches
    assert convbn.dil_fused_calls(m.module) == 2 and convbn.fused_calls(m.module) == 2
    assert torch.equal(_guard.raw_bytes(outs[0]), _guard.raw_bytes(outs[1]))         # no vendor convolution is left in the block
    assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(keep))
    _assert_within(outs[0], ref(m.module, _Val(x.double()), cuda, True), "dilbn + pwbn %s d%d %s" % (name, d, order))


@pytest.mark.parametrize("d", DILATIONS)
def test_beside_the_dilated_convolution_reclass(cuda, d, monkeypatch, _pin_vendor_library):
    """TSG_CONV_DIL=1 re-classes conv2 itself to DilatedConv2d: the fused path wins when its gate passes (the same kernel
    on the same pack: the same bits), and a decline runs whatever conv2 is."""
    from torchseg_amd.convbn import dil_fused_calls
    from torchseg_amd.dilconv import DilatedConv2d
    from torchseg_amd.infer import prepare_inference
    base = _randomise_bn(_build("bottleneck", d, 4), 11).eval()
    monkeypatch.delenv("TSG_CONV_DIL", raising=False)
    without = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_dilated=True)
    monkeypatch.setenv("TSG_CONV_DIL", "1")
    beside = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_dilated=True)
    stock = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_dilated=False)
    assert isinstance(beside.module.conv2, DilatedConv2d) and isinstance(stock.module.conv2, DilatedConv2d)
    assert not isinstance(without.module.conv2, DilatedConv2d) and beside.fused_dilated == 1
    x, xd = _input(256, cuda, seed=12)
    a, b = without(xd).clone(), beside(xd).clone()
    torch.cuda.synchronize()
    assert dil_fused_calls(beside.module) == 1 and torch.equal(_guard.raw_bytes(a), _guard.raw_bytes(b))
    # a decline (gradients enabled): conv2 is DilatedConv2d in both, bit for bit the un-installed copy
    with torch.enable_grad(), torch.autocast("cuda", dtype=BF):
        o_on, o_off = beside.module(xd).detach().clone(), stock.module(xd).detach().clone()
    torch.cuda.synchronize()
    assert dil_fused_calls(beside.module) == 1 and torch.equal(_guard.raw_bytes(o_on), _guard.raw_bytes(o_off))


# ---- PSPNet-R50 --------------------------------------------------------------------------------------------------------
def _psp50(seed):
    return _randomise_bn(_pspnet(50, seed), seed + 1).eval()


def test_pspnet_r50_runs_under_prepare_inference_with_every_fusion_off(cuda):
    """Establishes that the network runs under prepare_inference at all, before anything of this feature is switched on."""
    from torchseg_amd.convbn import _FusedConvBn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    m = prepare_inference(_psp50(1).to(cuda), dtype=BF, fuse_separable=False, fuse_convbn=False, fuse_pointwise=False,
                          fuse_dilated=False)
    assert m.fused_dilated == 0 and not any(isinstance(k, _FusedConvBn) for k in m.modules())
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = materialize(m(x))
    torch.cuda.synchronize()
    assert out.shape == (1, 19, 64, 128) and bool(torch.isfinite(out).all())


def test_pspnet_r50_backbone_and_logits_against_the_fp32_parity_run(cuda, _pin_vendor_library):
    """Per backbone stage (the dilated ResNet-50-v1c backbone on its own) and for the network's log-probabilities: with the
    dilated layers fused the bf16 network is at most 1.25 x as far from the fp32 parity run as the bf16 network without
    (the factor tests/test_convbn_gpu.py and tests/test_sepconv_gpu.py use for this comparison).  The vendor library, which
    runs every other convolution of both bf16 arms here, is pinned to its deterministic kernels so that the two distances
    are the same from run to run."""
    from torchseg_amd.convbn import dil_fused_calls, fused_calls
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    full = _psp50(11)
    backbone = copy.deepcopy(full.backbone)
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(14)).to(cuda)
    for label, base in (("backbone", backbone), ("network", full)):
        arms = dict(parity=prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_dilated=True),
                    unfused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_dilated=False),
                    fused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_dilated=True))
        outs = {}
        for k, m in arms.items():
            o = m(x)
            o = [materialize(o)] if label == "network" else list(o)
            outs[k] = [t.clone() for t in o]
        torch.cuda.synchronize()
        assert arms["fused"].fused_dilated == 8 and arms["parity"].fused_dilated == 8 and arms["unfused"].fused_dilated == 0
        assert dil_fused_calls(arms["fused"].module) == 8 and fused_calls(arms["fused"].module) == 8
        assert fused_calls(arms["unfused"].module) == 0
        assert fused_calls(arms["parity"].module) == 0                  # fp32: the parity mode stays on the exact kernels
        dist = []
        for k, (pu, pf, pp) in enumerate(zip(outs["unfused"], outs["fused"], outs["parity"])):
            u, f = _rel(pu, pp), _rel(pf, pp)
            dist.append((u, f))
            what = "stage 1/%d" % (4, 8, 8, 8)[k] + " (layer%d)" % (k + 1) if label == "backbone" else "log-probabilities"
            print("dilbn parity [%s] %s: max |d| / max |fp32 parity|: unfused bf16 %.4e, fused bf16 %.4e (ratio %.3f)"
                  % (label, what, u, f, f / u if u else float("nan")))
        for k, (u, f) in enumerate(dist):
            assert f <= 1.25 * u, (label, k, f, u)


def test_pspnet_r50_counts_eager_and_graph(cuda, _pin_vendor_library):
    """With every inference fusion on: 8 dilated layers installed and 8 launches of the dilated kernel per forward, the
    plain count what it is without this feature, an eager call and a graph replay bit-equal, two replays on different
    inputs different.  The deep stem, the stride-2 3x3 and the pyramid head's convolutions of this network are still the
    vendor library's, which at this size does not repeat from call to call unless it is pinned to its deterministic
    kernels; the fused kernels do not read the setting."""
    from torchseg_amd import convbn, pwbn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    net = _psp50(21).to(cuda)
    kw = dict(dtype=BF, fuse_convbn=True, fuse_pointwise=True)
    without = prepare_inference(copy.deepcopy(net), fuse_dilated=False, **kw)
    eager = prepare_inference(copy.deepcopy(net), fuse_dilated=True, **kw)
    graph = prepare_inference(copy.deepcopy(net), fuse_dilated=True, graph=True, **kw)
    assert eager.fused_dilated == 8 and graph.fused_dilated == 8 and without.fused_dilated == 0
    assert eager.fused_convbn == without.fused_convbn == 9 and eager.fused_pointwise == without.fused_pointwise
    replays = []
    for n, seed in enumerate((1, 2)):
        x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(seed)).to(cuda)
        a = materialize(eager(x)).clone()
        b = materialize(graph(x)).clone()
        torch.cuda.synchronize()
        assert a.shape == (1, 19, 64, 128) and bool(torch.isfinite(a).all())
        assert torch.equal(a, b), (seed, float((a - b).abs().max()))
        assert convbn.dil_fused_calls(eager.module) == 8 * (n + 1)
        replays.append(b)
    assert not torch.equal(replays[0], replays[1])
    assert convbn.dil_fused_calls(graph.module) == 2 * 8      # the warm-up and the capture; the packs were ready for the capture
    materialize(without(x))
    assert convbn.dil_fused_calls(without.module) == 0
    # the plain launches are the same with and without this feature; every Bottleneck of layer3 / layer4 is three launches
    assert convbn.fused_calls(eager.module) - 2 * 8 == 2 * convbn.fused_calls(without.module)
    assert pwbn.fused_calls(eager.module) == 2 * pwbn.fused_calls(without.module)


def test_switch_unset_installs_nothing(cuda, monkeypatch, _pin_vendor_library):
    """Unset, or 0: nothing is re-classed by this feature and the output is the path's without it, bit for bit, with the
    other switches the same (the vendor library pinned to its deterministic kernels: the dilated layers run on it)."""
    from torchseg_amd import convbn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    monkeypatch.delenv("TSG_DTYPE", raising=False)
    monkeypatch.delenv("TSG_DILBN_FUSED", raising=False)
    net = _psp50(41).to(cuda)
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(42)).to(cuda)
    kw = dict(dtype=BF, fuse_convbn=True, fuse_pointwise=True)
    outs = []
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("TSG_DILBN_FUSED", env)
        unset = prepare_inference(copy.deepcopy(net), **kw)
        off = prepare_inference(copy.deepcopy(net), fuse_dilated=False, **kw)
        for m in (unset, off):
            assert m.fused_dilated == 0 and m.fused_convbn == 9
            assert not any(k.tsg_cbn_dilated for k in m.modules() if isinstance(k, convbn._FusedConvBn))
            assert not any(isinstance(k, convbn._FusedConvBn) for k in m.modules() if convbn.eligible_dilated_layers(k))
        a, b = materialize(unset(x)).clone(), materialize(off(x)).clone()
        torch.cuda.synchronize()
        print("dilbn switch %r: max |unset - off| %.3e" % (env, float((a - b).abs().max())))
        assert torch.equal(a, b), env
        assert convbn.dil_fused_calls(unset.module) == 0
        outs.append(a)
    assert torch.equal(outs[0], outs[1])
    monkeypatch.setenv("TSG_DILBN_FUSED", "1")
    on = prepare_inference(copy.deepcopy(net), **kw)
    assert on.fused_dilated == 8 and on.fused_convbn == 9
    materialize(on(x))
    assert convbn.dil_fused_calls(on.module) == 8
    only = prepare_inference(copy.deepcopy(net), dtype=BF)               # with fuse_convbn off: the dilated blocks alone
    assert only.fused_dilated == 8 and only.fused_convbn == 0
    assert sum(isinstance(k, convbn._FusedConvBn) for k in only.modules()) == 8
