"""GPU: the fused stride-2 3x3 convolution + BatchNorm (+ residual) (+ ReLU) of inference (csrc/s2bn.hip) against torch's CPU
float64 `F.conv2d(..., stride=2, padding=1)` on the same bf16-rounded operands.  The conventions, the bound (_fused_tol:
derived from the formats, K = 9 C_in) and the helpers are tests/test_convbn_gpu.py's; the operand builder is this file's,
since the residual has the OUTPUT's shape.

  1. exact data: every sum is exact in fp32 in any order, the output must be BIT-equal to the float64 value rounded once;
  2. random data against float64 within _fused_tol, per element;
  3. operands and output inside poisoned guard bands (tests/_guard.py), three calls bit-identical, the same result with x,
     residual and y at 16-byte-aligned offsets inside larger allocations, x and the residual unchanged;
  4. modules: stride-2 ConvBnRelu layers, a stride-2 BasicBlock and a stride-2 Bottleneck with their `downsample`, against
     the float64 composition with the bound carried through the stages; the counters; the stock path in train mode and with
     gradients enabled; the pack cache; with pwbn's mixin in both install orders and as an upgrade of a plain install: no
     vendor convolution is left in the block, and eager calls and a graph replay repeat bit for bit WITHOUT pinning the
     vendor library;
  5. our SpatialPath through seg_oprs.cbr_chain;
  6. BiSeNet-R18 and PSPNet-R50 through prepare_inference: counts, eager against graph replay, the pending tail, the
     Evaluator, and the distance from the fp32 parity run against the same bf16 network's with the switch off;
  7. the switch's default.

Shapes (B, H, W, C_in, C_out), H and W of the INPUT -- the smallest at which stride, halo and tiling can go wrong:
  (1, 1, 3, 16, 64)       one input row: only kh = 1 is ever in range; output 1 x 2
  (1, 5, 7, 16, 64)       odd x odd: the last output row and column read one padding row / column below and right; smaller
                          than a tile, one chunk
  (1, 6, 8, 16, 64)       even x even: the last tap lands exactly on the last input row / column
  (2, 16, 64, 32, 64)     output exactly 8 x 32 per image, two images, two chunks (both halves of the double buffer)
  (1, 17, 66, 48, 128)    output 9 x 33, ragged both ways, odd chunk count, two oc tiles, odd H / even W
  (1, 34, 79, 64, 192)    output 17 x 40, several tiles, three oc tiles, even H / odd W
  (1, 143, 511, 16, 512)  output 72 x 256 at C_out = 512: 144 tiles for 64 persistent blocks per oc tile, a block walks
                          more than one tile"""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

import _guard
from test_convbn_cpu import _r18, _randomise_bn
from test_convbn_gpu import COMBOS, _Val, _assert_within, _epilogue64, _fused_tol, _layer64, _rel
from test_s2bn_cpu import GPU_CASES as CASES, LDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

pytestmark = pytest.mark.gpu

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


# ---- kernel level ------------------------------------------------------------------------------------------------------
def _out_hw(H, W):
    return (H + 1) // 2, (W + 1) // 2


def _operands(case, exact, seed=0):
    """CPU operands: x [B,Cin,H,W] and the residual [B,Cout,OH,OW] already rounded to bf16, w fp32 (bf16-representable when
    exact), fp32 a, b"""
    B, H, W, Cin, Cout = case
    OH, OW = _out_hw(H, W)
    g = torch.Generator().manual_seed(seed + 1000 * Cin + Cout + 7 * H)
    if exact:
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
        x = ri(-2, 2, B, Cin, H, W)
        w = ri(-1, 1, Cout, Cin, 3, 3)
        a = torch.pow(2.0, ri(-1, 1, Cout))
        b = ri(-16, 16, Cout) / 4
        res = ri(-4, 4, B, Cout, OH, OW)
    else:
        x = torch.randn(B, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
        a = 0.5 + torch.rand(Cout, generator=g)
        a = a * torch.where(torch.rand(Cout, generator=g) < 0.25, -1.0, 1.0)
        b = torch.randn(Cout, generator=g) * 0.5
        res = torch.randn(B, Cout, OH, OW, generator=g)
    return x.to(BF), w, a, b, res.to(BF)


_REF = {}


def _ref64(case, exact, seed=0):
    """(operands, u64, S): the float64 stride-2 convolution of the bf16-rounded operands and the same sum of absolute values;
    computed once per case and shared, never written"""
    key = (case, exact, seed)
    if key not in _REF:
        ops = _operands(case, exact, seed)
        x, w = ops[0].double(), ops[1].to(BF).double()
        _REF[key] = (ops, F.conv2d(x, w, None, 2, 1), F.conv2d(x.abs(), w.abs(), None, 2, 1))
    return _REF[key]


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
    print("s2bn %s: max err %.3e, max err / tol %.3f" % (what, float(err.max()), float((err / tol).max())))
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err - tol).max()))


def test_the_largest_case_makes_a_block_walk_more_than_one_tile(cuda):
    from torchseg_amd import kernels as K
    kp = K.provider()
    OH, OW, ntiles, nslots, noct, grid, lds = kp.conv3x3_s2_bnact_plan(*CASES[-1])
    assert (OH, OW, noct, lds) == (72, 256, 8, LDS) and ntiles > nslots
    for case in CASES[:-1]:
        _, _, ntiles, nslots, _, _, _ = kp.conv3x3_s2_bnact_plan(*case)
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
    assert kp.conv3x3_s2_bnact_supported(xd, Cout)
    pack = kp.conv3x3_bnact_pack(wd, None, fp)                          # the plain layer's pack: no routine of its own
    assert float(u.abs().max()) * 2 + 8 < 2 ** 12
    assert tuple(u.shape) == (B, Cout) + _out_hw(H, W)
    for with_res, relu in COMBOS:
        y = kp.conv3x3_s2_bnact_fwd(xd, pack, Cout, resd if with_res else None, relu)
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
        y = kp.conv3x3_s2_bnact_fwd(xd, pack, Cout, r, relu)
        y2 = kp.conv3x3_s2_bnact_fwd(xd, pack, Cout, r, relu)
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
    inside larger poisoned allocations: the same bits again, not a byte around y has moved, x and the residual are what
    they were."""
    from torchseg_amd import _lib, kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout = case
    ops, u, S = _ref64(case, False, seed=3)
    x, w, a, b, res = ops
    xd, wd, fp, resd = _device_operands(ops, cuda)

    def layer(xx, ww, fwd_pack, rr):
        return kp.conv3x3_s2_bnact_fwd(xx, kp.conv3x3_bnact_pack(ww, None, fwd_pack), Cout, rr, True)

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
    keep_x, keep_r = bx.clone(), br.clone()
    assert vx.data_ptr() % 32 == 16 and vy.data_ptr() % 16 == 0 and vr.data_ptr() % 16 == 0
    _lib.call(kp.lib.tsg_conv3x3_s2_bnact_fwd, vx.data_ptr(), wf.data_ptr(), ab.data_ptr(),
              vr.data_ptr() if with_res else None, vy.data_ptr(), B, H, W, Cin, Cout, 1, _lib.stream_ptr(vx))
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(vy), _guard.raw_bytes(plain))
    raw = by.view(torch.int16)
    assert bool((raw[:24] == 0x5a5a).all()) and bool((raw[24 + plain.numel():] == 0x5a5a).all())
    assert torch.equal(_guard.raw_bytes(bx), _guard.raw_bytes(keep_x)) and torch.equal(_guard.raw_bytes(br), _guard.raw_bytes(keep_r))
    # a misaligned operand is refused before any launch
    assert kp.lib.tsg_conv3x3_s2_bnact_fwd(vx.data_ptr() + 2, wf.data_ptr(), ab.data_ptr(), None, vy.data_ptr(), B, H, W, Cin,
                                           Cout, 1, _lib.stream_ptr(vx)) == -4
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(vy), _guard.raw_bytes(plain))


# ---- module level ------------------------------------------------------------------------------------------------------
class _ConvCounter(TorchDispatchMode):
    """counts the convolutions that reach the framework's dispatcher (the vendor library's): our kernels do not"""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if "convolution" in str(func):
            self.n += 1
        return func(*args, **(kwargs or {}))


def _cbr(seed, **kw):
    from seg_opr.seg_oprs import ConvBnRelu
    torch.manual_seed(seed)
    return ConvBnRelu(64, 64, 3, 2, 1, **kw)


def _basic(seed):
    from base_model.resnet import BasicBlock, _shortcut
    torch.manual_seed(seed)
    return BasicBlock(64, 128, 2, nn.BatchNorm2d, downsample=_shortcut(64, 128, 2, nn.BatchNorm2d, 1e-5, 0.1))


def _bottleneck(seed):
    from base_model.resnet import Bottleneck, _shortcut
    torch.manual_seed(seed)
    return Bottleneck(256, 128, 2, nn.BatchNorm2d, downsample=_shortcut(256, 512, 2, nn.BatchNorm2d, 1e-5, 0.1))


def _shortcut64(m, x, dev, fused):
    return _layer64(x, m.downsample[0], m.downsample[1], dev, relu=False, fused=fused)


def _cbr_ref(m, x, dev, pw):
    return _layer64(x, m.conv, m.bn, dev, relu=m.has_relu)


def _basic_ref(m, x, dev, pw):
    """both 3x3 layers are fused; with pwbn's mixin (`pw`) the shortcut too"""
    out = _layer64(x, m.conv1, m.bn1, dev)
    return _layer64(out, m.conv2, m.bn2, dev, res=_shortcut64(m, x, dev, pw))


def _bottleneck_ref(m, x, dev, pw):
    """conv2 + bn2 + relu is the one layer of ours; with pwbn's mixin the 1x1 layers and the shortcut are fused too"""
    out = _layer64(x, m.conv1, m.bn1, dev, fused=pw)
    out = _layer64(out, m.conv2, m.bn2, dev)
    return _layer64(out, m.conv3, m.bn3, dev, res=_shortcut64(m, x, dev, pw), fused=pw)


# name: (builder, input channels, float64 composition, launches of ours per call with fuse_strided alone, the BatchNorm of
# the stride-2 layer, pwbn's launches when its mixin is installed too)
MODULES = {"convbnrelu": (_cbr, 64, _cbr_ref, 1, "bn", 0),
           "convbnrelu-bias": (lambda s: _cbr(s, has_bias=True), 64, _cbr_ref, 1, "bn", 0),
           "convbnrelu-norelu": (lambda s: _cbr(s, has_relu=False), 64, _cbr_ref, 1, "bn", 0),
           "basicblock": (_basic, 64, _basic_ref, 2, "bn1", 1),
           "bottleneck": (_bottleneck, 256, _bottleneck_ref, 1, "bn2", 3)}


def _input(Cin, cuda, seed=8):
    x = torch.randn(2, Cin, 18, 40, generator=torch.Generator().manual_seed(seed)).to(BF)
    return x, x.to(cuda).contiguous(memory_format=CL)


@pytest.mark.parametrize("name", list(MODULES))
def test_modules(cuda, name, _pin_vendor_library):
    from torchseg_amd.convbn import fused_calls, s2_fused_calls
    from torchseg_amd.infer import prepare_inference
    build, Cin, ref, launches, bn_name, _ = MODULES[name]
    base = _randomise_bn(build(1), 7).eval()
    on = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_strided=True)
    off = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_strided=False)
    plain = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=True)       # the default selection
    assert on.fused_strided == 1 and off.fused_strided == 0 and plain.fused_strided == 0
    assert on.fused_convbn == off.fused_convbn == 0 and on.fused_dilated == 0 and on.fused_pointwise == 0
    assert plain.fused_convbn == (1 if name == "basicblock" else 0)
    x, xd = _input(Cin, cuda)
    keep = xd.clone()

    y = on(xd)
    torch.cuda.synchronize()
    assert s2_fused_calls(on.module) == 1 and fused_calls(on.module) == launches
    assert y.dtype == BF and tuple(y.shape[2:]) == (9, 20) and y.data_ptr() != xd.data_ptr()
    assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(keep))
    _assert_within(y, ref(on.module, _Val(x.double()), cuda, False), "s2bn %s" % name)
    # an install without `strided` makes no stride-2 launch
    plain(xd)
    torch.cuda.synchronize()
    assert s2_fused_calls(plain.module) == 0 and fused_calls(plain.module) == plain.fused_convbn

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
    arms[torch.float32] = (prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_strided=True),
                           prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_strided=False),
                           x.float().to(cuda).contiguous(memory_format=CL))
    assert arms[torch.float32][0].fused_strided == 1
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
            print("s2bn module %s %s train=%s grad=%s: re-classed and un-installed copy bit-equal: %s"
                  % (name, dtype, train, grad, same))
            if not same:
                mismatch.append((name, dtype, train, grad, float((o_on.float() - o_off.float()).abs().max())))
    assert not mismatch, mismatch
    assert s2_fused_calls(on.module) == 1 and s2_fused_calls(arms[torch.float32][0].module) == 0
    for (k, p), (_, q) in zip(on.module.state_dict().items(), off.module.state_dict().items()):
        assert torch.equal(p, q), k                                         # the running statistics moved alike

    # the pack cache: an in-place write to the convolution's weight and to running_var, then a whole state dict
    bn = getattr(on.module, bn_name)                                        # the BatchNorm of the stride-2 layer
    conv = getattr(on.module, bn_name.replace("bn", "conv"))
    before = on(xd).clone()
    with torch.no_grad():
        conv.weight.mul_(-0.5)
    mid = on(xd).clone()
    with torch.no_grad():
        bn.running_var.mul_(4.0)
    after = on(xd).clone()
    torch.cuda.synchronize()
    assert s2_fused_calls(on.module) == 4 and not torch.equal(before, mid) and not torch.equal(mid, after)
    _assert_within(after, ref(on.module, _Val(x.double()), cuda, False), name + " after weight.mul_ and running_var.mul_")
    other = _randomise_bn(build(2), 17).state_dict()
    on.module.load_state_dict(other)
    y3 = on(xd)
    torch.cuda.synchronize()
    assert s2_fused_calls(on.module) == 5
    _assert_within(y3, ref(on.module, _Val(x.double()), cuda, False), name + " after load_state_dict")
    # the fused layer's BatchNorm alone in train mode: the call is the stock one, the running statistics move inside a
    # kernel (no tensor version counts it), and the next eval call must read the moved values
    bn.train()
    on(xd)
    bn.eval()
    assert s2_fused_calls(on.module) == 5                                   # the whole module ran the replaced method
    y4 = on(xd)
    torch.cuda.synchronize()
    assert s2_fused_calls(on.module) == 6 and fused_calls(on.module) == 6 * launches
    _assert_within(y4, ref(on.module, _Val(x.double()), cuda, False), name + " after a train-mode call of the BatchNorm alone")


def _all_ours(base, order, cuda, graph=False):
    """the module under convbn (plain and strided) and pwbn, installed in the given order"""
    from torchseg_amd import convbn, pwbn
    from torchseg_amd.infer import prepare_inference
    net = copy.deepcopy(base).to(cuda)
    if order == "strided-first":                            # prepare_inference's own order: convbn, strided, pointwise
        m = prepare_inference(net, dtype=BF, graph=graph, fuse_convbn=True, fuse_strided=True, fuse_pointwise=True)
        assert m.fused_strided == 1
    elif order == "pointwise-first":                        # pwbn's mixin is there when ours arrives
        m = prepare_inference(net, dtype=BF, graph=graph, fuse_pointwise=True)
        assert m.fused_strided == 0 and not isinstance(m.module, convbn._FusedConvBn)
        assert convbn.install_fused_convbn(m.module, strided=True) >= 1
    else:                                                   # "upgrade": a plain install, pwbn, then the strided upgrade
        m = prepare_inference(net, dtype=BF, graph=graph, fuse_convbn=True, fuse_pointwise=True)
        assert m.fused_strided == 0
        n = convbn.install_fused_convbn(m.module, strided=True, plain=False)
        assert n == 1
    mro = type(m.module).__mro__
    assert issubclass(mro[1], pwbn._FusedPointwise) and isinstance(m.module, convbn._FusedConvBn) and m.module.tsg_cbn_strided
    return m


@pytest.mark.parametrize("order", ["strided-first", "pointwise-first", "upgrade"])
@pytest.mark.parametrize("name", ["basicblock", "bottleneck"])
def test_a_whole_stride2_block_runs_on_our_kernels_and_repeats(cuda, name, order):
    """BasicBlock: conv1 / 2 and conv2 + residual on csrc/s2bn.hip and csrc/convbn.hip, the shortcut on csrc/pwbn.hip: three
    launches.  Bottleneck: conv1, conv3 and the shortcut on csrc/pwbn.hip, conv2 / 2 on csrc/s2bn.hip: four.  No convolution
    reaches the vendor library, so five eager calls and a graph replay are bit-identical on each of two inputs WITHOUT the
    vendor library pinned: the property this kernel adds.  (A plain install alone does not re-class a stride-2 Bottleneck,
    so its "upgrade" is a first re-classing behind pwbn's mixin; the BasicBlock's is a true upgrade.)"""
    from torchseg_amd import convbn, pwbn
    assert not torch.backends.cudnn.deterministic
    build, Cin, ref, _, _, pw_launches = MODULES[name]
    ours = {"basicblock": 2, "bottleneck": 1}[name]
    base = _randomise_bn(build(3), 9).eval()
    if name == "bottleneck" and order == "upgrade":
        from torchseg_amd.infer import prepare_inference
        assert prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=True).fused_convbn == 0
    eager = _all_ours(base, order, cuda)
    graph = _all_ours(base, order, cuda, graph=True)
    for seed in (10, 11):
        x, xd = _input(Cin, cuda, seed=seed)
        keep = xd.clone()
        c0, p0, s0 = convbn.fused_calls(eager.module), pwbn.fused_calls(eager.module), convbn.s2_fused_calls(eager.module)
        with _ConvCounter() as counter:
            first = eager(xd).clone()
        torch.cuda.synchronize()
        assert counter.n == 0, (name, order, counter.n)                    # no vendor convolution is left in the block
        assert convbn.fused_calls(eager.module) - c0 == ours and pwbn.fused_calls(eager.module) - p0 == pw_launches
        assert convbn.s2_fused_calls(eager.module) - s0 == 1 and ours + pw_launches == {"basicblock": 3, "bottleneck": 4}[name]
        outs = [first] + [eager(xd).clone() for _ in range(4)]
        replay = graph(xd).clone()
        torch.cuda.synchronize()
        for k, o in enumerate(outs[1:] + [replay]):
            assert torch.equal(_guard.raw_bytes(first), _guard.raw_bytes(o)), (name, order, seed, k)
        assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(keep))
        _assert_within(first, ref(eager.module, _Val(x.double()), cuda, True), "s2bn + pwbn %s %s" % (name, order))


# ---- SpatialPath -------------------------------------------------------------------------------------------------------
def _spatial_path(seed):
    from torchseg_amd.workloads.bisenet import SpatialPath
    torch.manual_seed(seed)
    return _randomise_bn(SpatialPath(3, 128, nn.BatchNorm2d), seed + 1).eval()


def test_spatial_path_runs_its_two_stride2_layers_fused(cuda, _pin_vendor_library):
    """Our SpatialPath calls the parts of its modules through seg_oprs.cbr_chain; with a strided install and gradients
    disabled the chain runs the modules, so conv_3x3_1 and conv_3x3_2 are two stride-2 launches per forward and conv_1x1 goes
    through its module (pwbn takes it when installed).  With gradients enabled the direct path runs, bit for bit the
    un-installed module's (vendor library pinned).  Without a strided install no launch count changes."""
    from torchseg_amd import convbn, pwbn
    from torchseg_amd.infer import prepare_inference
    base = _spatial_path(5)
    on = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_strided=True)
    off = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_strided=False)
    both = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_strided=True, fuse_pointwise=True)
    pw_only = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_pointwise=True)
    assert on.fused_strided == 2 and off.fused_strided == 0 and both.fused_strided == 2 and pw_only.fused_strided == 0
    assert both.fused_pointwise == pw_only.fused_pointwise == 1
    img = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(6)).to(BF).float()
    xd = img.to(cuda)
    for n in (1, 2):
        y = on(xd)
        torch.cuda.synchronize()
        assert convbn.s2_fused_calls(on.module) == 2 * n and convbn.fused_calls(on.module) == 2 * n
    assert y.dtype == BF and tuple(y.shape) == (1, 128, 8, 16)
    # against float64: the stem and the 1x1 are the stock two-rounding chains, the two 3x3 / 2 layers are fused
    m = on.module
    v = _layer64(_Val(img.double()), m.conv_7x7.conv, m.conv_7x7.bn, cuda, fused=False)
    v = _layer64(v, m.conv_3x3_1.conv, m.conv_3x3_1.bn, cuda)
    v = _layer64(v, m.conv_3x3_2.conv, m.conv_3x3_2.bn, cuda)
    _assert_within(y, _layer64(v, m.conv_1x1.conv, m.conv_1x1.bn, cuda, fused=False), "s2bn SpatialPath")
    both(xd)
    pw_only(xd)
    off(xd)
    torch.cuda.synchronize()
    assert convbn.s2_fused_calls(both.module) == 2 and pwbn.fused_calls(both.module) == 1     # conv_1x1 through its module
    assert pwbn.fused_calls(pw_only.module) == 0            # without a strided install the direct path: as before this feature
    assert convbn.fused_calls(off.module) == 0
    # gradients enabled: the direct path, bit for bit the un-installed module's
    for m_ in (on.module, off.module):
        for p in m_.parameters():
            p.requires_grad_(True)
    with torch.enable_grad(), torch.autocast("cuda", dtype=BF):
        a, b = on.module(xd).detach().clone(), off.module(xd).detach().clone()
    torch.cuda.synchronize()
    assert convbn.s2_fused_calls(on.module) == 4 and torch.equal(_guard.raw_bytes(a), _guard.raw_bytes(b))


# ---- networks ----------------------------------------------------------------------------------------------------------
def test_r18_counts_eager_graph_and_pending_tail(cuda, _pin_vendor_library):
    """fuse_convbn + fuse_strided, and with fuse_pointwise added: five stride-2 layers installed and five launches of the
    stride-2 kernel per forward, the other counts what they are without this feature, an eager call and a graph replay
    bit-equal (vendor library pinned: the stems are still its), the head still pending."""
    from torchseg_amd import convbn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import pending_tail, prepare_inference
    net = _r18(21).eval().to(cuda)
    for pw in (False, True):
        kw = dict(dtype=BF, fuse_convbn=True, fuse_pointwise=pw)
        without = prepare_inference(copy.deepcopy(net), fuse_strided=False, **kw)
        eager = prepare_inference(copy.deepcopy(net), fuse_strided=True, **kw)
        graph = prepare_inference(copy.deepcopy(net), fuse_strided=True, graph=True, **kw)
        assert eager.fused_strided == 5 and graph.fused_strided == 5 and without.fused_strided == 0
        assert eager.fused_convbn == without.fused_convbn == 20 and eager.fused_dilated == 0
        assert eager.fused_pointwise >= without.fused_pointwise and (pw or eager.fused_pointwise == 0)
        replays = []
        for n, seed in enumerate((1, 2)):
            x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(seed)).to(cuda)
            out = eager(x)
            tail = pending_tail(out)
            assert tail is not None and tuple(tail[1]) == (64, 128) and tail[0].shape[1] == 19    # still the pending head
            a = materialize(out).clone()
            b = graph(x).clone()
            torch.cuda.synchronize()
            assert a.shape == (1, 19, 64, 128) and bool(torch.isfinite(a).all())
            assert torch.equal(a, b), (pw, seed, float((a - b).abs().max()))
            assert convbn.s2_fused_calls(eager.module) == 5 * (n + 1)
            replays.append(b)
        assert not torch.equal(replays[0], replays[1])
        assert convbn.s2_fused_calls(graph.module) == 2 * 5  # the warm-up and the capture; the packs were ready for the capture
        materialize(without(x))
        assert convbn.s2_fused_calls(without.module) == 0
        assert convbn.fused_calls(eager.module) - 2 * 5 == 2 * convbn.fused_calls(without.module) == 2 * 18
    only = prepare_inference(copy.deepcopy(net), dtype=BF, fuse_strided=True)      # without fuse_convbn: the same five layers
    assert only.fused_strided == 5 and only.fused_convbn == 0
    materialize(only(x))
    assert convbn.s2_fused_calls(only.module) == 5 and convbn.fused_calls(only.module) == 8


MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


def test_r18_evaluator_consumes_the_pending_tail(cuda, monkeypatch):
    """TSG_INFER=1 with TSG_CONVBN_FUSED=1 and TSG_S2BN_FUSED=1: sliding_eval takes the fused window tail, and the class map
    equals the one of the same evaluator on the eager path."""
    from engine.evaluator import Evaluator
    from torchseg_amd.convbn import s2_fused_calls
    net = _r18(31).eval()
    monkeypatch.delenv("TSG_DTYPE", raising=False)
    monkeypatch.setenv("TSG_INFER", "1")
    monkeypatch.setenv("TSG_CONVBN_FUSED", "1")
    monkeypatch.setenv("TSG_S2BN_FUSED", "1")
    img = np.random.RandomState(0).randint(0, 256, (96, 160, 3)).astype(np.uint8)
    ev = Evaluator(None, 19, MEAN, STD, copy.deepcopy(net), [1.0], False, [0])
    ev.val_func = ev.network
    taken = []
    stock = ev._fused_window_scores
    monkeypatch.setattr(ev, "_fused_window_scores", lambda *a, **k: taken.append(stock(*a, **k)) or taken[-1])
    pred = ev.sliding_eval(img, 96, 2 / 3, device=0)
    assert pred.shape == (96, 160) and pred.min() >= 0 and pred.max() < 19
    assert taken and all(t is not None for t in taken)
    assert ev._infer_net.fused_convbn == 20 and ev._infer_net.fused_strided == 5 and s2_fused_calls(ev._infer_net.module) >= 5
    monkeypatch.setattr(ev, "_fused_window_scores", lambda *a, **k: None)
    eager = ev.sliding_eval(img, 96, 2 / 3, device=0)
    assert np.array_equal(pred, eager), int((pred != eager).sum())


def test_r18_backbone_and_logits_against_the_fp32_parity_run(cuda, _pin_vendor_library):
    """Per backbone stage (ResNet-18 on its own) and for the network's log-probabilities: with the stride-2 layers fused the
    bf16 network is at most 1.25 x as far from the fp32 parity run as the same bf16 network with the switch off (the factor
    tests/test_convbn_gpu.py and tests/test_dilbn_gpu.py use for this comparison).  fuse_convbn is on in every arm.  The
    vendor library, which runs the stems of both bf16 arms, is pinned.  The ratios printed here are profiles/s2bn_parity.txt."""
    from base_model.resnet import resnet18
    from torchseg_amd.convbn import s2_fused_calls
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    torch.manual_seed(11)
    backbone = _randomise_bn(resnet18(None, norm_layer=nn.BatchNorm2d), 12).eval()
    full = _r18(13).eval()
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(14)).to(cuda)
    for label, base, n in (("backbone", backbone, 3), ("network", full, 5)):
        kw = dict(fuse_convbn=True)
        arms = dict(parity=prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_strided=True, **kw),
                    unfused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_strided=False, **kw),
                    fused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_strided=True, **kw))
        outs = {}
        for k, m in arms.items():
            o = m(x)
            o = [materialize(o)] if label == "network" else list(o)
            outs[k] = [t.clone() for t in o]
        torch.cuda.synchronize()
        assert arms["fused"].fused_strided == n and arms["unfused"].fused_strided == 0
        assert s2_fused_calls(arms["fused"].module) == n and s2_fused_calls(arms["unfused"].module) == 0
        assert s2_fused_calls(arms["parity"].module) == 0               # fp32: the parity mode stays on the exact kernels
        dist = []
        for k, (pu, pf, pp) in enumerate(zip(outs["unfused"], outs["fused"], outs["parity"])):
            u, f = _rel(pu, pp), _rel(pf, pp)
            dist.append((u, f))
            what = "stage 1/%d" % (4 << k) if label == "backbone" else "log-probabilities"
            print("s2bn parity [%s] %s: max |d| / max |fp32 parity|: switch off bf16 %.4e, switch on bf16 %.4e (ratio %.3f); "
                  "elements that differ between on and off: %d of %d"
                  % (label, what, u, f, f / u if u else float("nan"), int((pu != pf).sum()), pu.numel()))
        for k, (u, f) in enumerate(dist):
            assert f <= 1.25 * u, (label, k, f, u)


def test_pspnet_r50_takes_its_one_stride2_layer(cuda, _pin_vendor_library):
    """The dilated backbone keeps one stride-2 3x3 (layer2.0.conv2): fused_strided == 1, one launch per forward, the other
    counts what they are without this feature."""
    from test_dilbn_cpu import _pspnet
    from torchseg_amd import convbn, pwbn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    net = _randomise_bn(_pspnet(50, 21), 22).eval().to(cuda)
    kw = dict(dtype=BF, fuse_convbn=True, fuse_dilated=True, fuse_pointwise=True)
    without = prepare_inference(copy.deepcopy(net), fuse_strided=False, **kw)
    on = prepare_inference(copy.deepcopy(net), fuse_strided=True, **kw)
    assert on.fused_strided == 1 and without.fused_strided == 0
    assert (on.fused_convbn, on.fused_dilated) == (without.fused_convbn, without.fused_dilated) == (9, 8)
    assert on.fused_pointwise == without.fused_pointwise
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(2)).to(cuda)
    a, b = materialize(on(x)), materialize(without(x))
    torch.cuda.synchronize()
    assert a.shape == (1, 19, 64, 128) and bool(torch.isfinite(a).all())
    assert convbn.s2_fused_calls(on.module) == 1 and convbn.s2_fused_calls(without.module) == 0
    assert convbn.dil_fused_calls(on.module) == convbn.dil_fused_calls(without.module) == 8
    assert convbn.fused_calls(on.module) - 1 == convbn.fused_calls(without.module)
    assert pwbn.fused_calls(on.module) == pwbn.fused_calls(without.module)
    print("s2bn PSPNet-R50: max |on - off| / max |off| %.4e" % _rel(a, b))


def test_resnet50_takes_three(cuda):
    from test_s2bn_cpu import _r50
    from torchseg_amd import convbn
    from torchseg_amd.infer import prepare_inference
    on = prepare_inference(_r50(3).eval().to(cuda), dtype=BF, fuse_convbn=True, fuse_strided=True, fuse_pointwise=True)
    assert on.fused_strided == 3 and on.fused_convbn == 13
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(2)).to(cuda)
    with _ConvCounter() as counter:
        outs = on(x)
    torch.cuda.synchronize()
    assert convbn.s2_fused_calls(on.module) == 3 and all(bool(torch.isfinite(o).all()) for o in outs)
    assert counter.n <= 1, counter.n                        # at most the 7x7 stem is left to the vendor library


def test_switch_unset_installs_nothing(cuda, monkeypatch, _pin_vendor_library):
    """Unset, or 0: no module is strided-enabled and the output is the network's without this feature, bit for bit, with the
    other switches the same (the vendor library pinned: the stride-2 layers run on it)."""
    from torchseg_amd import convbn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    monkeypatch.delenv("TSG_DTYPE", raising=False)
    monkeypatch.delenv("TSG_S2BN_FUSED", raising=False)
    net = _r18(41).eval().to(cuda)
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(42)).to(cuda)
    kw = dict(dtype=BF, fuse_convbn=True, fuse_pointwise=True)
    outs = []
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("TSG_S2BN_FUSED", env)
        unset = prepare_inference(copy.deepcopy(net), **kw)
        off = prepare_inference(copy.deepcopy(net), fuse_strided=False, **kw)
        for m in (unset, off):
            assert m.fused_strided == 0 and m.fused_convbn == 20
            assert not any(getattr(k, "tsg_cbn_strided", False) for k in m.modules())
        a, b = materialize(unset(x)).clone(), materialize(off(x)).clone()
        torch.cuda.synchronize()
        print("s2bn switch %r: max |unset - off| %.3e" % (env, float((a - b).abs().max())))
        assert torch.equal(a, b), env
        assert convbn.s2_fused_calls(unset.module) == 0 and convbn.fused_calls(unset.module) == 18
        outs.append(a)
    assert torch.equal(outs[0], outs[1])
    monkeypatch.setenv("TSG_S2BN_FUSED", "1")
    on = prepare_inference(copy.deepcopy(net), **kw)
    assert on.fused_strided == 5 and on.fused_convbn == 20
    materialize(on(x))
    assert convbn.s2_fused_calls(on.module) == 5
