"""GPU: the image convolutions with their BatchNorm (+ ReLU) as one launch at inference (stem_bnact_fwd_k in
csrc/stemconv.hip, ds_bnact_fwd_k in csrc/deepstem.hip) and torchseg_amd/stembn.py, against torch's CPU float64
`F.conv2d` on the operands the kernels read (x and w rounded to bf16).  The conventions, the bound (_fused_tol: derived
from the formats, K = 27 for the 3x3 and 147 for the 7x7) and the module helpers are tests/test_convbn_gpu.py's.

  1. exact data: every sum is exact in fp32 in any order, the output must be BIT-equal to the float64 value rounded once;
  2. random data against float64 within _fused_tol, per element;
  3. operands, pack and output inside poisoned guard bands (tests/_guard.py), three calls bit-identical, x unchanged;
  4. modules: a SpatialPath and a deep-stem ResNet-50 through prepare_inference: counters, no convolution left to the
     vendor library, eager calls and a graph replay bit-identical WITHOUT pinning the vendor library;
  5. BiSeNet-R18 and PSPNet-R50: counts, the other installers' counts, the pending tail and the Evaluator, and the distance
     from the fp32 parity run against the same bf16 network's with the switch off;
  6. the switch's default.

Shapes (B, H, W) of the IMAGE -- the smallest at which padding, stride and tiling can go wrong:
  3x3: (1, 1, 1)      one pixel: only the centre tap is ever in range
       (1, 7, 9)      odd x odd, smaller than a tile
       (2, 8, 64)     output 4 x 32: exactly one tile per image
       (2, 18, 66)    output 9 x 33: ragged both ways
       (3, 34, 80)    output 17 x 40, three images, several tiles
  7x7: (1, 1, 2)      one row, the narrowest even width
       (1, 7, 10)     odd H, smaller than a tile
       (2, 8, 64), (2, 18, 66) as above
       (2, 198, 1024) output 99 x 512: 2 x 25 x 16 = 800 tiles for 768 persistent blocks, ragged rows: a block walks a
                      second tile (tests/test_stembn_cpu.py asserts it is the only such case)"""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _guard
from test_convbn_cpu import _r18, _randomise_bn
from test_convbn_gpu import _Val, _assert_within, _epilogue64, _fused_tol, _layer64, _rel
from test_s2bn_gpu import _ConvCounter
from test_stembn_cpu import GPU_CASES_3, GPU_CASES_7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
CASES = [(3,) + c for c in GPU_CASES_3] + [(7,) + c for c in GPU_CASES_7]      # (k, B, H, W)
_ids = lambda c: "%dx%d-" % (c[0], c[0]) + "x".join(map(str, c[1:]))
ALL = dict(fuse_convbn=True, fuse_dilated=True, fuse_strided=True, fuse_pointwise=True)


@pytest.fixture(autouse=True)
def _restore_process_globals(monkeypatch):
    """prepare_inference switches syncbn.PREFER_CHANNELS_LAST_OUTPUT on for the process"""
    from torchseg_amd import syncbn
    monkeypatch.setattr(syncbn, "PREFER_CHANNELS_LAST_OUTPUT", syncbn.PREFER_CHANNELS_LAST_OUTPUT)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", torch.backends.cudnn.benchmark)


@pytest.fixture
def _pin_vendor_library(monkeypatch):
    """a bit-for-bit comparison of the STOCK path against itself needs the vendor library's deterministic kernels; the
    fused kernels do not read the setting"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


# ---- kernel level ------------------------------------------------------------------------------------------------------
def _operands(case, exact, seed=0):
    """CPU operands: the image [B,3,H,W] already rounded to bf16, w fp32 [64,3,k,k] (bf16-representable when exact),
    fp32 a, b"""
    k, B, H, W = case
    g = torch.Generator().manual_seed(seed + 1000 * k + 64 + 7 * H)
    if exact:
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
        x = ri(-2, 2, B, 3, H, W)
        w = ri(-1, 1, 64, 3, k, k)
        a = torch.pow(2.0, ri(-1, 1, 64))
        b = ri(-16, 16, 64) / 4
    else:
        x = torch.randn(B, 3, H, W, generator=g)
        w = torch.randn(64, 3, k, k, generator=g) * (2.0 / (3 * k * k)) ** 0.5
        a = 0.5 + torch.rand(64, generator=g)
        a = a * torch.where(torch.rand(64, generator=g) < 0.25, -1.0, 1.0)
        b = torch.randn(64, generator=g) * 0.5
    return x.to(BF), w, a, b


_REF = {}


def _ref64(case, exact, seed=0):
    """(operands, u64, S): the float64 k x k / 2 / (k // 2) convolution of the bf16-rounded operands and the same sum of
    absolute values; computed once per case and shared, never written"""
    key = (case, exact, seed)
    if key not in _REF:
        ops = _operands(case, exact, seed)
        x, w = ops[0].double(), ops[1].to(BF).double()
        k = case[0]
        _REF[key] = (ops, F.conv2d(x, w, None, 2, k // 2), F.conv2d(x.abs(), w.abs(), None, 2, k // 2))
    return _REF[key]


def _device_operands(ops, dev):
    x, w, a, b = ops
    fp = torch.stack([a, b, torch.zeros_like(a)]).to(dev)                 # rows 0, 1 of a fwd_pack [3][64]
    return x.to(dev).contiguous(), w.to(dev), fp


def _check(got, case, u, S, a, b, relu, what):
    y64 = _epilogue64(u, a, b, None, relu)
    aS = a.double().abs().view(1, -1, 1, 1) * S
    mag = aS + b.double().abs().view(1, -1, 1, 1)
    tol = _fused_tol(y64, aS, mag, 3 * case[0] * case[0])                # K = 27 resp. 147
    err = (got.double().cpu() - y64).abs()
    bad = ~(err <= tol)
    print("stembn %s: max err %.3e, max err / tol %.3f" % (what, float(err.max()), float((err / tol).max())))
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err - tol).max()))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_exact_data_is_bit_equal_to_float64(cuda, case):
    """x in [-2, 2] integers, w in {-1, 0, 1}, a in {1/2, 1, 2}, b multiples of 1/4 in [-4, 4]: |u| <= 2 * 147 is an
    integer, a u + b a multiple of 1/4 below 2^10: exact in fp32 in any order; the only rounding is the last one."""
    from torchseg_amd import kernels as K
    kp = K.provider()
    k, B, H, W = case
    ops, u, _ = _ref64(case, True)
    x, w, a, b = ops
    xd, wd, fp = _device_operands(ops, cuda)
    assert kp.image_bnact_supported(xd, k)
    pack = kp.image_bnact_pack(wd, fp)
    assert float(u.abs().max()) * 2 + 4 < 2 ** 10
    assert tuple(u.shape) == (B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    for relu in (True, False):
        y = kp.image_bnact_fwd(xd, pack, k, relu)
        want = _epilogue64(u, a, b, None, relu)
        assert torch.equal(want, want.float().double())                 # the float64 value is an fp32 number
        want = want.float().to(BF)
        assert y.dtype == BF and y.shape == want.shape and y.is_contiguous(memory_format=CL)
        got = y.cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
            (case, relu, int((got != want).sum()), float((got.float() - want.float()).abs().max()))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_random_data_against_float64(cuda, case):
    from torchseg_amd import kernels as K
    kp = K.provider()
    k = case[0]
    ops, u, S = _ref64(case, False)
    x, w, a, b = ops
    xd, wd, fp = _device_operands(ops, cuda)
    pack = kp.image_bnact_pack(wd, fp)
    keep = xd.clone()
    for relu in (True, False):
        y = kp.image_bnact_fwd(xd, pack, k, relu)
        y2 = kp.image_bnact_fwd(xd, pack, k, relu)
        torch.cuda.synchronize()
        assert y.dtype == BF and y.is_contiguous(memory_format=CL)
        assert torch.equal(_guard.raw_bytes(y), _guard.raw_bytes(y2))   # bit-identical from launch to launch
        _check(y, case, u, S, a, b, relu, (case, relu))
    assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(keep))
    # the accumulator is the unfused kernel's: with a = 1, b = 0 and no ReLU the result is that kernel's, bit for bit
    one = torch.stack([torch.ones(64), torch.zeros(64), torch.zeros(64)]).to(cuda)
    plain = kp.stem_conv_fwd(xd, wd) if k == 7 else kp.stem3_conv_fwd(xd, wd)
    same = kp.image_bnact_fwd(xd, kp.image_bnact_pack(wd, one), k, False)
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(plain), _guard.raw_bytes(same))


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_inside_guard_bands(cuda, case, relu):
    """The image, the weight and the BatchNorm pack in guarded arenas, the filter pack, ab and the output allocated
    through Guarded(fill) under both fills: no guard byte moves and the three results are bit-identical; x is unchanged;
    then the raw entry point with y at a 48-byte offset inside a larger poisoned allocation: the same bits, and not a
    byte around y has moved."""
    from torchseg_amd import _lib, kernels as K
    kp = K.provider()
    k, B, H, W = case
    ops, u, S = _ref64(case, False, seed=3)
    x, w, a, b = ops
    xd, wd, fp = _device_operands(ops, cuda)
    keep = xd.clone()

    def layer(xx, ww, fwd_pack):
        return kp.image_bnact_fwd(xx, kp.image_bnact_pack(ww, fwd_pack), k, relu)

    plain = _guard.three_calls(layer, [xd, wd, fp])[0]
    _check(plain, case, u, S, a, b, relu, (case, relu, "guarded"))
    assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(keep))

    wp, ab = kp.image_bnact_pack(wd, fp)
    n, off = plain.numel(), 24
    buf = torch.full((n + 2 * off + 64,), 0x5a5a, dtype=torch.int16, device=cuda).view(BF)
    vy = buf[off:off + n].view(plain.shape[0], plain.shape[2], plain.shape[3], plain.shape[1]).permute(0, 3, 1, 2)
    assert vy.data_ptr() % 16 == 0
    entry = kp.lib.tsg_stem_conv_bnact_fwd if k == 7 else kp.lib.tsg_stem3_conv_bnact_fwd
    _lib.call(entry, xd.data_ptr(), wp.data_ptr(), ab.data_ptr(), vy.data_ptr(), B, H, W, int(relu), _lib.stream_ptr(xd))
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(vy), _guard.raw_bytes(plain))
    raw = buf.view(torch.int16)
    assert bool((raw[:off] == 0x5a5a).all()) and bool((raw[off + n:] == 0x5a5a).all())
    # a misaligned output is refused before any launch
    assert entry(xd.data_ptr(), wp.data_ptr(), ab.data_ptr(), vy.data_ptr() + 8, B, H, W, int(relu), _lib.stream_ptr(xd)) == -4
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(vy), _guard.raw_bytes(plain))


# ---- modules -----------------------------------------------------------------------------------------------------------
def _image(seed, cuda, B=1, H=64, W=128):
    img = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed)).to(BF).float()
    return img, img.to(cuda)


def _spatial_path(seed):
    from torchseg_amd.workloads.bisenet import SpatialPath
    torch.manual_seed(seed)
    return _randomise_bn(SpatialPath(3, 128, nn.BatchNorm2d), seed + 1).eval()


def test_spatial_path_runs_on_our_kernels_only(cuda, _pin_vendor_library):
    """fuse_stem + fuse_strided + fuse_pointwise: the 7x7 stem is one launch of the image kernel, the two stride-2 layers
    and the 1x1 are the other installers', and no convolution reaches the dispatcher.  Against the float64 composition of
    its own modules, every layer fused.  With the stem switch alone the chain still runs the modules, and the result is
    within the bound of the composition with only the stem fused.  With gradients enabled the direct path runs, bit for
    bit the un-installed module's."""
    from torchseg_amd import convbn, pwbn, stembn
    from torchseg_amd.infer import prepare_inference
    base = _spatial_path(5)
    on = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_stem=True, fuse_strided=True, fuse_pointwise=True)
    stem_only = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_stem=True)
    off = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_stem=False)
    assert on.fused_stem == 1 and stem_only.fused_stem == 1 and off.fused_stem == 0
    assert on.fused_strided == 2 and on.fused_pointwise == 1 and stem_only.fused_strided == 0
    img, xd = _image(6, cuda)
    keep = xd.clone()
    for n in (1, 2):
        with _ConvCounter() as counter:
            y = on(xd)
        torch.cuda.synchronize()
        assert counter.n == 0, counter.n
        assert stembn.image_fused_calls(on.module) == n and stembn.fused_calls(on.module) == n
        assert convbn.s2_fused_calls(on.module) == 2 * n and pwbn.fused_calls(on.module) == n
    assert y.dtype == BF and tuple(y.shape) == (1, 128, 8, 16) and torch.equal(xd, keep)
    m = on.module
    v = _layer64(_Val(img.double()), m.conv_7x7.conv, m.conv_7x7.bn, cuda)
    v1 = _layer64(v, m.conv_3x3_1.conv, m.conv_3x3_1.bn, cuda)
    v2 = _layer64(v1, m.conv_3x3_2.conv, m.conv_3x3_2.bn, cuda)
    _assert_within(y, _layer64(v2, m.conv_1x1.conv, m.conv_1x1.bn, cuda), "stembn SpatialPath, all fused")
    ys = stem_only(xd)
    torch.cuda.synchronize()
    assert stembn.image_fused_calls(stem_only.module) == 1 and convbn.fused_calls(stem_only.module) == 0
    v1 = _layer64(v, m.conv_3x3_1.conv, m.conv_3x3_1.bn, cuda, fused=False)
    v2 = _layer64(v1, m.conv_3x3_2.conv, m.conv_3x3_2.bn, cuda, fused=False)
    _assert_within(ys, _layer64(v2, m.conv_1x1.conv, m.conv_1x1.bn, cuda, fused=False), "stembn SpatialPath, stem fused")
    off(xd)
    assert stembn.fused_calls(off.module) == 0
    # the pack cache: an in-place write to the weight and to running_var show in the next call
    before = on(xd).clone()
    with torch.no_grad():
        m.conv_7x7.conv.weight.mul_(-0.5)
        m.conv_7x7.bn.running_var.mul_(4.0)
    after = on(xd).clone()
    torch.cuda.synchronize()
    assert not torch.equal(before, after)
    v = _layer64(_Val(img.double()), m.conv_7x7.conv, m.conv_7x7.bn, cuda)
    v2 = _layer64(_layer64(v, m.conv_3x3_1.conv, m.conv_3x3_1.bn, cuda), m.conv_3x3_2.conv, m.conv_3x3_2.bn, cuda)
    _assert_within(after, _layer64(v2, m.conv_1x1.conv, m.conv_1x1.bn, cuda), "stembn SpatialPath after in-place writes")
    # gradients enabled, and train mode: the replaced path, bit for bit the un-installed module's (vendor library pinned)
    calls = stembn.fused_calls(stem_only.module)
    for m_ in (stem_only.module, off.module):
        for p in m_.parameters():
            p.requires_grad_(True)
    with torch.enable_grad(), torch.autocast("cuda", dtype=BF):
        a, b = stem_only.module(xd).detach().clone(), off.module(xd).detach().clone()
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(a), _guard.raw_bytes(b)) and stembn.fused_calls(stem_only.module) == calls
    # fp32 (the parity mode): nothing is fused
    par = prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_stem=True)
    par(xd)
    assert par.fused_stem == 1 and stembn.fused_calls(par.module) == 0


def _deep_r50(seed):
    from base_model.resnet import resnet50
    torch.manual_seed(seed)
    return _randomise_bn(resnet50(None, norm_layer=nn.BatchNorm2d, deep_stem=True, stem_width=64), seed + 1).eval()


def _stem64(m, x, dev, fused=(True, True, True)):
    """the deep stem in front of the pool as a float64 composition"""
    c = m.conv1
    v = _layer64(x, c[0], c[1], dev, fused=fused[0])
    v = _layer64(v, c[3], c[4], dev, fused=fused[1])
    return _layer64(v, c[6], m.bn1, dev, fused=fused[2])


def test_deep_stem_resnet50_runs_no_vendor_convolution_and_repeats(cuda):
    """All five switches on a deep-stem ResNet-50: fused_stem == 3, three launches through this installer per forward (one
    of them an image kernel), no convolution reaches the dispatcher, so five eager calls and a graph replay are
    bit-identical on each of two inputs WITHOUT the vendor library pinned.  The stem's output against float64."""
    from torchseg_amd import stembn
    from torchseg_amd.infer import prepare_inference
    assert not torch.backends.cudnn.deterministic
    base = _deep_r50(3)
    eager = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_stem=True, **ALL)
    graph = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_stem=True, graph=True, **ALL)
    off = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_stem=False, **ALL)
    assert eager.fused_stem == 3 and graph.fused_stem == 3 and off.fused_stem == 0
    for name in ("fused_convbn", "fused_dilated", "fused_strided", "fused_pointwise"):
        assert getattr(eager, name) == getattr(off, name), name
    for seed in (10, 11):
        img, xd = _image(seed, cuda)
        keep = xd.clone()
        c0, i0 = stembn.fused_calls(eager.module), stembn.image_fused_calls(eager.module)
        with _ConvCounter() as counter:
            first = [t.clone() for t in eager(xd)]
        torch.cuda.synchronize()
        assert counter.n == 0, counter.n                                   # no vendor convolution is left in the backbone
        assert stembn.fused_calls(eager.module) - c0 == 3 and stembn.image_fused_calls(eager.module) - i0 == 1
        outs = [[t.clone() for t in eager(xd)] for _ in range(4)]
        replay = [t.clone() for t in graph(xd)]
        torch.cuda.synchronize()
        for k, o in enumerate(outs + [replay]):
            for u, v in zip(first, o):
                assert torch.equal(_guard.raw_bytes(u), _guard.raw_bytes(v)), (seed, k)
        assert torch.equal(xd, keep) and all(bool(torch.isfinite(t).all()) for t in first)
        assert stembn.fused_calls(eager.module) - c0 == 15 and stembn.image_fused_calls(eager.module) - i0 == 5
        # the stem alone, against float64 (the pool selects: it is exact and cannot widen a difference)
        m = eager.module
        with torch.no_grad(), torch.autocast("cuda", dtype=BF):
            got = m._stem(xd)
        want = _stem64(m, _Val(img.double()), cuda)
        _assert_within(got, _Val(F.max_pool2d(want.v, 3, 2, 1), F.max_pool2d(want.tol, 3, 2, 1)), "stembn deep stem")
    with _ConvCounter() as counter:
        off(xd)
    assert counter.n >= 1 and stembn.fused_calls(off.module) == 0           # the switch-off arm: the image layer at least


def test_deep_stem_layers_fuse_on_their_own_terms(cuda, _pin_vendor_library):
    """A hook on the first BatchNorm of the stem: the image layer runs its stock modules (the hook fires), the two inner
    layers still fuse.  The module in train mode, or gradients enabled: the replaced method, bit for bit (vendor library
    pinned), and the packs are rebuilt by the next fused call."""
    from torchseg_amd import stembn
    from torchseg_amd.infer import prepare_inference
    base = _deep_r50(4)
    on = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_stem=True)
    off = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_stem=False)
    img, xd = _image(12, cuda)
    m = on.module
    fired = []
    handle = m.conv1[1].register_forward_hook(lambda *a: fired.append(1))
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        got = m._stem(xd)
    torch.cuda.synchronize()
    assert fired == [1] and stembn.fused_calls(m) == 2 and stembn.image_fused_calls(m) == 0
    want = _stem64(m, _Val(img.double()), cuda, fused=(False, True, True))
    _assert_within(got, _Val(F.max_pool2d(want.v, 3, 2, 1), F.max_pool2d(want.tol, 3, 2, 1)), "stembn deep stem, c0 stock")
    handle.remove()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        m._stem(xd)
    assert stembn.fused_calls(m) == 5 and stembn.image_fused_calls(m) == 1
    for train, grad in ((True, False), (False, True)):
        outs = []
        for net in (on.module, off.module):
            net.train(train)
            with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=BF):
                outs.append([t.detach().clone() for t in net(xd)])
            net.eval()
        torch.cuda.synchronize()
        for u, v in zip(*outs):
            assert torch.equal(_guard.raw_bytes(u), _guard.raw_bytes(v)), (train, grad)
    assert stembn.fused_calls(m) == 5
    for (k, p), (_, q) in zip(on.module.state_dict().items(), off.module.state_dict().items()):
        assert torch.equal(p, q), k                                         # the running statistics moved alike
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):                 # the train-mode call dropped the packs
        got = m._stem(xd)
    want = _stem64(m, _Val(img.double()), cuda)
    _assert_within(got, _Val(F.max_pool2d(want.v, 3, 2, 1), F.max_pool2d(want.tol, 3, 2, 1)), "stembn deep stem after train()")
    assert stembn.fused_calls(m) == 8


# ---- networks ----------------------------------------------------------------------------------------------------------
def _pspnet50(seed):
    from test_dilbn_cpu import _pspnet
    return _randomise_bn(_pspnet(50, seed), seed + 1).eval()


@pytest.mark.parametrize("which", ["r18", "pspnet"])
def test_networks_counts_eager_graph_and_pending_tail(cuda, which, _pin_vendor_library):
    """Every switch on: 1 layer in BiSeNet-R18, 3 in PSPNet-R50, that many launches through this installer per forward,
    the other installers' counts and launches equal with the switch on and off, the output finite, the head still pending,
    and an eager call equal to a graph replay bit for bit (vendor library pinned: the heads' classifiers are still its)."""
    from torchseg_amd import convbn, pwbn, stembn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import pending_tail, prepare_inference
    net, n = ((_r18(21).eval(), 1) if which == "r18" else (_pspnet50(21), 3))
    net = net.to(cuda)
    without = prepare_inference(copy.deepcopy(net), dtype=BF, fuse_stem=False, **ALL)
    eager = prepare_inference(copy.deepcopy(net), dtype=BF, fuse_stem=True, **ALL)
    graph = prepare_inference(copy.deepcopy(net), dtype=BF, fuse_stem=True, graph=True, **ALL)
    assert eager.fused_stem == n and graph.fused_stem == n and without.fused_stem == 0
    for name in ("fused_convbn", "fused_dilated", "fused_strided", "fused_pointwise", "fused_separable"):
        assert getattr(eager, name) == getattr(without, name), name
    for k, seed in enumerate((1, 2)):
        _, x = _image(seed, cuda)
        out = eager(x)
        tail = pending_tail(out)
        assert tail is not None and tuple(tail[1]) == (64, 128) and tail[0].shape[1] == 19    # still the pending head
        a = materialize(out).clone()
        b = graph(x).clone()
        torch.cuda.synchronize()
        assert a.shape == (1, 19, 64, 128) and bool(torch.isfinite(a).all())
        assert torch.equal(a, b), (which, seed, float((a - b).abs().max()))
        assert stembn.fused_calls(eager.module) == n * (k + 1) and stembn.image_fused_calls(eager.module) == k + 1
    assert stembn.fused_calls(graph.module) == 2 * n           # the warm-up and the capture; the packs were ready for it
    materialize(without(x))
    materialize(without(x))
    assert stembn.fused_calls(without.module) == 0
    assert convbn.fused_calls(eager.module) == convbn.fused_calls(without.module)
    assert convbn.s2_fused_calls(eager.module) == convbn.s2_fused_calls(without.module)
    assert convbn.dil_fused_calls(eager.module) == convbn.dil_fused_calls(without.module)
    assert pwbn.fused_calls(eager.module) == pwbn.fused_calls(without.module)


MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


def test_r18_evaluator_consumes_the_pending_tail(cuda, monkeypatch):
    """TSG_INFER=1 with TSG_STEMBN_FUSED=1 beside the other switches: sliding_eval takes the fused window tail, and the
    class map equals the one of the same evaluator on the eager path."""
    from engine.evaluator import Evaluator
    from torchseg_amd.stembn import image_fused_calls
    net = _r18(31).eval()
    monkeypatch.delenv("TSG_DTYPE", raising=False)
    monkeypatch.setenv("TSG_INFER", "1")
    for name in ("TSG_CONVBN_FUSED", "TSG_S2BN_FUSED", "TSG_PWBN_FUSED", "TSG_STEMBN_FUSED"):
        monkeypatch.setenv(name, "1")
    img = np.random.RandomState(0).randint(0, 256, (96, 160, 3)).astype(np.uint8)
    ev = Evaluator(None, 19, MEAN, STD, copy.deepcopy(net), [1.0], False, [0])
    ev.val_func = ev.network
    taken = []
    stock = ev._fused_window_scores
    monkeypatch.setattr(ev, "_fused_window_scores", lambda *a, **k: taken.append(stock(*a, **k)) or taken[-1])
    pred = ev.sliding_eval(img, 96, 2 / 3, device=0)
    assert pred.shape == (96, 160) and pred.min() >= 0 and pred.max() < 19
    assert taken and all(t is not None for t in taken)
    assert ev._infer_net.fused_stem == 1 and ev._infer_net.fused_strided == 5 and image_fused_calls(ev._infer_net.module) >= 1
    monkeypatch.setattr(ev, "_fused_window_scores", lambda *a, **k: None)
    eager = ev.sliding_eval(img, 96, 2 / 3, device=0)
    assert np.array_equal(pred, eager), int((pred != eager).sum())


def test_backbone_stages_and_logits_against_the_fp32_parity_run(cuda, _pin_vendor_library):
    """Per backbone stage (the deep-stem ResNet-50 on its own) and for the log-probabilities of BiSeNet-R18 and PSPNet-R50:
    with the stems fused the bf16 network is at most 1.25 x as far from the fp32 parity run as the same bf16 network with
    the switch off (the factor tests/test_convbn_gpu.py, test_dilbn_gpu.py and test_s2bn_gpu.py use for this comparison).
    Every other switch is on in every arm.  The ratios printed here are profiles/stembn_parity.txt."""
    from torchseg_amd import stembn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    _, x = _image(14, cuda)
    for label, base, n in (("deep-stem R50 backbone", _deep_r50(11), 3), ("BiSeNet-R18", _r18(13).eval(), 1),
                           ("PSPNet-R50", _pspnet50(15), 3)):
        arms = dict(parity=prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_stem=True, **ALL),
                    unfused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_stem=False, **ALL),
                    fused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_stem=True, **ALL))
        outs = {}
        for k, m in arms.items():
            o = m(x)
            o = list(o) if label.endswith("backbone") else [materialize(o)]
            outs[k] = [t.clone() for t in o]
        torch.cuda.synchronize()
        assert arms["fused"].fused_stem == n and arms["unfused"].fused_stem == 0
        assert stembn.fused_calls(arms["fused"].module) == n and stembn.fused_calls(arms["unfused"].module) == 0
        assert stembn.fused_calls(arms["parity"].module) == 0               # fp32: the parity mode stays on the exact kernels
        dist = []
        for k, (pu, pf, pp) in enumerate(zip(outs["unfused"], outs["fused"], outs["parity"])):
            u, f = _rel(pu, pp), _rel(pf, pp)
            dist.append((u, f))
            what = "stage 1/%d" % (4 << k) if label.endswith("backbone") else "log-probabilities"
            print("stembn parity [%s] %s: max |d| / max |fp32 parity|: switch off bf16 %.4e, switch on bf16 %.4e (ratio %.3f); "
                  "elements that differ between on and off: %d of %d"
                  % (label, what, u, f, f / u if u else float("nan"), int((pu != pf).sum()), pu.numel()))
        for k, (u, f) in enumerate(dist):
            assert f <= 1.25 * u, (label, k, f, u)


def test_switch_unset_installs_nothing(cuda, monkeypatch, _pin_vendor_library):
    """Unset, or 0: no module is re-classed by this installer and the output is the network's without this feature, bit
    for bit, with the other switches the same (the vendor library pinned: the deep stem runs on it)."""
    from torchseg_amd import stembn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    monkeypatch.delenv("TSG_DTYPE", raising=False)
    monkeypatch.delenv("TSG_STEMBN_FUSED", raising=False)
    _, x = _image(42, cuda)
    for which, net, n in (("r18", _r18(41).eval().to(cuda), 1), ("pspnet", _pspnet50(43).to(cuda), 3)):
        outs = []
        for env in (None, "0"):
            if env is not None:
                monkeypatch.setenv("TSG_STEMBN_FUSED", env)
            unset = prepare_inference(copy.deepcopy(net), dtype=BF, **ALL)
            off = prepare_inference(copy.deepcopy(net), dtype=BF, fuse_stem=False, **ALL)
            for m in (unset, off):
                assert m.fused_stem == 0
                assert not any(isinstance(k, stembn._FusedStem) or getattr(k, "tsg_stem_fused", False) for k in m.modules())
            a, b = materialize(unset(x)).clone(), materialize(off(x)).clone()
            torch.cuda.synchronize()
            print("stembn switch %r [%s]: max |unset - off| %.3e" % (env, which, float((a - b).abs().max())))
            assert torch.equal(a, b), (which, env)
            assert stembn.fused_calls(unset.module) == 0
            outs.append(a)
        assert torch.equal(outs[0], outs[1])
        monkeypatch.setenv("TSG_STEMBN_FUSED", "1")
        on = prepare_inference(copy.deepcopy(net), dtype=BF, **ALL)
        assert on.fused_stem == n
        materialize(on(x))
        assert stembn.fused_calls(on.module) == n and stembn.image_fused_calls(on.module) == 1
        monkeypatch.delenv("TSG_STEMBN_FUSED", raising=False)
