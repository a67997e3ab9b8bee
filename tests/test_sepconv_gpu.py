"""GPU: the fused separable unit (csrc/sepconv.hip) against torch's CPU float64 convolutions on the same rounded inputs.

  1. exact data (bf16): every sum is exact in any order, the output must be BIT-equal to the float64 value rounded once;
  2. random data, both dtypes, against float64 within bounds derived from the formats (see _check);
  3. every operand, the output and the pack inside poisoned guard bands (tests/_guard.py);
  4. the Xception39 backbone: all 51 units fused, error against the fp32 parity run no worse than 1.25 x the unfused
     bf16 path's, also after the running statistics or the whole state dict changed (the pack cache);
  5. through prepare_inference: eager, graph replay, the pending head tail, the Evaluator, and the switch's default;
  6. training through the DDP wrapper is bit for bit what it was.

Shapes: the fifteen (C_in, C_out, stride) combinations of Xception39 at 2 x 13 x 19, three of them at a single row, a map
smaller than a strip, an odd map of several strips and 96 x 192 (32-pixel strips), and two at 128 x 256 = 32768 pixels,
the size from which the launcher takes 64-pixel strips (one with fewer tiles than waves, one with two tiles per wave)."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _guard
from test_sepconv_cpu import X39_UNITS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

pytestmark = pytest.mark.gpu

# (B, H, W, C_in, C_out, stride)
CASES = [(2, 13, 19) + u for u in X39_UNITS]
CASES += [(b, h, w) + u for u in ((8, 16, 2), (64, 64, 1), (256, 64, 1))
          for b, h, w in ((1, 1, 9), (3, 7, 5), (2, 33, 47), (1, 96, 192))]
CASES += [(1, 128, 256, 16, 16, 1), (1, 128, 256, 32, 128, 1)]            # 64-pixel strips
COMBOS = [(False, True), (False, False), (True, True), (True, False)]      # (residual, relu)
CL = torch.channels_last


@pytest.fixture(autouse=True)
def _restore_process_globals(monkeypatch):
    """prepare_inference and the DDP wrapper switch syncbn.PREFER_CHANNELS_LAST_OUTPUT on for the process"""
    from torchseg_amd import syncbn
    monkeypatch.setattr(syncbn, "PREFER_CHANNELS_LAST_OUTPUT", syncbn.PREFER_CHANNELS_LAST_OUTPUT)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", torch.backends.cudnn.benchmark)


def _out(n, s):
    return (n - 1) // s + 1


def _operands(case, dtype, exact, seed=0):
    """CPU operands: x and residual already rounded to `dtype`; fp32 filters; fp32 a, b"""
    B, H, W, Cin, Cout, s = case
    g = torch.Generator().manual_seed(seed + 1000 * Cin + Cout + 7 * H)
    OH, OW = _out(H, s), _out(W, s)
    if exact:
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
        x = ri(-2, 2, B, Cin, H, W)
        wd = ri(-2, 2, Cin, 1, 3, 3) / 2
        wp = ri(-1, 1, Cout, Cin, 1, 1)
        a = torch.pow(2.0, ri(-1, 1, Cout))
        b = ri(-16, 16, Cout) / 4
        res = ri(-4, 4, B, Cout, OH, OW)
    else:
        x = torch.randn(B, Cin, H, W, generator=g)
        wd = torch.randn(Cin, 1, 3, 3, generator=g) * 0.3
        wp = torch.randn(Cout, Cin, 1, 1, generator=g) * (2.0 / Cin) ** 0.5
        a = 0.5 + torch.rand(Cout, generator=g)
        a = a * torch.where(torch.rand(Cout, generator=g) < 0.25, -1.0, 1.0)
        b = torch.randn(Cout, generator=g) * 0.5
        res = torch.randn(B, Cout, OH, OW, generator=g)
    return x.to(dtype), wd, wp, a, b, res.to(dtype)


def _ref64(x, wd, wp, stride, round_wp):
    """u64 = W_p . dw3x3(x, W_d) in float64, and S = the same composition of absolute values"""
    Cin = x.shape[1]
    wp64 = (wp.bfloat16() if round_wp else wp).double()
    u = F.conv2d(F.conv2d(x.double(), wd.double(), None, stride, 1, 1, Cin), wp64)
    S = F.conv2d(F.conv2d(x.double().abs(), wd.double().abs(), None, stride, 1, 1, Cin), wp64.abs())
    return u, S


def _epilogue64(u, a, b, res, relu):
    v = a.double().view(1, -1, 1, 1) * u + b.double().view(1, -1, 1, 1)
    if res is not None:
        v = v + res.double()
    return v.clamp_min(0.0) if relu else v


def _ulp(v, mant):
    """one unit in the last place of the float64 value v in a format with `mant` explicit mantissa bits"""
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-38)))
    return torch.pow(2.0, e - mant)


def _check(got, y64, S, a, b, res, dtype, what):
    """|y - y64| <= 1 ulp of y64 in the output format + the unit's own rounding:
    bf16: 2^-8 |a| S (one rounding of t, <= 2^-9 relative, + fp32 accumulation over <= 9 taps and <= 256 channels,
          <= 2^-15) + 2^-22 (|a| S + |b| + |residual|) for the fp32 epilogue;
    fp32: 2^-44 (|a| S + |b| + |residual|): fp64 sums of <= 9 + 256 terms and the fp64 affine"""
    aS = a.double().abs().view(1, -1, 1, 1) * S
    mag = aS + b.double().abs().view(1, -1, 1, 1) + (res.double().abs() if res is not None else 0.0)
    if dtype == torch.bfloat16:
        tol = _ulp(y64, 7) + 2.0 ** -8 * aS + 2.0 ** -22 * mag
    else:
        tol = _ulp(y64, 23) + 2.0 ** -44 * mag
    err = (got.double().cpu() - y64).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err - tol).max()))


def _device_operands(ops, dev):
    x, wd, wp, a, b, res = ops
    fp = torch.stack([a, b, torch.zeros_like(a)]).to(dev)                 # rows 0, 1 of a fwd_pack [3][C_out]
    return x.to(dev).contiguous(memory_format=CL), wd.to(dev), wp.to(dev), fp, res.to(dev).contiguous(memory_format=CL)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_data_is_bit_equal_to_float64(cuda, case):
    """x in [-2, 2] integers, W_d in {-1, -1/2, 0, 1/2, 1}, W_p in {-1, 0, 1}, a in {1/2, 1, 2}, b multiples of 1/4 in
    [-4, 4], residual integers in [-4, 4]: |t| <= 18 in steps of 1/2 is exact in bf16, |a u| < 2^14 in steps of 1/4 is
    exact in fp32 in any order; the only rounding is the last one."""
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout, s = case
    ops = _operands(case, torch.bfloat16, exact=True)
    x, wd, wp, a, b, res = ops
    xd, wdd, wpd, fp, resd = _device_operands(ops, cuda)
    assert kp.sepconv_supported(xd, Cout, s)
    pack = kp.sepconv_pack(wdd, wpd, fp, torch.bfloat16)
    u, _ = _ref64(x, wd, wp, s, round_wp=True)
    assert float(u.abs().max()) * 2 < 2 ** 14
    for with_res, relu in COMBOS:
        y = kp.sepconv_fwd(xd, pack, Cout, s, resd if with_res else None, relu)
        want = _epilogue64(u, a, b, res if with_res else None, relu)
        assert torch.equal(want, want.float().double())                 # the float64 value is an fp32 number
        want = want.float().bfloat16()
        assert y.dtype == torch.bfloat16 and y.shape == want.shape and y.is_contiguous(memory_format=CL)
        got = y.cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
            (case, with_res, relu, int((got != want).sum()), float((got.float() - want.float()).abs().max()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_random_data_against_float64(cuda, case, dtype):
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout, s = case
    ops = _operands(case, dtype, exact=False)
    x, wd, wp, a, b, res = ops
    xd, wdd, wpd, fp, resd = _device_operands(ops, cuda)
    assert kp.sepconv_supported(xd, Cout, s)
    pack = kp.sepconv_pack(wdd, wpd, fp, dtype)
    u, S = _ref64(x, wd, wp, s, round_wp=dtype == torch.bfloat16)
    for with_res, relu in COMBOS:
        r = resd if with_res else None
        y = kp.sepconv_fwd(xd, pack, Cout, s, r, relu)
        y2 = kp.sepconv_fwd(xd, pack, Cout, s, r, relu)
        torch.cuda.synchronize()
        assert y.dtype == dtype and y.is_contiguous(memory_format=CL)
        assert torch.equal(_guard.raw_bytes(y), _guard.raw_bytes(y2))   # bit-identical from launch to launch
        y64 = _epilogue64(u, a, b, res if with_res else None, relu)
        _check(y, y64, S, a, b, res if with_res else None, dtype, (case, with_res, relu))


GUARDED_CASES = [((2, 13, 19, 8, 64, 2), False),          # the zero-padded K path
                 ((1, 7, 5, 256, 64, 1), False),
                 ((2, 1, 9, 16, 16, 1), True),            # with residual; C_out below one MFMA tile
                 ((1, 1, 1, 128, 256, 2), False)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case,with_res", GUARDED_CASES, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_inside_guard_bands(cuda, case, with_res, dtype):
    """Operands in guarded arenas, the pack and the output allocated through Guarded(fill) under both fills: no guard byte
    moves, and pack and output are bit-identical across the fills and to the plain call."""
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, H, W, Cin, Cout, s = case
    ops = _operands(case, dtype, exact=False, seed=3)
    xd, wdd, wpd, fp, resd = _device_operands(ops, cuda)

    def unit(x, wd, wp, fwd_pack, res):
        pack = kp.sepconv_pack(wd, wp, fwd_pack, x.dtype)
        return kp.sepconv_fwd(x, pack, Cout, s, res, True), pack

    plain = _guard.three_calls(unit, [xd, wdd, wpd, fp, resd if with_res else None])[0]
    x, wd, wp, a, b, res = ops
    u, S = _ref64(x, wd, wp, s, round_wp=dtype == torch.bfloat16)
    r = res if with_res else None
    _check(plain[0], _epilogue64(u, a, b, r, True), S, a, b, r, dtype, case)


# ---- module level ----------------------------------------------------------------------------------------------------
def _randomise_bn(net, seed):
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            with torch.no_grad():
                m.weight.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
    return net


def _backbone(seed):
    from torchseg_amd.workloads.bisenet_x39 import xception39
    torch.manual_seed(seed)
    return _randomise_bn(xception39(None, norm_layer=nn.BatchNorm2d), seed + 1).eval()


def _stage_errors(outs, parity):
    return [float((o.float() - p.float()).abs().max() / p.float().abs().max()) for o, p in zip(outs, parity)]


def test_xception39_backbone_fused_against_the_fp32_parity_run(cuda):
    from torchseg_amd.infer import prepare_inference
    from torchseg_amd.sepconv import fused_calls
    base = _backbone(11)
    arms = dict(parity=prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_separable=False),
                unfused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.bfloat16, fuse_separable=False),
                fused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.bfloat16, fuse_separable=True))
    assert arms["fused"].fused_separable == 51 and arms["unfused"].fused_separable == 0
    x = torch.randn(2, 3, 96, 160, generator=torch.Generator().manual_seed(12)).to(cuda)

    def compare(label, calls):
        outs = {k: [o.clone() for o in m(x)] for k, m in arms.items()}
        torch.cuda.synchronize()
        assert fused_calls(arms["fused"].module) == calls and fused_calls(arms["unfused"].module) == 0
        assert [tuple(o.shape[1:]) for o in outs["fused"]] == [(64, 12, 20), (128, 6, 10), (256, 3, 5)]
        eu, ef = _stage_errors(outs["unfused"], outs["parity"]), _stage_errors(outs["fused"], outs["parity"])
        for k, (u, f) in enumerate(zip(eu, ef)):
            print("sepconv parity [%s] stage 1/%d: max |d| / max |fp32 parity|: unfused bf16 %.4e, fused bf16 %.4e (ratio %.3f)"
                  % (label, 8 << k, u, f, f / u))
        for k, (u, f) in enumerate(zip(eu, ef)):
            assert f <= 1.25 * u, (label, k, f, u)

    compare("seeded weights", 51)                        # every unit took the fused kernel, once
    for m in arms.values():                              # an in-place write to one unit's running statistics
        m.module.layer2[1].residual_branch[0].point_wise_cbr.bn.running_mean.add_(1.0)
    compare("after running_mean.add_(1)", 102)
    other = _backbone(21).state_dict()
    for m in arms.values():
        m.module.load_state_dict(other)
    compare("after load_state_dict", 153)


def _bisenet_x39(seed=0):
    from torchseg_amd.workloads.bisenet_x39 import BiSeNetX39
    torch.manual_seed(seed)
    return _randomise_bn(BiSeNetX39(19, False, None, None, pretrained_model=None, norm_layer=nn.BatchNorm2d), seed + 1).eval()


def test_graph_capture_includes_the_image_cast(cuda):
    """prepare_inference(graph=True) in bf16 on the image stem alone (tsg_stem_conv_fwd, bit-reproducible): the replay of a
    second image equals the eager result for THAT image.  The stems' cast cache used to serve the warm-up's bf16 copy of
    the static input during the capture, so the cast was not in the graph and every replay of BiSeNet's detail branch
    saw the first image (and, once the cache moved on, freed memory)."""
    from torchseg_amd.infer import prepare_inference
    from torchseg_amd.stemconv import StemConv2d
    torch.manual_seed(2)
    stem = nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3, bias=False)).to(cuda)
    eager = prepare_inference(copy.deepcopy(stem), dtype=torch.bfloat16)
    graph = prepare_inference(stem, dtype=torch.bfloat16, graph=True)
    assert isinstance(graph.module[0], StemConv2d)
    outs = []
    for seed in (1, 2, 1):
        x = torch.randn(1, 3, 96, 160, generator=torch.Generator().manual_seed(seed)).to(cuda)
        a, b = eager(x).clone(), graph(x).clone()
        torch.cuda.synchronize()
        assert a.dtype == torch.bfloat16 and torch.equal(a, b), seed
        outs.append(b)
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])


def test_prepare_inference_eager_graph_and_pending_tail(cuda):
    """Eager against graph replay bit for bit in the fp32 parity mode, where every layer of the network is one of this
    package's fixed-order kernels.  In bf16 two EAGER calls of BiSeNet-X39 on one input already differ now and then, with
    the switch off as well (max |d log p| 9e-4 .. 4e-3 in 3 of about 30 calls, the vendor library's convolutions), so
    bit-equality there would test that library; bf16 is checked for what is ours: the pending head, all 51 units fused in
    the eager call, in the warm-up and in the capture, replays that follow their input
    (test_graph_capture_includes_the_image_cast pins the cast), and the backbone against the parity run above."""
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import pending_tail, prepare_inference
    from torchseg_amd.sepconv import fused_calls
    net = _bisenet_x39().to(cuda)
    bf16 = prepare_inference(copy.deepcopy(net), dtype=torch.bfloat16, fuse_separable=True)
    bf16g = prepare_inference(copy.deepcopy(net), dtype=torch.bfloat16, graph=True, fuse_separable=True)
    shown = []
    for seed in (1, 2):
        x = torch.randn(1, 3, 96, 160, generator=torch.Generator().manual_seed(seed)).to(cuda)
        out = bf16(x)
        tail = pending_tail(out)
        assert tail is not None and tuple(tail[1]) == (96, 160) and tail[0].shape[1] == 19
        a, b = materialize(out).clone(), bf16g(x).clone()
        torch.cuda.synchronize()
        assert b.shape == a.shape and bool(torch.isfinite(b).all())
        print("bf16 BiSeNet-X39, fused: max |graph replay - eager| = %.3e (max |log p| %.3f)"
              % (float((a - b).abs().max()), float(a.abs().max())))
        shown.append(b)
    assert not torch.equal(shown[0], shown[1])
    assert bf16.fused_separable == 51 and fused_calls(bf16.module) == 2 * 51 and fused_calls(bf16g.module) == 2 * 51
    eager = prepare_inference(copy.deepcopy(net), dtype=torch.float32, fuse_separable=True)
    graph = prepare_inference(net, dtype=torch.float32, graph=True, fuse_separable=True)
    assert eager.fused_separable == 51 and graph.fused_separable == 51
    replays = []
    for seed in (1, 2):
        x = torch.randn(1, 3, 96, 160, generator=torch.Generator().manual_seed(seed)).to(cuda)
        out = eager(x)
        tail = pending_tail(out)
        assert tail is not None and tuple(tail[1]) == (96, 160) and tail[0].shape[1] == 19     # still the pending head
        a = materialize(out).clone()
        b = graph(x).clone()
        torch.cuda.synchronize()
        assert a.shape == (1, 19, 96, 160) and torch.equal(a, b)
        replays.append(b)
    assert not torch.equal(replays[0], replays[1])
    assert fused_calls(eager.module) == 2 * 51
    assert fused_calls(graph.module) == 2 * 51           # the warm-up and the capture; the packs were ready for the capture


MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


def test_evaluator_and_the_switch_default(cuda, monkeypatch):
    from engine.evaluator import Evaluator
    from torchseg_amd.infer import prepare_inference
    from torchseg_amd.sepconv import _FusedSeparable, fused_calls
    net = _bisenet_x39()
    monkeypatch.delenv("TSG_DTYPE", raising=False)
    monkeypatch.delenv("TSG_SEPCONV_FUSED", raising=False)
    for kw in ({}, {"fuse_separable": False}):           # unset, or off: nothing is re-classed
        plain = prepare_inference(copy.deepcopy(net).to(cuda), **kw)
        assert plain.fused_separable == 0 and not any(isinstance(m, _FusedSeparable) for m in plain.modules())
    monkeypatch.setenv("TSG_INFER", "1")
    monkeypatch.setenv("TSG_SEPCONV_FUSED", "1")
    img = np.random.RandomState(0).randint(0, 256, (96, 160, 3)).astype(np.uint8)
    ev = Evaluator(None, 19, MEAN, STD, copy.deepcopy(net), [1.0], False, [0])
    ev.val_func = ev.network
    pred = ev.sliding_eval(img, 96, 2 / 3, device=0)
    assert pred.shape == (96, 160) and pred.min() >= 0 and pred.max() < 19
    assert ev._infer_net.fused_separable == 51 and fused_calls(ev._infer_net.module) >= 51


def test_training_through_the_ddp_wrapper_is_untouched(cuda):
    """One fp32 step (the parity mode: every kernel of the step sums in a fixed order, so two copies of one network give
    the same bits) of BiSeNet-X39 behind the DDP wrapper, with and without install_fused_separable: the loss and every
    gradient are bit-equal, and no unit took the fused kernel.  In bf16 the forward is compared the same way."""
    from torchseg_amd.ddp import DistributedDataParallel
    from torchseg_amd.losses import ProbOhemCrossEntropy2d
    from torchseg_amd.sepconv import fused_calls, install_fused_separable
    from torchseg_amd.syncbn import SyncBatchNorm
    from torchseg_amd.workloads.bisenet_x39 import BiSeNetX39
    B, S = 2, 96
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, S, S, generator=g).to(cuda)
    y = torch.randint(0, 19, (B, S, S), generator=g)
    y[:, :8] = 255
    y = y.to(cuda)
    for dtype in (torch.float32, torch.bfloat16):
        steps = []
        for fuse in (False, True):
            torch.manual_seed(4)
            net = BiSeNetX39(19, True, None, ProbOhemCrossEntropy2d(255, thresh=0.7, min_kept=B * S * S // 16),
                             norm_layer=SyncBatchNorm)
            net = DistributedDataParallel(net.to(cuda), compute_dtype=dtype)
            if fuse:
                assert install_fused_separable(net.module) == 51
            net.train()
            loss = net(x, y)
            if dtype == torch.float32:
                loss.backward()
            torch.cuda.synchronize()
            assert fused_calls(net.module) == 0
            steps.append((loss.detach().clone(), {n: p.grad.clone() for n, p in net.module.named_parameters()
                                                  if p.grad is not None}))
        (l0, g0), (l1, g1) = steps
        assert torch.equal(l0, l1), (dtype, l0.item(), l1.item())
        assert sorted(g0) == sorted(g1) and (dtype != torch.float32 or len(g0) > 100)
        for n in g0:
            assert torch.equal(g0[n], g1[n]), (dtype, n)
