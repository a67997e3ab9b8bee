"""The autograd nodes in the states their parity tests leave out: eval-mode BatchNorm in a backward pass (alone, and frozen
behind a train-mode producer), frozen parameters, inputs without a gradient, accumulation into an existing .grad, a second
backward pass over a retained graph.  The reference is always the stock torch module sequence in float64 on the CPU, on the
bf16-rounded operands where the kernels read bf16; every bound is the one of the family's own parity test (quoted where it
is used); every case asserts by call counter which provider methods ran."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _states as T
from _states import BN_STATES, BnCase, bf16r, counted

pytestmark = pytest.mark.gpu

CL = dict(memory_format=torch.channels_last)


def _kp():
    from torchseg_amd import kernels as K
    return K.provider()


def _rel_l2(got, want):
    want = want.double().cpu()
    return ((got.double().cpu() - want).norm() / want.norm().clamp_min(1e-30)).item()


def _max_rel(got, want):
    want = want.double().cpu()
    return (got.double().cpu() - want).abs().max().item() / max(want.abs().max().item(), 1e-3)


def _bn_ref(C, gamma, beta, rm0, rv0, training):
    bn = nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
    return bn.train(training)


def _bn_dev(C, gamma, beta, rm0, rv0, training, frozen, cuda):
    from torchseg_amd.syncbn import SyncBatchNorm
    bn = SyncBatchNorm(C)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
    bn.train(training)
    if frozen:
        bn.weight.requires_grad_(False); bn.bias.requires_grad_(False)
    return bn.to(cuda)


def _bn_numbers(C, g):
    return (torch.randn(C, generator=g) * 0.4 + 1.0, torch.randn(C, generator=g) * 0.2, torch.randn(C, generator=g) * 0.3,
            torch.rand(C, generator=g) + 0.5)


def _stats(bn):
    return bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()


def _assert_stats_unchanged(bn, before):
    for a, b in zip(_stats(bn), before):
        assert torch.equal(a, b)


def _assert_eval_bn_calls(counts):
    """running estimates: folded by bn_affine; no statistics pass, no finalize, no statistics epilogue of a producer"""
    assert counts.get("bn_affine") == 1, counts
    for name in ("bn_stats", "bn_finalize", "stem_conv_fwd_stats", "stem_conv_stats", "bn_collapse"):
        assert name not in counts, (name, counts)


# ---- SyncBatchNorm (_SyncBNFn) -----------------------------------------------------------------------------------------
BN_SHAPES = [((2, 19, 7, 5), "nchw"), ((2, 19, 7, 5), "nhwc"), ((3, 24, 8, 8), "nchw"), ((3, 24, 8, 8), "nhwc"),
             ((2, 64, 33, 47), "nhwc")]


@pytest.mark.parametrize("state", BN_STATES)
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,layout", BN_SHAPES)
def test_syncbn(cuda, monkeypatch, shape, layout, dtype, relu, res, state):
    from torchseg_amd import kernels as K, syncbn
    monkeypatch.setattr(syncbn, "PREFER_CHANNELS_LAST_OUTPUT", False)
    monkeypatch.setattr(syncbn, "_MASKBITS", True)
    kp = _kp()
    case = BnCase(cuda, shape, layout, dtype, relu, res, state)
    lay = K.bn_layout(case.x)
    bits = bool(relu and res and kp.bn_maskbits_supported(case.x, lay[0], lay[2], lay[3]))
    if relu and res and shape[1] == 64:
        assert bits                                        # the block tail at C = 64 is the mask-bit kernels' case
    if bits:
        counts = case.run(kp, fwd="bn_apply_fwd_bits", bwd=("bn_bwd_reduce_bits", "bn_bwd_apply_bits"))
    else:
        counts = case.run(kp)
    assert ("bn_apply_fwd_bits" in counts) == bits


@pytest.mark.parametrize("state", BN_STATES)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_syncbn_mixed_layout(cuda, monkeypatch, dtype, relu, state):
    """NCHW in, channels_last out (and channels_last dy in, NCHW dx out)"""
    from torchseg_amd import syncbn
    monkeypatch.setattr(syncbn, "PREFER_CHANNELS_LAST_OUTPUT", True)
    kp = _kp()
    case = BnCase(cuda, (2, 64, 32, 32), "mixed", dtype, relu, False, state)
    assert kp.bn_mixed_supported(case.x)
    y = case.forward()
    assert y.is_contiguous(**CL) and not y.is_contiguous()
    case = BnCase(cuda, (2, 64, 32, 32), "mixed", dtype, relu, False, state)
    case.run(kp, fwd="bn_apply_fwd_mixed", bwd=("bn_bwd_reduce_mixed", "bn_bwd_apply_mixed"))
    if state != "no_dx":
        assert case.x.grad.is_contiguous()


# ---- bn_relu_maxpool (_BnReluPoolFn) -----------------------------------------------------------------------------------
def _pool_bounds(dtype, name, got, want):
    """tests/test_stemfuse_gpu.py:196-200: fp32 1e-3 of the tensor's scale; bf16 3e-2 of it, and — pooling windows whose
    near-ties pick another pixel than float64 re-route whole gradient entries — relative L2 0.2 for the gradients."""
    if dtype == torch.bfloat16 and name in ("dx", "dw", "dgamma", "dbeta"):
        err, bound = _rel_l2(got, want), 0.2
    else:
        err, bound = _max_rel(got, want), (1e-3 if dtype == torch.float32 else 3e-2)
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("state", ["eval", "frozen_affine", "accumulate"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", [(2, 16, 9, 11), (2, 8, 7, 30)])          # the two smallest CASES of test_stemfuse_gpu.py:51
def test_bn_relu_maxpool(cuda, case, dtype, state):
    from torchseg_amd.pool import MaxPool2d
    from torchseg_amd.syncbn import bn_relu_maxpool
    N, C, H, W = case
    g = torch.Generator().manual_seed(sum(case))
    x = (torch.randn(case, generator=g) * 1.5 + 0.4).to(dtype)
    nums = _bn_numbers(C, g)
    training = state != "eval"
    ref = _bn_ref(C, *nums, training)
    xr = x.double().requires_grad_(True)
    yr = F.max_pool2d(torch.relu(ref(xr)), 3, 2, 1)
    dys = [torch.randn(yr.shape, generator=g).to(dtype) for _ in range(2)]
    dxr, dgr, dbr = torch.autograd.grad(yr, [xr, ref.weight, ref.bias], dys[0].double())

    bn = _bn_dev(C, *nums, training, state == "frozen_affine", cuda)
    pool = MaxPool2d(3, 2, 1)
    xd = x.to(cuda).contiguous(**CL).requires_grad_(True)
    dyd = [d.to(cuda).contiguous(**CL) for d in dys]
    leaves = [xd] + list(bn.parameters())
    before = _stats(bn)

    def step(dy):
        y = bn_relu_maxpool(bn, xd, pool)
        assert y is not None
        y.backward(dy)
        return y

    counts = {}
    with counted(_kp(), counts):
        y = step(dyd[0])
    for name in ("bn_relu_pool_fwd", "bn_relu_pool_bwd_reduce", "bn_bwd_coeffs", "bn_relu_pool_bwd_apply"):
        assert counts.get(name) == 1, (name, counts)
    for name in ("bn_apply_fwd", "maxpool_fwd", "maxpool_bwd", "bn_bwd_reduce", "bn_bwd_apply"):
        assert name not in counts, (name, counts)
    _pool_bounds(dtype, "y", y.detach(), yr.detach())
    _pool_bounds(dtype, "dx", xd.grad, dxr)
    if state == "frozen_affine":
        assert bn.weight.grad is None and bn.bias.grad is None
    else:
        _pool_bounds(dtype, "dgamma", bn.weight.grad, dgr)
        _pool_bounds(dtype, "dbeta", bn.bias.grad, dbr)
    if training:
        assert counts.get("bn_stats") == 1 and counts.get("bn_finalize") == 1 and "bn_affine" not in counts, counts
        _pool_bounds(dtype, "running_mean", bn.running_mean, ref.running_mean)
        _pool_bounds(dtype, "running_var", bn.running_var, ref.running_var)
    else:
        _assert_eval_bn_calls(counts)
        _assert_stats_unchanged(bn, before)
    if state == "accumulate":
        T.check_accumulate(step, leaves, dyd[0], dyd[1], T.grads_of(leaves))


# ---- stem_bn_relu_maxpool (_StemConvBnReluPoolFn) ------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["bn_eval", "frozen_affine", "frozen_w", "accumulate"])
@pytest.mark.parametrize("form", [2, 1])
@pytest.mark.parametrize("image", [(2, 3, 64, 64), (1, 3, 70, 96)])
def test_stem_bn_relu_maxpool(cuda, monkeypatch, image, form, state):
    """The ResNet stem as one node, activation stored (TSG_STEM_RECOMPUTE=2) or re-evaluated (1).  Bounds:
    tests/test_stemfuse_gpu.py:196-200 (bf16)."""
    from torchseg_amd import syncbn
    from torchseg_amd.pool import MaxPool2d
    from torchseg_amd.stemconv import install_stem_conv
    monkeypatch.setattr(syncbn, "_STEM_RECOMPUTE", form)
    monkeypatch.setattr(syncbn, "_FUSE_STEM_POOL", True)
    monkeypatch.setattr(syncbn, "_STEM_WRW_READS_Y", False)
    g = torch.Generator().manual_seed(sum(image) + form)
    img = bf16r(torch.randn(image, generator=g))
    w = bf16r(torch.randn(64, 3, 7, 7, generator=g) * 0.1)
    nums = _bn_numbers(64, g)
    bn_training = state != "bn_eval"
    ref = _bn_ref(64, *nums, bn_training)
    wr = w.double().requires_grad_(True)
    yr = F.max_pool2d(torch.relu(ref(F.conv2d(img.double(), wr, None, 2, 3))), 3, 2, 1)
    dys = [bf16r(torch.randn(yr.shape, generator=g)) for _ in range(2)]
    dwr, dgr, dbr = torch.autograd.grad(yr, [wr, ref.weight, ref.bias], dys[0].double())

    conv = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    conv = conv.to(cuda)
    assert install_stem_conv(conv) == 1
    conv.train()                                           # the producer stays in train(): only the BatchNorm is frozen
    conv.weight.requires_grad_(state != "frozen_w")
    bn = _bn_dev(64, *nums, bn_training, state == "frozen_affine", cuda)
    pool = MaxPool2d(3, 2, 1)
    imgd = img.to(cuda).bfloat16()
    dyd = [d.to(cuda).bfloat16().contiguous(**CL) for d in dys]
    leaves = [conv.weight] + list(bn.parameters())
    before = _stats(bn)

    def step(dy):
        y = syncbn.stem_bn_relu_maxpool(conv, bn, imgd, pool)
        assert y is not None
        y.backward(dy)
        return y

    counts = {}
    with counted(_kp(), counts):
        y = step(dyd[0])
    torch.cuda.synchronize()
    full = form == 1
    fwd = ["stem_conv_bn_relu_pool_fwd"] if full else ["bn_relu_pool_fwd"]
    if bn_training:
        fwd += ["stem_conv_stats" if full else "stem_conv_fwd_stats", "bn_finalize"]
    elif not full:
        fwd += ["stem_conv_fwd"]
    bwd = ["stem_conv_bn_relu_pool_bwd_reduce" if full else "bn_relu_pool_bwd_reduce", "bn_bwd_coeffs"]
    for name in fwd + bwd:
        assert counts.get(name) == 1, (name, counts)
    assert "bn_stats" not in counts and "bn_relu_pool_bwd_apply" not in counts and "stem_conv_wrw" not in counts, counts
    if bn_training:
        assert "bn_affine" not in counts, counts
    else:
        _assert_eval_bn_calls(counts)
        _assert_stats_unchanged(bn, before)
    _pool_bounds(torch.bfloat16, "y", y.detach(), yr.detach())
    if state == "frozen_w":
        assert "stem_conv_wrw_bn_pool" not in counts and conv.weight.grad is None, counts     # the needs_input_grad[1] arm
    else:
        assert counts.get("stem_conv_wrw_bn_pool") == 1, counts
        _pool_bounds(torch.bfloat16, "dw", conv.weight.grad, dwr)
    if state == "frozen_affine":
        assert bn.weight.grad is None and bn.bias.grad is None
    else:
        _pool_bounds(torch.bfloat16, "dgamma", bn.weight.grad, dgr)
        _pool_bounds(torch.bfloat16, "dbeta", bn.bias.grad, dbr)
    if state == "accumulate":
        T.check_accumulate(step, leaves, dyd[0], dyd[1], T.grads_of(leaves))


# ---- bn_relu_conv (_BnReluConvFn) ----------------------------------------------------------------------------------------
def _bnconv_bound(name, got, want):
    """tests/test_bnconv_gpu.py:95-97: relative L2 2e-2 for the output and every gradient, 1e-3 for the running statistics"""
    err = _rel_l2(got, want)
    assert err <= (2e-2 if name in ("out", "dx", "dw", "dgamma", "dbeta", "dw_stem") else 1e-3), (name, err)


@pytest.mark.parametrize("state", ["bn_eval", "eval", "frozen_affine", "frozen_w", "accumulate"])
@pytest.mark.parametrize("shape,cout,stride", [((2, 64, 24, 40), 64, 1), ((2, 64, 24, 40), 64, 2), ((2, 128, 12, 40), 64, 1)])
def test_bn_relu_conv(cuda, monkeypatch, shape, cout, stride, state):
    from torchseg_amd import convwrw
    from torchseg_amd.convwrw import bn_relu_conv, install_conv_wrw
    from torchseg_amd.stemconv import attach_bn_partial, take_bn_partial
    monkeypatch.setattr(convwrw, "_BN_ON_LOAD", True)
    monkeypatch.setattr(convwrw, "_GEN_BN_ON_LOAD", True)         # the general kernel's form is opt-in
    monkeypatch.setattr(convwrw, "_BN_BSUM", False)
    for name in ("_OWN_C64", "_OWN_C64_S1", "_C64_STATS", "_OWN_GEN", "_GEN_STATS"):
        monkeypatch.setattr(convwrw, name, True)
    N, cin, H, W = shape
    gen = cin != 64
    g = torch.Generator().manual_seed(sum(shape) + stride)
    x = bf16r(torch.randn(shape, generator=g) * 1.5 + 0.4)
    w = bf16r(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5)
    nums = _bn_numbers(cin, g)
    bn_training = state not in ("bn_eval", "eval")
    ref = _bn_ref(cin, *nums, bn_training)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(torch.relu(ref(xr)), wr, None, stride, 1)
    dys = [bf16r(torch.randn(yr.shape, generator=g)) for _ in range(2)]
    dxr, dwr, dgr, dbr = torch.autograd.grad(yr, [xr, wr, ref.weight, ref.bias], dys[0].double())

    conv = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    conv = conv.to(cuda).to(**CL)
    assert install_conv_wrw(conv) == 1
    conv.train(state != "eval")
    conv.weight.requires_grad_(state != "frozen_w")
    bn = _bn_dev(cin, *nums, bn_training, state == "frozen_affine", cuda)
    relu = nn.ReLU()
    xd = x.to(cuda).bfloat16().contiguous(**CL).requires_grad_(True)
    dyd = [d.to(cuda).bfloat16().contiguous(**CL) for d in dys]
    leaves = [xd, conv.weight] + list(bn.parameters())
    before = _stats(bn)
    marker = torch.full((1, 2, cin), 1e6, device=cuda)
    if state == "bn_eval":
        attach_bn_partial(xd, marker)                      # what a train-mode producer leaves: an eval BatchNorm ignores it

    def step(dy):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = bn_relu_conv(bn, relu, xd, conv)
        y.backward(dy)
        return y

    counts = {}
    with counted(_kp(), counts):
        y = step(dyd[0])
    torch.cuda.synchronize()
    fwd_kernel = "conv3x3_gen_fwd" if gen else "conv3x3_c64_fwd"
    if state == "frozen_w":
        # the three modules: BatchNorm + ReLU as a pass of their own, the stock convolution behind them
        for name in ("bn_apply_fwd", "bn_bwd_reduce", "bn_bwd_apply"):
            assert counts.get(name) == 1, (name, counts)
        for name in ("conv3x3_wrw", "conv3x3_c64_fwd", "conv3x3_gen_fwd", "conv3x3_c64_s2_dgrad"):
            assert name not in counts, (name, counts)
        assert conv.weight.grad is None
    else:
        assert "bn_apply_fwd" not in counts, counts                     # the normalised activation is never written
        for name in ("conv3x3_wrw", "bn_bwd_reduce", "bn_bwd_coeffs", "bn_bwd_apply"):
            assert counts.get(name) == 1, (name, counts)
        if stride == 2:
            assert counts.get(fwd_kernel) == 1 and counts.get("conv3x3_c64_s2_dgrad") == 1, counts
        else:
            assert counts.get(fwd_kernel) == 2, counts                  # forward, and the data gradient as a forward
        _bnconv_bound("dw", conv.weight.grad, dwr)
        # the statistics partial of the output: only a convolution in train() collects it
        assert (take_bn_partial(y) is not None) == (state != "eval")
    if bn_training:
        assert counts.get("bn_stats") == 1 and counts.get("bn_finalize") == 1 and "bn_affine" not in counts, counts
        _bnconv_bound("running_mean", bn.running_mean, ref.running_mean)
        _bnconv_bound("running_var", bn.running_var, ref.running_var)
    else:
        _assert_eval_bn_calls(counts)
        _assert_stats_unchanged(bn, before)
    if state == "bn_eval":
        assert take_bn_partial(xd) is marker
    _bnconv_bound("out", y.detach(), yr.detach())
    _bnconv_bound("dx", xd.grad, dxr)
    if state == "frozen_affine":
        assert bn.weight.grad is None and bn.bias.grad is None
    else:
        _bnconv_bound("dgamma", bn.weight.grad, dgr)
        _bnconv_bound("dbeta", bn.bias.grad, dbr)
    if state == "accumulate":
        T.check_accumulate(step, leaves, dyd[0], dyd[1], T.grads_of(leaves))


# ---- stem_bn_relu_conv (_StemBnReluConvFn) -------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["bn_eval", "frozen_affine", "accumulate"])
def test_stem_bn_relu_conv(cuda, monkeypatch, state):
    """SpatialPath's first two layers as one node.  Bounds: tests/test_bnconv_gpu.py:95-97."""
    from torchseg_amd import convwrw
    from torchseg_amd.convwrw import install_conv_wrw, stem_bn_relu_conv
    from torchseg_amd.stemconv import install_stem_conv, take_bn_partial
    monkeypatch.setattr(convwrw, "_BN_ON_LOAD", True)
    monkeypatch.setattr(convwrw, "_STEM_BN_WRW", True)
    monkeypatch.setattr(convwrw, "_BN_BSUM", False)
    g = torch.Generator().manual_seed(41)
    img = bf16r(torch.randn(2, 3, 64, 64, generator=g))
    w0 = bf16r(torch.randn(64, 3, 7, 7, generator=g) * 0.1)
    w1 = bf16r(torch.randn(64, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5)
    nums = _bn_numbers(64, g)
    bn_training = state != "bn_eval"
    ref = _bn_ref(64, *nums, bn_training)
    w0r, w1r = w0.double().requires_grad_(True), w1.double().requires_grad_(True)
    yr = F.conv2d(torch.relu(ref(F.conv2d(img.double(), w0r, None, 2, 3))), w1r, None, 2, 1)
    dys = [bf16r(torch.randn(yr.shape, generator=g)) for _ in range(2)]
    dw0r, dw1r, dgr, dbr = torch.autograd.grad(yr, [w0r, w1r, ref.weight, ref.bias], dys[0].double())

    stem, conv = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.Conv2d(64, 64, 3, 2, 1, bias=False)
    with torch.no_grad():
        stem.weight.copy_(w0); conv.weight.copy_(w1)
    stem, conv = stem.to(cuda), conv.to(cuda).to(**CL)
    assert install_stem_conv(stem) == 1 and install_conv_wrw(conv) == 1
    stem.train(); conv.train()
    bn = _bn_dev(64, *nums, bn_training, state == "frozen_affine", cuda)
    relu = nn.ReLU()
    imgd = img.to(cuda).bfloat16()
    dyd = [d.to(cuda).bfloat16().contiguous(**CL) for d in dys]
    leaves = [stem.weight, conv.weight] + list(bn.parameters())
    before = _stats(bn)

    def step(dy):
        y = stem_bn_relu_conv(stem, bn, relu, imgd, conv)
        assert y is not None
        y.backward(dy)
        return y

    counts = {}
    with counted(_kp(), counts):
        y = step(dyd[0])
    torch.cuda.synchronize()
    for name in ("conv3x3_c64_fwd", "conv3x3_c64_s2_dgrad", "conv3x3_wrw", "bn_bwd_reduce", "bn_bwd_coeffs", "stem_conv_wrw_bn"):
        assert counts.get(name) == 1, (name, counts)
    for name in ("bn_apply_fwd", "bn_bwd_apply", "bn_stats", "stem_conv_wrw"):
        assert name not in counts, (name, counts)
    if bn_training:
        assert counts.get("stem_conv_fwd_stats") == 1 and counts.get("bn_finalize") == 1 and "bn_affine" not in counts, counts
    else:
        assert counts.get("stem_conv_fwd") == 1, counts
        _assert_eval_bn_calls(counts)
        _assert_stats_unchanged(bn, before)
    assert take_bn_partial(y) is not None                  # the 64 -> 64 convolution is in train()
    _bnconv_bound("out", y.detach(), yr.detach())
    _bnconv_bound("dw", conv.weight.grad, dw1r)
    _bnconv_bound("dw_stem", stem.weight.grad, dw0r)
    if state == "frozen_affine":
        assert bn.weight.grad is None and bn.bias.grad is None
    else:
        _bnconv_bound("dgamma", bn.weight.grad, dgr)
        _bnconv_bound("dbeta", bn.bias.grad, dbr)
    if state == "accumulate":
        T.check_accumulate(step, leaves, dyd[0], dyd[1], T.grads_of(leaves))


# ---- WrwConv2d: conv64, the general kernel, the stride-2 parity data gradient ----------------------------------------------
WRW_ROUTES = {"c64": ((2, 64, 9, 33), 64, 1), "gen": ((1, 128, 8, 32), 128, 1), "s2": ((2, 64, 13, 70), 128, 2)}
_DGRAD_CALLS = ("conv3x3_s2_dgrad", "conv3x3_c64_s2_dgrad", "conv3x3_weight_rot180_t")


def _wrw_case(cuda, route, seed=0):
    from torchseg_amd.convwrw import WrwConv2d, install_conv_wrw
    shape, cout, stride = WRW_ROUTES[route]
    cin = shape[1]
    g = torch.Generator().manual_seed(sum(shape) + seed)
    x = bf16r(torch.randn(shape, generator=g))
    w = bf16r(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, stride, 1)
    dys = [bf16r(torch.randn(yr.shape, generator=g)) for _ in range(2)]
    dxr, dwr = torch.autograd.grad(yr, [xr, wr], dys[0].double())
    conv = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    conv = conv.to(cuda).to(**CL)
    assert install_conv_wrw(conv) == 1 and isinstance(conv, WrwConv2d)
    xd = x.to(cuda).bfloat16().contiguous(**CL)
    dyd = [d.to(cuda).bfloat16().contiguous(**CL) for d in dys]
    return conv, xd, dyd, yr.detach(), dxr, dwr


@pytest.mark.parametrize("state", ["no_dx", "frozen_w", "eval"])
@pytest.mark.parametrize("route", list(WRW_ROUTES))
def test_wrw_conv(cuda, monkeypatch, route, state):
    """Bounds: _check of tests/test_conv3g_gpu.py:29-32 for y and dx, the 2e-3 of test_conv3g_gpu.py:147 for dw."""
    from torchseg_amd import convwrw
    from torchseg_amd.stemconv import take_bn_partial
    for name in ("_OWN_C64", "_OWN_C64_S1", "_C64_STATS", "_OWN_GEN", "_GEN_STATS", "_OWN_S2_DGRAD"):
        monkeypatch.setattr(convwrw, name, True)
    conv, xd, dyd, yr, dxr, dwr = _wrw_case(cuda, route)
    conv.train(state != "eval")
    conv.weight.requires_grad_(state != "frozen_w")
    xd.requires_grad_(state != "no_dx")
    counts = {}
    with counted(_kp(), counts):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = conv(xd)
        part = take_bn_partial(y)
        y.backward(dyd[0])
    torch.cuda.synchronize()
    fwd_kernel = {"c64": "conv3x3_c64_fwd", "gen": "conv3x3_gen_fwd", "s2": None}[route]
    T.conv_check(y.detach(), yr, "y")
    if state == "frozen_w":
        # not ours: the stock convolution, no kernel of the package's convolution families
        for name in ("conv3x3_wrw", "conv3x3_c64_fwd", "conv3x3_gen_fwd") + _DGRAD_CALLS:
            assert name not in counts, (name, counts)
        assert conv.weight.grad is None and part is None
        T.conv_check(xd.grad, dxr, "dx")
        return
    assert counts.get("conv3x3_wrw") == 1, counts
    T.wgrad_check(conv.weight.grad, dwr, "dw")
    if state == "no_dx":
        assert xd.grad is None
        if fwd_kernel is not None:
            assert counts.get(fwd_kernel) == 1, counts                 # the forward alone: no data-gradient launch
        for name in _DGRAD_CALLS:
            assert name not in counts, (name, counts)
        assert (part is not None) == (route != "s2")                    # train(): conv64 and the general kernel collect it
        return
    assert part is None                                                 # eval: no statistics partial
    T.conv_check(xd.grad, dxr, "dx")
    if route == "s2":
        assert counts.get("conv3x3_s2_dgrad") == 1, counts
    else:
        assert counts.get(fwd_kernel) == 2, counts


def test_wrw_conv_deferred_launch_list_and_accumulation(cuda, monkeypatch):
    """convwrw._DEFER open (a caller that launches the weight gradients later) across two backward passes without zero_grad:
    the first pass (no gradient yet) may list its launch; the second must compute in place — AccumulateGrad adds the tensor
    it is handed at once — and the parameter ends with g1 + g2."""
    from torchseg_amd import convwrw
    conv, xd, dyd, yr, dxr, dwr = _wrw_case(cuda, "c64", seed=1)
    xd.requires_grad_(True)
    leaves = [xd, conv.weight]
    listed = []

    def step(dy):
        monkeypatch.setattr(convwrw, "_DEFER", [])
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                conv(xd).backward(dy)
            todo = list(convwrw._DEFER)
        finally:
            monkeypatch.setattr(convwrw, "_DEFER", None)
        listed.append(len(todo))
        for launch, _operands, _buf in todo:              # the caller's part: run the list
            launch()

    with torch.autocast("cuda", dtype=torch.bfloat16):
        conv(xd).backward(dyd[0])                          # in place, nothing deferred: g1
    g1 = T.grads_of(leaves)
    T.wgrad_check(g1[1], dwr, "dw")
    T.check_accumulate(step, leaves, dyd[0], dyd[1], g1)
    # single pass (dy2) | dy1, dy2 onto nothing | dy1, dy2 onto zeroed gradients: only a pass onto NO gradient defers
    assert listed == [1, 1, 0, 0, 0], listed


# ---- DilatedConv2d (_DilConvFn) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["no_dx", "frozen_w", "eval", "accumulate", "retain"])
@pytest.mark.parametrize("case", [(1, 16, 64, 5, 37, 2), (1, 64, 128, 3, 7, 4)])     # the smallest SHAPES of test_dilconv_gpu.py:28
def test_dilated_conv(cuda, case, state):
    """Bounds: _check (tests/test_dilconv_gpu.py:57-61, the same as test_conv3g_gpu.py:29-32) and the 2e-3 weight-gradient
    bound of test_conv3g_gpu.py:147."""
    from torchseg_amd.dilconv import DilatedConv2d, install_dilated_conv
    from torchseg_amd.stemconv import take_bn_partial
    B, Cin, Cout, H, W, d = case
    g = torch.Generator().manual_seed(sum(case))
    x = bf16r(torch.randn(B, Cin, H, W, generator=g))
    w = bf16r(torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5)
    dys = [bf16r(torch.randn(B, Cout, H, W, generator=g)) for _ in range(2)]
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, 1, d, d)
    dxr, dwr = torch.autograd.grad(yr, [xr, wr], dys[0].double())
    conv = nn.Conv2d(Cin, Cout, 3, 1, d, d, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    conv = conv.to(cuda).to(**CL)
    assert install_dilated_conv(conv) == 1 and type(conv) is DilatedConv2d
    conv.train(state != "eval")
    conv.weight.requires_grad_(state != "frozen_w")
    xd = x.to(cuda).bfloat16().contiguous(**CL).requires_grad_(state != "no_dx")
    dyd = [t.to(cuda).bfloat16().contiguous(**CL) for t in dys]
    leaves = [xd, conv.weight]

    def forward():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return conv(xd)

    def step(dy):
        forward().backward(dy)

    counts = {}
    with counted(_kp(), counts):
        y = forward()
        part = take_bn_partial(y)
        y.backward(dyd[0], retain_graph=state == "retain")
    torch.cuda.synchronize()
    need_dx, need_dw = state != "no_dx", state != "frozen_w"
    assert counts.get("conv3x3_dil_fwd") == 1 + need_dx, counts          # the data gradient is the same kernel, mode-1 filter
    assert counts.get("conv3x3_dil_dgrad", 0) == int(need_dx) and counts.get("conv3x3_dil_wrw", 0) == int(need_dw), counts
    assert (part is not None) == (state != "eval")                      # eval: no statistics partial is attached
    T.conv_check(y.detach(), yr.detach(), "y")
    if need_dx:
        T.conv_check(xd.grad, dxr, "dx")
    else:
        assert xd.grad is None
    if need_dw:
        T.wgrad_check(conv.weight.grad, dwr, "dw")
    else:
        assert conv.weight.grad is None
    if state == "retain":
        T.check_retain(y, dyd[0], leaves, T.grads_of(leaves))
    if state == "accumulate":
        T.check_accumulate(step, leaves, dyd[0], dyd[1], T.grads_of(leaves))


# ---- DepthwiseConv2d (_DwConvFn) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["no_dx", "frozen_w", "retain"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [(2, 24, 13, 29, 1), (3, 8, 7, 5, 2)])     # smallest stride-1 / stride-2 CASES, test_dwconv_gpu.py:14
def test_depthwise_conv(cuda, case, dtype, state):
    """Bounds: tests/test_dwconv_gpu.py:72-79 (one ulp of the float64 value in the output format + the accumulation's own
    rounding).  bf16 under autocast, fp32 outside it (the parity mode), as the module takes them."""
    from torchseg_amd.dwconv import DepthwiseConv2d, install_depthwise_conv
    B, C, H, W, stride = case
    g = torch.Generator().manual_seed(sum(case))
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(B, C, H, W, generator=g).to(dtype)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.3
    dy = torch.randn(B, C, OH, OW, generator=g).to(dtype)
    xr, wr, gr = x.double(), w.double(), dy.double()
    yr = F.conv2d(xr, wr, None, stride, 1, 1, C)
    dxr = torch.nn.grad.conv2d_input(xr.shape, wr, gr, stride, 1, 1, C)
    dwr = torch.nn.grad.conv2d_weight(xr, wr.shape, gr, stride, 1, 1, C)
    ay = F.conv2d(xr.abs(), wr.abs(), None, stride, 1, 1, C)
    adx = torch.nn.grad.conv2d_input(xr.shape, wr.abs(), gr.abs(), stride, 1, 1, C)
    adw = torch.nn.grad.conv2d_weight(xr.abs(), wr.shape, gr.abs(), stride, 1, 1, C)
    holder = nn.Sequential(nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False))
    with torch.no_grad():
        holder[0].weight.copy_(w)
    holder = holder.to(cuda)
    assert install_depthwise_conv(holder) == 1 and isinstance(holder[0], DepthwiseConv2d)
    conv = holder[0]
    conv.weight.requires_grad_(state != "frozen_w")
    xd = x.to(cuda).contiguous(**CL).requires_grad_(state != "no_dx")
    dyd = dy.to(cuda).contiguous(**CL)
    leaves = [xd, conv.weight]
    counts = {}
    with counted(_kp(), counts):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            y = conv(xd)
        y.backward(dyd, retain_graph=state == "retain")
    torch.cuda.synchronize()
    need_dx, need_dw = state != "no_dx", state != "frozen_w"
    assert counts.get("dwconv3x3_fwd") == 1 and counts.get("dwconv3x3_dgrad", 0) == int(need_dx) \
        and counts.get("dwconv3x3_wgrad", 0) == int(need_dw), counts
    mant, eps, eps_w = (7, 9 * 2.0 ** -24, 2.0 ** -18) if dtype == torch.bfloat16 else (23, 2.0 ** -48, 2.0 ** -44)
    assert y.dtype == dtype
    T.ulp_check(y.detach(), yr, ay, mant, eps, "y")
    if need_dx:
        T.ulp_check(xd.grad, dxr, adx, mant, eps, "dx")
    else:
        assert xd.grad is None
    if need_dw:
        T.ulp_check(conv.weight.grad, dwr, adw, 23, eps_w, "dw")
    else:
        assert conv.weight.grad is None
    if state == "retain":
        T.check_retain(y, dyd, leaves, T.grads_of(leaves))


# ---- PointwiseConv2d (_PointwiseFn) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["no_dx", "frozen_w", "accumulate"])
@pytest.mark.parametrize("hip_wgrad", [False, True])
def test_pointwise_conv(cuda, monkeypatch, hip_wgrad, state):
    """64 -> 128 at 24 x 40 (CASES[0] of tests/test_pwconv_gpu.py).  Bounds: y and dx as test_pwconv_gpu.py:55-58 (the _check
    form); dw relative L2 1e-5 (test_pwconv_gpu.py:59-60) for the batched-GEMM fold, 1e-4 of the scale + 1e-6
    (tests/test_pwwgrad_gpu.py:130) for the HIP kernel."""
    from torchseg_amd import pwconv
    from torchseg_amd.pwconv import PointwiseConv2d, install_pointwise_conv
    monkeypatch.setattr(pwconv, "_HIP_WGRAD", hip_wgrad)
    monkeypatch.setattr(pwconv, "ENABLED", True)
    monkeypatch.setattr(pwconv, "_DGRAD_MM", True)
    B, cin, cout, H, W = 2, 64, 128, 24, 40
    g = torch.Generator().manual_seed(298)
    x = bf16r(torch.randn(B, cin, H, W, generator=g))
    w = bf16r(torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5)
    dys = [bf16r(torch.randn(B, cout, H, W, generator=g)) for _ in range(2)]
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr)
    dxr, dwr = torch.autograd.grad(yr, [xr, wr], dys[0].double())
    conv = nn.Conv2d(cin, cout, 1, 1, 0, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    conv = conv.to(cuda).to(**CL)
    assert install_pointwise_conv(nn.Sequential(conv)) == 1 and isinstance(conv, PointwiseConv2d)
    conv.weight.requires_grad_(state != "frozen_w")
    xd = x.to(cuda).bfloat16().contiguous(**CL).requires_grad_(state != "no_dx")
    dyd = [t.to(cuda).bfloat16().contiguous(**CL) for t in dys]
    leaves = [xd, conv.weight]
    taken = []
    orig = pwconv._PointwiseFn.apply
    monkeypatch.setattr(pwconv._PointwiseFn, "apply", staticmethod(lambda *a: (taken.append(1), orig(*a))[1]))

    def step(dy):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = conv(xd)
        y.backward(dy)
        return y

    counts = {}
    with counted(_kp(), counts):
        y = step(dyd[0])
    torch.cuda.synchronize()
    T.conv_check(y.detach(), yr.detach(), "y")
    if state == "frozen_w":
        assert not taken and "pw_wgrad" not in counts and conv.weight.grad is None, counts        # the stock convolution
    else:
        assert len(taken) == 1 and counts.get("pw_wgrad", 0) == int(hip_wgrad), counts
        if hip_wgrad:
            err = (conv.weight.grad.double().cpu() - dwr).abs().max().item()
            assert err <= 1e-4 * dwr.abs().max().item() + 1e-6, err
        else:
            rel = _rel_l2(conv.weight.grad, dwr)
            assert rel <= 1e-5, rel
    if state == "no_dx":
        assert xd.grad is None
    else:
        T.conv_check(xd.grad, dxr, "dx")
    if state == "accumulate":
        T.check_accumulate(step, leaves, dyd[0], dyd[1], T.grads_of(leaves))
        assert len(taken) == 6                              # every pass took the module's own functions


def test_pointwise_conv_deferred_launch_list_and_accumulation(cuda, monkeypatch):
    """The same as test_wrw_conv_deferred_launch_list_and_accumulation for the 1x1 layers' own deferral (pwconv)."""
    from torchseg_amd import convwrw, pwconv
    from torchseg_amd.pwconv import install_pointwise_conv
    monkeypatch.setattr(pwconv, "_HIP_WGRAD", False)
    monkeypatch.setattr(pwconv, "_DEFER_OK", True)
    g = torch.Generator().manual_seed(77)
    conv = nn.Conv2d(64, 128, 1, 1, 0, bias=False)
    with torch.no_grad():
        conv.weight.copy_(bf16r(torch.randn(128, 64, 1, 1, generator=g) * (2.0 / 64) ** 0.5))
    conv = conv.to(cuda).to(**CL)
    assert install_pointwise_conv(nn.Sequential(conv)) == 1
    xd = torch.randn(2, 64, 24, 40, generator=g).to(cuda).bfloat16().contiguous(**CL).requires_grad_(True)
    dyd = [torch.randn(2, 128, 24, 40, generator=g).to(cuda).bfloat16().contiguous(**CL) for _ in range(2)]
    leaves = [xd, conv.weight]
    listed = []

    def step(dy):
        monkeypatch.setattr(convwrw, "_DEFER", [])
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                conv(xd).backward(dy)
            todo = list(convwrw._DEFER)
        finally:
            monkeypatch.setattr(convwrw, "_DEFER", None)
        listed.append(len(todo))
        for launch, _operands, _buf in todo:
            launch()

    with torch.autocast("cuda", dtype=torch.bfloat16):
        conv(xd).backward(dyd[0])
    T.check_accumulate(step, leaves, dyd[0], dyd[1], T.grads_of(leaves))
    assert listed == [1, 1, 0, 0, 0], listed


# ---- ClsHeadConv2d / ClsHeadWideConv2d (_ClsHeadFn) ------------------------------------------------------------------------
CLS_CASES = [("narrow", (1, 32, 4, 4, 7, False)), ("narrow", (3, 32, 8, 10, 1, True)),     # tests/test_clshead_gpu.py:16-18
             ("wide", (2, 192, 2, 2, 97, True))]                                            # tests/test_clshead_wide_gpu.py:24-32


@pytest.mark.parametrize("kind,case,state", [(k, c, s) for k, c in CLS_CASES for s in ("no_dx", "frozen_w", "frozen_bias", "accumulate")
                                             if c[5] or s != "frozen_bias"])      # (no bias: nothing to freeze)
def test_cls_head(cuda, monkeypatch, kind, case, state):
    """Bounds: tests/test_clshead_gpu.py:45,55-58 and tests/test_clshead_wide_gpu.py:73,82-89 (the same numbers)."""
    from torchseg_amd import clshead
    monkeypatch.setattr(clshead, "ENABLED", True)
    B, Cin, H, W, N, has_bias = case
    g = torch.Generator().manual_seed(sum(case[:5]))
    x = bf16r(torch.randn(B, Cin, H, W, generator=g))
    w = bf16r(torch.randn(N, Cin, 1, 1, generator=g) * (1.0 / Cin) ** 0.5)
    bias = torch.randn(N, generator=g) if has_bias else None
    dzs = [bf16r(torch.randn(B, N, H, W, generator=g)) for _ in range(2)]
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = bias.double().requires_grad_(True) if has_bias else None
    zr = F.conv2d(xr, wr, br)
    got = torch.autograd.grad(zr, [xr, wr] + ([br] if has_bias else []), dzs[0].double())
    dxr, dwr, dbr = got[0], got[1], (got[2] if has_bias else None)
    conv = nn.Conv2d(Cin, N, 1, bias=has_bias)
    with torch.no_grad():
        conv.weight.copy_(w)
        if has_bias:
            conv.bias.copy_(bias)
    conv = conv.to(cuda)
    assert clshead.install_cls_head(nn.Sequential(conv), wide=True) == 1
    assert type(conv) is (clshead.ClsHeadWideConv2d if kind == "wide" else clshead.ClsHeadConv2d)
    conv.weight.requires_grad_(state != "frozen_w")
    if state == "frozen_bias":
        conv.bias.requires_grad_(False)
    xd = x.to(cuda).bfloat16().contiguous(**CL).requires_grad_(state != "no_dx")
    dzd = [t.to(cuda).bfloat16().contiguous() for t in dzs]
    leaves = [xd] + list(conv.parameters())
    fwd, bwd = ("cls_head_wide_fwd", "cls_head_wide_bwd") if kind == "wide" else ("cls_head_fwd", "cls_head_bwd")
    kw = []
    kp = _kp()
    T.spy_kwargs(kp, bwd, kw)

    def step(dz):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            z = conv(xd)
        z.backward(dz)
        return z

    counts = {}
    with counted(kp, counts):
        z = step(dzd[0])
    torch.cuda.synchronize()
    assert counts.get(fwd) == 1 and counts.get(bwd) == 1, counts
    assert len(kw) == 1 and kw[0]["need_dx"] == (state != "no_dx"), kw            # the need_dx arm of the kernel
    assert z.is_contiguous() and z.dtype == torch.bfloat16
    T.conv_check(z.detach(), zr.detach(), "z")
    if state == "no_dx":
        assert xd.grad is None
    else:
        T.conv_check(xd.grad, dxr, "dx")
    if state == "frozen_w":
        assert conv.weight.grad is None
    else:
        err = (conv.weight.grad.double().cpu() - dwr).abs().max().item()
        assert err <= 1e-4 * dwr.abs().max().item() + 1e-6, err
    if has_bias and state != "frozen_bias":
        err = (conv.bias.grad.double().cpu() - dbr).abs().max().item()
        assert err <= 1e-4 * dbr.abs().max().item() + 1e-6, err
    elif has_bias:
        assert conv.bias.grad is None
    if state == "accumulate":
        T.check_accumulate(step, leaves, dzd[0], dzd[1], T.grads_of(leaves))


# ---- PooledConv2d and pooled_layer (_PooledConvFn, _PooledLayerFn) -----------------------------------------------------------
@pytest.mark.parametrize("state", ["bn_eval", "frozen_affine", "no_dx"])
@pytest.mark.parametrize("fused", [True, False])
def test_pooled_layer(cuda, monkeypatch, fused, state):
    """ConvBnRelu on a pooled [4, 128, 1, 1] map: one launch per direction (pooled_layer), or PooledConv2d -> SyncBatchNorm.
    Bounds: tests/test_vecconv_gpu.py:150 (y: 2^-7 of max(1, |y|)) and :152-156 (every gradient: relative L2 2e-2)."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "torchseg_amd", "furnace"))
    from seg_opr.seg_oprs import ConvBnRelu
    from torchseg_amd import vecconv
    from torchseg_amd.syncbn import SyncBatchNorm
    monkeypatch.setattr(vecconv, "POOLED_LAYER", fused)
    monkeypatch.setattr(vecconv, "ENABLED", True)
    B, C = 4, 128
    g = torch.Generator().manual_seed(17)
    x = bf16r(torch.randn(B, C, 1, 1, generator=g) * 2)
    w = bf16r(torch.randn(C, C, 1, 1, generator=g) * (2.0 / C) ** 0.5)
    dy = bf16r(torch.randn(B, C, 1, 1, generator=g))
    nums = _bn_numbers(C, g)
    bn_training = state != "bn_eval"
    ref = _bn_ref(C, *nums, bn_training)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = torch.relu(ref(F.conv2d(xr, wr)))
    dxr, dwr, dgr, dbr = torch.autograd.grad(yr, [xr, wr, ref.weight, ref.bias], dy.double())

    seq = nn.Sequential(nn.AdaptiveAvgPool2d(1), ConvBnRelu(C, C, 1, 1, 0, has_bn=True, norm_layer=SyncBatchNorm, has_relu=True,
                                                            has_bias=False)).to(cuda)
    assert vecconv.install_pooled_conv(seq) == 1
    m = seq[1]
    with torch.no_grad():
        m.conv.weight.copy_(w)
        for t, v in zip((m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var), nums):
            t.copy_(v)
    m.bn.eps = ref.eps
    seq.train()
    m.bn.train(bn_training)                                # bn_eval: only the BatchNorm is frozen
    if state == "frozen_affine":
        m.bn.weight.requires_grad_(False); m.bn.bias.requires_grad_(False)
    xd = x.to(cuda).bfloat16().requires_grad_(state != "no_dx")
    before = _stats(m.bn)
    kp = _kp()
    bwd = "conv1x1_vec_bnact_bwd" if fused else "conv1x1_vec_bwd"
    kw = []
    T.spy_kwargs(kp, bwd, kw)
    counts = {}
    with counted(kp, counts):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(xd)
        y.backward(dy.to(cuda).bfloat16())
    torch.cuda.synchronize()
    if fused:
        assert counts.get("conv1x1_vec_bnact_fwd") == 1 and counts.get(bwd) == 1, counts
        for name in ("conv1x1_vec_fwd", "bn_apply_fwd", "bn_stats", "bn_finalize", "bn_affine"):
            assert name not in counts, (name, counts)
    else:
        for name in ("conv1x1_vec_fwd", bwd, "bn_apply_fwd", "bn_bwd_reduce", "bn_bwd_coeffs", "bn_bwd_apply"):
            assert counts.get(name) == 1, (name, counts)
        assert "conv1x1_vec_bnact_fwd" not in counts, counts
        if bn_training:
            assert counts.get("bn_stats") == 1 and counts.get("bn_finalize") == 1 and "bn_affine" not in counts, counts
        else:
            _assert_eval_bn_calls(counts)
    assert len(kw) == 1 and kw[0].get("need_dx", True) == (state != "no_dx"), kw
    if not bn_training:
        _assert_stats_unchanged(m.bn, before)
    else:
        assert int(m.bn.num_batches_tracked) == 1
        torch.testing.assert_close(m.bn.running_mean.double().cpu(), ref.running_mean, rtol=2e-2, atol=2e-2)
    err = (y.detach().double().cpu() - yr.detach()).abs().max().item()
    assert err <= 2.0 ** -7 * max(1.0, yr.abs().max().item()), err
    checks = [("dw", m.conv.weight.grad, dwr)]
    if state != "no_dx":
        checks.append(("dx", xd.grad, dxr))
    else:
        assert xd.grad is None
    if state != "frozen_affine":
        checks += [("dgamma", m.bn.weight.grad, dgr), ("dbeta", m.bn.bias.grad, dbr)]
    else:
        assert m.bn.weight.grad is None and m.bn.bias.grad is None
    for name, got, want in checks:
        rel = _rel_l2(got, want)
        assert rel < 2e-2, (name, rel)


# ---- StemConv2d / DeepStemConv2d (_StemConvFn, _DeepStemConvFn) ------------------------------------------------------------
@pytest.mark.parametrize("state", ["accumulate", "retain", "eval"])
@pytest.mark.parametrize("deep", [False, True])
def test_stem_convs(cuda, monkeypatch, deep, state):
    """Image (2, 3, 22, 130).  Bounds: tests/test_stemconv_gpu.py:32-39 and tests/test_deepstem_gpu.py:47-52 (y: the _check
    form; dw: relative L2 1e-4)."""
    from torchseg_amd import stemconv
    from torchseg_amd.stemconv import take_bn_partial
    monkeypatch.setattr(stemconv, "_STEM_STATS", True)
    k, pad, scale = (3, 1, 0.2) if deep else (7, 3, 0.1)
    g = torch.Generator().manual_seed(152 + k)
    img = bf16r(torch.randn(2, 3, 22, 130, generator=g))
    w = bf16r(torch.randn(64, 3, k, k, generator=g) * scale)
    wr = w.double().requires_grad_(True)
    yr = F.conv2d(img.double(), wr, None, 2, pad)
    dys = [bf16r(torch.randn(yr.shape, generator=g)) for _ in range(2)]
    (dwr,) = torch.autograd.grad(yr, [wr], dys[0].double())
    conv = nn.Conv2d(3, 64, k, 2, pad, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    conv = conv.to(cuda)
    assert (stemconv.install_deep_stem_conv if deep else stemconv.install_stem_conv)(conv) == 1
    conv.train(state != "eval")
    imgd = img.to(cuda).bfloat16()
    dyd = [t.to(cuda).bfloat16().contiguous(**CL) for t in dys]
    leaves = [conv.weight]

    def step(dy):
        conv(imgd).backward(dy)

    counts = {}
    with counted(_kp(), counts):
        y = conv(imgd)
        part = take_bn_partial(y)
        y.backward(dyd[0], retain_graph=state == "retain")
    torch.cuda.synchronize()
    if deep:
        assert counts.get("stem3_conv_fwd") == 1 and counts.get("stem3_conv_wrw") == 1 and part is None, counts
    elif state == "eval":
        assert counts.get("stem_conv_fwd") == 1 and "stem_conv_fwd_stats" not in counts and part is None, counts
        assert counts.get("stem_conv_wrw") == 1, counts
    else:
        assert counts.get("stem_conv_fwd_stats") == 1 and "stem_conv_fwd" not in counts and part is not None, counts
        assert counts.get("stem_conv_wrw") == 1, counts
    T.conv_check(y.detach(), yr.detach(), "y")
    rel = _rel_l2(conv.weight.grad, dwr)
    assert rel <= 1e-4, rel
    if state == "retain":
        T.check_retain(y, dyd[0], leaves, T.grads_of(leaves))
    if state == "accumulate":
        T.check_accumulate(step, leaves, dyd[0], dyd[1], T.grads_of(leaves))


# ---- gated_scale (_GapLinkedFn, _ChanScaleLinkedFn, _GateLink.pending) -------------------------------------------------------
class _Affine(nn.Module):
    """element-wise branch body, as in tests/test_pool_gpu.py:174-181 (no vendor kernel between the pool and the gate)"""

    def __init__(self, C, g):
        super().__init__()
        self.w = nn.Parameter(torch.randn(1, C, 1, 1, generator=g) * 0.5 + 1.0)
        self.b = nn.Parameter(torch.randn(1, C, 1, 1, generator=g) * 0.3)

    def forward(self, v):
        return v * self.w + self.b


@pytest.mark.parametrize("state", ["no_dx", "frozen_branch", "retain", "accumulate"])
@pytest.mark.parametrize("ident", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 64, 33, 47), (1, 8, 5, 7)])
def test_gated_scale(cuda, monkeypatch, shape, dtype, ident, state):
    """`x * branch(x)` (+ x) against the same statement in float64.  Bounds: tests/test_pool_gpu.py:50-57 (test_channel_scale:
    y and dx 1e-5 / 1e-6 in fp32, 1e-2 in bf16; sums over the plane 1e-4 sqrt(n) in fp32, 2e-2 sqrt(n) in bf16)."""
    from torchseg_amd import pool
    monkeypatch.setattr(pool, "_GATE_SPLIT", True)
    N, C, H, W = shape
    n = H * W
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).to(dtype)
    dys = [torch.randn(shape, generator=g).to(dtype) for _ in range(2)]
    body = _Affine(C, g)
    ref_body = _Affine(C, g).double()
    with torch.no_grad():
        body.w.copy_(body.w.to(dtype)); body.b.copy_(body.b.to(dtype))
        ref_body.w.copy_(body.w.double()); ref_body.b.copy_(body.b.double())
    xr = x.double().requires_grad_(True)
    sr = torch.sigmoid(ref_body(xr.mean((2, 3), keepdim=True)))
    yr = xr * sr + xr if ident else xr * sr
    dxr, dwr, dbr = torch.autograd.grad(yr, [xr, ref_body.w, ref_body.b], dys[0].double())

    branch = nn.Sequential(pool.GlobalAvgPool(1), body, nn.Sigmoid()).to(cuda).to(dtype)
    if state == "frozen_branch":
        for p in branch.parameters():
            p.requires_grad_(False)
    xd = x.to(cuda).contiguous(**CL).requires_grad_(state != "no_dx")
    dyd = [t.to(cuda).contiguous(**CL) for t in dys]
    leaves = [xd] + list(branch.parameters())

    def step(dy):
        y = pool.gated_scale(xd, branch, add_identity=ident)
        y.backward(dy)
        return y

    counts = {}
    with counted(_kp(), counts):
        y = pool.gated_scale(xd, branch, add_identity=ident)
        y.backward(dyd[0], retain_graph=state == "retain")
    torch.cuda.synchronize()
    assert counts.get("chanscale_fwd") == 1, counts
    if state == "no_dx":
        # the routing falls back to channel_scale: the plain gate's backward, nothing left with the pool node
        assert counts.get("chanscale_bwd") == 1 and "chanscale_bwd_ds" not in counts and "chanscale_bwd_dx" not in counts, counts
        assert xd.grad is None and not hasattr(y.grad_fn, "link")
    else:
        assert counts.get("chanscale_bwd_ds") == 1 and counts.get("chanscale_bwd_dx") == 1 and "chanscale_bwd" not in counts, counts
        assert y.grad_fn.link.pending is None              # taken by the pool node
    tol = dict(rtol=1e-5, atol=1e-6) if dtype == torch.float32 else dict(rtol=1e-2, atol=1e-2)
    ptol = dict(rtol=1e-4, atol=1e-4 * n ** 0.5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2 * n ** 0.5)
    torch.testing.assert_close(y.detach().double().cpu(), yr.detach(), **tol)
    if state != "no_dx":
        torch.testing.assert_close(xd.grad.double().cpu(), dxr, **tol)
    if state == "frozen_branch":
        assert all(p.grad is None for p in branch.parameters())
    else:
        torch.testing.assert_close(body.w.grad.double().cpu(), dwr, **ptol)
        torch.testing.assert_close(body.b.grad.double().cpu(), dbr, **ptol)
    if state == "retain":
        T.check_retain(y, dyd[0], leaves, T.grads_of(leaves))
        assert y.grad_fn.link.pending is None
    if state == "accumulate":
        T.check_accumulate(step, leaves, dyd[0], dyd[1], T.grads_of(leaves))


# ---- upsample_presum (_PresumUpFn) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("without", [0, 1])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_upsample_presum_with_one_addend_without_a_gradient(cuda, dtype, channels_last, without):
    """(1, 16, 5, 7) -> (13, 9).  Reference: F.interpolate of the stored sum round_T(a + b) in float64.  Bounds:
    tests/test_upsample_gpu.py:189-194."""
    from torchseg_amd.fusion import upsample_presum
    n, c, ih, iw, oh, ow = 1, 16, 5, 7, 13, 9
    g = torch.Generator().manual_seed(ih * ow)
    a = torch.randn(n, c, ih, iw, generator=g).to(dtype)
    b = torch.randn(n, c, ih, iw, generator=g).to(dtype)
    dy = torch.randn(n, c, oh, ow, generator=g).to(dtype)
    sr = (a.float() + b.float()).to(dtype).double().requires_grad_(True)          # what the eager in-place add stores
    yr = F.interpolate(sr, size=(oh, ow), mode="bilinear", align_corners=True)
    (dr,) = torch.autograd.grad(yr, [sr], dy.double())
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    ops = [t.to(cuda).contiguous(memory_format=fmt).requires_grad_(i != without) for i, t in enumerate((a, b))]
    counts = {}
    with counted(_kp(), counts):
        y = upsample_presum(ops[0], ops[1], size=(oh, ow))
        y.backward(dy.to(cuda).contiguous(memory_format=fmt))
    torch.cuda.synchronize()
    assert counts.get("upsample_presum_fwd") == 1, counts
    assert counts.get("upsample_bwd", 0) + counts.get("upsample_bwd_nhwc", 0) == 1, counts
    assert ops[without].grad is None
    got = ops[1 - without].grad
    if dtype == torch.float32:
        np.testing.assert_allclose(y.detach().cpu().numpy(), yr.detach().numpy(), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(got.cpu().numpy(), dr.numpy(), rtol=1e-4, atol=1e-4 * max(1.0, oh / ih))
    else:
        np.testing.assert_allclose(y.detach().float().cpu().numpy(), yr.detach().numpy(), rtol=8e-3, atol=8e-3)
        np.testing.assert_allclose(got.float().cpu().numpy(), dr.numpy(), rtol=1e-2, atol=1e-2 * dr.abs().max().item())
