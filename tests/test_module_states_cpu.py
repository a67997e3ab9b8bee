"""CPU twin of tests/test_module_states_gpu.py: the HOST logic of the autograd nodes in the states the parity tests leave
out (eval-mode statistics in a backward pass, frozen affine parameters, affine=False, track_running_stats=False, an input
without a gradient, accumulation, a retained graph), with tests/_cpu_provider.OracleProvider in the kernels' place and
nn.BatchNorm2d in float64 as the reference; and the routing decisions that need no kernel at all."""
import pytest
import torch
import torch.nn as nn

from _states import BN_STATES, BnCase


class _OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda like a HIP tensor: the routing conditions are then decided by everything else."""
    is_cuda = property(lambda self: True)


class _Provider:
    """OracleProvider plus the capability questions the routing asks before it picks a fused node."""

    def __new__(cls):
        from _cpu_provider import OracleProvider

        class P(OracleProvider):
            def stem_conv_supported(self, *a):
                return True

            def chanscale_split_supported(self, *a):
                return True

            def chanscale_bwd_ds(self, *a):
                raise AssertionError("no kernel may run in a routing test")
        return P()


@pytest.fixture()
def standin():
    from torchseg_amd import kernels as K
    prov = _Provider()
    old = K._set_provider_for_tests(prov)
    yield prov
    K._set_provider_for_tests(old)


# ---- SyncBatchNorm: the matrix of the GPU file, fp32 -----------------------------------------------------------------
@pytest.mark.parametrize("state", ("train",) + BN_STATES)
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("shape,layout", [((2, 19, 7, 5), "nchw"), ((2, 19, 7, 5), "nhwc"), ((3, 24, 8, 8), "nhwc"),
                                          ((2, 64, 33, 47), "nhwc")])
def test_syncbn_states_behind_the_stand_in_provider(standin, shape, layout, relu, res, state):
    """Every output, input gradient, parameter gradient and running statistic within 1e-5 of nn.BatchNorm2d in float64.
    (Flip use_batch_stats to True in the last line of syncbn._backward_pack and the eval cases fail on dx.)"""
    case = BnCase(torch.device("cpu"), shape, layout, torch.float32, relu, res, state)
    case.run(standin, fp32_tol=1e-5)


# ---- routing decisions that need no kernel ---------------------------------------------------------------------------
def _pair(frozen_w):
    from torchseg_amd.convwrw import install_conv_wrw
    from torchseg_amd.syncbn import SyncBatchNorm
    bn, relu, conv = SyncBatchNorm(64), nn.ReLU(), nn.Conv2d(64, 64, 3, 1, 1, bias=False)
    assert install_conv_wrw(conv) == 1
    conv.weight.requires_grad_(not frozen_w)
    x = torch.randn(2, 64, 6, 8).bfloat16().contiguous(memory_format=torch.channels_last).as_subclass(_OnDevice)
    return bn, relu, conv, x.requires_grad_(True)


@pytest.mark.parametrize("frozen_w", [False, True])
def test_bn_relu_conv_runs_the_three_modules_for_a_frozen_convolution_weight(standin, monkeypatch, frozen_w):
    from torchseg_amd import convwrw
    bn, relu, conv, x = _pair(frozen_w)
    asked, fused = [], torch.zeros(1)
    monkeypatch.setattr(convwrw, "_route", lambda c, xb, general=True: (asked.append(c), convwrw.Route(
        "c64", False, True, False, True, False))[1])

    class Node:
        @staticmethod
        def apply(*a):
            return fused, torch.empty(0)
    monkeypatch.setattr(convwrw, "_BnReluConvFn", Node)
    conv.forward = lambda t: ("stock", t)                   # what the fallback ends in: conv(norm_act(bn, relu, x))
    out = convwrw.bn_relu_conv(bn, relu, x, conv)
    if not frozen_w:
        assert out is fused and asked == [conv]
        return
    assert asked == [] and isinstance(out, tuple) and out[0] == "stock"
    want = torch.relu(nn.functional.batch_norm(x.detach().as_subclass(torch.Tensor).double(), None, None, bn.weight.double(),
                                               bn.bias.double(), True, 0.1, bn.eps))
    assert out[1].dtype == torch.bfloat16
    torch.testing.assert_close(out[1].detach().as_subclass(torch.Tensor).double(), want, rtol=8e-3, atol=8e-3)


@pytest.mark.parametrize("frozen", [None, "conv", "stem"])
def test_stem_bn_relu_conv_declines_frozen_weights(standin, monkeypatch, frozen):
    from torchseg_amd import convwrw
    from torchseg_amd.stemconv import install_stem_conv
    bn, relu, conv, _ = _pair(frozen == "conv")
    stem = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    assert install_stem_conv(stem) == 1
    stem.weight.requires_grad_(frozen != "stem")
    img = torch.randn(2, 3, 16, 16).bfloat16().as_subclass(_OnDevice)
    asked, fused = [], torch.zeros(1)
    monkeypatch.setattr(convwrw, "_route", lambda c, xb, general=True: (asked.append(c), convwrw.Route(
        "c64", False, True, False, True, False))[1])

    class Node:
        @staticmethod
        def apply(*a):
            return fused, torch.empty(0)
    monkeypatch.setattr(convwrw, "_StemBnReluConvFn", Node)
    out = convwrw.stem_bn_relu_conv(stem, bn, relu, img, conv)
    if frozen is None:
        assert out is fused and asked == [conv]
    else:
        assert out is None and asked == []


class _Linked(Exception):
    pass


@pytest.mark.parametrize("add_identity", [False, True])
@pytest.mark.parametrize("needs_grad", [True, False])
def test_gated_scale_takes_the_plain_gate_for_an_input_without_a_gradient(standin, monkeypatch, needs_grad, add_identity):
    from torchseg_amd import pool

    class Gap(pool.GlobalAvgPool):
        def forward(self, x):
            return x.as_subclass(torch.Tensor).float().mean((2, 3), keepdim=True)

    class Node:
        @staticmethod
        def apply(*a):
            raise _Linked()
    monkeypatch.setattr(pool, "_GapLinkedFn", Node)
    monkeypatch.setattr(pool, "channel_scale", lambda x, s, add_identity=False: ("plain", x, s, add_identity))
    branch = nn.Sequential(Gap(1), nn.Sigmoid())
    x = torch.randn(2, 8, 5, 7).contiguous(memory_format=torch.channels_last).as_subclass(_OnDevice)
    x.requires_grad_(needs_grad)
    if needs_grad:
        with pytest.raises(_Linked):
            pool.gated_scale(x, branch, add_identity)
        return
    tag, x_, s, add = pool.gated_scale(x, branch, add_identity)
    assert tag == "plain" and x_ is x and add is add_identity
    torch.testing.assert_close(s, torch.sigmoid(x.detach().as_subclass(torch.Tensor).mean((2, 3), keepdim=True)))


@pytest.mark.parametrize("training", [False, True])
def test_eval_batchnorm_ignores_the_partial_of_a_train_mode_producer(standin, training):
    """Frozen-BN fine-tuning: the producer in train() attaches its statistics partial; a BatchNorm in eval() must leave it
    where it is and normalise with the running estimates.  (In train() the same partial IS what the layer normalises with:
    the control that the marker below would be seen.)"""
    from torchseg_amd import kernels as K
    from torchseg_amd.stemconv import attach_bn_partial, take_bn_partial
    from torchseg_amd.syncbn import SyncBatchNorm
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(3, 8, 5, 6, generator=g) * 1.5 + 0.4).requires_grad_(True)
    dy = torch.randn(3, 8, 5, 6, generator=g)
    bn = SyncBatchNorm(8)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(8, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(8, generator=g) + 0.5)
        bn.weight.copy_(torch.randn(8, generator=g) * 0.5 + 1.0)
    bn.train(training)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    # a partial that is NOT the statistics of x: sums of 2 x, so whoever reads it is found out
    wrong, _ = standin.bn_stats(2.0 * x.detach(), None, 3, 8, 30)
    attach_bn_partial(x, wrong)
    cnt = K.CallCounter(standin)
    try:
        y = bn(x)
        y.backward(dy)
    finally:
        counts = cnt.stop()
    if training:
        assert take_bn_partial(x) is wrong and "bn_stats" not in counts and counts.get("bn_finalize") == 1
        x2 = 2.0 * x.detach().double()                      # x normalised with the mean and variance of 2 x
        mean, var = x2.mean((0, 2, 3)), x2.var((0, 2, 3), unbiased=False)
        want = (x.detach().double() - mean.view(1, -1, 1, 1)) * (var.view(1, -1, 1, 1) + bn.eps).rsqrt() \
            * bn.weight.double().view(1, -1, 1, 1) + bn.bias.double().view(1, -1, 1, 1)
        torch.testing.assert_close(y.detach().double(), want, rtol=1e-5, atol=1e-5)
        return
    assert take_bn_partial(x) is wrong                      # untouched, still attached
    assert "bn_stats" not in counts and "bn_finalize" not in counts and counts.get("bn_affine") == 1, counts
    assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv) and int(bn.num_batches_tracked) == 0
    xr = x.detach().double().requires_grad_(True)
    yr = nn.functional.batch_norm(xr, rm.double(), rv.double(), bn.weight.double(), bn.bias.double(), False, 0.1, bn.eps)
    yr.backward(dy.double())
    torch.testing.assert_close(y.detach().double(), yr.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(x.grad.double(), xr.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(x.grad.double(), dy.double() * (bn.weight.double() * (rv.double() + bn.eps).rsqrt()).view(1, -1, 1, 1),
                               rtol=1e-5, atol=1e-5)


# ---- the deferred-launch list of the weight gradients (convwrw._DEFER) -------------------------------------------------------
class _Layer(torch.autograd.Function):
    """y = x; the "weight gradient" sum(dy) in every element, computed where wrw_on_side_stream puts it"""

    @staticmethod
    def forward(ctx, x, w):
        ctx.w = w
        return x.clone()

    @staticmethod
    def backward(ctx, dy):
        from torchseg_amd import convwrw
        w = ctx.w

        def launch(out=None):
            out = torch.empty_like(w, dtype=torch.float32) if out is None else out
            return out.fill_(float(dy.sum()))
        return dy, convwrw.wrw_on_side_stream(launch, w, dy, defer_out=(w.shape[0], w.shape[1])).to(w.dtype)


def _backward_with_open_list(monkeypatch, loss):
    """loss.backward() with convwrw._DEFER open; runs the list afterwards as its owner would.  -> how many were listed"""
    from torchseg_amd import convwrw
    monkeypatch.setattr(convwrw, "_DEFER", [])
    try:
        loss.backward()
        todo = list(convwrw._DEFER)
    finally:
        monkeypatch.setattr(convwrw, "_DEFER", None)
    for launch, _operands, _buf in todo:
        launch()
    return len(todo)


def _weight(dtype=torch.float32, channels_last=True):
    w = torch.zeros(4, 2, 3, 3, dtype=dtype)
    return nn.Parameter(w.contiguous(memory_format=torch.channels_last) if channels_last else w)


def test_weight_gradient_is_deferred_only_onto_an_empty_grad():
    """Accumulation: the pass onto no gradient lists its launch, the pass onto an existing one computes in place (AccumulateGrad
    adds what it is handed at once), and the parameter ends with g1 + g2 — also after zero_grad(set_to_none=False)."""
    mp = pytest.MonkeyPatch()
    try:
        w = _weight()
        x1, x2 = torch.full((3,), 1.0, requires_grad=True), torch.full((3,), 2.0, requires_grad=True)
        assert _backward_with_open_list(mp, (_Layer.apply(x1, w) * 1.0).sum()) == 1
        assert torch.equal(w.grad, torch.full_like(w, 3.0))
        assert _backward_with_open_list(mp, (_Layer.apply(x2, w) * 2.0).sum()) == 0
        assert torch.equal(w.grad, torch.full_like(w, 3.0 + 6.0))
        w.grad.zero_()
        assert _backward_with_open_list(mp, (_Layer.apply(x1, w) * 1.0).sum()) == 0
        assert torch.equal(w.grad, torch.full_like(w, 3.0))
    finally:
        mp.undo()


def test_parameter_used_twice_in_one_backward_pass_is_not_left_deferred():
    """Both uses see `grad is None`; the engine sums their results when the second arrives: the first, listed launch runs then
    and leaves the list, the second is computed in place."""
    mp = pytest.MonkeyPatch()
    try:
        w = _weight()
        x1, x2 = torch.full((3,), 1.0, requires_grad=True), torch.full((3,), 2.0, requires_grad=True)
        loss = _Layer.apply(x1, w).sum() + (_Layer.apply(x2, w) * 5.0).sum()
        assert _backward_with_open_list(mp, loss) == 0
        assert torch.equal(w.grad, torch.full_like(w, 3.0 + 15.0))
        w.grad = None                                      # the note of this pass is gone with it: the next pass defers again
        assert _backward_with_open_list(mp, _Layer.apply(x1, w).sum()) == 1
        assert torch.equal(w.grad, torch.full_like(w, 3.0))
    finally:
        mp.undo()


@pytest.mark.parametrize("why", ["bf16 parameter", "parameter not channels_last", "tensor hook", "post-accumulate hook"])
def test_weight_gradient_something_reads_at_once_is_not_deferred(why):
    mp = pytest.MonkeyPatch()
    try:
        w = _weight(torch.bfloat16 if why == "bf16 parameter" else torch.float32, why != "parameter not channels_last")
        seen = []
        if why == "tensor hook":
            w.register_hook(lambda g: seen.append(g.clone()) or g)
        if why == "post-accumulate hook":
            w.register_post_accumulate_grad_hook(lambda p: seen.append(p.grad.clone()))
        x = torch.full((3,), 1.0, requires_grad=True)
        assert _backward_with_open_list(mp, _Layer.apply(x, w).sum()) == 0
        assert torch.equal(w.grad.float(), torch.full((4, 2, 3, 3), 3.0))
        for g in seen:                                     # what the hook read was the finished gradient
            assert torch.equal(g.float(), torch.full((4, 2, 3, 3), 3.0))
    finally:
        mp.undo()
