"""GPU: torchseg_amd.infer.prepare_inference, the Evaluator's TSG_INFER=1 path and compute_speed on a prepared network."""
import copy
import logging
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_process_globals(monkeypatch):
    """prepare_inference / compute_speed set process-wide switches (channels_last BatchNorm output, the library's
    autotuned convolution selection); later test modules must not inherit them."""
    from torchseg_amd import syncbn
    monkeypatch.setattr(syncbn, "PREFER_CHANNELS_LAST_OUTPUT", syncbn.PREFER_CHANNELS_LAST_OUTPUT)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", torch.backends.cudnn.benchmark)


def _r18(seed=0):
    from torchseg_amd.workloads.bisenet import BiSeNet
    torch.manual_seed(seed)
    net = BiSeNet(19, False, None, None, nn.BatchNorm2d)
    # non-trivial running statistics, so that eval-mode BatchNorm is not the identity
    g = torch.Generator().manual_seed(seed + 1)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(0.1 * torch.randn(m.num_features, generator=g))
            m.running_var.copy_(1.0 + 0.2 * torch.rand(m.num_features, generator=g))
    return net.eval()


def _x39(seed=0):
    from torchseg_amd.workloads.bisenet_x39 import BiSeNetX39
    torch.manual_seed(seed)
    return BiSeNetX39(19, False, None, None, pretrained_model=None, norm_layer=nn.BatchNorm2d).eval()


@pytest.mark.parametrize("build", [_r18, _x39])
def test_prepared_fp32_matches_stock_fp32(cuda, build):
    """fp32 parity mode: the prepared network's log-probabilities within 1e-4 of the stock fp32 network's."""
    from torchseg_amd.fusion import DeferredLogSoftmax, materialize
    from torchseg_amd.infer import prepare_inference
    net = build().to(cuda)
    stock = copy.deepcopy(net)
    x = torch.randn(2, 3, 256, 512, device=cuda)
    with torch.no_grad():
        ref = stock(x)
    prep = prepare_inference(net, dtype=torch.float32)
    out = prep(x)
    assert isinstance(out, DeferredLogSoftmax) and out.tail          # the head's tail stays pending
    got = materialize(out)
    torch.cuda.synchronize()
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = (got - ref).abs().max().item()
    print("prepared fp32 vs stock fp32: max |d log p| = %.3e" % err)
    assert err <= 1e-4, err


def test_prepared_bf16_close_to_float64(cuda):
    """bf16: the prepared R18 is no further from the float64 network than CPU bf16 autocast x 1.5."""
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    net = _r18()
    x = torch.randn(1, 3, 128, 256)
    with torch.no_grad():
        truth = copy.deepcopy(net).double()(x.double())
        with torch.autocast("cpu", dtype=torch.bfloat16):
            cpu_bf16 = copy.deepcopy(net)(x).float()
    prep = prepare_inference(net.to(cuda), dtype=torch.bfloat16)
    got = materialize(prep(x.to(cuda))).double().cpu()
    d_ours = (got - truth).abs().max().item()
    d_cpu = (cpu_bf16.double() - truth).abs().max().item()
    print("bf16 vs float64: prepared %.3e, CPU bf16 autocast %.3e" % (d_ours, d_cpu))
    assert d_ours <= 1.5 * d_cpu, (d_ours, d_cpu)


def test_graph_replay_equals_eager(cuda):
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    net = _r18().to(cuda)
    eager = prepare_inference(copy.deepcopy(net), dtype=torch.float32)
    graph = prepare_inference(net, dtype=torch.float32, graph=True)
    for seed in (1, 2):
        x = torch.randn(1, 3, 128, 256, generator=torch.Generator().manual_seed(seed)).to(cuda)
        a = materialize(eager(x)).clone()
        b = graph(x).clone()
        torch.cuda.synchronize()
        assert torch.equal(a, b)


MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


@pytest.mark.parametrize("scales,flip", [([1.0], False), ([0.75, 1.0, 1.25], True)])
def test_evaluator_tsg_infer_matches_default(cuda, monkeypatch, scales, flip):
    """TSG_INFER=1 (fp32 parity mode) against the default path (the stock fp32 network): sliding_scores within 1e-5
    relative, class maps equal except where the default's top-2 margin is below that tolerance."""
    from engine.evaluator import Evaluator
    net = _r18()
    g = np.random.RandomState(0)
    img = g.randint(0, 256, (300, 500, 3)).astype(np.uint8)
    crop = 256
    monkeypatch.setenv("TSG_DTYPE", "fp32")
    monkeypatch.delenv("TSG_INFER", raising=False)
    ev = Evaluator(None, 19, MEAN, STD, copy.deepcopy(net), scales, flip, [0])
    ev.val_func = ev.network
    ref = ev.sliding_scores(img, crop, 2 / 3, device=0)
    monkeypatch.setenv("TSG_INFER", "1")
    ev2 = Evaluator(None, 19, MEAN, STD, copy.deepcopy(net), scales, flip, [0])
    ev2.val_func = ev2.network
    got = ev2.sliding_scores(img, crop, 2 / 3, device=0)
    torch.cuda.synchronize()
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    print("TSG_INFER=1 vs default: max relative %.3e" % rel)
    assert rel <= 1e-5, rel
    top2 = ref.topk(2, dim=0).values
    margin = (top2[0] - top2[1]) / ref.abs().max()
    differ = got.argmax(0) != ref.argmax(0)
    assert not (differ & (margin > 1e-5)).any()


def test_compute_speed_on_prepared_r18(cuda, monkeypatch, caplog):
    from tools.benchmark import compute_speed
    caplog.set_level(logging.INFO)
    for graph in ("0", "1"):
        monkeypatch.setenv("TSG_INFER", "1")
        monkeypatch.setenv("TSG_INFER_GRAPH", graph)
        caplog.clear()
        per_iter = compute_speed(_r18(), (1, 3, 256, 512), 0, 5)
        assert per_iter > 0
        assert "FPS:" in caplog.text and "prepared for inference (graph=%s)" % (graph == "1") in caplog.text
