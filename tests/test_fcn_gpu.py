"""GPU: FCN-32s (torchseg_amd.workloads.fcn; the reference is not read here).

- The fused head at x32 and x16 with 21 classes (the two heads of FCN into nn.CrossEntropyLoss(ignore_index=255)):
  loss and gradient w.r.t. the low-resolution logits against a float64 oracle (tests/_fcn.py).
- A bf16 FCN step behind the DDP wrapper against the same network on the CPU in fp32, with the gradient bar of
  test_families_gpu.py: our distance from the CPU at most 2x that of stock torch on the same device (here under the same
  bf16 autocast) + 1e-3, over the heads' gradients and over all gradients.  The loss is held to 1e-2 relative, the bf16
  bar of test_stemconv_gpu.py (the families' 1e-4 is an fp32 bar).
- The fp32 parity mode's logits against float64.
- sliding_eval: equal class maps with TSG_INFER=0 and TSG_INFER=1 (FCN returns raw logits: exp(logits) is the score).
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _fcn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

pytestmark = pytest.mark.gpu

NCLS = 21


@pytest.fixture(autouse=True)
def _restore_process_globals(monkeypatch):
    """the DDP wrapper / prepare_inference switch process-wide settings: give them back to later test files"""
    from torchseg_amd import syncbn
    monkeypatch.setattr(syncbn, "PREFER_CHANNELS_LAST_OUTPUT", syncbn.PREFER_CHANNELS_LAST_OUTPUT)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", torch.backends.cudnn.benchmark)


def _counting(monkeypatch, names):
    from torchseg_amd import kernels as K
    kp = K.provider()
    calls = dict.fromkeys(names, 0)
    for name in names:
        orig = getattr(kp, name)

        def f(*a, _n=name, _o=orig, **k):
            calls[_n] += 1
            return _o(*a, **k)
        monkeypatch.setattr(kp, name, f)
    return calls


def _head_case(B, IH, IW, scale, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    OH, OW = IH * scale, IW * scale
    z = (2.0 * torch.randn(B, NCLS, IH, IW, generator=g)).to(dtype)
    t = torch.randint(0, NCLS, (B, OH, OW), generator=g)
    t[:, : OH // 16] = 255
    t[torch.rand(t.shape, generator=g) < 0.05] = 255
    return z, t, (OH, OW)


@pytest.mark.parametrize("scale,IH,IW", [(32, 16, 16), (16, 32, 32), (32, 4, 4), (16, 8, 8), (32, 5, 7), (16, 9, 6)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fused_head_vs_float64(cuda, monkeypatch, scale, IH, IW, dtype):
    from torchseg_amd.losses import cross_entropy_2d
    from torchseg_amd.upsample import DeferredUpsample
    calls = _counting(monkeypatch, ["ohem_up_fwd", "ohem_up_bwd"])
    z, t, size = _head_case(2, IH, IW, scale, seed=scale * 100 + IH, dtype=dtype)
    want, dz_want = _fcn.ce_upsample_ref64(z, t, size)              # z is already bf16-rounded in the bf16 case
    zd = z.to(cuda).requires_grad_(True)
    loss = cross_entropy_2d(DeferredUpsample(zd, size), t.to(cuda), ignore_index=255)
    loss.backward()
    torch.cuda.synchronize()
    assert calls["ohem_up_fwd"] == 1 and calls["ohem_up_bwd"] == 1, calls      # the fused kernels, not a materialised map
    assert abs(loss.item() - want.item()) <= 1e-5 * max(1.0, abs(want.item())), (loss.item(), want.item())
    assert zd.grad.dtype == dtype
    gscale = dz_want.abs().max().item()
    err = (zd.grad.double().cpu() - dz_want).abs()
    bound = 2e-4 * gscale if dtype == torch.float32 else 2.0 ** -8 * dz_want.abs() + 2e-4 * gscale
    assert bool((err <= bound).all()), (err.max().item(), gscale)


def _fcn_pair(cuda, compute_dtype, seed=304, classifier_scale=1.0):
    """(CPU fp32 oracle with nn.BatchNorm2d, ours behind the DDP wrapper, stock copy on the GPU), Dropout2d at p = 0
    (the CPU and GPU RNG streams differ).  `classifier_scale` multiplies the two 1x1 classifiers' weights."""
    from torchseg_amd.ddp import DistributedDataParallel
    from torchseg_amd.syncbn import SyncBatchNorm
    from torchseg_amd.workloads.fcn import FCN
    from utils.init_func import init_weight
    crit = nn.CrossEntropyLoss(reduction='mean', ignore_index=255)
    torch.manual_seed(seed)
    ref = FCN(NCLS, crit, norm_layer=nn.BatchNorm2d)
    init_weight(ref.business_layer, nn.init.kaiming_normal_, nn.BatchNorm2d, 1e-5, 0.1, mode='fan_out',
                nonlinearity='relu')
    for m in ref.modules():
        if isinstance(m, nn.Dropout2d):
            m.p = 0.0
    with torch.no_grad():
        ref.head.conv1x1.weight.mul_(classifier_scale)
        ref.aux_head.conv1x1.weight.mul_(classifier_scale)
    net = FCN(NCLS, nn.CrossEntropyLoss(reduction='mean', ignore_index=255), norm_layer=SyncBatchNorm)
    net.load_state_dict(ref.state_dict())
    for m in net.modules():
        if isinstance(m, nn.Dropout2d):
            m.p = 0.0
    stock = copy.deepcopy(ref).to(cuda)
    net = DistributedDataParallel(net.to(cuda), compute_dtype=compute_dtype)
    return ref, net, stock


def _batch(B, S, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, S, S, generator=g)
    y = torch.randint(0, NCLS, (B, S, S), generator=g)
    y[:, : S // 16] = 255
    return x, y


def _rel(model, ref, keep):
    num = den = 0.0
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n
        if q.grad is None or not keep(n):
            continue
        d = p.grad.detach().cpu().double() - q.grad.double()
        num += float((d * d).sum())
        den += float((q.grad.double() ** 2).sum())
    return (num / den) ** 0.5


def test_bf16_step_against_cpu_fp32(cuda, monkeypatch):
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    calls = _counting(monkeypatch, ["ohem_up_fwd", "ohem_up_bwd"])
    # classifiers at 1/10 of train.py's kaiming init: with it as drawn the seeded network's logits are so large (loss 10.5
    # for 21 classes) that bf16 rounding alone moves every gradient by more than its own norm (rel-L2 1.4 for stock
    # torch as well as for ours), and nothing is checked
    ref, net, stock = _fcn_pair(cuda, torch.bfloat16, classifier_scale=0.1)
    x, y = _batch(2, 256)
    loss_ref = ref(x, y)
    loss_ref.backward()
    loss = net(x.to(cuda), y.to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    assert calls["ohem_up_fwd"] == 2 and calls["ohem_up_bwd"] == 2, calls     # both heads on the fused kernels
    from torchseg_amd import workloads
    monkeypatch.setattr(workloads, "NATIVE_FUSIONS", False)                  # stock: the literal statements
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss_stock = stock(x.to(cuda), y.to(cuda))
    loss_stock.backward()
    torch.cuda.synchronize()
    assert calls["ohem_up_fwd"] == 2, calls
    is_head = lambda n: not n.startswith("backbone.")
    ours_head, ours_all = _rel(net.module, ref, is_head), _rel(net.module, ref, lambda n: True)
    stock_head, stock_all = _rel(stock, ref, is_head), _rel(stock, ref, lambda n: True)
    d_ours, d_stock = abs(loss.item() - loss_ref.item()), abs(loss_stock.item() - loss_ref.item())
    print("FCN bf16: loss %.6f (cpu fp32 %.6f, stock bf16 %.6f)  grad rel-L2 vs cpu: heads %.2e (stock %.2e), "
          "all %.2e (stock %.2e)" % (loss.item(), loss_ref.item(), loss_stock.item(), ours_head, stock_head, ours_all,
                                     stock_all))
    assert d_ours <= 1e-2 * abs(loss_ref.item()), (d_ours, d_stock)          # bf16: the bar of test_stemconv_gpu.py
    assert ours_head <= 2.0 * stock_head + 1e-3, (ours_head, stock_head)
    assert ours_all <= 2.0 * stock_all + 1e-3, (ours_all, stock_all)


def test_fp32_logits_against_float64(cuda):
    ref, net, _ = _fcn_pair(cuda, torch.float32)
    ref64 = copy.deepcopy(ref).double().eval()
    net.eval()
    x, _ = _batch(1, 128)
    with torch.no_grad():
        want = ref64(x.double())
        got = net(x.to(cuda))
        from torchseg_amd.fusion import materialize
        got = materialize(got)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (1, NCLS, 128, 128)
    err = (got.double().cpu() - want).abs().max().item()
    print("FCN fp32 logits: max |logit - float64| %.2e (scale %.2f)" % (err, want.abs().max().item()))
    assert err <= 1e-4 * max(1.0, want.abs().max().item()), err


MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.224])


def _eval_fcn(cuda):
    """An eval-mode FCN whose logits are O(1) (the classifier scaled on a probe batch) so that exp() stays finite."""
    from torchseg_amd.workloads.fcn import FCN
    torch.manual_seed(3)
    net = FCN(NCLS, None, norm_layer=nn.BatchNorm2d)
    g = torch.Generator().manual_seed(4)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(0.1 * torch.randn(m.num_features, generator=g))
            m.running_var.copy_(1.0 + 0.2 * torch.rand(m.num_features, generator=g))
    net = net.eval().to(cuda)
    with torch.no_grad():
        m = net(torch.randn(1, 3, 256, 256, generator=g).to(cuda)).abs().max().item()
        net.head.conv1x1.weight.mul_(4.0 / m)
        net.head.conv1x1.bias.mul_(4.0 / m)
    return net.cpu()


@pytest.mark.parametrize("scales,flip", [([1.0], False), ([0.75, 1.0], True)])
def test_sliding_eval_same_classes_with_and_without_tsg_infer(cuda, monkeypatch, scales, flip):
    from engine.evaluator import Evaluator
    net = _eval_fcn(cuda)
    img = np.random.RandomState(0).randint(0, 256, (300, 420, 3)).astype(np.uint8)
    crop = 256
    monkeypatch.setenv("TSG_DTYPE", "fp32")
    out = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("TSG_INFER", flag)
        ev = Evaluator(None, NCLS, MEAN, STD, copy.deepcopy(net), scales, flip, [0])
        ev.val_func = ev.network
        out[flag] = (ev.sliding_scores(img, crop, 2 / 3, device=0), ev.sliding_eval(img, crop, 2 / 3, device=0))
    torch.cuda.synchronize()
    ref, got = out["0"][0], out["1"][0]
    assert torch.isfinite(ref).all() and torch.isfinite(got).all()
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    print("FCN sliding scores, TSG_INFER=1 vs 0: max relative %.3e" % rel)
    assert rel <= 1e-4, rel
    top2 = ref.topk(2, dim=0).values
    margin = ((top2[0] - top2[1]) / ref.abs().max()).cpu().numpy()
    p0, p1 = np.asarray(out["0"][1]), np.asarray(out["1"][1])
    assert p0.shape == p1.shape == img.shape[:2]
    assert not ((p0 != p1) & (margin > 1e-4)).any()
    assert (p0 == p1).mean() >= 0.999
