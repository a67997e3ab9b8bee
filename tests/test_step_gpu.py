"""torchseg_amd.step.ReplayedStep on the GPU: warm-up -> capture -> replay must follow the eager trajectory.

The small network below is made of layers whose kernels are ours and reproducible (stem 7x7, 64-channel 3x3, SyncBatchNorm,
the 19-class 1x1 classifier, the bilinear x2 head, the OHEM criterion), so "follows" means bit-equal in every loss and every
parameter; test A first asserts that two EAGER runs are bit-equal, which is the precondition for asking it of the replay.
BiSeNet-R18 (test C) contains vendor-library convolutions that are not reproducible between two eager runs: there the
bound is the rtol = 2e-2 tests/test_graph_gpu.py holds bench.GraphedStep to (see the test's docstring)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BASE_LR, TOTAL = 1e-2, 40


class _SegNet(nn.Module):
    def __init__(self, dropout=False):
        super().__init__()
        from torchseg_amd.losses import ProbOhemCrossEntropy2d
        from torchseg_amd.syncbn import SyncBatchNorm
        self.stem = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn0 = SyncBatchNorm(64)
        self.c1 = nn.Conv2d(64, 64, 3, 1, 1, bias=False)
        self.bn1 = SyncBatchNorm(64)
        self.c2 = nn.Conv2d(64, 64, 3, 1, 1, bias=False)
        self.bn2 = SyncBatchNorm(64)
        self.drop = nn.Dropout2d(0.5) if dropout else None
        self.cls = nn.Conv2d(64, 19, 1)
        self.criterion = ProbOhemCrossEntropy2d(ignore_label=255, thresh=0.7, min_kept=2 * 64 * 64 // 16, use_weight=False)

    def forward(self, data, label):
        h = F.relu(self.bn0(self.stem(data)))
        h = F.relu(self.bn1(self.c1(h)))
        if self.drop is not None:
            h = self.drop(h)
        h = F.relu(self.bn2(self.c2(h)))
        z = F.interpolate(self.cls(h), scale_factor=2, mode="bilinear", align_corners=True)
        return self.criterion(z, label)


def _build(cuda, fused=True, dropout=False, lr=BASE_LR, wd=5e-4):
    from torchseg_amd.ddp import DistributedDataParallel
    from torchseg_amd.optim import FusedSGD
    torch.manual_seed(11)
    net = _SegNet(dropout).to(cuda)
    groups = [dict(params=list(net.stem.parameters()) + list(net.bn0.parameters()), lr=lr),
              dict(params=[p for m in (net.c1, net.bn1, net.c2, net.bn2) for p in m.parameters()], lr=lr),
              dict(params=list(net.cls.parameters()), lr=lr * 10)]
    cls = FusedSGD if fused else torch.optim.SGD
    opt = cls(groups, lr=lr, momentum=0.9, weight_decay=wd)
    model = DistributedDataParallel(net, compute_dtype=torch.bfloat16)
    model.train()
    return model, opt


def _batch(cuda, it, size=64):
    g = torch.Generator(device=cuda).manual_seed(1000 + it)
    imgs = torch.randn(2, 3, size, size, generator=g, device=cuda)
    gts = torch.randint(0, 19, (2, size, size), generator=g, device=cuda)
    gts[:, :4] = 255
    return imgs, gts


def _set_lr(opt, it):
    lr = BASE_LR * (1 - float(it) / TOTAL) ** 0.9                  # engine/lr_policy.py PolyLR
    for i, g in enumerate(opt.param_groups):
        g["lr"] = lr if i < 2 else lr * 10


def _run(cuda, steps, replayed, fused=True, size_of=None, before=None, **kw):
    """`steps` training steps, hand-written (replayed=False) or through ReplayedStep -> (losses, parameters + buffers, step).
    `size_of(it)`: the crop of step `it`; `before(it, model, opt)`: what the caller does ahead of step `it`."""
    from torchseg_amd.step import ReplayedStep
    model, opt = _build(cuda, fused)
    step = ReplayedStep(model, opt, **kw) if replayed else None
    losses, marks = [], []
    for it in range(steps):
        if before is not None:
            before(it, model, opt)
        batch = _batch(cuda, it, 64 if size_of is None else size_of(it))
        _set_lr(opt, it)
        if replayed:
            loss = step(*batch)
            marks.append((step.captures, step.replays, step.mode))
        else:
            opt.zero_grad()
            loss = model(*batch)
            loss.backward()
            opt.step()
        losses.append(loss.detach().float().clone())
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in model.module.state_dict().items()}
    return torch.stack(losses).cpu(), state, step, marks


def _assert_same(a, b):
    assert torch.isfinite(a[0]).all()
    assert torch.equal(a[0], b[0]), (a[0].tolist(), b[0].tolist())
    assert a[1].keys() == b[1].keys()
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


_REF = {}


def _eager8(cuda):
    """The eager run of test A (FusedSGD, 8 steps at 2 x 3 x 64 x 64), computed once."""
    if "a" not in _REF:
        _REF["a"] = _run(cuda, 8, False)
    return _REF["a"]


def test_a_replayed_trajectory_is_bit_equal_to_eager(cuda):
    eager = _eager8(cuda)
    again = _run(cuda, 8, False)
    _assert_same(eager, again)                 # precondition: otherwise the network has a non-reproducible layer
    got = _run(cuda, 8, True, warmup=3)
    print("eager ", eager[0].tolist(), "\nreplay", got[0].tolist())
    _assert_same(eager, got)
    step, marks = got[2], got[3]
    assert step.mode == "replay" and step.captures == 1 and step.replays == 5 and step.steps == 8, step.reason
    assert [m[0] for m in marks] == [0, 0, 0, 1, 1, 1, 1, 1]


def test_b_torch_sgd_runs_behind_the_graph(cuda):
    eager = _run(cuda, 8, False, fused=False)
    got = _run(cuda, 8, True, fused=False, warmup=3)
    _assert_same(eager, got)
    assert got[2].mode == "replay" and got[2].captures == 1 and not got[2]._opt_inside, got[2].reason


def test_c_bisenet_r18(cuda):
    """BiSeNet-R18 from bench.build_model at 2 x 3 x 128 x 128: 3 warm-up steps, 6 replays, against the eager loop.

    Both arms run with torch.backends.cudnn.deterministic = True.  Measured on an MI355X, four eager and four replayed runs
    in one process: without it the vendor library's convolutions do not reproduce (the first loss of two EAGER runs already
    differs, 9.983093 ... 9.983097, once 9.9818) and nine steps at this tiny shape (BatchNorm over 2 x 4 x 4 values, heads
    at 10 x the learning rate) amplify that to 0.6 - 1.0 % between two eager runs and 0.5 - 2.1 % between a replayed and an
    eager run: the 2e-2 below would then hold or not by chance.  With it all eight trajectories were equal bit for bit.
    The bound is the one tests/test_graph_gpu.py holds bench.GraphedStep to."""
    import bench
    from torchseg_amd.ddp import DistributedDataParallel
    from torchseg_amd.losses import ProbOhemCrossEntropy2d
    from torchseg_amd.step import ReplayedStep
    from torchseg_amd.syncbn import SyncBatchNorm
    from torchseg_amd.workloads import ensure_furnace_on_path
    ensure_furnace_on_path()
    from engine.lr_policy import PolyLR
    B, S, warm, replays = 2, 128, 3, 6
    out = {}
    old_det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for replayed in (False, True):
            model, opt, base_lr = bench.build_model(cuda, B, S, ProbOhemCrossEntropy2d, SyncBatchNorm, fused_sgd=True)
            model = DistributedDataParallel(model, compute_dtype=torch.bfloat16)
            model.train()
            batch = bench.synthetic_batch(cuda, B, S)
            pol = PolyLR(base_lr, 0.9, 1000)
            step = ReplayedStep(model, opt, warmup=warm) if replayed else None
            losses = []
            for it in range(warm + replays):
                lr = pol.get_lr(it)
                for i, g in enumerate(opt.param_groups):
                    g["lr"] = lr if i < 2 else lr * 10
                if replayed:
                    loss = step(*batch)
                else:
                    opt.zero_grad()
                    loss = model(*batch)
                    loss.backward()
                    opt.step()
                losses.append(loss.detach().float().clone())
            out[replayed] = torch.stack(losses).cpu().numpy()
            if replayed:
                assert step.mode == "replay" and step.captures == 1 and step.replays == replays, step.reason
            del model, opt, step
            torch.cuda.empty_cache()
    finally:
        torch.backends.cudnn.deterministic = old_det
    print("eager ", out[False].tolist(), "\nreplay", out[True].tolist())
    assert np.isfinite(out[True]).all(), out[True]
    assert np.allclose(out[True], out[False], rtol=2e-2, atol=0), (out[True], out[False])


class _ThreeInputs(nn.Module):
    """forward(data, label, aux_label): the signature of DFN's training call"""

    def __init__(self):
        super().__init__()
        self.body = nn.Conv2d(3, 8, 3, 1, 1)
        self.main = nn.Conv2d(8, 5, 1)
        self.aux = nn.Conv2d(8, 3, 1)

    def forward(self, data, label, aux_label):
        h = torch.relu(self.body(data))
        return F.cross_entropy(self.main(h), label) + 0.5 * F.cross_entropy(self.aux(h), aux_label)


def test_d_three_inputs_are_all_staged(cuda):
    from torchseg_amd.step import ReplayedStep
    torch.manual_seed(5)
    net = _ThreeInputs().to(cuda)
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=0.0)                # the parameters stay put: the loss depends on the batch only
    g = torch.Generator(device=cuda).manual_seed(9)
    data = torch.randn(2, 3, 16, 16, generator=g, device=cuda)
    label = torch.randint(0, 5, (2, 16, 16), generator=g, device=cuda)
    aux1 = torch.randint(0, 3, (2, 16, 16), generator=g, device=cuda)
    aux2 = (aux1 + 1) % 3
    step = ReplayedStep(net, opt, warmup=1)
    step(data, label, aux1)
    step(data, label, aux1)                                         # captures
    assert step.captures == 1
    l1 = step(data, label, aux1).clone()
    l2 = step(data, label, aux2).clone()
    l3 = step(data * 0.5, label, aux2).clone()
    l4 = step(data, label, aux1).clone()
    assert step.captures == 1 and step.replays == 5 and step.mode == "replay"
    assert l1.item() != l2.item() and l2.item() != l3.item()
    assert torch.equal(l1, l4)
    with torch.no_grad():
        want = [net(data, label, aux1), net(data, label, aux2), net(data * 0.5, label, aux2)]
    # the same fp32 arithmetic, but the vendor library may choose another convolution algorithm inside a capture: a few ulp
    for got, w in zip((l1, l2, l3), want):
        assert abs(got.item() - w.item()) <= 1e-5 * abs(w.item()), (got.item(), w.item())


def _sizes(it):
    return (64, 96, 64)[it // 5]


def test_e_one_capture_per_shape_and_lru_eviction(cuda):
    eager = _run(cuda, 15, False, size_of=_sizes)
    got = _run(cuda, 15, True, size_of=_sizes, warmup=3)
    _assert_same(eager, got)
    caps = [m[0] for m in got[3]]
    assert caps == [0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2], caps      # the third phase replays the first graph
    assert got[2].replays == 2 + 2 + 5
    one = _run(cuda, 15, True, size_of=_sizes, warmup=3, max_graphs=1)
    _assert_same(eager, one)
    caps = [m[0] for m in one[3]]
    assert caps == [0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 3, 3, 3, 3, 3], caps      # evicted, so captured again when it comes back
    assert len(one[2]._graphs) == 1


def test_f_dropout_draws_a_new_mask_at_every_replay(cuda):
    from torchseg_amd.step import ReplayedStep
    model, opt = _build(cuda, dropout=True, lr=0.0, wd=0.0)
    for g in opt.param_groups:
        g["lr"] = 0.0
    step = ReplayedStep(model, opt, warmup=2)
    batch = _batch(cuda, 0)
    vals = [step(*batch).item() for _ in range(6)]
    assert step.captures == 1 and step.replays == 4
    replayed = vals[2:]
    assert np.isfinite(replayed).all()
    assert len(set(replayed)) == len(replayed), vals


def test_g_invalidation(cuda):
    def before(it, model, opt):
        if it == 5:
            opt.load_state_dict(opt.state_dict())
        if it == 10:
            model.eval()
        if it == 11:
            model.train()

    eager = _run(cuda, 16, False, before=before)
    got = _run(cuda, 16, True, before=before, warmup=3)
    _assert_same(eager, got)
    marks = got[3]
    caps = [m[0] for m in marks]
    # 0-2 warm-up, 3 capture, 4 replay | reload: 5-7 warm-up, 8 capture, 9 replay | 10 eval: eager | 11-13 warm-up, 14 capture
    assert caps == [0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3], caps
    reps = [m[1] for m in marks]
    assert reps[4] == 2 and reps[5] == reps[6] == reps[7] == 2 and reps[8] == 3, reps   # the old graph is not replayed
    assert marks[10][2] == "eager" and reps[10] == reps[9]
    assert marks[15][2] == "replay" and reps[15] == reps[13] + 2


def test_g2_model_load_state_dict_needs_no_new_capture(cuda):
    saved = {}

    def before(it, model, opt):
        if it == 1:
            saved.update({k: v.detach().clone() for k, v in model.state_dict().items()})
        if it == 6:
            model.load_state_dict(saved)                            # copies in place
            saved.clear()

    eager = _run(cuda, 9, False, before=before)
    got = _run(cuda, 9, True, before=before, warmup=3)
    _assert_same(eager, got)
    assert got[2].captures == 1 and got[2].replays == 6
    sgd = _run(cuda, 9, True, fused=False, before=before, warmup=3)
    _assert_same(_run(cuda, 9, False, fused=False, before=before), sgd)
    assert sgd[2].captures == 1


class _Item(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 5, 3, 1, 1)

    def forward(self, data, label):
        scale = 1.0 + 0.0 * data.mean().item()                     # a host read: refused while the stream is capturing
        return F.cross_entropy(self.conv(data) * scale, label)


def _item_setup(cuda):
    torch.manual_seed(2)
    net = _Item().to(cuda)
    net.train()
    g = torch.Generator(device=cuda).manual_seed(4)
    batch = (torch.randn(2, 3, 16, 16, generator=g, device=cuda), torch.randint(0, 5, (2, 16, 16), generator=g, device=cuda))
    return net, torch.optim.SGD(net.parameters(), lr=0.1), batch


def test_h_capture_failure_falls_back_and_leaves_the_stream_usable(cuda):
    from torchseg_amd.step import ReplayedStep
    net, opt, batch = _item_setup(cuda)
    want = []
    for _ in range(3):
        opt.zero_grad()
        loss = net(*batch)
        loss.backward()
        opt.step()
        want.append(loss.item())
    net, opt, batch = _item_setup(cuda)
    step = ReplayedStep(net, opt, warmup=1, strict=False)
    got = [step(*batch).item() for _ in range(3)]                  # warm-up, failed capture (run eagerly), eager
    assert step.mode == "eager" and step.captures == 0 and step.steps == 3
    assert "capture failed" in step.reason and "Error" in step.reason, step.reason
    assert np.allclose(got, want, rtol=1e-5, atol=0), (got, want)  # no iteration lost: the third loss has seen two updates
    assert not torch.cuda.is_current_stream_capturing()
    # an unrelated step captures and replays correctly afterwards
    after = _run(cuda, 8, True, warmup=3)
    _assert_same(_eager8(cuda), after)
    assert after[2].captures == 1 and after[2].mode == "replay"
    # strict: the exception is the caller's
    net, opt, batch = _item_setup(cuda)
    strict = ReplayedStep(net, opt, warmup=1, strict=True)
    strict(*batch)
    with pytest.raises(Exception):
        strict(*batch)
    assert strict.captures == 0
    assert not torch.cuda.is_current_stream_capturing()
    again = _run(cuda, 8, True, warmup=3)
    _assert_same(_eager8(cuda), again)


def test_i_loss_ring(cuda):
    from torchseg_amd.step import ReplayedStep
    model, opt = _build(cuda)
    step = ReplayedStep(model, opt, warmup=3, loss_ring=4)
    returned = []
    for it in range(7):
        _set_lr(opt, it)
        returned.append(step(*_batch(cuda, it)).detach().float().clone())
    assert step.captures == 1 and step.replays == 4
    ring = step.losses()
    assert ring.shape == (4,) and torch.equal(ring, torch.stack(returned[3:]).cpu()), (ring, returned)
    assert torch.equal(torch.stack(returned).cpu(), _eager8(cuda)[0][:7])
