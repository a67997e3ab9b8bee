"""torchseg_amd.step.ReplayedStep where there is nothing to capture: on the CPU, with a process group, with the switch off.
The step must then BE the hand-written loop (zero_grad -> forward -> backward -> optimizer.step) and say why."""
import os
import socket

import torch
import torch.nn as nn


class _Net(nn.Module):
    """Two convolutions, BatchNorm, cross-entropy: forward(data, label) returns the scalar loss."""

    def __init__(self):
        super().__init__()
        self.c1 = nn.Conv2d(3, 8, 3, 1, 1, bias=False)
        self.bn = nn.BatchNorm2d(8)
        self.c2 = nn.Conv2d(8, 5, 1)

    def forward(self, data, label):
        return nn.functional.cross_entropy(self.c2(torch.relu(self.bn(self.c1(data)))), label)


def _setup(seed=7):
    torch.manual_seed(seed)
    net = _Net()
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    return net, opt


def _batch(it):
    g = torch.Generator().manual_seed(100 + it)
    return torch.randn(2, 3, 12, 10, generator=g), torch.randint(0, 5, (2, 12, 10), generator=g)


def _set_lr(opt, it):
    for g in opt.param_groups:
        g["lr"] = 0.05 * (1 - it / 10.0) ** 0.9


def _hand_written(steps):
    net, opt = _setup()
    losses = []
    for it in range(steps):
        _set_lr(opt, it)
        opt.zero_grad()
        loss = net(*_batch(it))
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return losses, net


def _replayed(steps, **kw):
    from torchseg_amd.step import ReplayedStep
    net, opt = _setup()
    step = ReplayedStep(net, opt, **kw)
    losses = []
    for it in range(steps):
        _set_lr(opt, it)
        losses.append(step(*_batch(it)).detach().clone())
    return losses, net, step


def _assert_same(a_losses, a_net, b_losses, b_net):
    assert len(a_losses) == len(b_losses)
    assert all(torch.equal(a, b) for a, b in zip(a_losses, b_losses)), (a_losses, b_losses)
    for (n, a), (_, b) in zip(a_net.state_dict().items(), b_net.state_dict().items()):
        assert torch.equal(a, b), n


def test_cpu_step_equals_the_hand_written_loop():
    want, want_net = _hand_written(5)
    got, got_net, step = _replayed(5, warmup=3)
    _assert_same(want, want_net, got, got_net)
    assert step.mode == "eager" and "device" in step.reason and "cpu" in step.reason
    assert step.captures == 0 and step.steps == 5


def test_process_group_falls_back_to_eager():
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    old = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT", "RANK", "WORLD_SIZE")}
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        want, want_net = _hand_written(3)
        got, got_net, step = _replayed(3)
        assert step.mode == "eager" and "process group" in step.reason
        _assert_same(want, want_net, got, got_net)
    finally:
        dist.destroy_process_group()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_switch_off_names_the_switch(monkeypatch):
    monkeypatch.setenv("TSG_STEP_REPLAY", "0")
    want, want_net = _hand_written(3)
    got, got_net, step = _replayed(3)
    assert step.mode == "eager" and "TSG_STEP_REPLAY=0" in step.reason
    _assert_same(want, want_net, got, got_net)


def test_loss_ring_in_eager_mode_keeps_the_last_steps_in_order():
    got, _, step = _replayed(6, loss_ring=4)
    ring = step.losses()
    assert ring.dtype == torch.float32 and ring.shape == (4,)
    assert torch.equal(ring, torch.stack([l.float() for l in got[2:6]]))        # steps 3-6 of six
    # fewer steps than slots: only what was written
    got2, _, step2 = _replayed(2, loss_ring=4)
    assert torch.equal(step2.losses(), torch.stack([l.float() for l in got2]))


def test_engine_offers_the_step(monkeypatch):
    import sys
    from torchseg_amd.workloads import ensure_furnace_on_path
    ensure_furnace_on_path()
    from engine.engine import Engine
    from torchseg_amd.step import ReplayedStep
    monkeypatch.setattr(sys, "argv", ["train.py"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    net, opt = _setup()
    with Engine() as engine:
        step = engine.replayed_step(net, opt, warmup=2, loss_ring=3)
    assert isinstance(step, ReplayedStep) and step.warmup == 2
