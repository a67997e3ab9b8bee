"""Host side of the fused head for 33..256 classes (TSG_FUSE_HEAD_WIDE): the C ABI declares the query, the switch is off
by default, and fusion.FuseMode / losses.ohem_cross_entropy defer a 150-channel head only with the switch on and only
through a provider that has the wide kernels.  The kernels themselves: tests/test_fused_head_wide_gpu.py."""
import os
import re
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def standin(monkeypatch):
    from _cpu_provider import OracleProvider
    from torchseg_amd import fusion, kernels as K
    prov = OracleProvider()
    prov.calls = []
    old = K._set_provider_for_tests(prov)
    monkeypatch.setattr(fusion, "_is_map", lambda t: isinstance(t, torch.Tensor) and t.dim() == 4
                        and t.dtype in (torch.float32, torch.bfloat16))
    monkeypatch.setattr(fusion, "_TARGET_ON_DEVICE", False)
    yield prov
    K._set_provider_for_tests(old)


def test_header_declares_the_wide_query():
    with open(os.path.join(ROOT, "include", "tsg_hip.h")) as f:
        text = f.read()
    assert re.search(r"\bint\s+tsg_ohem_up_wide_supported\s*\(\s*int C,\s*int IH,\s*int IW,\s*int OH,\s*int OW\s*\)\s*;", text)
    # the narrow query keeps its prototype
    assert re.search(r"\bint\s+tsg_ohem_up_supported\s*\(int C, int IH, int IW, int OH, int OW, float thresh\);", text)


def test_switch_is_off_by_default():
    from torchseg_amd import losses
    assert isinstance(losses.FUSE_HEAD_WIDE, bool)
    assert losses.FUSE_HEAD_WIDE == (os.environ.get("TSG_FUSE_HEAD_WIDE", "0") == "1")     # opt-in: unset means off
    if "TSG_FUSE_HEAD_WIDE" not in os.environ:
        assert losses.FUSE_HEAD_WIDE is False


def _head150():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 150, 3, 4, generator=g)
    y = torch.randint(0, 150, (1, 24, 32), generator=g)
    y[:, :2] = 255
    return x, y


def _run_head(x, y, fused):
    from torchseg_amd.fusion import FuseMode
    crit = nn.CrossEntropyLoss(reduction='mean', ignore_index=255)
    xf = x.clone().requires_grad_(True)

    def head(t):       # pspnet network.py:46-56
        return crit(F.log_softmax(F.interpolate(t * 1.5, scale_factor=8, mode='bilinear', align_corners=True), dim=1), y)

    if fused:
        with FuseMode(head=True):
            out = head(xf)
    else:
        out = head(xf)
    out.backward()
    return out.detach(), xf.grad


def test_150_channel_head_is_not_deferred_with_the_switch_off(standin, monkeypatch):
    from torchseg_amd import fusion, losses
    from torchseg_amd.fusion import FuseMode
    from torchseg_amd.upsample import DeferredUpsample
    monkeypatch.setattr(losses, "FUSE_HEAD_WIDE", False)
    x, y = _head150()
    before = fusion.stats["head_deferred"]
    with FuseMode(head=True):
        up = F.interpolate(x.clone().requires_grad_(True), scale_factor=8, mode='bilinear', align_corners=True)
    assert isinstance(up, torch.Tensor) and not isinstance(up, DeferredUpsample)
    assert fusion.stats["head_deferred"] == before
    ref = _run_head(x, y, False)
    got = _run_head(x, y, True)
    assert "ohem_up_fwd" not in standin.calls and standin.calls == ["ohem_fwd", "ohem_bwd"]
    torch.testing.assert_close(got[0], ref[0], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(got[1], ref[1], rtol=1e-5, atol=1e-7)


def test_150_channel_head_is_deferred_with_the_switch_on(standin, monkeypatch):
    from torchseg_amd import fusion, losses
    from torchseg_amd.fusion import FuseMode
    from torchseg_amd.upsample import DeferredUpsample
    monkeypatch.setattr(losses, "FUSE_HEAD_WIDE", True)
    wide_calls = []
    # the stand-in has no wide kernels of its own: give this instance the query, its ohem_up_* take any C
    standin.ohem_up_wide_supported = lambda z, OH, OW: (wide_calls.append(tuple(z.shape)), 32 < z.shape[1] <= 256)[1]
    x, y = _head150()
    before = fusion.stats["head_deferred"]
    with FuseMode(head=True):
        up = F.interpolate(x.clone().requires_grad_(True), scale_factor=8, mode='bilinear', align_corners=True)
        assert isinstance(up, DeferredUpsample)
        feat = torch.randn(1, 512, 3, 4, requires_grad=True)          # a feature map is still not a head
        assert not isinstance(F.interpolate(feat, scale_factor=8, mode='bilinear', align_corners=True), DeferredUpsample)
    assert fusion.stats["head_deferred"] == before + 1
    ref = _run_head(x, y, False)
    got = _run_head(x, y, True)
    assert standin.calls == ["ohem_up_fwd", "ohem_up_bwd"] and wide_calls == [(1, 150, 3, 4)]
    torch.testing.assert_close(got[0], ref[0], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(got[1], ref[1], rtol=1e-5, atol=1e-7)


def test_provider_without_the_wide_query_materialises(standin, monkeypatch):
    """The switch on, a provider that has no ohem_up_wide_supported: the deferred head is materialised, nothing raises."""
    from torchseg_amd import losses
    monkeypatch.setattr(losses, "FUSE_HEAD_WIDE", True)
    assert not hasattr(standin, "ohem_up_wide_supported")
    x, y = _head150()
    ref = _run_head(x, y, False)
    got = _run_head(x, y, True)
    assert standin.calls == ["upsample_fwd", "ohem_fwd", "ohem_bwd", "upsample_bwd"], standin.calls
    torch.testing.assert_close(got[0], ref[0], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(got[1], ref[1], rtol=1e-5, atol=1e-7)
