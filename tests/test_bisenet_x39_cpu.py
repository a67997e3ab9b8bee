"""CPU: BiSeNet-X39 (cityscapes.bisenet.X39 and X39.speed) on our furnace.

The reference's unchanged network.py files import `xception39` from base_model and build on our furnace with the state
dict, parameter count, seeded init, loss and gradients of the reference's own code (tests/golden/x39_golden.*, written by
tests/golden/make_x39_golden.py from the reference's network.py on the reference's furnace); our workload builder is the
same network; every import of X39's scripts resolves; the depthwise installer takes exactly Xception39's 51 layers and
nothing of the other models; the library's support predicate takes the nine shapes of the benchmark."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _x39
from _dropin import GOLDEN, ROOT, have_reference, run_in, stage
from test_dropin_cpu import _IMPORTS


def _golden():
    with open(os.path.join(GOLDEN, "x39_golden.json")) as fh:
        g = json.load(fh)
    g["arrays"] = dict(np.load(os.path.join(GOLDEN, "x39_golden.npz")))
    return g


def _key(exp):
    return "speed" if exp.endswith(".speed") else "X39"


def _check(out, g, arrays, key):
    assert out["keys"] == g["keys"], "state-dict keys / shapes differ"
    assert out["nparam"] == g["nparam"] == 1842289
    assert out["dw_names"] == g["dw_names"] and len(out["dw_names"]) == 51
    for (k, s, q), (rk, rs, rq) in zip(out["fp"], g["fp"]):
        assert k == rk
        assert abs(s - rs) <= 1e-6 * max(1.0, abs(rs)) and abs(q - rq) <= 1e-6 * max(1.0, abs(rq)), (k, s, rs, q, rq)
    assert abs(out["loss"] - g["loss"]) <= 1e-5 * abs(g["loss"]), (out["loss"], g["loss"])
    dw = np.asarray(out["dw_grad"], np.float64)
    dw_ref = arrays[key + "_dw_grad"].astype(np.float64)
    assert dw.shape == dw_ref.shape
    assert np.abs(dw - dw_ref).max() <= 1e-4 * g["dw_gmax"]
    sample = np.asarray(out["grad_sample"], np.float64)
    assert np.abs(sample - arrays[key + "_grad_sample"]).max() <= 1e-4 * g["gmax"]


@pytest.mark.parametrize("exp", _x39.EXPS)
def test_unchanged_network_builds_on_our_furnace(tmp_path, exp):
    """The reference's X39 / X39.speed network.py (staged against OUR furnace) gives the reference's numbers."""
    if not have_reference():
        pytest.skip("the unchanged network.py is not in the repository; "
                    "test_workload_builder_equals_reference covers our side against the golden data")
    g = _golden()
    d = stage(tmp_path, "bisenet", exp)
    out = json.loads(run_in(d, _x39.script("ref", exp)).strip().splitlines()[-1])
    _check(out, g[_key(exp)], g["arrays"], _key(exp))


@pytest.mark.parametrize("exp", _x39.EXPS)
def test_workload_builder_equals_reference(tmp_path, exp):
    """torchseg_amd.workloads.bisenet_x39 is the X39 network (the .speed heads by their scales alone)."""
    g = _golden()
    gk = g[_key(exp)]
    out = json.loads(run_in(str(tmp_path), _x39.script("ours", exp, seed=gk["seed"], ncls=gk["ncls"]),
                            furnace=True).strip().splitlines()[-1])
    _check(out, gk, g["arrays"], _key(exp))


def test_every_import_of_the_x39_scripts_resolves(tmp_path):
    exp = _x39.EXPS[0]
    if have_reference():
        d = stage(tmp_path, "bisenet", exp, files=("config.py", "network.py", "train.py", "eval.py", "dataloader.py"))
        out = json.loads(run_in(d, _IMPORTS % dict(ref=True)).strip().splitlines()[-1])
    else:
        with open(str(tmp_path / "statements.json"), "w") as fh:
            json.dump(_golden()["imports"], fh)
        out = json.loads(run_in(str(tmp_path), _IMPORTS % dict(ref=False), furnace=True).strip().splitlines()[-1])
    assert any(s[1] == "base_model" for s in _golden()["imports"]) or out["statements"]
    assert out["statements"]
    assert not out["missing"], out["missing"]


_INSTALL = r'''
import json, torch.nn as nn
from oracle.ohem_ref import ProbOhemCrossEntropy2d
from torchseg_amd.dwconv import DepthwiseConv2d, install_depthwise_conv
from torchseg_amd.workloads.bisenet import BiSeNet
from torchseg_amd.workloads.bisenet_x39 import BiSeNetX39
from torchseg_amd.workloads.dfn import DFN
from torchseg_amd.workloads.pspnet import PSPNet, PSANet
from oracle.focal_ref import SigmoidFocalLoss
ohem = ProbOhemCrossEntropy2d(ignore_label=255, thresh=0.7, min_kept=1000, use_weight=False)
ce = nn.CrossEntropyLoss(ignore_index=255)
models = dict(
    x39=BiSeNetX39(19, True, None, ohem, norm_layer=nn.BatchNorm2d),
    r18=BiSeNet(19, True, ohem, None, nn.BatchNorm2d),
    pspnet=PSPNet(150, ce, None, nn.BatchNorm2d, depth=50),
    psanet=PSANet(150, ce, None, nn.BatchNorm2d, depth=50),
    dfn=DFN(19, ce, SigmoidFocalLoss(ignore_label=255, gamma=2.0, alpha=0.25), 0.1, None, nn.BatchNorm2d))
out = {}
for name, m in models.items():
    keys = list(m.state_dict().keys())
    n = install_depthwise_conv(m)
    assert list(m.state_dict().keys()) == keys
    assert sum(isinstance(x, DepthwiseConv2d) for x in m.modules()) == n
    out[name] = n
print(json.dumps(out))
'''


def test_depthwise_installer_takes_x39_layers_only(tmp_path):
    out = json.loads(run_in(str(tmp_path), _INSTALL, timeout=900, furnace=True).strip().splitlines()[-1])
    assert out == dict(x39=51, r18=0, pspnet=0, psanet=0, dfn=0), out


def test_installer_rejects_other_convolutions():
    from torchseg_amd.dwconv import install_depthwise_conv
    hooked = nn.Conv2d(16, 16, 3, 1, 1, groups=16, bias=False)
    hooked.register_forward_hook(lambda *a: None)
    m = nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1, groups=16, bias=False),       # taken
                      nn.Conv2d(16, 16, 3, 2, 1, groups=16, bias=False),       # taken
                      nn.Conv2d(16, 16, 3, 1, 1, groups=16, bias=True),
                      nn.Conv2d(16, 16, 5, 1, 2, groups=16, bias=False),
                      nn.Conv2d(16, 16, 3, 1, 2, dilation=2, groups=16, bias=False),
                      nn.Conv2d(16, 16, 3, 3, 1, groups=16, bias=False),
                      nn.Conv2d(16, 16, 3, 1, 1, groups=8, bias=False),
                      nn.Conv2d(16, 32, 3, 1, 1, groups=16, bias=False),
                      nn.Conv2d(16, 16, 3, 1, 1, bias=False),
                      nn.Conv2d(16, 16, 3, 1, 1, groups=16, bias=False, padding_mode="reflect"),
                      hooked)
    assert install_depthwise_conv(m) == 2
    assert [type(x).__name__ for x in m[:3]] == ["DepthwiseConv2d", "DepthwiseConv2d", "Conv2d"]
    x = torch.randn(1, 16, 8, 8)
    ref = nn.functional.conv2d(x, m[0].weight, None, 1, 1, 1, 16)
    assert torch.equal(m[0](x), ref)               # CPU input: the stock forward


# (C, H_in, stride): the depthwise layers of Xception39 at 16 x 1024^2
SHAPES = [(8, 256, 2), (16, 128, 1), (64, 128, 1), (64, 128, 2), (32, 64, 1), (128, 64, 1), (128, 64, 2), (64, 32, 1),
          (256, 32, 1)]


def test_library_support_predicate():
    from torchseg_amd import _lib
    lib = _lib.lib()
    for dt in (_lib.BF16, _lib.F32):
        for C, H, s in SHAPES:
            assert lib.tsg_dwconv3x3_supported(dt, C, 3, 3, s, 1, 1, C, H, H) == 1, (dt, C, H, s)
            assert lib.tsg_dwconv3x3_wgrad_ws_bytes(16, H, H, C, s, dt) > 0
        assert lib.tsg_dwconv3x3_supported(dt, 64, 5, 5, 1, 2, 1, 64, 32, 32) == 0         # kernel 5
        assert lib.tsg_dwconv3x3_supported(dt, 64, 3, 3, 1, 2, 2, 64, 32, 32) == 0         # dilation 2
        assert lib.tsg_dwconv3x3_supported(dt, 64, 3, 3, 1, 1, 1, 32, 32, 32) == 0         # groups != C
        assert lib.tsg_dwconv3x3_supported(dt, 64, 3, 3, 1, 1, 1, 1, 32, 32) == 0
        assert lib.tsg_dwconv3x3_supported(dt, 12, 3, 3, 1, 1, 1, 12, 32, 32) == 0         # C % 8 != 0
        assert lib.tsg_dwconv3x3_supported(dt, 64, 3, 3, 3, 1, 1, 64, 32, 32) == 0         # stride 3
        assert lib.tsg_dwconv3x3_supported(dt, 64, 3, 3, 1, 0, 1, 64, 32, 32) == 0         # padding 0
    assert lib.tsg_dwconv3x3_supported(7, 64, 3, 3, 1, 1, 1, 64, 32, 32) == 0               # dtype
    # shape-only partial count: fp64 partials in the parity mode are twice the fp32 ones
    assert lib.tsg_dwconv3x3_wgrad_ws_bytes(2, 64, 64, 32, 1, _lib.F32) == 2 * lib.tsg_dwconv3x3_wgrad_ws_bytes(
        2, 64, 64, 32, 1, _lib.BF16)
    assert lib.tsg_dwconv3x3_wgrad_ws_bytes(2, 64, 64, 12, 1, _lib.BF16) == 0
    assert lib.tsg_dwconv3x3_fwd(None, None, None, _lib.BF16, 1, 8, 8, 8, 1, None) < 0
    assert lib.tsg_dwconv3x3_wgrad(None, None, None, _lib.BF16, 1, 8, 8, 8, 1, None, 0, None) < 0


def test_supported_wrapper_refuses_nchw_and_bad_filters():
    from torchseg_amd import kernels as K
    kp = K.HipKernels()
    w = torch.randn(16, 1, 3, 3)
    x = torch.randn(2, 16, 8, 8)
    assert not kp.dwconv3x3_supported(x, w, 1, 1, 1, 16)                                          # NCHW
    xc = x.contiguous(memory_format=torch.channels_last)
    assert kp.dwconv3x3_supported(xc, w, 1, 1, 1, 16)
    assert kp.dwconv3x3_supported(xc.bfloat16(), w, 2, 1, 1, 16)
    assert not kp.dwconv3x3_supported(xc.half(), w, 1, 1, 1, 16)
    assert not kp.dwconv3x3_supported(xc, w.bfloat16(), 1, 1, 1, 16)
    assert not kp.dwconv3x3_supported(xc, torch.randn(16, 1, 9, 3)[:, :, ::3], 1, 1, 1, 16)       # strided filter
