"""FCN-32s (model/fcn/voc.fcn32s.R101_v1c) on the CPU, against what the reference's own network.py computes on its own
furnace (tests/golden/make_fcn_golden.py).

The unchanged network.py builds on our furnace with the reference's state-dict keys, parameter count, seeded init, loss
(with and without a Dropout2d mask) and gradients; so does torchseg_amd.workloads.fcn; every import of FCN's scripts
resolves, seg_opr.sync_bn included; the deep-stem installer (TSG_DEEP_STEM_CONV=1) takes exactly conv1[0] of each v1c
model and nothing else; the library's support predicate takes the deep-stem shapes.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _fcn
from _dropin import GOLDEN, have_reference, run_in, stage
from test_dropin_cpu import _IMPORTS


def _golden():
    with open(os.path.join(GOLDEN, "fcn_golden.json")) as fh:
        g = json.load(fh)
    g["arrays"] = dict(np.load(os.path.join(GOLDEN, "fcn_golden.npz")))
    return g


def _check(out, g):
    assert out["keys"] == g["keys"], "state-dict keys / shapes differ"
    assert out["nparam"] == g["nparam"]
    for (k, s, q), (rk, rs, rq) in zip(out["fp"], g["fp"]):
        assert k == rk
        assert abs(s - rs) <= 1e-6 * max(1.0, abs(rs)) and abs(q - rq) <= 1e-6 * max(1.0, abs(rq)), (k, s, rs, q, rq)
    assert abs(out["loss"] - g["loss"]) <= 1e-5 * abs(g["loss"]), (out["loss"], g["loss"])
    assert out["dropout_p"] == g["dropout_p"] == [0.1, 0.1]
    assert abs(out["loss_drop"] - g["loss_drop"]) <= 1e-5 * abs(g["loss_drop"]), (out["loss_drop"], g["loss_drop"])
    sample = np.asarray(out["grad_sample"], np.float64)
    assert np.abs(sample - g["arrays"]["grad_sample"]).max() <= 1e-4 * g["gmax"]
    stem = np.asarray(out["stem_grad"], np.float64)
    ref = g["arrays"]["stem_grad"].astype(np.float64)
    assert stem.shape == ref.shape == (64 * 27,)
    assert np.abs(stem - ref).max() <= 1e-4 * np.abs(ref).max()


def test_unchanged_network_builds_on_our_furnace(tmp_path):
    """The reference's FCN network.py (staged against OUR furnace) gives the reference's numbers."""
    if not have_reference():
        pytest.skip("the unchanged network.py is not in the repository; "
                    "test_workload_builder_equals_reference covers our side against the golden data")
    d = stage(tmp_path, "fcn", _fcn.EXP)
    _check(json.loads(run_in(d, _fcn.script("ref"), timeout=900).strip().splitlines()[-1]), _golden())


def test_workload_builder_equals_reference(tmp_path):
    """torchseg_amd.workloads.fcn is the FCN-32s network."""
    g = _golden()
    assert g["seed"] == 304 and g["ncls"] == 21
    out = json.loads(run_in(str(tmp_path), _fcn.script("ours", seed=g["seed"], ncls=g["ncls"]), timeout=900,
                            furnace=True).strip().splitlines()[-1])
    _check(out, g)


def test_every_import_of_the_fcn_scripts_resolves(tmp_path):
    if have_reference():
        d = stage(tmp_path, "fcn", _fcn.EXP, files=("config.py", "network.py", "train.py", "eval.py", "dataloader.py"))
        out = json.loads(run_in(d, _IMPORTS % dict(ref=True)).strip().splitlines()[-1])
    else:
        with open(str(tmp_path / "statements.json"), "w") as fh:
            json.dump(_golden()["imports"], fh)
        out = json.loads(run_in(str(tmp_path), _IMPORTS % dict(ref=False), furnace=True).strip().splitlines()[-1])
    assert ["train.py", "seg_opr.sync_bn", ["DataParallelModel", "Reduce", "BatchNorm2d"]] in _golden()["imports"]
    assert out["statements"]
    assert not out["missing"], out["missing"]


_SYNC_BN = r'''
import json, torch, torch.nn as nn
from seg_opr.sync_bn import BatchNorm2d, DataParallelModel, Reduce
from torchseg_amd.syncbn import SyncBatchNorm
assert BatchNorm2d is SyncBatchNorm
lin = nn.Linear(4, 1)
m = DataParallelModel(lin, [0])
x = torch.randn(3, 4)
out = m(x)
assert isinstance(out, list) and len(out) == 1
loss = Reduce.apply(*[o.sum() for o in out])
loss.backward()
assert torch.allclose(loss, lin(x).sum())
assert torch.allclose(lin.weight.grad, x.sum(0, keepdim=True))
a, b = torch.tensor(2.0, requires_grad=True), torch.tensor(3.0, requires_grad=True)
s = Reduce.apply(a, b)
s.backward()
assert s.item() == 5.0 and a.grad.item() == 1.0 and b.grad.item() == 1.0
try:
    DataParallelModel(lin, [0, 1])
    err = ""
except RuntimeError as e:
    err = str(e)
print(json.dumps(dict(err=err)))
'''


def test_sync_bn_compatibility_names(tmp_path):
    out = json.loads(run_in(str(tmp_path), _SYNC_BN, furnace=True).strip().splitlines()[-1])
    assert "distributed" in out["err"] and "single device" in out["err"], out["err"]


_INSTALL = r'''
import json, os, torch, torch.nn as nn
from oracle.ohem_ref import ProbOhemCrossEntropy2d
from oracle.focal_ref import SigmoidFocalLoss
from torchseg_amd import ddp
from torchseg_amd.stemconv import DeepStemConv2d
from torchseg_amd.workloads.bisenet import BiSeNet
from torchseg_amd.workloads.bisenet_x39 import BiSeNetX39
from torchseg_amd.workloads.dfn import DFN
from torchseg_amd.workloads.fcn import FCN
from torchseg_amd.workloads.pspnet import PSPNet, PSANet
ohem = ProbOhemCrossEntropy2d(ignore_label=255, thresh=0.7, min_kept=1000, use_weight=False)
ce = nn.CrossEntropyLoss(ignore_index=255)
builders = dict(
    fcn=lambda: FCN(21, ce, norm_layer=nn.BatchNorm2d),
    pspnet=lambda: PSPNet(150, ce, None, nn.BatchNorm2d, depth=50),
    psanet=lambda: PSANet(150, ce, None, nn.BatchNorm2d, depth=101),
    dfn=lambda: DFN(19, ce, SigmoidFocalLoss(ignore_label=255, gamma=2.0, alpha=0.25), 0.1, None, nn.BatchNorm2d),
    r18=lambda: BiSeNet(19, True, ohem, None, nn.BatchNorm2d),
    x39=lambda: BiSeNetX39(19, True, None, ohem, norm_layer=nn.BatchNorm2d))
out = {}
for flag in ("unset", "0", "1"):
    if flag == "unset":
        os.environ.pop("TSG_DEEP_STEM_CONV", None)
    else:
        os.environ["TSG_DEEP_STEM_CONV"] = flag
    for name, build in builders.items():
        m = build()
        keys = list(m.state_dict().keys())
        ddp.install_kernels(m, torch.bfloat16)
        assert list(m.state_dict().keys()) == keys
        out["%s/%s" % (flag, name)] = [n for n, x in m.named_modules() if isinstance(x, DeepStemConv2d)]
print(json.dumps(out))
'''


def test_deep_stem_installer_takes_conv1_0_under_the_flag_only(tmp_path):
    out = json.loads(run_in(str(tmp_path), _INSTALL, timeout=900, furnace=True).strip().splitlines()[-1])
    for name in ("fcn", "pspnet", "psanet", "dfn"):
        assert out["1/" + name] == ["backbone.conv1.0"], (name, out["1/" + name])
    for name in ("r18", "x39"):
        assert out["1/" + name] == [], (name, out["1/" + name])
    for flag in ("unset", "0"):
        for name in ("fcn", "pspnet", "psanet", "dfn", "r18", "x39"):
            assert out["%s/%s" % (flag, name)] == [], (flag, name)


def test_deep_stem_installer_rejects_other_convolutions():
    from torchseg_amd.stemconv import install_deep_stem_conv
    m = nn.Sequential(nn.Conv2d(3, 64, 3, 2, 1, bias=False),                    # taken
                      nn.Conv2d(3, 64, 3, 2, 1, bias=True),
                      nn.Conv2d(3, 32, 3, 2, 1, bias=False),
                      nn.Conv2d(3, 64, 3, 1, 1, bias=False),
                      nn.Conv2d(3, 64, 7, 2, 3, bias=False),
                      nn.Conv2d(3, 64, 3, 2, 2, dilation=2, bias=False),
                      nn.Conv2d(4, 64, 3, 2, 1, bias=False),
                      nn.Conv2d(3, 64, 3, 2, 1, bias=False, padding_mode="reflect"))
    assert install_deep_stem_conv(m) == 1
    assert [type(x).__name__ for x in m[:2]] == ["DeepStemConv2d", "Conv2d"]
    x = torch.randn(1, 3, 9, 9)
    ref = nn.functional.conv2d(x, m[0].weight, None, 2, 1)
    assert torch.equal(m[0](x), ref)               # CPU input: the stock forward


# (H, W) of the deep stem's input: training crops of the v1c configs, odd and even sizes, eval windows
SHAPES = [(512, 512), (720, 720), (769, 769), (1024, 1024), (480, 480), (713, 713), (128, 128), (97, 130), (1, 1),
          (2, 3), (1024, 2048)]


def test_library_support_predicate():
    from torchseg_amd import _lib
    lib = _lib.lib()
    for H, W in SHAPES:
        assert lib.tsg_stem3_conv_supported(_lib.BF16, 3, 64, 3, 3, 2, 1, 1, 1, H, W) == 1, (H, W)
    assert lib.tsg_stem3_conv_supported(_lib.F32, 3, 64, 3, 3, 2, 1, 1, 1, 64, 64) == 0            # fp32: stock / exact
    assert lib.tsg_stem3_conv_supported(_lib.BF16, 4, 64, 3, 3, 2, 1, 1, 1, 64, 64) == 0           # C_in
    assert lib.tsg_stem3_conv_supported(_lib.BF16, 3, 32, 3, 3, 2, 1, 1, 1, 64, 64) == 0           # C_out
    assert lib.tsg_stem3_conv_supported(_lib.BF16, 3, 64, 7, 7, 2, 3, 1, 1, 64, 64) == 0           # the 7x7 stem
    assert lib.tsg_stem3_conv_supported(_lib.BF16, 3, 64, 3, 3, 1, 1, 1, 1, 64, 64) == 0           # stride 1
    assert lib.tsg_stem3_conv_supported(_lib.BF16, 3, 64, 3, 3, 2, 0, 1, 1, 64, 64) == 0           # padding 0
    assert lib.tsg_stem3_conv_supported(_lib.BF16, 3, 64, 3, 3, 2, 2, 2, 1, 64, 64) == 0           # dilation 2
    assert lib.tsg_stem3_conv_supported(_lib.BF16, 3, 64, 3, 3, 2, 1, 1, 3, 64, 64) == 0           # groups
    assert lib.tsg_stem3_conv_supported(_lib.BF16, 3, 64, 3, 3, 2, 1, 1, 1, 0, 64) == 0            # empty
    assert lib.tsg_stem3_conv_ws_bytes() > 0
    assert lib.tsg_stem3_conv_fwd(None, None, None, 1, 8, 8, None, 0, None) < 0
    assert lib.tsg_stem3_conv_wrw(None, None, None, 1, 8, 8, None, 0, None) < 0


def test_supported_wrapper_refuses_fp32_and_bad_layouts():
    from torchseg_amd import kernels as K
    kp = K.HipKernels()
    w = torch.randn(64, 3, 3, 3)
    x = torch.randn(2, 3, 17, 18).bfloat16()
    assert kp.stem3_conv_supported(x, w, 2, 1, 1, 1)
    assert not kp.stem3_conv_supported(x.float(), w, 2, 1, 1, 1)                                   # fp32
    assert not kp.stem3_conv_supported(x.contiguous(memory_format=torch.channels_last), w, 2, 1, 1, 1)
    assert not kp.stem3_conv_supported(x, torch.randn(64, 3, 7, 7), 2, 1, 1, 1)
    assert not kp.stem3_conv_supported(x, w, 1, 1, 1, 1)
