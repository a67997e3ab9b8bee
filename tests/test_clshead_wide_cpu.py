"""CPU side of the wide classifier convolutions (csrc/clswide.hip, TSG_CLS_HEAD_WIDE): the C ABI declares and exports the
five entry points and leaves the narrow ones alone, argument validation and the shape predicate answer without a GPU,
the switch is off by default, the installer re-classes exactly the layers it should, a provider without the wide kernels
falls back, and the generated gfx950 ISA keeps to the register plan of DESIGN.md 7.  The kernels themselves:
tests/test_clshead_wide_gpu.py."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BF16, F32 = 1, 0
E_SHAPE, E_ALIGN, E_NULL, E_WS = -3, -4, -5, -6

WIDE_PROTOS = {
    "tsg_cls_head_wide_supported": "int tsg_cls_head_wide_supported(int dtype, int Cin, int n_classes, int64_t HW);",
    "tsg_cls_head_wide_fwd": "int tsg_cls_head_wide_fwd(const void* x, const float* w, const float* bias, void* z, int64_t B, "
                             "int64_t HW, int Cin, int n_classes, void* stream);",
    "tsg_cls_head_wide_dgrad": "int tsg_cls_head_wide_dgrad(const void* dz, const float* w, void* dx, int64_t B, int64_t HW, "
                               "int Cin, int n_classes, void* stream);",
    "tsg_cls_head_wide_wgrad_ws_bytes": "size_t tsg_cls_head_wide_wgrad_ws_bytes(int64_t B, int64_t HW, int Cin, int n_classes);",
    "tsg_cls_head_wide_wgrad": "int tsg_cls_head_wide_wgrad(const void* dz, const void* x, float* dw, float* dbias, int64_t B, "
                               "int64_t HW, int Cin, int n_classes, void* ws, size_t ws_bytes, void* stream);",
}
NARROW_PROTOS = [
    "int tsg_cls_head_supported(int dtype, int Cin, int n_classes, int64_t HW);",
    "int tsg_cls_head_fwd(const void* x, const float* w, const float* bias, void* z, int64_t B, int64_t HW, int Cin, "
    "int n_classes, void* stream);",
    "int tsg_cls_head_dgrad(const void* dz, const float* w, void* dx, int64_t B, int64_t HW, int Cin, int n_classes, "
    "void* stream);",
    "size_t tsg_cls_head_wgrad_ws_bytes(int64_t B, int Cin, int n_classes);",
    "int tsg_cls_head_wgrad(const void* dz, const void* x, float* dw, float* dbias, int64_t B, int64_t HW, int Cin, "
    "int n_classes, void* ws, size_t ws_bytes, void* stream);",
]


def _header_decls():
    with open(os.path.join(ROOT, "include", "tsg_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {" ".join(d.split()) + ";" for d in text.split(";")}


def test_header_declares_the_wide_entry_points_and_keeps_the_narrow_ones():
    decls = _header_decls()
    for proto in list(WIDE_PROTOS.values()) + NARROW_PROTOS:
        assert proto in decls, proto
    from torchseg_amd import _lib
    i, i64, sz, p = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p
    assert _lib._PROTOS["tsg_cls_head_wide_supported"] == (i, [i, i, i, i64])
    assert _lib._PROTOS["tsg_cls_head_wide_fwd"] == (i, [p, p, p, p, i64, i64, i, i, p])
    assert _lib._PROTOS["tsg_cls_head_wide_dgrad"] == (i, [p, p, p, i64, i64, i, i, p])
    assert _lib._PROTOS["tsg_cls_head_wide_wgrad_ws_bytes"] == (sz, [i64, i64, i, i])
    assert _lib._PROTOS["tsg_cls_head_wide_wgrad"] == (i, [p, p, p, p, i64, i64, i, i, p, sz, p])
    assert _lib._PROTOS["tsg_cls_head_wgrad_ws_bytes"] == (sz, [i64, i, i])


def test_library_exports_the_wide_entry_points():
    from torchseg_amd import _lib
    _lib.lib()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in WIDE_PROTOS:
        assert hasattr(h, name), name


# the three real layers at 8100 (90^2), 3600 (60^2) and 256 (16^2) pixels; (Cin, n_classes)
REAL = [(512, 150), (1024, 150), (512, 21)]
REJECTS = {
    "no classes": (BF16, 512, 0, 8100),
    "257 classes": (BF16, 512, 257, 8100),
    "C_in 32": (BF16, 32, 150, 8100),
    "C_in 96": (BF16, 96, 150, 8100),
    "C_in 1088": (BF16, 1088, 150, 8100),
    "HW 6": (BF16, 512, 150, 6),
    "HW 0": (BF16, 512, 150, 0),
    "fp32": (F32, 512, 150, 8100),
}


def test_supported_table():
    from torchseg_amd import _lib
    lib = _lib.lib()
    for cin, n in REAL:
        for hw in (8100, 3600, 256):
            assert lib.tsg_cls_head_wide_supported(BF16, cin, n, hw) == 1, (cin, n, hw)
    for args in [(BF16, 64, 1, 4), (BF16, 64, 33, 96), (BF16, 256, 256, 20), (BF16, 192, 97, 4), (BF16, 1024, 256, 36),
                 (BF16, 64, 19, 16384)]:
        assert lib.tsg_cls_head_wide_supported(*args) == 1, args
    for why, args in REJECTS.items():
        assert lib.tsg_cls_head_wide_supported(*args) == 0, why
    # the narrow query is what it was
    assert lib.tsg_cls_head_supported(BF16, 64, 150, 256) == 0
    assert lib.tsg_cls_head_supported(BF16, 256, 150, 16384) == 0
    assert lib.tsg_cls_head_supported(BF16, 512, 21, 256) == 0
    assert lib.tsg_cls_head_supported(BF16, 64, 19, 16384) == 1
    assert lib.tsg_cls_head_supported(BF16, 64, 19, 8100) == 0               # HW % 16


def test_argument_validation_without_gpu():
    """every refusal comes back before a launch: the pointers are made-up addresses nothing may dereference"""
    from torchseg_amd import _lib
    lib = _lib.lib()
    A, M = 0x10000, 0x10008                                                  # 16-byte aligned / not
    B, HW, C, N = 2, 36, 512, 150
    need = lib.tsg_cls_head_wide_wgrad_ws_bytes(B, HW, C, N)
    assert need >= (N * C + B * N) * 4 and need % 4 == 0
    assert need == lib.tsg_cls_head_wide_wgrad_ws_bytes(B, HW, C, N)         # a function of the shape only

    def fwd(x=A, w=A, bias=A, z=A, B=B, HW=HW, C=C, N=N):
        return lib.tsg_cls_head_wide_fwd(x, w, bias, z, B, HW, C, N, None)

    def dgrad(dz=A, w=A, dx=A, B=B, HW=HW, C=C, N=N):
        return lib.tsg_cls_head_wide_dgrad(dz, w, dx, B, HW, C, N, None)

    def wgrad(dz=A, x=A, dw=A, db=A, B=B, HW=HW, C=C, N=N, ws=A, wsb=need):
        return lib.tsg_cls_head_wide_wgrad(dz, x, dw, db, B, HW, C, N, ws, wsb, None)

    assert fwd(x=None) == fwd(w=None) == fwd(z=None) == E_NULL
    assert dgrad(dz=None) == dgrad(w=None) == dgrad(dx=None) == E_NULL
    assert wgrad(dz=None) == wgrad(x=None) == wgrad(dw=None) == wgrad(ws=None) == E_NULL
    for call in (fwd, dgrad, wgrad):
        for bad in (dict(N=0), dict(N=257), dict(C=32), dict(C=96), dict(C=1088), dict(HW=6), dict(B=0)):
            assert call(**bad) == E_SHAPE, (call.__name__, bad)
    assert lib.tsg_cls_head_wide_wgrad_ws_bytes(B, 6, C, N) == 0
    assert wgrad(wsb=need - 1) == E_WS and wgrad(wsb=0) == E_WS
    assert fwd(x=M) == E_ALIGN and fwd(w=M) == E_ALIGN
    assert dgrad(dz=M) == E_ALIGN and dgrad(dx=M) == E_ALIGN
    assert wgrad(x=M) == E_ALIGN and wgrad(dz=M) == E_ALIGN and wgrad(ws=M) == E_ALIGN


def test_switch_is_off_by_default(monkeypatch):
    from torchseg_amd import clshead
    monkeypatch.delenv("TSG_CLS_HEAD_WIDE", raising=False)
    assert clshead.wide_enabled() is False
    monkeypatch.setenv("TSG_CLS_HEAD_WIDE", "0")
    assert clshead.wide_enabled() is False
    monkeypatch.setenv("TSG_CLS_HEAD_WIDE", "1")
    assert clshead.wide_enabled() is True


def _heads():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(64, 19, 1), nn.Conv2d(512, 150, 1), nn.Conv2d(1024, 150, 1), nn.Conv2d(512, 21, 1),
                         nn.Conv2d(171, 19, 1))


def _classes(net):
    return [type(m).__name__ for m in net]


def _same_as_conv2d(net):
    for m in net:
        x = torch.randn(2, m.in_channels, 3, 4, requires_grad=True)
        y = m(x)
        dy = torch.randn_like(y)
        y.backward(dy)
        xr = x.detach().clone().requires_grad_(True)
        wr, br = m.weight.detach().clone().requires_grad_(True), m.bias.detach().clone().requires_grad_(True)
        yr = F.conv2d(xr, wr, br)
        yr.backward(dy)
        assert torch.equal(y, yr) and torch.equal(x.grad, xr.grad), type(m).__name__
        assert torch.equal(m.weight.grad, wr.grad) and torch.equal(m.bias.grad, br.grad), type(m).__name__
        m.zero_grad()


@pytest.mark.parametrize("value", [None, "0", "1"])
def test_install_cls_head_follows_the_switch(monkeypatch, value):
    from torchseg_amd.clshead import ClsHeadConv2d, ClsHeadWideConv2d, install_cls_head
    if value is None:
        monkeypatch.delenv("TSG_CLS_HEAD_WIDE", raising=False)
    else:
        monkeypatch.setenv("TSG_CLS_HEAD_WIDE", value)
    net = _heads()
    keys = list(net.state_dict().keys())
    n = install_cls_head(net)
    if value == "1":
        assert n == 4 and _classes(net) == ["ClsHeadConv2d", "ClsHeadWideConv2d", "ClsHeadWideConv2d", "ClsHeadWideConv2d",
                                            "Conv2d"]
        assert all(type(m) is ClsHeadWideConv2d for m in list(net)[1:4])
    else:
        assert n == 1 and _classes(net) == ["ClsHeadConv2d", "Conv2d", "Conv2d", "Conv2d", "Conv2d"]
        assert all(type(m) is nn.Conv2d for m in list(net)[1:])
    assert type(net[0]) is ClsHeadConv2d and type(net[4]) is nn.Conv2d         # the 171-channel DFN layer never changes
    assert list(net.state_dict().keys()) == keys
    assert install_cls_head(net) == 0                                           # nothing left to re-class
    _same_as_conv2d(net)


def test_install_cls_head_argument_overrides_the_environment(monkeypatch):
    from torchseg_amd.clshead import install_cls_head
    monkeypatch.setenv("TSG_CLS_HEAD_WIDE", "1")
    net = _heads()
    assert install_cls_head(net, wide=False) == 1 and _classes(net)[1:] == ["Conv2d"] * 4
    monkeypatch.setenv("TSG_CLS_HEAD_WIDE", "0")
    assert install_cls_head(net, wide=True) == 3 and _classes(net)[1:4] == ["ClsHeadWideConv2d"] * 3


def test_only_biased_heads_are_taken():
    """a bias-free 1x1 layer in the range is a bottleneck convolution of the backbone, not a classifier"""
    from torchseg_amd.clshead import install_cls_head
    net = nn.Sequential(nn.Conv2d(256, 64, 1, bias=False), nn.Conv2d(1024, 256, 1, bias=False), nn.Conv2d(512, 150, 3, padding=1),
                        nn.Conv2d(512, 150, 1, stride=2), nn.Conv2d(512, 300, 1), nn.Conv2d(2048, 150, 1))
    assert install_cls_head(net, wide=True) == 0 and _classes(net) == ["Conv2d"] * 6


@pytest.mark.parametrize("value", [None, "0", "1"])
def test_install_kernels_follows_the_switch(monkeypatch, value):
    from torchseg_amd import ddp
    if value is None:
        monkeypatch.delenv("TSG_CLS_HEAD_WIDE", raising=False)
    else:
        monkeypatch.setenv("TSG_CLS_HEAD_WIDE", value)
    net = _heads()
    keys = list(net.state_dict().keys())
    ddp.install_kernels(net, torch.bfloat16)
    wide = ["ClsHeadWideConv2d"] * 3 if value == "1" else ["BiasSplitConv2d"] * 3
    assert _classes(net) == ["ClsHeadConv2d"] + wide + ["BiasSplitConv2d"]
    assert list(net.state_dict().keys()) == keys
    _same_as_conv2d(net)


def test_provider_without_the_wide_kernels_falls_back():
    """the module asks with getattr: the stand-in provider has no cls_head_wide_* and is never called; one that has the
    query is asked"""
    from _cpu_provider import OracleProvider
    from torchseg_amd import kernels as K
    from torchseg_amd.clshead import ClsHeadWideConv2d, install_cls_head

    class WithQuery(OracleProvider):
        def __init__(self, answer):
            self.asked, self.answer = [], answer

        def cls_head_wide_supported(self, x, weight):
            self.asked.append((tuple(x.shape), tuple(weight.shape)))
            return self.answer

    net = nn.Sequential(nn.Conv2d(512, 150, 1))
    assert install_cls_head(net, wide=True) == 1 and type(net[0]) is ClsHeadWideConv2d
    xb = torch.randn(1, 512, 2, 2).bfloat16().contiguous(memory_format=torch.channels_last)
    plain = OracleProvider()
    assert not hasattr(plain, "cls_head_wide_supported")
    old = K._set_provider_for_tests(plain)
    try:
        assert net[0]._supported(xb) is False
        for answer in (True, False):
            prov = WithQuery(answer)
            K._set_provider_for_tests(prov)
            assert net[0]._supported(xb) is answer and prov.asked == [((1, 512, 2, 2), (150, 512, 1, 1))]
        K._set_provider_for_tests(plain)
        y = net[0](xb.float())                                                  # and the module still computes its convolution
        assert torch.equal(y, F.conv2d(xb.float(), net[0].weight, net[0].bias))
    finally:
        K._set_provider_for_tests(old)


# ---- build-time guard on the generated ISA (the style of tests/test_dilconv_cpu.py) ----
@pytest.fixture(scope="module")
def wide_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "clswide.hip.s"
    cmd = [HIPCC, "-x", "hip", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-gpu-rdc", "-ffp-contract=off",
           "--cuda-device-only", "-S", os.path.join(ROOT, "torchseg_amd", "csrc", "clswide.hip"),
           "-I", os.path.join(ROOT, "include"), "-o", str(out)]
    subprocess.run(cmd, check=True, cwd=str(out.parent), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out.read_text()


def _kernels(isa):
    """name -> (vgpr_spill_count, private_segment_fixed_size, vgpr_count, body)"""
    meta = {}
    for block in isa.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", block)
        scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        vgpr = re.search(r"\.vgpr_count:\s+(\d+)", block)
        if name and spill and scratch and vgpr:
            meta[name.group(1)] = (int(spill.group(1)), int(scratch.group(1)), int(vgpr.group(1)))
    bodies = re.split(r"\n(_ZN3tsg\w+):", isa)
    body = {n: b.split("s_endpgm")[0] for n, b in zip(bodies[1::2], bodies[2::2])}
    return {n: v + (body.get(n, ""),) for n, v in meta.items()}


def test_wide_mfma_kernels_do_not_spill_and_keep_the_register_plan(wide_isa):
    ks = _kernels(wide_isa)
    mfma = {n: v for n, v in ks.items() if "v_mfma_f32_32x32x16_bf16" in v[3]}
    # forward and data gradient three blocks of 256 threads per CU (<= 168 registers), weight gradient two (<= 256)
    plan = {"clw_fwd_k": 168, "clw_dgrad_k": 168, "clw_wgrad_k": 256}
    assert len(mfma) == 3 and all(any(k in n for n in mfma) for k in plan), sorted(ks)
    for n, (spill, scratch, vgpr, _) in mfma.items():
        assert spill == 0 and scratch == 0, (n, spill, scratch)
        limit = next(v for k, v in plan.items() if k in n)
        assert vgpr <= limit, (n, vgpr, limit)
