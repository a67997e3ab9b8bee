"""The 1x1 convolutions' weight-gradient family (csrc/pwwgrad.hip, csrc/pw_geom.h) as far as it can be checked without a
GPU: the C-ABI's argument validation, the slicing queries, the host plan under ASan + UBSan (tests/pw_geom_check.cpp, a
stand-alone program run as a child process) and the routing switch of torchseg_amd.pwconv.pointwise_wgrad."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

E_DTYPE, E_SHAPE, E_ALIGN, E_NULL, E_WS = -1, -3, -4, -5, -6

# (Cin, Cout, B, H, W, stride)
SUPPORTED = [(64, 64, 1, 1, 1, 1), (64, 128, 2, 5, 7, 1), (128, 64, 1, 9, 9, 2), (64, 64, 2, 8, 6, 2), (192, 320, 1, 6, 6, 1),
             (2048, 512, 1, 3, 3, 1), (512, 2048, 1, 3, 3, 1), (64, 64, 4, 64, 64, 1), (256, 64, 2, 46, 45, 2),
             (64, 128, 16, 256, 256, 2), (128, 128, 16, 128, 128, 1), (256, 256, 16, 128, 128, 1), (2048, 512, 2, 32, 32, 1),
             (1024, 512, 2, 64, 64, 1), (256, 64, 2, 256, 256, 1), (1024, 2048, 2, 129, 129, 2), (64, 64, 1, 4096, 8191, 1),
             (2048, 2048, 1, 1, 1, 1), (64, 64, 1, 1, 257, 1), (64, 64, 1031, 1, 1, 2)]
UNSUPPORTED = [(72, 64, 1, 8, 8, 1), (64, 72, 1, 8, 8, 1), (32, 64, 1, 8, 8, 1), (64, 4096, 1, 8, 8, 1), (64, 64, 1, 8, 8, 3),
               (64, 64, 1, 8, 8, 0), (64, 64, 0, 8, 8, 1), (64, 64, 1, 0, 8, 1), (64, 64, 1, 8, 0, 1), (64, 64, 1, 4096, 8192, 1),
               (64, 128, 1, 4096, 4096, 1), (64, 64, 2 ** 40, 8, 8, 1)]


def _lib():
    from torchseg_amd import _lib
    return _lib, _lib.lib()


def test_abi_and_argument_validation_without_gpu():
    L, lib = _lib()
    for name in ("tsg_pw_wgrad_supported", "tsg_pw_wgrad_slices", "tsg_pw_wgrad_ws_bytes", "tsg_pw_wgrad"):
        assert name in L._PROTOS, name
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name), name
    C = ctypes
    assert L._PROTOS["tsg_pw_wgrad_supported"] == (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int])
    assert L._PROTOS["tsg_pw_wgrad_slices"] == (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int])
    assert L._PROTOS["tsg_pw_wgrad_ws_bytes"] == (C.c_size_t, [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int])
    assert L._PROTOS["tsg_pw_wgrad"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int64] + [C.c_int] * 5
                                         + [C.c_void_p, C.c_size_t, C.c_void_p])

    assert lib.tsg_pw_wgrad_supported(L.BF16, 256, 64, 2, 46, 45, 2) == 1
    assert lib.tsg_pw_wgrad_supported(L.F32, 256, 64, 2, 46, 45, 2) == 0
    assert lib.tsg_pw_wgrad_supported(L.BF16, 72, 64, 2, 46, 45, 2) == 0
    assert lib.tsg_pw_wgrad_supported(L.BF16, 256, 64, 2, 46, 45, 3) == 0
    assert lib.tsg_pw_wgrad_supported(L.BF16, 256, 64, 0, 46, 45, 2) == 0

    # never dereferenced: every call below is refused before any launch.  A shape with several slices, so that the
    # workspace arguments are looked at: (B, Cin, Cout, H, W, stride) = (2, 256, 64, 46, 45, 2)
    X, DY, DW, WS = 0x10000, 0x20000, 0x30000, 0x40000
    geo = (2, 46, 45, 256, 64, 2)                       # B, H, W, Cin, Cout, stride as tsg_pw_wgrad takes them
    S = lib.tsg_pw_wgrad_slices(256, 64, 2, 46, 45, 2)
    wsb = lib.tsg_pw_wgrad_ws_bytes(256, 64, 2, 46, 45, 2)
    assert S >= 2 and wsb == S * 64 * 256 * 4

    def call(x=X, dy=DY, dw=DW, dtype=L.BF16, geo=geo, ws=WS, ws_bytes=wsb):
        return lib.tsg_pw_wgrad(x, dy, dw, dtype, *geo, ws, ws_bytes, None)

    assert call(geo=(2, 46, 45, 72, 64, 2)) == E_SHAPE                  # C_in = 72
    assert call(geo=(2, 46, 45, 256, 64, 3)) == E_SHAPE                 # stride 3
    assert call(geo=(0, 46, 45, 256, 64, 2)) == E_SHAPE                 # P = 0
    assert call(geo=(2, 0, 45, 256, 64, 2)) == E_SHAPE
    assert call(dtype=L.F32) == E_DTYPE
    assert call(dtype=7) == E_DTYPE
    assert call(x=None) == E_NULL and call(dy=None) == E_NULL and call(dw=None) == E_NULL
    assert call(ws=None) == E_NULL                                       # several slices need a workspace
    assert call(x=X + 8) == E_ALIGN and call(dy=DY + 2) == E_ALIGN and call(dw=DW + 4) == E_ALIGN
    assert call(ws=WS + 8) == E_ALIGN
    assert call(ws_bytes=wsb - 1) == E_WS
    assert call(ws_bytes=0) == E_WS


def test_slicing_queries():
    _, lib = _lib()
    multi = 0
    for (Cin, Cout, B, H, W, st) in SUPPORTED:
        a = (Cin, Cout, B, H, W, st)
        assert lib.tsg_pw_wgrad_supported(1, *a) == 1, a
        S = lib.tsg_pw_wgrad_slices(*a)
        ws = lib.tsg_pw_wgrad_ws_bytes(*a)
        assert S >= 1, a
        assert ws == (S * Cout * Cin * 4 if S > 1 else 0), (a, S, ws)
        P = B * ((H - 1) // st + 1) * ((W - 1) // st + 1)
        assert S <= P, (a, S)                                            # no slice without a pixel
        for _ in range(3):                                               # a function of the shape alone
            assert lib.tsg_pw_wgrad_slices(*a) == S and lib.tsg_pw_wgrad_ws_bytes(*a) == ws
        multi += S > 1
    assert multi >= 5
    # the same C_in, C_out and pixel count give the same S however the pixels are arranged
    assert lib.tsg_pw_wgrad_slices(64, 64, 4, 64, 64, 1) == lib.tsg_pw_wgrad_slices(64, 64, 1, 128, 128, 1) \
        == lib.tsg_pw_wgrad_slices(64, 64, 1, 256, 256, 2)
    for a in UNSUPPORTED:
        assert lib.tsg_pw_wgrad_supported(1, *a) == 0, a
        assert lib.tsg_pw_wgrad_slices(*a) == 0 and lib.tsg_pw_wgrad_ws_bytes(*a) == 0, a


def test_host_plan_under_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path / "pw_geom_check"
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "pw_geom_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr


def _cpu_bmm(monkeypatch):
    """torch.bmm(..., out_dtype=) exists for HIP tensors only: on the CPU the tests put a stand-in behind that one call
    (bf16 operands widened exactly, fp32 product), so that the unchanged framework path of pointwise_wgrad can run here"""
    orig = torch.bmm

    def bmm(a, b, out_dtype=None):
        return orig(a, b) if out_dtype is None else orig(a.to(out_dtype), b.to(out_dtype))

    monkeypatch.setattr(torch, "bmm", bmm)


class _Raises:
    """a provider whose pw_wgrad* methods must not be reached"""

    def __getattr__(self, name):
        raise AssertionError("provider attribute %s touched" % name)


def test_routing_on_cpu_tensors(monkeypatch):
    from torchseg_amd import kernels, pwconv
    _cpu_bmm(monkeypatch)
    assert pwconv._HIP_WGRAD is (os.environ.get("TSG_PW_WGRAD_HIP", "0") == "1")
    g = torch.Generator().manual_seed(5)
    for stride, (H, W) in ((1, (16, 16)), (2, (17, 16))):
        x = torch.randn(2, 64, H, W, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dy = torch.randn(2, 128, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=g).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        res = {}
        for flag in (False, True):
            monkeypatch.setattr(pwconv, "_HIP_WGRAD", flag)
            # CPU operands never reach a provider, with the switch on or off
            monkeypatch.setattr(kernels, "provider", lambda: _Raises())
            res[flag] = pwconv.pointwise_wgrad(x, dy, stride)
            out = torch.full((128, 64, 1, 1), float("nan"))
            assert pwconv.pointwise_wgrad(x, dy, stride, out=out) is out
            assert torch.equal(out, res[flag])
        assert res[True].shape == (128, 64, 1, 1) and res[True].dtype == torch.float32
        assert torch.equal(res[True].view(torch.int32), res[False].view(torch.int32))
        ref = torch.nn.grad.conv2d_weight(x.double(), (128, 64, 1, 1), dy.double(), stride=stride)
        assert (res[False].double() - ref).abs().max() <= 1e-4 * ref.abs().max() + 1e-6


def test_switch_off_never_asks_the_provider(monkeypatch):
    """_HIP_WGRAD false: a provider that raises on any pw_wgrad* call is never touched, whatever the operands claim"""
    from torchseg_amd import kernels, pwconv

    class Stub:
        def pw_wgrad_supported(self, *a, **k):
            raise AssertionError("pw_wgrad_supported called with the switch off")

        def pw_wgrad(self, *a, **k):
            raise AssertionError("pw_wgrad called with the switch off")

    _cpu_bmm(monkeypatch)
    monkeypatch.setattr(kernels, "provider", lambda: Stub())
    monkeypatch.setattr(pwconv, "_HIP_WGRAD", False)
    x = torch.randn(1, 64, 16, 16).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(1, 64, 16, 16).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dw = pwconv.pointwise_wgrad(x, dy, 1)
    assert dw.shape == (64, 64, 1, 1)
    # and with the switch on the provider IS what decides: operands that report themselves as HIP tensors reach the stub
    monkeypatch.setattr(pwconv, "_HIP_WGRAD", True)

    class FakeHip:
        is_cuda = True

    with pytest.raises(AssertionError, match="pw_wgrad_supported called"):
        pwconv.pointwise_wgrad(FakeHip(), FakeHip(), 1)
