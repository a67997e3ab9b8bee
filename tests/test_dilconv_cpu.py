"""CPU side of the dilated 3x3 convolutions (csrc/dilconv.hip, torchseg_amd/dilconv.py): the shape predicate of the C-ABI,
the installer's selection and its pass-through on the CPU, the count of layers it finds in PSPNet-R50, and the build-time
guards on the generated gfx950 ISA (no GPU needed: hipcc cross-compiles)."""
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BF16, F32 = 1, 0


def test_supported_table():
    from torchseg_amd import _lib as L
    sup = L.lib().tsg_conv3x3_dil_supported
    # (dtype, Cin, Cout, kh, kw, stride, pad, dilation, groups)
    for cin, cout, d in [(256, 256, 2), (512, 512, 2), (512, 512, 4), (16, 64, 2)]:
        assert sup(BF16, cin, cout, 3, 3, 1, d, d, 1) == 1, (cin, cout, d)
    no = {
        "dilation 1": (BF16, 256, 256, 3, 3, 1, 1, 1, 1),
        "stride 2": (BF16, 256, 256, 3, 3, 2, 2, 2, 1),
        "pad != dilation": (BF16, 256, 256, 3, 3, 1, 1, 2, 1),
        "pad != dilation (4)": (BF16, 256, 256, 3, 3, 1, 2, 4, 1),
        "groups": (BF16, 256, 256, 3, 3, 1, 2, 2, 2),
        "Cin 24": (BF16, 24, 64, 3, 3, 1, 2, 2, 1),
        "Cout 96": (BF16, 64, 96, 3, 3, 1, 2, 2, 1),
        "fp32": (F32, 256, 256, 3, 3, 1, 2, 2, 1),
        "1x1": (BF16, 256, 256, 1, 1, 1, 2, 2, 1),
        "5x5": (BF16, 256, 256, 5, 5, 1, 2, 2, 1),
        "dilation 3": (BF16, 256, 256, 3, 3, 1, 3, 3, 1),
    }
    for why, args in no.items():
        assert sup(*args) == 0, why


def test_installer_selects_only_the_eligible_layers_and_passes_through_on_cpu():
    from torchseg_amd.dilconv import DilatedConv2d, install_dilated_conv
    torch.manual_seed(0)
    net = nn.Sequential(
        nn.Conv2d(64, 64, 3, 1, 2, dilation=2, bias=False),      # -> DilatedConv2d
        nn.Conv2d(64, 128, 3, 1, 4, dilation=4, bias=False),     # -> DilatedConv2d
        nn.Conv2d(128, 64, 3, 1, 2, dilation=2, bias=True),      # biased            -> untouched
        nn.Conv2d(64, 64, 3, 1, 1, dilation=2, bias=False),      # pad != dilation   -> untouched
        nn.Conv2d(64, 64, 3, 1, 1, bias=False),                  # dilation 1        -> untouched
        nn.Conv2d(64, 96, 3, 1, 2, dilation=2, bias=False),      # C_out % 64        -> untouched
        nn.Conv2d(96, 64, 3, 2, 2, dilation=2, bias=False),      # stride 2          -> untouched
    )
    ref = [m.weight.detach().clone() for m in net]
    keys = list(net.state_dict().keys())
    assert install_dilated_conv(net) == 2
    assert [type(m) is DilatedConv2d for m in net] == [True, True, False, False, False, False, False]
    assert all(type(m) is nn.Conv2d for m in list(net)[2:])
    assert list(net.state_dict().keys()) == keys
    assert all(torch.equal(m.weight, r) for m, r in zip(net, ref))
    assert install_dilated_conv(net) == 0                         # idempotent: nothing left to re-class
    # on the CPU a re-classed layer is nn.Conv2d, bit for bit, forward and backward
    for m in list(net)[:2]:
        xi = torch.randn(2, m.in_channels, 9, 11, requires_grad=True)
        y = m(xi)
        dy = torch.randn_like(y)
        y.backward(dy)
        xr = xi.detach().clone().requires_grad_(True)
        wr = m.weight.detach().clone().requires_grad_(True)
        yr = F.conv2d(xr, wr, None, 1, m.padding, m.dilation)
        yr.backward(dy)
        assert torch.equal(y, yr) and torch.equal(xi.grad, xr.grad) and torch.equal(m.weight.grad, wr.grad)


def test_pspnet_r50_dilated_layers_are_all_found():
    from torchseg_amd.dilconv import DilatedConv2d, install_dilated_conv
    from torchseg_amd.workloads import ensure_furnace_on_path
    ensure_furnace_on_path()
    from torchseg_amd.workloads.pspnet import PSPNet
    net = PSPNet(19, nn.CrossEntropyLoss(ignore_index=255), depth=50)
    want = sum(1 for m in net.modules()
               if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and max(m.dilation) > 1)
    assert want >= 8, want
    keys = list(net.state_dict().keys())
    assert install_dilated_conv(net) == want
    assert sum(1 for m in net.modules() if type(m) is DilatedConv2d) == want
    assert list(net.state_dict().keys()) == keys
    # convwrw still calls them "not ours"; exactconv (the fp32 parity mode) still recognises the re-classed module
    from torchseg_amd import exactconv
    from torchseg_amd.convwrw import install_conv_wrw, WrwConv2d
    install_conv_wrw(net)
    assert not any(type(m) is WrwConv2d and max(m.dilation) > 1 for m in net.modules())
    n_conv = sum(1 for m in net.modules() if isinstance(m, nn.Conv2d))
    assert exactconv.install(net) == n_conv
    assert sum(1 for m in net.modules() if isinstance(m, DilatedConv2d)) == want
    exactconv.uninstall(net)
    assert sum(1 for m in net.modules() if type(m) is DilatedConv2d) == want


def test_install_kernels_switch(monkeypatch):
    """ddp.install_kernels re-classes the dilated layers under TSG_CONV_DIL=1 only, and never a plain layer."""
    from torchseg_amd import ddp
    from torchseg_amd.dilconv import DilatedConv2d

    def net():
        return nn.Sequential(nn.Conv2d(64, 64, 3, 1, 2, dilation=2, bias=False), nn.Conv2d(64, 64, 3, 1, 1, bias=False))
    for value, want in (("0", 0), ("1", 1)):
        monkeypatch.setenv("TSG_CONV_DIL", value)
        m = net()
        ddp.install_kernels(m, torch.bfloat16)
        assert sum(type(c) is DilatedConv2d for c in m) == want, value
        assert type(m[1]) is not DilatedConv2d
    monkeypatch.delenv("TSG_CONV_DIL")
    m = net()
    ddp.install_kernels(m, torch.bfloat16)
    assert sum(type(c) is DilatedConv2d for c in m) == 0             # opt-in: DESIGN.md 4.4


# ---- build-time guards on the generated ISA (the style of test_isa_guards_cpu.py) ----
@pytest.fixture(scope="module")
def dil_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "dilconv.hip.s"
    cmd = [HIPCC, "-x", "hip", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-gpu-rdc", "-ffp-contract=off",
           "--cuda-device-only", "-S", os.path.join(ROOT, "torchseg_amd", "csrc", "dilconv.hip"),
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


def test_dilated_mfma_kernels_do_not_spill(dil_isa):
    ks = _kernels(dil_isa)
    mfma = {n: v for n, v in ks.items() if "v_mfma_f32_32x32x16_bf16" in v[3]}
    fwd = [n for n in mfma if "dil3_fwd_k" in n]
    wrw = [n for n in mfma if "dil3_wrw_k" in n]
    assert len(fwd) == 4 and len(wrw) == 2, sorted(ks)         # d = 2 / 4, with / without statistics; d = 2 / 4
    for n, (spill, scratch, vgpr, _) in mfma.items():
        assert spill == 0 and scratch == 0, (n, spill, scratch)
    for n in fwd:                                                # two blocks of 256 threads per CU
        assert mfma[n][2] <= 256, (n, mfma[n][2])
    for n in wrw:                                                # one block per CU
        assert mfma[n][2] <= 512, (n, mfma[n][2])


def test_dilated_forward_stages_the_filter_by_lds_dma(dil_isa):
    ks = _kernels(dil_isa)
    for n, (_, _, _, body) in ks.items():
        if "dil3_fwd_k" in n:
            assert re.search(r"global_load_lds_dwordx4|global_load_dwordx4 .* lds|buffer_load_dwordx4 .* lds", body), n
