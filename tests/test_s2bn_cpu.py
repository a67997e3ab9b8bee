"""The fused stride-2 3x3 convolution + BatchNorm (+ residual) (+ ReLU) of inference (csrc/s2bn.hip, the `strided=True` side
of torchseg_amd/convbn.py) as far as it can be checked without a GPU: the C-ABI's support predicate, plan query and
argument-validation order, the host plan under sanitizers (tests/s2b_geom_check.cpp), that the kernel neither spills nor
uses scratch and fits two blocks per compute unit, the installer's counts (fresh, upgrade of a plain install, `plain=False`,
a second call) on BiSeNet-R18, ResNet-50 and a Bottleneck net, what is and is not a stride-2 3x3, that every call the fused
kernel cannot take (CPU input in eval mode, train mode, gradients enabled) is bit for bit the stock network, and the
switch's default."""
import copy
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from test_convbn_cpu import HIPCC, _BottleneckNet, _r18, _randomise_bn
from test_isa_guards_cpu import _isa, _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

# (B, H, W, C_in, C_out), H and W of the INPUT: the GPU test's shapes (tests/test_s2bn_gpu.py says what each one catches)
GPU_CASES = [(1, 1, 3, 16, 64), (1, 5, 7, 16, 64), (1, 6, 8, 16, 64), (2, 16, 64, 32, 64), (1, 17, 66, 48, 128),
             (1, 34, 79, 64, 192), (1, 143, 511, 16, 512)]
# the stride-2 layers of BiSeNet-R18 (detail branch, layer2 / 3 / 4) and of ResNet-50 at 768 x 1536
LAYERS = [(1, 384, 768, 64, 64), (1, 192, 384, 64, 64), (1, 192, 384, 64, 128), (1, 96, 192, 128, 256),
          (1, 48, 96, 256, 512), (1, 192, 384, 128, 128), (1, 96, 192, 256, 256), (1, 48, 96, 512, 512)]
LDS = 74304


def test_support_predicate_plan_and_null_pointers():
    from torchseg_amd import _lib
    lib = _lib.lib()
    plan = (ctypes.c_int * 7)()
    for B, H, W, Cin, Cout in GPU_CASES + LAYERS:
        assert lib.tsg_conv3x3_s2_bnact_supported(_lib.BF16, B, H, W, Cin, Cout) == 1
        assert lib.tsg_conv3x3_s2_bnact_supported(_lib.F32, B, H, W, Cin, Cout) == 0       # the parity mode is not ours
        assert lib.tsg_conv3x3_s2_bnact_supported(7, B, H, W, Cin, Cout) == 0
        assert lib.tsg_conv3x3_s2_bnact_plan(B, H, W, Cin, Cout, plan) == 0
        OH, OW, ntiles, nslots, noct, grid, lds = plan
        assert (OH, OW) == ((H + 1) // 2, (W + 1) // 2)
        assert (OH, OW) == ((H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1)                     # torch's formula for 3 / 2 / 1
        assert ntiles == B * ((OH + 3) // 4) * ((OW + 31) // 32) and noct == Cout // 64     # tiles over the OUTPUT
        assert nslots % 8 == 0 and nslots >= 8 and grid == nslots * noct
        assert lds == LDS and 2 * lds <= 160 * 1024
    assert lib.tsg_conv3x3_s2_bnact_supported(_lib.BF16, 1, 17, 66, 24, 64) == 0
    assert lib.tsg_conv3x3_s2_bnact_supported(_lib.BF16, 1, 17, 66, 16, 96) == 0
    assert lib.tsg_conv3x3_s2_bnact_supported(_lib.BF16, 0, 17, 66, 16, 64) == 0
    assert lib.tsg_conv3x3_s2_bnact_supported(_lib.BF16, 1, 0, 66, 16, 64) == 0
    assert lib.tsg_conv3x3_s2_bnact_supported(_lib.BF16, 1, 17, 0, 16, 64) == 0
    assert lib.tsg_conv3x3_s2_bnact_supported(_lib.BF16, 1, 17, 66, 0, 64) == 0
    assert lib.tsg_conv3x3_s2_bnact_supported(_lib.BF16, 1, 17, 66, 16, 0) == 0
    assert lib.tsg_conv3x3_s2_bnact_supported(_lib.BF16, 1, 8192, 8192, 16, 64) == 1       # 2^30 elements of x and of y
    assert lib.tsg_conv3x3_s2_bnact_supported(_lib.BF16, 1, 16384, 8192, 16, 64) == 0      # 2^31 elements per image of x
    assert lib.tsg_conv3x3_s2_bnact_supported(_lib.BF16, 1, 8192, 8192, 16, 128) == 0      # 2^31 elements per image of y
    assert lib.tsg_conv3x3_s2_bnact_plan(1, 17, 66, 24, 64, plan) == -3                     # TSG_E_SHAPE
    assert lib.tsg_conv3x3_s2_bnact_plan(1, 17, 66, 16, 64, None) == -5                     # TSG_E_NULL
    assert lib.tsg_conv3x3_s2_bnact_plan(1, 17, 66, 24, 64, None) == -5                     # null before shape
    # null pointers, then the shape, then the alignment: all before any launch
    for args in ((None, 16, 16, None, 16), (16, None, 16, None, 16), (16, 16, None, None, 16), (16, 16, 16, None, None)):
        assert lib.tsg_conv3x3_s2_bnact_fwd(*args, 1, 17, 66, 16, 64, 1, None) == -5
        assert lib.tsg_conv3x3_s2_bnact_fwd(*args, 1, 17, 66, 24, 64, 1, None) == -5        # null before shape
    assert lib.tsg_conv3x3_s2_bnact_fwd(16, 16, 16, None, 16, 1, 17, 66, 24, 64, 1, None) == -3
    assert lib.tsg_conv3x3_s2_bnact_fwd(16, 16, 16, None, 16, 1, 17, 66, 16, 96, 1, None) == -3
    assert lib.tsg_conv3x3_s2_bnact_fwd(16, 16, 16, None, 16, 0, 17, 66, 16, 64, 1, None) == -3
    assert lib.tsg_conv3x3_s2_bnact_fwd(16, 16, 16, None, 16, 1, 16384, 8192, 16, 64, 1, None) == -3
    assert lib.tsg_conv3x3_s2_bnact_fwd(16, 16, 16, None, 24, 1, 17, 66, 24, 64, 1, None) == -3   # shape before alignment
    assert lib.tsg_conv3x3_s2_bnact_fwd(16, 16, 16, None, 24, 1, 17, 66, 16, 64, 1, None) == -4   # TSG_E_ALIGN
    assert lib.tsg_conv3x3_s2_bnact_fwd(16, 16, 16, 8, 16, 1, 17, 66, 16, 64, 1, None) == -4
    assert lib.tsg_conv3x3_s2_bnact_fwd(16, 16, 4, None, 16, 1, 17, 66, 16, 64, 1, None) == -4
    assert lib.tsg_conv3x3_s2_bnact_fwd(16, 24, 16, None, 16, 1, 17, 66, 16, 64, 1, None) == -4
    assert lib.tsg_conv3x3_s2_bnact_fwd(24, 16, 16, None, 16, 1, 17, 66, 16, 64, 1, None) == -4


def test_plan_walks_more_than_one_tile_only_in_the_largest_case():
    from torchseg_amd import kernels as K
    kp = K.provider()
    OH, OW, ntiles, nslots, noct, grid, lds = kp.conv3x3_s2_bnact_plan(*GPU_CASES[-1])
    assert (OH, OW, noct) == (72, 256, 8) and ntiles > nslots
    for case in GPU_CASES[:-1]:
        _, _, ntiles, nslots, _, _, _ = kp.conv3x3_s2_bnact_plan(*case)
        assert ntiles <= nslots


def test_provider_twins_check_their_arguments():
    from torchseg_amd import _lib, kernels as K
    kp = K.provider()
    assert kp.conv3x3_s2_bnact_plan(1, 17, 66, 48, 128)[:2] == (9, 33)
    with pytest.raises(_lib.TsgError):
        kp.conv3x3_s2_bnact_plan(1, 17, 66, 24, 128)
    x = torch.zeros(1, 16, 17, 66, dtype=torch.bfloat16)
    assert not kp.conv3x3_s2_bnact_supported(x, 64)                                     # NCHW
    xc = x.contiguous(memory_format=torch.channels_last)
    assert kp.conv3x3_s2_bnact_supported(xc, 64)
    assert not kp.conv3x3_s2_bnact_supported(xc.float(), 64) and not kp.conv3x3_s2_bnact_supported(xc, 96)
    wf, ab = torch.zeros(9 * 16 * 64, dtype=torch.bfloat16), torch.zeros(2, 64)
    with pytest.raises(_lib.TsgError, match="pack"):
        kp.conv3x3_s2_bnact_fwd(xc, (wf[:-16], ab), 64, None, True)
    with pytest.raises(_lib.TsgError, match="pack"):
        kp.conv3x3_s2_bnact_fwd(xc, (wf, ab[:1]), 64, None, True)
    with pytest.raises(_lib.TsgError, match="residual"):                                # the INPUT's shape is not the output's
        kp.conv3x3_s2_bnact_fwd(xc, (wf, ab), 64, torch.zeros(1, 64, 17, 66, dtype=torch.bfloat16), True)
    with pytest.raises(_lib.TsgError, match="residual"):                                # NCHW
        kp.conv3x3_s2_bnact_fwd(xc, (wf, ab), 64, torch.zeros(1, 64, 9, 33, dtype=torch.bfloat16), True)


def test_host_plan_under_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path / "s2b_geom_check"
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "s2b_geom_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr


def test_kernel_does_not_spill_and_fits_two_blocks_per_cu(tmp_path_factory):
    """One kernel; no scratch, no spills; at most 256 VGPRs + AGPRs (two 4-wave blocks on a CU's four SIMDs are two waves per
    SIMD of a 512 register file); twice the block's LDS inside the CU's 160 KB; one unrolled chunk of 9 taps x 2 channel
    blocks = 18 MFMAs; no atomics."""
    from torchseg_amd import _lib
    isa = _isa(tmp_path_factory, "s2bn.hip")
    meta = _kernel_meta(isa)
    assert len(meta) == 1 and "s2b_fwd_k" in next(iter(meta)), sorted(meta)
    for name, (spill, scratch) in meta.items():
        assert spill == 0 and scratch == 0, (name, spill, scratch)
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", isa)]
    agprs = [int(v) for v in re.findall(r"\.agpr_count:\s+(\d+)", isa)]
    assert len(vgprs) == 1 and len(agprs) == 1 and vgprs[0] + agprs[0] <= 256, (vgprs, agprs)
    plan = (ctypes.c_int * 7)()
    assert _lib.lib().tsg_conv3x3_s2_bnact_plan(1, 143, 511, 16, 512, plan) == 0
    assert plan[6] == LDS and 2 * plan[6] <= 160 * 1024
    name = next(iter(meta))
    body = isa[isa.index("\n" + name + ":"):].split("s_endpgm")[0]
    assert len(re.findall(r"\n\s*v_mfma_f32_32x32x16_bf16", body)) == 18
    assert "global_atomic" not in body and "buffer_atomic" not in body and "flat_atomic" not in body


def _r50(seed=0):
    from base_model.resnet import resnet50
    torch.manual_seed(seed)
    return _randomise_bn(resnet50(None, norm_layer=nn.BatchNorm2d), seed + 1)


def test_installer_counts_upgrade_and_state_dict():
    from torchseg_amd.convbn import (_FusedBasicBlock, _FusedBottleneck, _FusedCbr, _FusedConvBn, eligible_layers,
                                     eligible_strided_layers, fused_calls, install_fused_convbn, s2_fused_calls)
    from torchseg_amd.pwbn import _FusedPointwise, install_fused_pointwise
    net = _r18()
    keys = list(net.state_dict().keys())
    s2 = [cb for m in net.modules() for cb in eligible_strided_layers(m)]
    assert sorted((c.in_channels, c.out_channels) for c, _ in s2) == [(64, 64), (64, 64), (64, 128), (128, 256), (256, 512)]
    assert sum(len(eligible_layers(m)[1]) for m in net.modules()) == 20                 # the default selection is what it was
    assert sum(len(eligible_layers(m, strided=True)[1]) for m in net.modules()) == 25

    def flagged(n):
        return [m for m in n.modules() if isinstance(m, _FusedConvBn) and m.tsg_cbn_strided]

    fresh = copy.deepcopy(net)                              # fresh net, strided=True: 25, then 0
    assert install_fused_convbn(fresh, strided=True) == 25
    assert install_fused_convbn(fresh, strided=True) == 0 and install_fused_convbn(fresh) == 0
    assert install_fused_convbn(fresh, strided=True, plain=False) == 0
    kinds = [type(m).__mro__[1] for m in fresh.modules() if isinstance(m, _FusedConvBn)]
    assert kinds.count(_FusedBasicBlock) == 8 and kinds.count(_FusedCbr) == 9 and kinds.count(_FusedBottleneck) == 0
    assert list(fresh.state_dict().keys()) == keys and fused_calls(fresh) == 0 and s2_fused_calls(fresh) == 0

    two = copy.deepcopy(net)                                # a plain install, then the upgrade: 20, 5, 0
    assert install_fused_convbn(two) == 20 and not flagged(two)
    assert install_fused_convbn(two) == 0
    assert install_fused_convbn(two, strided=True, plain=False) == 5
    assert len(flagged(two)) == 5                           # three upgraded blocks, two newly re-classed ConvBnRelu
    assert all(eligible_strided_layers(m) for m in flagged(two))
    assert sum(isinstance(m, _FusedConvBn) for m in two.modules()) == 15 + 2
    assert install_fused_convbn(two, strided=True, plain=False) == 0 and install_fused_convbn(two, strided=True) == 0
    assert list(two.state_dict().keys()) == keys

    only = copy.deepcopy(net)                               # fresh, plain=False: two ConvBnRelu + three blocks of two layers
    assert install_fused_convbn(only, strided=True, plain=False) == 8
    assert sum(isinstance(m, _FusedConvBn) for m in only.modules()) == 5 and len(flagged(only)) == 5
    assert install_fused_convbn(only, strided=True, plain=False) == 0
    assert install_fused_convbn(only) == 17 and len(flagged(only)) == 5                 # the rest (20 - 3 conv2), plain
    assert list(only.state_dict().keys()) == keys

    assert install_fused_convbn(copy.deepcopy(net), plain=False) == 0                   # nothing without a keyword
    assert install_fused_convbn(copy.deepcopy(net), dilated=True, plain=False) == 0

    # ResNet-50: layer{2,3,4}.0.conv2; 13 plain Bottlenecks
    r50 = _r50()
    keys50 = list(r50.state_dict().keys())
    assert len([cb for m in r50.modules() for cb in eligible_strided_layers(m)]) == 3
    a = copy.deepcopy(r50)
    assert install_fused_convbn(a, strided=True, plain=False) == 3 and len(flagged(a)) == 3
    assert all(isinstance(m, _FusedBottleneck) for m in flagged(a))
    b = copy.deepcopy(r50)
    assert install_fused_convbn(b) == 13 and install_fused_convbn(b, strided=True, plain=False) == 3
    assert install_fused_convbn(copy.deepcopy(r50), strided=True) == 16
    assert list(a.state_dict().keys()) == keys50 and list(b.state_dict().keys()) == keys50

    # a stride-2 Bottleneck net, with pwbn's mixin in either order and as an upgrade behind it
    bott = _BottleneckNet()
    keysb = list(bott.state_dict().keys())
    assert install_fused_convbn(copy.deepcopy(bott)) == 1
    c = copy.deepcopy(bott)
    assert install_fused_convbn(c, strided=True, plain=False) == 1 and isinstance(c.b0, _FusedBottleneck)
    assert c.b0.tsg_cbn_strided and not isinstance(c.b1, _FusedConvBn)
    install_fused_pointwise(c)
    assert issubclass(type(c.b0).__mro__[1], _FusedPointwise) and isinstance(c.b0, _FusedConvBn) and c.b0.tsg_cbn_strided
    d = copy.deepcopy(bott)
    install_fused_pointwise(d)
    assert install_fused_convbn(d, strided=True, plain=False) == 1
    assert issubclass(type(d.b0).__mro__[1], _FusedPointwise) and isinstance(d.b0, _FusedConvBn) and d.b0.tsg_cbn_strided
    assert list(c.state_dict().keys()) == keysb and list(d.state_dict().keys()) == keysb
    # the upgrade behind pwbn's mixin: a BasicBlock re-classed by a plain install, then pwbn, then strided
    from base_model.resnet import BasicBlock, _shortcut
    blk = BasicBlock(64, 128, 2, nn.BatchNorm2d, downsample=_shortcut(64, 128, 2, nn.BatchNorm2d, 1e-5, 0.1))
    assert install_fused_convbn(blk) == 1 and install_fused_pointwise(blk) == 1
    cls = type(blk)
    assert install_fused_convbn(blk, strided=True, plain=False) == 1 and type(blk) is cls and blk.tsg_cbn_strided
    assert copy.deepcopy(blk).tsg_cbn_strided                                           # the flag travels with a copy


def test_what_is_and_is_not_a_stride2_3x3():
    """test_convbn_cpu's pile rebuilt: without `strided` its stride-2 ConvBnRelu stays un-re-classed, with it that one is
    taken; stride 2 with dilation 2, grouped, 24-channel, hooked, BatchNorm-less and 1x1 layers never are."""
    from seg_opr.seg_oprs import ConvBnRelu
    from torchseg_amd.convbn import _FusedCbr, fused_calls, install_fused_convbn

    def pile():
        torch.manual_seed(0)
        hooked = ConvBnRelu(16, 64, 3, 2, 1)
        hooked.bn.register_forward_hook(lambda *a: None)
        return nn.Sequential(ConvBnRelu(16, 64, 3, 1, 1, has_bias=True), ConvBnRelu(64, 64, 3, 2, 1),
                             ConvBnRelu(64, 64, 3, 1, 2, dilation=2), ConvBnRelu(64, 64, 1, 1, 0),
                             ConvBnRelu(64, 64, 3, 1, 1, groups=2), ConvBnRelu(24, 64, 3, 1, 1),
                             ConvBnRelu(64, 64, 3, 1, 1, has_bn=False), hooked, ConvBnRelu(64, 128, 3, 1, 1, has_relu=False),
                             ConvBnRelu(64, 64, 3, 2, 2, dilation=2), ConvBnRelu(64, 64, 3, 2, 1, groups=2),
                             ConvBnRelu(24, 64, 3, 2, 1), ConvBnRelu(64, 96, 3, 2, 1), ConvBnRelu(64, 64, 3, 2, 0),
                             ConvBnRelu(64, 64, 3, (2, 1), 1), ConvBnRelu(64, 64, 1, 2, 0), ConvBnRelu(64, 64, 3, 2, 1, has_bn=False),
                             ConvBnRelu(16, 128, 3, 2, 1, has_bias=True, has_relu=False))
    plain = pile()
    assert install_fused_convbn(plain) == 2
    assert [isinstance(m, _FusedCbr) for m in plain] == [True] + [False] * 7 + [True] + [False] * 9
    assert install_fused_convbn(copy.deepcopy(plain), dilated=True, plain=False) == 1    # the dilated install: no stride-2 layer
    assert install_fused_convbn(pile(), plain=False) == 0
    only = pile()
    assert install_fused_convbn(only, strided=True, plain=False) == 2
    assert [isinstance(m, _FusedCbr) for m in only] == [False, True] + [False] * 15 + [True]
    both = pile()
    assert install_fused_convbn(both, strided=True) == 4
    assert [isinstance(m, _FusedCbr) for m in both] == [True, True] + [False] * 6 + [True] + [False] * 8 + [True]
    assert install_fused_convbn(both, strided=True) == 0 and install_fused_convbn(both, strided=True, plain=False) == 0
    assert install_fused_convbn(plain, strided=True, plain=False) == 2                   # after the plain install
    assert [isinstance(m, _FusedCbr) for m in plain] == [isinstance(m, _FusedCbr) for m in both]
    x = torch.randn(1, 64, 6, 5)
    both.eval()
    with torch.no_grad():
        assert torch.equal(both[1](x), ConvBnRelu.forward(both[1], x))
    fired = []
    both[1].conv.register_forward_hook(lambda *a: fired.append(1))
    with torch.no_grad():
        both[1](x)
    assert fired == [1] and fused_calls(both) == 0


class _ChainNet(nn.Module):
    """our SpatialPath (through seg_oprs.cbr_chain) in front of a stride-2 Bottleneck net"""

    def __init__(self):
        super().__init__()
        from torchseg_amd.workloads.bisenet import SpatialPath
        self.sp = SpatialPath(3, 64)
        self.net = _BottleneckNet()
        self.net.stem = nn.Conv2d(64, 64, 1, bias=False)

    def forward(self, x):
        return self.net(self.sp(x))


@pytest.mark.parametrize("which", ["r18", "bottleneck", "r18-upgrade", "chain-pointwise"])
def test_reclassed_network_is_the_stock_network_wherever_the_kernel_does_not_apply(which):
    """CPU input in eval mode, train mode, and gradients enabled (every parameter gradient too): bit-identical."""
    from torchseg_amd.convbn import fused_calls, install_fused_convbn, s2_fused_calls
    from torchseg_amd.pwbn import install_fused_pointwise
    torch.manual_seed(2)
    stock = {"r18": _r18, "r18-upgrade": _r18, "bottleneck": lambda: _randomise_bn(_BottleneckNet(), 3),
             "chain-pointwise": lambda: _randomise_bn(_ChainNet(), 4)}[which]()
    ours = copy.deepcopy(stock)
    if which == "r18":
        assert install_fused_convbn(ours, strided=True) == 25
    elif which == "r18-upgrade":
        assert install_fused_convbn(ours) == 20 and install_fused_convbn(ours, strided=True, plain=False) == 5
    elif which == "bottleneck":
        assert install_fused_convbn(ours, strided=True) == 2
    else:
        install_fused_pointwise(ours)
        assert install_fused_convbn(ours, strided=True) == 4
    assert list(ours.state_dict().keys()) == list(stock.state_dict().keys())
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, 96, generator=g)

    stock.eval(), ours.eval()
    with torch.no_grad():
        assert torch.equal(stock(x), ours(x))

    stock.train(), ours.train()
    with torch.no_grad():
        assert torch.equal(stock(x), ours(x))
    for (k, u), (_, v) in zip(stock.state_dict().items(), ours.state_dict().items()):
        assert torch.equal(u, v), k                              # the running statistics moved alike

    for mode in (True, False):                                   # gradients enabled, in train and in eval mode
        stock.train(mode), ours.train(mode)
        outs = []
        for net in (stock, ours):
            net.zero_grad(set_to_none=True)
            y = net(x)
            y.square().mean().backward()
            outs.append(y.detach())
        assert torch.equal(outs[0], outs[1])
        for (n, p), (_, q) in zip(stock.named_parameters(), ours.named_parameters()):
            assert (p.grad is None) == (q.grad is None), n
            if p.grad is not None:
                assert torch.equal(p.grad, q.grad), n
    assert fused_calls(ours) == 0 and s2_fused_calls(ours) == 0


def test_prepare_inference_switch_defaults_to_off(monkeypatch):
    """The signature carries the switch with None as its default; then TSG_S2BN_FUSED decides, and unset means off (no GPU:
    the constructor is not run here, tests/test_s2bn_gpu.py covers the effect).  The switch is documented with the others,
    and the DDP side never installs this."""
    import inspect
    from torchseg_amd import convbn, infer
    import torchseg_amd.ddp as ddp
    for fn in (infer.prepare_inference, infer.InferenceModule.__init__):
        assert inspect.signature(fn).parameters["fuse_strided"].default is None
    for fn in (convbn.install_fused_convbn, convbn.eligible_layers):
        assert inspect.signature(fn).parameters["strided"].default is False
    sig = inspect.signature(convbn.install_fused_convbn).parameters
    assert list(sig) == ["module", "dilated", "plain", "strided"] and sig["plain"].default is True
    src = inspect.getsource(infer.InferenceModule.__init__)
    assert 'ddp._env_flag("TSG_S2BN_FUSED", False)' in src
    assert "install_fused_convbn(self.module, strided=True, plain=False)" in src
    assert src.index("TSG_DILBN_FUSED") < src.index("TSG_S2BN_FUSED") < src.index("TSG_PWBN_FUSED")    # the install order
    monkeypatch.delenv("TSG_S2BN_FUSED", raising=False)
    assert ddp._env_flag("TSG_S2BN_FUSED", False) is False
    monkeypatch.setenv("TSG_S2BN_FUSED", "0")
    assert ddp._env_flag("TSG_S2BN_FUSED", False) is False
    monkeypatch.setenv("TSG_S2BN_FUSED", "1")
    assert ddp._env_flag("TSG_S2BN_FUSED", False) is True
    src = inspect.getsource(ddp)
    assert "install_fused_convbn" not in src and "strided=True" not in src
    for doc in (ddp.__doc__, infer.__doc__, convbn.__doc__):
        assert "TSG_S2BN_FUSED" in doc
        assert "stride-2 3x3 layers stay unfused" not in " ".join(doc.split())
