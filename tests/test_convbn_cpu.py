"""The fused 3x3 convolution + BatchNorm (+ residual) (+ ReLU) of inference (csrc/convbn.hip, csrc/cbn_geom.h,
torchseg_amd/convbn.py) as far as it can be checked without a GPU: the C-ABI's support predicate, plan query and argument
validation, the host plan under ASan + UBSan (tests/cbn_geom_check.cpp, a stand-alone program run as a child process),
that the kernel does not spill, uses no scratch and fits two blocks per compute unit, the installer's counts on BiSeNet-R18
and a Bottleneck network, and that every call the fused kernel cannot take (CPU input in eval mode, train mode, gradients
enabled) is bit for bit the stock network."""
import copy
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from test_isa_guards_cpu import _isa, _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (B, H, W, C_in, C_out): the GPU test's shapes
CASES = [(1, 5, 7, 16, 64), (2, 8, 32, 32, 64), (1, 9, 33, 48, 128), (1, 17, 40, 64, 192), (1, 72, 256, 16, 512)]
# BiSeNet-R18's four backbone stages at 768 x 1536
R18_STAGES = [(1, 192, 384, 64, 64), (1, 96, 192, 128, 128), (1, 48, 96, 256, 256), (1, 24, 48, 512, 512)]


def test_support_predicate_plan_and_null_pointers():
    from torchseg_amd import _lib
    lib = _lib.lib()
    plan = (ctypes.c_int * 5)()
    for B, H, W, Cin, Cout in CASES + R18_STAGES:
        assert lib.tsg_conv3x3_bnact_supported(_lib.BF16, B, H, W, Cin, Cout) == 1
        assert lib.tsg_conv3x3_bnact_supported(_lib.F32, B, H, W, Cin, Cout) == 0          # the parity mode is not ours
        assert lib.tsg_conv3x3_bnact_supported(7, B, H, W, Cin, Cout) == 0
        assert lib.tsg_conv3x3_bnact_plan(B, H, W, Cin, Cout, plan) == 0
        ntiles, nslots, noct, grid, lds = plan
        assert ntiles == B * ((H + 7) // 8) * ((W + 31) // 32) and noct == Cout // 64
        assert nslots % 8 == 0 and nslots >= 8 and grid == nslots * noct and lds == 69504
    assert lib.tsg_conv3x3_bnact_supported(_lib.BF16, 1, 9, 33, 24, 64) == 0
    assert lib.tsg_conv3x3_bnact_supported(_lib.BF16, 1, 9, 33, 16, 96) == 0
    assert lib.tsg_conv3x3_bnact_supported(_lib.BF16, 0, 9, 33, 16, 64) == 0
    assert lib.tsg_conv3x3_bnact_supported(_lib.BF16, 1, 0, 33, 16, 64) == 0
    assert lib.tsg_conv3x3_bnact_supported(_lib.BF16, 1, 9, 0, 16, 64) == 0
    assert lib.tsg_conv3x3_bnact_supported(_lib.BF16, 1, 8192, 8192, 16, 64) == 0           # 2^32 elements per image
    assert lib.tsg_conv3x3_bnact_plan(1, 9, 33, 24, 64, plan) == -3                          # TSG_E_SHAPE
    assert lib.tsg_conv3x3_bnact_plan(1, 9, 33, 16, 64, None) == -5                          # TSG_E_NULL
    assert lib.tsg_conv3x3_bnact_row_perm(None) == -5
    # null pointers, then the shape, then the alignment: all before any launch
    for args in ((None, 16, 16, None, 16), (16, None, 16, None, 16), (16, 16, None, None, 16), (16, 16, 16, None, None)):
        assert lib.tsg_conv3x3_bnact_fwd(*args, 1, 9, 33, 16, 64, 1, None) == -5
    assert lib.tsg_conv3x3_bnact_fwd(16, 16, 16, None, 16, 1, 9, 33, 24, 64, 1, None) == -3
    assert lib.tsg_conv3x3_bnact_fwd(16, 16, 16, None, 16, 1, 9, 33, 16, 96, 1, None) == -3
    assert lib.tsg_conv3x3_bnact_fwd(16, 16, 16, None, 24, 1, 9, 33, 16, 64, 1, None) == -4   # TSG_E_ALIGN
    assert lib.tsg_conv3x3_bnact_fwd(16, 16, 16, 8, 16, 1, 9, 33, 16, 64, 1, None) == -4
    assert lib.tsg_conv3x3_bnact_fwd(16, 16, 4, None, 16, 1, 9, 33, 16, 64, 1, None) == -4


def test_row_permutation_is_the_accumulator_order():
    """perm[q] = the weight's output channel (within a group of 64) that goes to packed row q; register r of lane half h of
    a 32-row MFMA tile is row (r & 3) + 8 (r >> 2) + 4 h, and must be channel 16 h + r of the tile"""
    from torchseg_amd import _lib
    perm = (ctypes.c_int * 64)()
    assert _lib.lib().tsg_conv3x3_bnact_row_perm(perm) == 0
    perm = list(perm)
    assert sorted(perm) == list(range(64))
    for t in range(2):
        for h in range(2):
            for r in range(16):
                assert perm[32 * t + (r & 3) + 8 * (r >> 2) + 4 * h] == 32 * t + 16 * h + r


def test_host_plan_under_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path / "cbn_geom_check"
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cbn_geom_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr


def test_kernel_does_not_spill_and_fits_two_blocks_per_cu(tmp_path_factory):
    """No scratch, no spills; at most 256 VGPRs (two 4-wave blocks on a CU's four SIMDs are two waves per SIMD of a 512
    register file) and twice the block's LDS inside the CU's 160 KB."""
    from torchseg_amd import _lib
    isa = _isa(tmp_path_factory, "convbn.hip")
    meta = _kernel_meta(isa)
    assert len(meta) == 1 and "cbn_fwd_k" in next(iter(meta)), sorted(meta)
    for name, (spill, scratch) in meta.items():
        assert spill == 0 and scratch == 0, (name, spill, scratch)
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", isa)]
    agprs = [int(v) for v in re.findall(r"\.agpr_count:\s+(\d+)", isa)]
    assert len(vgprs) == 1 and vgprs[0] + agprs[0] <= 256, (vgprs, agprs)
    plan = (ctypes.c_int * 5)()
    assert _lib.lib().tsg_conv3x3_bnact_plan(1, 72, 256, 16, 512, plan) == 0
    assert 2 * plan[4] <= 160 * 1024
    body = isa[isa.index("cbn_fwd_k"):]
    assert len(re.findall(r"\n\s*v_mfma_f32_32x32x16_bf16", body.split("s_endpgm")[0])) == 36      # one chunk, unrolled once


def _randomise_bn(net, seed):
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            with torch.no_grad():
                m.weight.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
    return net


def _r18(seed=0):
    from torchseg_amd.workloads.bisenet import BiSeNet
    torch.manual_seed(seed)
    return _randomise_bn(BiSeNet(19, False, None, None, nn.BatchNorm2d), seed + 1)


class _BottleneckNet(nn.Module):
    """two Bottlenecks behind a 1x1 stem: the first with a stride-2 conv2 and a shortcut (nothing to fuse), the second plain"""

    def __init__(self):
        super().__init__()
        from base_model.resnet import Bottleneck, _shortcut
        self.stem = nn.Conv2d(3, 64, 1, bias=False)
        self.b0 = Bottleneck(64, 64, 2, nn.BatchNorm2d, downsample=_shortcut(64, 256, 2, nn.BatchNorm2d, 1e-5, 0.1))
        self.b1 = Bottleneck(256, 64, 1, nn.BatchNorm2d)

    def forward(self, x):
        return self.b1(self.b0(self.stem(x)))


def test_installer_counts_and_keeps_the_state_dict():
    from torchseg_amd.convbn import (_FusedBasicBlock, _FusedBottleneck, _FusedCbr, _FusedConvBn, eligible_layers,
                                     fused_calls, install_fused_convbn)
    net = _r18()
    keys = list(net.state_dict().keys())
    # 13 stride-1 3x3 of the backbone (8 blocks, three of them with a stride-2 conv1), 2 attention-refinement 3x3, 2 refines
    # and the 3x3 of each of the three heads the module tree holds (inference calls one of them: 18 launches per forward)
    assert sum(len(eligible_layers(m)[1]) for m in net.modules()) == 20
    assert install_fused_convbn(net) == 20
    assert list(net.state_dict().keys()) == keys
    kinds = [type(m).__mro__[1] for m in net.modules() if isinstance(m, _FusedConvBn)]
    assert kinds.count(_FusedBasicBlock) == 8 and kinds.count(_FusedCbr) == 7 and kinds.count(_FusedBottleneck) == 0
    assert install_fused_convbn(net) == 0                       # nothing left to take
    assert fused_calls(net) == 0
    bott = _BottleneckNet()
    keys = list(bott.state_dict().keys())
    assert install_fused_convbn(bott) == 1 and isinstance(bott.b1, _FusedBottleneck) and not isinstance(bott.b0, _FusedConvBn)
    assert list(bott.state_dict().keys()) == keys
    # structure, not class; a stride-2, dilated, 1x1, grouped or 24-channel convolution, a module without BatchNorm or a
    # hooked layer is left alone
    from seg_opr.seg_oprs import ConvBnRelu
    hooked = ConvBnRelu(16, 64, 3, 1, 1)
    hooked.bn.register_forward_hook(lambda *a: None)
    pile = nn.Sequential(ConvBnRelu(16, 64, 3, 1, 1, has_bias=True), ConvBnRelu(64, 64, 3, 2, 1), ConvBnRelu(64, 64, 3, 1, 2, dilation=2),
                         ConvBnRelu(64, 64, 1, 1, 0), ConvBnRelu(64, 64, 3, 1, 1, groups=2), ConvBnRelu(24, 64, 3, 1, 1),
                         ConvBnRelu(64, 64, 3, 1, 1, has_bn=False), hooked, ConvBnRelu(64, 128, 3, 1, 1, has_relu=False))
    assert install_fused_convbn(pile) == 2
    assert [isinstance(m, _FusedCbr) for m in pile] == [True] + [False] * 7 + [True]
    assert isinstance(pile[0], ConvBnRelu)
    x = torch.randn(1, 16, 6, 5)
    pile.eval()
    with torch.no_grad():
        assert torch.equal(pile[0](x), ConvBnRelu.forward(pile[0], x))
    # a hook registered after the install: the call declines (here it would anyway: CPU), the hook still fires
    fired = []
    pile[0].conv.register_forward_hook(lambda *a: fired.append(1))
    with torch.no_grad():
        pile[0](x)
    assert fired == [1] and fused_calls(pile) == 0


@pytest.mark.parametrize("which", ["r18", "bottleneck"])
def test_reclassed_network_is_the_stock_network_wherever_the_kernel_does_not_apply(which):
    """CPU input in eval mode, train mode, and gradients enabled (every parameter gradient too): bit-identical."""
    from torchseg_amd.convbn import fused_calls, install_fused_convbn
    stock = _r18() if which == "r18" else _randomise_bn(_BottleneckNet(), 3)
    ours = copy.deepcopy(stock)
    assert install_fused_convbn(ours) == (20 if which == "r18" else 1)
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
    assert fused_calls(ours) == 0


def test_prepare_inference_switch_defaults_to_off():
    """The signature carries the switch with None as its default (then TSG_CONVBN_FUSED decides; no GPU: the constructor
    is not run here, tests/test_convbn_gpu.py covers the effect), and the switch is documented with the others."""
    import inspect
    from torchseg_amd import infer
    for fn in (infer.prepare_inference, infer.InferenceModule.__init__):
        assert inspect.signature(fn).parameters["fuse_convbn"].default is None
    import torchseg_amd.ddp as ddp
    assert not hasattr(ddp, "install_fused_convbn")
    assert "TSG_CONVBN_FUSED" in ddp.__doc__
