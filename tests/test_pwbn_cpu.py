"""The fused 1x1 convolution + BatchNorm (+ residual) (+ ReLU) of inference (csrc/pwbn.hip, csrc/pwb_geom.h,
torchseg_amd/pwbn.py) as far as it can be checked without a GPU: the C-ABI's support predicate, plan query and argument
validation, the host plan and the filter layout under ASan + UBSan (tests/pwb_geom_check.cpp, a stand-alone program run
as a child process), that the kernel does not spill, uses no scratch and fits two blocks per compute unit, the installer's
counts on BiSeNet-R18 and ResNet-50 in both orders relative to convbn's installer, and that every call the fused kernel
cannot take (CPU input in eval mode, train mode, gradients enabled) is bit for bit the stock network."""
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

from test_convbn_cpu import _r18, _randomise_bn
from test_isa_guards_cpu import _isa, _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (B, H, W, C_in, C_out, stride): the GPU test's shapes; the last one makes a block walk two pixel tiles at C_out = 512
CASES = [(1, 5, 7, 64, 64, 1), (2, 8, 32, 128, 64, 1), (1, 9, 33, 192, 128, 1), (2, 9, 33, 64, 192, 2),
         (1, 18, 40, 256, 64, 2), (1, 130, 129, 64, 512, 1)]
# ResNet-50 stage entries and BiSeNet-R18's shortcuts / ffm.conv_1x1 at 768 x 1536
LAYERS = [(1, 192, 384, 64, 256, 1), (1, 192, 384, 256, 512, 2), (1, 96, 192, 512, 1024, 2), (1, 48, 96, 1024, 2048, 2),
          (1, 24, 48, 2048, 512, 1), (1, 192, 384, 64, 128, 2), (1, 96, 192, 256, 256, 1)]
# the 1x1 layers of BiSeNet-R18 by structure; an inference forward launches the first four (cbr_chain calls the parts of
# spatial_path.conv_1x1 directly, and the pooled [B,C,1,1] maps of the other three stay with vecconv.pooled_layer)
R18_ON_PATH = ["context_path.layer2.0", "context_path.layer3.0", "context_path.layer4.0", "ffm.conv_1x1"]
R18_INSTALLED = R18_ON_PATH + ["spatial_path.conv_1x1", "global_context.1", "arms.0.channel_attention.1",
                               "arms.1.channel_attention.1"]


def test_support_predicate_plan_and_null_pointers():
    from torchseg_amd import _lib
    lib = _lib.lib()
    plan = (ctypes.c_int * 5)()
    for B, H, W, Cin, Cout, s in CASES + LAYERS:
        assert lib.tsg_conv1x1_bnact_supported(_lib.BF16, B, H, W, Cin, Cout, s) == 1
        assert lib.tsg_conv1x1_bnact_supported(_lib.F32, B, H, W, Cin, Cout, s) == 0       # the parity mode is not ours
        assert lib.tsg_conv1x1_bnact_supported(7, B, H, W, Cin, Cout, s) == 0
        assert lib.tsg_conv1x1_bnact_plan(B, H, W, Cin, Cout, s, plan) == 0
        ntiles, nslots, noct, grid, lds = plan
        P = B * ((H - 1) // s + 1) * ((W - 1) // s + 1)
        assert ntiles == (P + 255) // 256 and noct == Cout // 64
        assert nslots % 8 == 0 and nslots >= 8 and grid == nslots * noct and lds == 16384
        assert nslots == max(8, (min(512 // noct, ntiles) + 7) // 8 * 8)
        assert lib.tsg_conv1x1_bnact_filter_bytes(Cin, Cout) == 2 * Cin * Cout
    for bad in ((1, 9, 33, 32, 64, 1), (1, 9, 33, 96, 64, 1), (1, 9, 33, 64, 96, 1), (1, 9, 33, 2112, 64, 1),
                (1, 9, 33, 64, 2112, 1), (1, 9, 33, 64, 64, 0), (1, 9, 33, 64, 64, 3), (0, 9, 33, 64, 64, 1),
                (1, 0, 33, 64, 64, 1), (1, 9, 0, 64, 64, 1), (1, 1024, 1024, 2048, 64, 1), (1, 1024, 1024, 64, 2048, 1),
                (1, 2047, 2047, 64, 2048, 2)):
        assert lib.tsg_conv1x1_bnact_supported(_lib.BF16, *bad) == 0, bad
    assert lib.tsg_conv1x1_bnact_supported(_lib.BF16, 1, 1024, 1023, 2048, 64, 1) == 1      # x: 2^31 - 2^21 elements
    assert lib.tsg_conv1x1_bnact_supported(_lib.BF16, 1, 2045, 2047, 64, 2048, 2) == 1      # y: 1023 x 1024 x 2048
    assert lib.tsg_conv1x1_bnact_filter_bytes(32, 64) == 0 and lib.tsg_conv1x1_bnact_filter_bytes(64, 2112) == 0
    assert lib.tsg_conv1x1_bnact_plan(1, 9, 33, 96, 64, 1, plan) == -3                       # TSG_E_SHAPE
    assert lib.tsg_conv1x1_bnact_plan(1, 9, 33, 64, 64, 1, None) == -5                       # TSG_E_NULL
    # null pointers, then the shape, then the alignment: all before any launch
    for args in ((None, 16, 16, None, 16), (16, None, 16, None, 16), (16, 16, None, None, 16), (16, 16, 16, None, None)):
        assert lib.tsg_conv1x1_bnact_fwd(*args, 1, 9, 33, 64, 64, 1, 1, None) == -5
        assert lib.tsg_conv1x1_bnact_fwd(*args, 1, 9, 33, 96, 64, 1, 1, None) == -5          # null before shape
    assert lib.tsg_conv1x1_bnact_fwd(16, 16, 16, None, 16, 1, 9, 33, 96, 64, 1, 1, None) == -3
    assert lib.tsg_conv1x1_bnact_fwd(16, 16, 16, None, 16, 1, 9, 33, 64, 96, 1, 1, None) == -3
    assert lib.tsg_conv1x1_bnact_fwd(16, 16, 16, None, 16, 1, 9, 33, 64, 64, 3, 1, None) == -3
    assert lib.tsg_conv1x1_bnact_fwd(24, 16, 16, None, 16, 1, 9, 33, 96, 64, 1, 1, None) == -3   # shape before alignment
    assert lib.tsg_conv1x1_bnact_fwd(16, 16, 16, None, 24, 1, 9, 33, 64, 64, 1, 1, None) == -4   # TSG_E_ALIGN
    assert lib.tsg_conv1x1_bnact_fwd(18, 16, 16, None, 16, 1, 9, 33, 64, 64, 2, 1, None) == -4
    assert lib.tsg_conv1x1_bnact_fwd(16, 16, 16, 8, 16, 1, 9, 33, 64, 64, 1, 1, None) == -4
    assert lib.tsg_conv1x1_bnact_fwd(16, 16, 4, None, 16, 1, 9, 33, 64, 64, 1, 1, None) == -4
    assert lib.tsg_conv1x1_bnact_fwd(16, 8, 16, None, 16, 1, 9, 33, 64, 64, 1, 1, None) == -4
    assert lib.tsg_conv1x1_bnact_prep_filter(None, 16, 64, 64, None) == -5
    assert lib.tsg_conv1x1_bnact_prep_filter(16, None, 64, 64, None) == -5
    assert lib.tsg_conv1x1_bnact_prep_filter(16, 16, 96, 64, None) == -3
    assert lib.tsg_conv1x1_bnact_prep_filter(8, 16, 96, 64, None) == -3
    assert lib.tsg_conv1x1_bnact_prep_filter(8, 16, 64, 64, None) == -4
    assert lib.tsg_conv1x1_bnact_prep_filter(16, 8, 64, 64, None) == -4


def test_host_plan_and_filter_layout_under_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path / "pwb_geom_check"
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "pwb_geom_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr


def test_kernel_does_not_spill_and_fits_two_blocks_per_cu(tmp_path_factory):
    """No scratch, no spills; at most 256 VGPRs + AGPRs (two 4-wave blocks on a CU's four SIMDs are two waves per SIMD of a
    512 register file) and twice the block's LDS inside the CU's 160 KB."""
    from torchseg_amd import _lib
    isa = _isa(tmp_path_factory, "pwbn.hip")
    meta = _kernel_meta(isa)
    assert len(meta) == 2 and any("pwb_fwd_k" in k for k in meta) and any("pwb_prep_filter_k" in k for k in meta), sorted(meta)
    for name, (spill, scratch) in meta.items():
        assert spill == 0 and scratch == 0, (name, spill, scratch)
    fwd = [b for b in isa.split("  - .agpr_count:")[1:] if "pwb_fwd_k" in b]
    assert len(fwd) == 1
    agpr = int(re.match(r"\s*(\d+)", fwd[0]).group(1))
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", fwd[0]).group(1))
    assert vgpr + agpr <= 256, (vgpr, agpr)
    plan = (ctypes.c_int * 5)()
    assert _lib.lib().tsg_conv1x1_bnact_plan(*CASES[-1], plan) == 0
    assert 2 * plan[4] <= 160 * 1024
    assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", fwd[0]).group(1)) == plan[4]
    body = isa[isa.index("pwb_fwd_k"):].split("s_endpgm")[0]
    # a chunk is 4 steps x 2 oc blocks x 2 pixel groups; the chunk loop is unrolled twice
    assert len(re.findall(r"\n\s*v_mfma_f32_32x32x16_bf16", body)) == 32
    assert "global_load_lds_dwordx4" in body                       # the filter slab goes to LDS by LDS-DMA


def _names(net):
    from torchseg_amd.pwbn import eligible_layers
    return [n for n, m in net.named_modules() if eligible_layers(m)[0] is not None]


def _r50(seed=0):
    from base_model.resnet import resnet50
    torch.manual_seed(seed)
    return _randomise_bn(resnet50(None, norm_layer=nn.BatchNorm2d), seed + 1)


def test_installer_counts_and_keeps_the_state_dict():
    from torchseg_amd import convbn
    from torchseg_amd.pwbn import (_FusedPointwise, _FusedPwBottleneck, _FusedPwCbr, _FusedPwShortcut, eligible_layers,
                                   fused_calls, install_fused_pointwise)
    net = _r18()
    keys = list(net.state_dict().keys())
    assert sorted(_names(net)) == sorted(R18_INSTALLED)
    assert all(len(eligible_layers(m)[1]) == 1 for m in net.modules() if eligible_layers(m)[0] is not None)
    assert install_fused_pointwise(net) == len(R18_INSTALLED) == 8
    assert list(net.state_dict().keys()) == keys
    kinds = {n: type(m).__mro__[1] for n, m in net.named_modules() if isinstance(m, _FusedPointwise)}
    assert all(kinds[n] is (_FusedPwShortcut if "layer" in n else _FusedPwCbr) for n in R18_INSTALLED), kinds
    assert install_fused_pointwise(net) == 0                     # nothing left to take
    assert fused_calls(net) == 0
    assert convbn.install_fused_convbn(net) == 20                # convbn's own count does not move
    assert install_fused_pointwise(net) == 0 and convbn.install_fused_convbn(net) == 0

    # resnet50: 16 Bottlenecks x (conv1, conv3) + the four stage shortcuts; both orders, the same classes
    a, b = _r50(), _r50()
    keys = list(a.state_dict().keys())
    assert sum(len(eligible_layers(m)[1]) for m in a.modules()) == 36
    assert install_fused_pointwise(a) == 36 and convbn.install_fused_convbn(a) == 13
    assert convbn.install_fused_convbn(b) == 13 and install_fused_pointwise(b) == 36
    assert install_fused_pointwise(a) == 0 and convbn.install_fused_convbn(a) == 0
    assert list(a.state_dict().keys()) == keys and list(b.state_dict().keys()) == keys
    for (n, ma), (_, mb) in zip(a.named_modules(), b.named_modules()):
        assert type(ma) is type(mb), n
        if isinstance(ma, _FusedPointwise):
            mro = type(ma).__mro__
            assert mro[1] is _FusedPwBottleneck                 # our mixin in front, whichever installer ran first
            if isinstance(ma, convbn._FusedConvBn):
                assert mro.index(convbn._FusedBottleneck) > mro.index(_FusedPwBottleneck)
    blocks = [m for m in a.modules() if isinstance(m, _FusedPointwise)]
    assert len(blocks) == 16 and sum(isinstance(m, convbn._FusedConvBn) for m in blocks) == 13

    # structure, not class; a 3x3, padded, grouped, 96-channel or 4096-channel convolution, a module without BatchNorm or a
    # hooked layer is left alone; stride 2 and a bias are taken
    from seg_opr.seg_oprs import ConvBnRelu
    hooked = ConvBnRelu(64, 64, 1, 1, 0)
    hooked.bn.register_forward_hook(lambda *a: None)
    pile = nn.Sequential(ConvBnRelu(128, 192, 1, 1, 0, has_bias=True), ConvBnRelu(64, 64, 3, 1, 1), ConvBnRelu(64, 64, 1, 1, 1),
                         ConvBnRelu(64, 64, 1, 1, 0, groups=2), ConvBnRelu(96, 64, 1, 1, 0), ConvBnRelu(64, 4096, 1, 1, 0),
                         ConvBnRelu(64, 64, 1, 1, 0, has_bn=False), hooked, ConvBnRelu(64, 19, 1, 1, 0),
                         ConvBnRelu(64, 128, 1, 2, 0, has_relu=False), ConvBnRelu(64, 64, 1, 1, 0, dilation=2))
    assert install_fused_pointwise(pile) == 3
    assert [isinstance(m, _FusedPwCbr) for m in pile] == [True] + [False] * 8 + [True, True]
    assert isinstance(pile[0], ConvBnRelu)
    x = torch.randn(1, 128, 6, 5)
    pile.eval()
    with torch.no_grad():
        assert torch.equal(pile[0](x), ConvBnRelu.forward(pile[0], x))
    fired = []
    pile[0].conv.register_forward_hook(lambda *a: fired.append(1))
    with torch.no_grad():
        pile[0](x)
    assert fired == [1] and fused_calls(pile) == 0


@pytest.mark.parametrize("which", ["r18", "r50", "r50-convbn-first"])
def test_reclassed_network_is_the_stock_network_wherever_the_kernel_does_not_apply(which):
    """CPU input in eval mode, train mode, and gradients enabled (every parameter gradient too): bit-identical, and no
    counter moves."""
    from torchseg_amd import convbn
    from torchseg_amd.pwbn import fused_calls, install_fused_pointwise
    stock = _r18() if which == "r18" else _r50(3)
    ours = copy.deepcopy(stock)
    if which == "r50-convbn-first":
        assert convbn.install_fused_convbn(ours) == 13
    assert install_fused_pointwise(ours) == (8 if which == "r18" else 36)
    if which == "r50":
        assert convbn.install_fused_convbn(ours) == 13
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, 96, generator=g)
    outs_of = lambda o: list(o) if isinstance(o, (list, tuple)) else [o]      # the backbone returns its four stages

    for mode in (False, True):                                   # eval, then train: no gradients
        stock.train(mode), ours.train(mode)
        with torch.no_grad():
            for u, v in zip(outs_of(stock(x)), outs_of(ours(x))):
                assert torch.equal(u, v), mode
    for (k, u), (_, v) in zip(stock.state_dict().items(), ours.state_dict().items()):
        assert torch.equal(u, v), k                              # the running statistics moved alike

    for mode in (True, False):                                   # gradients enabled, in train and in eval mode
        stock.train(mode), ours.train(mode)
        outs = []
        for net in (stock, ours):
            net.zero_grad(set_to_none=True)
            y = sum(t.square().mean() for t in outs_of(net(x)))
            y.backward()
            outs.append(y.detach())
        assert torch.equal(outs[0], outs[1])
        for (n, p), (_, q) in zip(stock.named_parameters(), ours.named_parameters()):
            assert (p.grad is None) == (q.grad is None), n
            if p.grad is not None:
                assert torch.equal(p.grad, q.grad), n
    assert fused_calls(ours) == 0 and convbn.fused_calls(ours) == 0


def test_prepare_inference_switch_defaults_to_off():
    """The signature carries the switch with None as its default (then TSG_PWBN_FUSED decides; no GPU: the constructor is
    not run here, tests/test_pwbn_gpu.py covers the effect), and the switch is documented with the others."""
    import inspect
    from torchseg_amd import infer
    for fn in (infer.prepare_inference, infer.InferenceModule.__init__):
        assert inspect.signature(fn).parameters["fuse_pointwise"].default is None
    import torchseg_amd.ddp as ddp
    assert not hasattr(ddp, "install_fused_pointwise")
    assert "TSG_PWBN_FUSED" in ddp.__doc__
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "TSG_PWBN_FUSED" in f.read()
