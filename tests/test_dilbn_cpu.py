"""The fused dilated 3x3 convolution + BatchNorm (+ residual) (+ ReLU) of inference (csrc/dilbn.hip, the `dilated=True` side
of torchseg_amd/convbn.py) as far as it can be checked without a GPU: the C-ABI's support predicate, plan query and
argument-validation order, that neither instantiation of the kernel spills or uses scratch and both fit two blocks per
compute unit, the installer's counts on PSPNet-R50 / -R101 and BiSeNet-R18 with and without `dilated=True`, that every call
the fused kernel cannot take (CPU input in eval mode, train mode, gradients enabled) is bit for bit the stock module, and
the switch's default."""
import copy
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn as nn

from test_convbn_cpu import CASES, _r18, _randomise_bn
from test_isa_guards_cpu import _isa, _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

# (B, H, W, C_in, C_out): the GPU test's shapes, and the three layer shapes of the 96 x 192 map
GPU_CASES = [(1, 3, 5, 16, 64), (2, 8, 32, 32, 64), (1, 9, 33, 48, 128), (1, 17, 40, 64, 192), (1, 72, 256, 16, 512)]
LAYERS = [(1, 96, 192, 256, 256), (1, 96, 192, 512, 512)]
LDS = {2: 78336, 4: 77824}


def test_support_predicate_plan_and_null_pointers():
    from torchseg_amd import _lib
    lib = _lib.lib()
    plan, plain = (ctypes.c_int * 5)(), (ctypes.c_int * 5)()
    for d in (2, 4):
        for B, H, W, Cin, Cout in CASES + GPU_CASES + LAYERS:
            assert lib.tsg_conv3x3_dil_bnact_supported(_lib.BF16, B, H, W, Cin, Cout, d) == 1
            assert lib.tsg_conv3x3_dil_bnact_supported(_lib.F32, B, H, W, Cin, Cout, d) == 0   # the parity mode is not ours
            assert lib.tsg_conv3x3_dil_bnact_supported(7, B, H, W, Cin, Cout, d) == 0
            assert lib.tsg_conv3x3_dil_bnact_plan(B, H, W, Cin, Cout, d, plan) == 0
            assert lib.tsg_conv3x3_bnact_plan(B, H, W, Cin, Cout, plain) == 0
            assert list(plan)[:4] == list(plain)[:4]                # the tiling does not depend on the dilation
            ntiles, nslots, noct, grid, lds = plan
            assert ntiles == B * ((H + 7) // 8) * ((W + 31) // 32) and noct == Cout // 64
            assert nslots % 8 == 0 and nslots >= 8 and grid == nslots * noct
            assert lds == LDS[d] and lds <= 81920 and 2 * lds <= 160 * 1024
        assert lib.tsg_conv3x3_dil_bnact_supported(_lib.BF16, 1, 9, 33, 24, 64, d) == 0
        assert lib.tsg_conv3x3_dil_bnact_supported(_lib.BF16, 1, 9, 33, 16, 96, d) == 0
        assert lib.tsg_conv3x3_dil_bnact_supported(_lib.BF16, 0, 9, 33, 16, 64, d) == 0
        assert lib.tsg_conv3x3_dil_bnact_supported(_lib.BF16, 1, 0, 33, 16, 64, d) == 0
        assert lib.tsg_conv3x3_dil_bnact_supported(_lib.BF16, 1, 9, 0, 16, 64, d) == 0
        assert lib.tsg_conv3x3_dil_bnact_supported(_lib.BF16, 1, 8192, 8192, 16, 64, d) == 0    # 2^32 elements per image
        assert lib.tsg_conv3x3_dil_bnact_plan(1, 9, 33, 24, 64, d, plan) == -3                   # TSG_E_SHAPE
        assert lib.tsg_conv3x3_dil_bnact_plan(1, 9, 33, 16, 64, d, None) == -5                   # TSG_E_NULL
    for d in (1, 3, 8, 0, -2):                                      # dilation 1 stays with tsg_conv3x3_bnact_*
        for B, H, W, Cin, Cout in CASES:
            assert lib.tsg_conv3x3_dil_bnact_supported(_lib.BF16, B, H, W, Cin, Cout, d) == 0
        assert lib.tsg_conv3x3_dil_bnact_plan(1, 9, 33, 16, 64, d, plan) == -3
        assert lib.tsg_conv3x3_dil_bnact_fwd(16, 16, 16, None, 16, 1, 9, 33, 16, 64, d, 1, None) == -3
    # null pointers, then the shape (the dilation included), then the alignment: all before any launch
    for d in (2, 4):
        for args in ((None, 16, 16, None, 16), (16, None, 16, None, 16), (16, 16, None, None, 16), (16, 16, 16, None, None)):
            assert lib.tsg_conv3x3_dil_bnact_fwd(*args, 1, 9, 33, 16, 64, d, 1, None) == -5
            assert lib.tsg_conv3x3_dil_bnact_fwd(*args, 1, 9, 33, 24, 64, 3, 1, None) == -5      # null before shape
        assert lib.tsg_conv3x3_dil_bnact_fwd(16, 16, 16, None, 16, 1, 9, 33, 24, 64, d, 1, None) == -3
        assert lib.tsg_conv3x3_dil_bnact_fwd(16, 16, 16, None, 16, 1, 9, 33, 16, 96, d, 1, None) == -3
        assert lib.tsg_conv3x3_dil_bnact_fwd(16, 16, 16, None, 24, 1, 9, 33, 24, 64, d, 1, None) == -3   # shape before alignment
        assert lib.tsg_conv3x3_dil_bnact_fwd(16, 16, 16, None, 24, 1, 9, 33, 16, 64, d, 1, None) == -4   # TSG_E_ALIGN
        assert lib.tsg_conv3x3_dil_bnact_fwd(16, 16, 16, 8, 16, 1, 9, 33, 16, 64, d, 1, None) == -4
        assert lib.tsg_conv3x3_dil_bnact_fwd(16, 16, 4, None, 16, 1, 9, 33, 16, 64, d, 1, None) == -4
        assert lib.tsg_conv3x3_dil_bnact_fwd(24, 16, 16, None, 16, 1, 9, 33, 16, 64, d, 1, None) == -4


def test_provider_twins_check_their_arguments():
    from torchseg_amd import _lib, kernels as K
    kp = K.provider()
    for d in (2, 4):
        assert kp.conv3x3_dil_bnact_plan(1, 72, 256, 16, 512, d) == kp.conv3x3_bnact_plan(1, 72, 256, 16, 512)[:4] + (LDS[d],)
    with pytest.raises(_lib.TsgError):
        kp.conv3x3_dil_bnact_plan(1, 72, 256, 16, 512, 1)
    x = torch.zeros(1, 16, 9, 33, dtype=torch.bfloat16)
    assert not kp.conv3x3_dil_bnact_supported(x, 64, 2)                                 # NCHW
    xc = x.contiguous(memory_format=torch.channels_last)
    assert kp.conv3x3_dil_bnact_supported(xc, 64, 2) and kp.conv3x3_dil_bnact_supported(xc, 64, 4)
    assert not kp.conv3x3_dil_bnact_supported(xc, 64, 1) and not kp.conv3x3_dil_bnact_supported(xc, 64, 3)
    assert not kp.conv3x3_dil_bnact_supported(xc.float(), 64, 2) and not kp.conv3x3_dil_bnact_supported(xc, 96, 2)
    wf, ab = torch.zeros(9 * 16 * 64, dtype=torch.bfloat16), torch.zeros(2, 64)
    with pytest.raises(_lib.TsgError, match="pack"):
        kp.conv3x3_dil_bnact_fwd(xc, (wf[:-16], ab), 64, 2, None, True)
    with pytest.raises(_lib.TsgError, match="pack"):
        kp.conv3x3_dil_bnact_fwd(xc, (wf, ab[:1]), 64, 2, None, True)
    with pytest.raises(_lib.TsgError, match="residual"):
        kp.conv3x3_dil_bnact_fwd(xc, (wf, ab), 64, 2, torch.zeros(1, 64, 9, 33, dtype=torch.bfloat16), True)


def test_kernels_do_not_spill_and_fit_two_blocks_per_cu(tmp_path_factory):
    """Exactly the two instantiations; no scratch, no spills; at most 256 VGPRs + AGPRs each (two 4-wave blocks on a CU's
    four SIMDs are two waves per SIMD of a 512 register file); one unrolled chunk of 36 MFMAs each."""
    isa = _isa(tmp_path_factory, "dilbn.hip")
    meta = _kernel_meta(isa)
    assert len(meta) == 2 and all("dbn_fwd_k" in k for k in meta), sorted(meta)
    assert sorted(re.search(r"dbn_fwd_kILi(\d)E", k).group(1) for k in meta) == ["2", "4"]
    for name, (spill, scratch) in meta.items():
        assert spill == 0 and scratch == 0, (name, spill, scratch)
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", isa)]
    agprs = [int(v) for v in re.findall(r"\.agpr_count:\s+(\d+)", isa)]
    assert len(vgprs) == 2 and len(agprs) == 2
    for v, a in zip(vgprs, agprs):
        assert v + a <= 256, (vgprs, agprs)
    for name in meta:
        body = isa[isa.index("\n" + name + ":"):].split("s_endpgm")[0]
        assert len(re.findall(r"\n\s*v_mfma_f32_32x32x16_bf16", body)) == 36, name
        assert "global_atomic" not in body and "buffer_atomic" not in body and "flat_atomic" not in body, name


def _pspnet(depth, seed=0):
    from torchseg_amd.workloads.pspnet import PSPNet
    torch.manual_seed(seed)
    return PSPNet(19, None, None, nn.BatchNorm2d, depth=depth)


def test_installer_counts():
    from torchseg_amd.convbn import (_FusedBottleneck, _FusedConvBn, dil_fused_calls, eligible_dilated_layers, eligible_layers,
                                     fused_calls, install_fused_convbn)
    net = _pspnet(50)
    keys = list(net.state_dict().keys())
    dil = [cb for m in net.modules() for cb in eligible_dilated_layers(m)]
    # layer3: 5 x 256 -> 256 at dilation 2 (its first block's stride-2 3x3 became a plain one); layer4: 512 -> 512 at 2, 2 x at 4
    assert sorted((c.in_channels, c.dilation[0]) for c, _ in dil) == [(256, 2)] * 5 + [(512, 2)] + [(512, 4)] * 2
    # what the default finds, before and after this feature: 3 + 3 + 1 plain Bottlenecks of layer1 / layer2 / layer3, the 3x3 of
    # the pyramid head and of the auxiliary head
    plain = sum(len(eligible_layers(m)[1]) for m in net.modules())
    assert plain == 9
    assert sum(len(eligible_layers(m, True)[1]) for m in net.modules()) == plain + 8
    both = copy.deepcopy(net)
    assert install_fused_convbn(both, dilated=True) == plain + 8
    assert sum(isinstance(m, _FusedBottleneck) and m.tsg_cbn_dilated for m in both.modules()) == 7 + 8
    assert install_fused_convbn(both, dilated=True) == 0 and install_fused_convbn(both) == 0      # nothing left to take
    assert list(both.state_dict().keys()) == keys
    # the default: the dilated blocks are left alone, and the dilated install then takes exactly them
    two = copy.deepcopy(net)
    assert install_fused_convbn(two) == plain
    marked = [m for m in two.modules() if isinstance(m, _FusedConvBn)]
    assert len(marked) == plain and not any(m.tsg_cbn_dilated for m in marked)
    assert not any(isinstance(m, _FusedConvBn) for m in two.modules() if eligible_dilated_layers(m))
    assert install_fused_convbn(two, dilated=True, plain=False) == 8
    assert sum(m.tsg_cbn_dilated for m in two.modules() if isinstance(m, _FusedConvBn)) == 8
    # only the dilated blocks on a fresh network
    only = copy.deepcopy(net)
    assert install_fused_convbn(only, dilated=True, plain=False) == 8
    assert sum(isinstance(m, _FusedConvBn) for m in only.modules()) == 8
    assert list(only.state_dict().keys()) == keys and fused_calls(only) == 0 and dil_fused_calls(only) == 0
    # R101: 22 + 1 + 2, counted with the eligibility function alone
    r101 = _pspnet(101)
    dil = [c for m in r101.modules() for c, _ in eligible_dilated_layers(m)]
    assert len(dil) == 25
    assert sorted((c.in_channels, c.dilation[0]) for c in dil) == [(256, 2)] * 22 + [(512, 2)] + [(512, 4)] * 2
    # BiSeNet-R18 has no dilated layer: nothing changes
    r18 = _r18()
    assert sum(len(eligible_dilated_layers(m)) for m in r18.modules()) == 0
    assert sum(len(eligible_layers(m, True)[1]) for m in r18.modules()) == 20
    assert install_fused_convbn(copy.deepcopy(r18), dilated=True, plain=False) == 0
    assert install_fused_convbn(copy.deepcopy(r18), dilated=True) == 20 and install_fused_convbn(r18) == 20


def test_what_is_and_is_not_a_dilated_3x3():
    from seg_opr.seg_oprs import ConvBnRelu
    from torchseg_amd.convbn import _FusedCbr, install_fused_convbn
    pile = nn.Sequential(ConvBnRelu(16, 64, 3, 1, 2, dilation=2), ConvBnRelu(64, 64, 3, 1, 4, dilation=4),
                         ConvBnRelu(64, 64, 3, 1, 3, dilation=3), ConvBnRelu(64, 64, 3, 1, 1, dilation=2),
                         ConvBnRelu(64, 64, 3, 2, 2, dilation=2), ConvBnRelu(64, 64, 3, 1, 2, dilation=2, groups=2),
                         ConvBnRelu(24, 64, 3, 1, 2, dilation=2), ConvBnRelu(64, 96, 3, 1, 4, dilation=4),
                         ConvBnRelu(64, 64, 3, 1, 8, dilation=8), ConvBnRelu(64, 64, 3, 1, 1))
    assert install_fused_convbn(copy.deepcopy(pile)) == 1
    assert install_fused_convbn(copy.deepcopy(pile), plain=False) == 0           # nothing without `dilated`
    assert install_fused_convbn(copy.deepcopy(pile), dilated=True, plain=False) == 2
    assert install_fused_convbn(pile, dilated=True) == 3
    assert [isinstance(m, _FusedCbr) for m in pile] == [True, True] + [False] * 7 + [True]


def _dilated_bottleneck(d, shortcut):
    from base_model.resnet import Bottleneck, _shortcut
    from torchseg_amd.workloads.pspnet import _nostride_dilate
    ds = _shortcut(128, 256, 1, nn.BatchNorm2d, 1e-5, 0.1) if shortcut else None
    m = Bottleneck(128 if shortcut else 256, 64, 1, nn.BatchNorm2d, downsample=ds)
    m.apply(lambda k: _nostride_dilate(k, d))
    assert m.conv2.dilation == (d, d) and m.conv2.padding == (d, d) and m.conv2.stride == (1, 1)
    return m


def _dilated_cbr(d):
    from seg_opr.seg_oprs import ConvBnRelu
    return ConvBnRelu(48, 128, 3, 1, d, dilation=d, has_bias=True)


@pytest.mark.parametrize("d", [2, 4])
@pytest.mark.parametrize("which", ["bottleneck", "bottleneck-downsample", "convbnrelu"])
def test_reclassed_module_is_the_stock_module_wherever_the_kernel_does_not_apply(which, d):
    """CPU input in eval mode, train mode, and gradients enabled (every parameter gradient too): bit-identical to the deep
    copy taken before the install; with pwbn's mixin in front as well."""
    from torchseg_amd.convbn import _FusedConvBn, dil_fused_calls, fused_calls, install_fused_convbn
    from torchseg_amd.pwbn import install_fused_pointwise
    torch.manual_seed(3 + d)
    stock = _randomise_bn(_dilated_cbr(d) if which == "convbnrelu" else _dilated_bottleneck(d, which != "bottleneck"), 4)
    cin = stock.conv.in_channels if which == "convbnrelu" else stock.conv1.in_channels
    ours, both = copy.deepcopy(stock), copy.deepcopy(stock)
    assert install_fused_convbn(copy.deepcopy(stock)) == 0           # the default leaves a dilated module alone
    assert install_fused_convbn(ours, dilated=True) == 1 and isinstance(ours, _FusedConvBn) and ours.tsg_cbn_dilated
    install_fused_pointwise(both)
    assert install_fused_convbn(both, dilated=True, plain=False) == 1 and both.tsg_cbn_dilated
    assert list(ours.state_dict().keys()) == list(stock.state_dict().keys()) == list(both.state_dict().keys())
    x = torch.randn(2, cin, 11, 13, generator=torch.Generator().manual_seed(5))

    for net in (ours, both):
        stock.eval(), net.eval()
        with torch.no_grad():
            assert torch.equal(stock(x), net(x))
        ref = copy.deepcopy(stock)
        ref.train(), net.train()
        with torch.no_grad():
            assert torch.equal(ref(x), net(x))
        for mode in (True, False):                                   # gradients enabled, in train and in eval mode
            ref.train(mode), net.train(mode)
            outs = []
            for m in (ref, net):
                m.zero_grad(set_to_none=True)
                y = m(x)
                y.square().mean().backward()
                outs.append(y.detach())
            assert torch.equal(outs[0], outs[1])
            for (n, p), (_, q) in zip(ref.named_parameters(), net.named_parameters()):
                assert (p.grad is None) == (q.grad is None), n
                if p.grad is not None:
                    assert torch.equal(p.grad, q.grad), n
        for (k, u), (_, v) in zip(ref.state_dict().items(), net.state_dict().items()):
            assert torch.equal(u, v), k                              # the running statistics moved alike
        net.load_state_dict(stock.state_dict())
        assert fused_calls(net) == 0 and dil_fused_calls(net) == 0


def test_prepare_inference_switch_defaults_to_off(monkeypatch):
    """The signature carries the switch with None as its default; then TSG_DILBN_FUSED decides, and unset means off (no GPU:
    the constructor is not run here, tests/test_dilbn_gpu.py covers the effect).  The switch is documented with the others,
    and the DDP side never installs this."""
    import inspect
    from torchseg_amd import convbn, infer
    import torchseg_amd.ddp as ddp
    for fn in (infer.prepare_inference, infer.InferenceModule.__init__):
        assert inspect.signature(fn).parameters["fuse_dilated"].default is None
    for fn in (convbn.install_fused_convbn, convbn.eligible_layers):
        assert inspect.signature(fn).parameters["dilated"].default is False
    assert 'ddp._env_flag("TSG_DILBN_FUSED", False)' in inspect.getsource(infer.InferenceModule.__init__)
    monkeypatch.delenv("TSG_DILBN_FUSED", raising=False)
    assert ddp._env_flag("TSG_DILBN_FUSED", False) is False
    monkeypatch.setenv("TSG_DILBN_FUSED", "0")
    assert ddp._env_flag("TSG_DILBN_FUSED", False) is False
    monkeypatch.setenv("TSG_DILBN_FUSED", "1")
    assert ddp._env_flag("TSG_DILBN_FUSED", False) is True
    src = inspect.getsource(ddp)
    assert "install_fused_convbn" not in src and "dilated=True" not in src
    for doc in (ddp.__doc__, infer.__doc__, convbn.__doc__):
        assert "TSG_DILBN_FUSED" in doc
