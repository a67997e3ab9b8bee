"""The fused image stems and deep stem of inference (stem_bnact_fwd_k in csrc/stemconv.hip, ds_bnact_fwd_k in
csrc/deepstem.hip, torchseg_amd/stembn.py) as far as they can be checked without a GPU: the C-ABI's support predicates,
filter sizes and argument-validation order, the provider methods' argument checks, that the two kernels neither spill nor
use scratch, hold no more LDS than their unfused siblings and keep the occupancy their launch bounds ask for, the
installer's counts, what is and is not taken, that every call the fused kernels cannot take (CPU input in eval mode, train
mode, gradients enabled) is bit for bit the stock network, and the switch's default."""
import copy
import os
import re
import sys

import pytest
import torch
import torch.nn as nn

from test_convbn_cpu import _r18, _randomise_bn
from test_dilbn_cpu import _pspnet
from test_isa_guards_cpu import _isa, _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

# (B, H, W) of the IMAGE: the GPU test's shapes (tests/test_stembn_gpu.py says what each one catches)
GPU_CASES_3 = [(1, 1, 1), (1, 7, 9), (2, 8, 64), (2, 18, 66), (3, 34, 80)]
GPU_CASES_7 = [(1, 1, 2), (1, 7, 10), (2, 8, 64), (2, 18, 66), (2, 198, 1024)]
STEM_BLOCKS = 768                       # the persistent grid of stem_fwd_k and stem_bnact_fwd_k


def _tiles(B, H, W):
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return B * ((OH + 3) // 4) * ((OW + 31) // 32)


def test_support_predicates_filter_bytes_and_validation_order():
    from torchseg_amd import _lib
    lib = _lib.lib()
    assert lib.tsg_stem3_conv_bnact_filter_bytes() == 64 * 32 * 2
    assert lib.tsg_stem_conv_bnact_filter_bytes() == 64 * 176 * 2
    for name, cases in (("tsg_stem3_conv_bnact", GPU_CASES_3 + [(1, 768, 1536), (1, 1025, 2047)]),
                        ("tsg_stem_conv_bnact", GPU_CASES_7 + [(1, 768, 1536), (1, 1025, 2048)])):
        sup, pack, fwd = (getattr(lib, name + s) for s in ("_supported", "_pack", "_fwd"))
        for B, H, W in cases:
            assert sup(_lib.BF16, B, H, W) == 1
            assert sup(_lib.F32, B, H, W) == 0                       # the parity mode is not ours
            assert sup(7, B, H, W) == 0
        for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -8)):
            assert sup(_lib.BF16, *bad) == 0
            assert fwd(16, 16, 16, 16, *bad, 1, None) == -3             # TSG_E_SHAPE
            assert fwd(16, 16, 16, 24, *bad, 1, None) == -3             # shape before alignment
            assert fwd(None, 16, 16, 16, *bad, 1, None) == -5           # null before shape
        # null pointers, then the shape, then the alignment: all before any launch
        for args in ((None, 16, 16, 16), (16, None, 16, 16), (16, 16, None, 16), (16, 16, 16, None)):
            assert fwd(*args, 1, 8, 8, 1, None) == -5                   # TSG_E_NULL
        assert fwd(16, 16, 16, 24, 1, 8, 8, 1, None) == -4              # TSG_E_ALIGN: y
        assert fwd(16, 24, 16, 16, 1, 8, 8, 1, None) == -4              # wp
        assert fwd(16, 16, 8, 16, 1, 8, 8, 1, None) == -4               # ab
        assert fwd(17, 16, 16, 16, 1, 8, 8, 1, None) == -4              # x: an odd address
        assert pack(None, 16, None) == -5 and pack(16, None, None) == -5
        assert pack(16, 24, None) == -4 and pack(18, 16, None) == -4
    # the 7x7 reads the image in aligned pairs: W even, x 4-byte aligned; the 3x3 takes any W and a 2-byte aligned x
    assert lib.tsg_stem_conv_bnact_supported(_lib.BF16, 1, 7, 9) == 0
    assert lib.tsg_stem_conv_bnact_supported(_lib.BF16, 1, 7, 10) == 1
    assert lib.tsg_stem3_conv_bnact_supported(_lib.BF16, 1, 7, 9) == 1
    assert lib.tsg_stem_conv_bnact_fwd(16, 16, 16, 16, 1, 7, 9, 1, None) == -3
    assert lib.tsg_stem_conv_bnact_fwd(18, 16, 16, 16, 1, 8, 8, 1, None) == -4
    assert lib.tsg_stem3_conv_bnact_supported(_lib.BF16, 1, 1 << 31, 8) == 0
    # what the unfused entry points take is what the predicates say (their own predicates with the layer's hyper-parameters)
    for B, H, W in GPU_CASES_3 + GPU_CASES_7 + [(1, 9, 9), (1, 0, 8)]:
        assert lib.tsg_stem_conv_bnact_supported(_lib.BF16, B, H, W) == \
            lib.tsg_stem_conv_supported(_lib.BF16, 3, 64, 7, 7, 2, 3, 1, 1, H, W)
        assert lib.tsg_stem3_conv_bnact_supported(_lib.BF16, B, H, W) == \
            lib.tsg_stem3_conv_supported(_lib.BF16, 3, 64, 3, 3, 2, 1, 1, 1, H, W)


def test_only_the_largest_7x7_case_walks_a_second_tile():
    """stem_bnact_fwd_k is persistent over at most 768 blocks: (2, 198, 1024) is 2 x 25 x 16 = 800 tiles with ragged rows
    (99 = 24 x 4 + 3), the one GPU case in which a block walks a second tile.  The 3x3 kernel runs one tile per block."""
    assert _tiles(*GPU_CASES_7[-1]) == 800 > STEM_BLOCKS and ((198 - 1) // 2 + 1) % 4 == 3
    for case in GPU_CASES_7[:-1]:
        assert _tiles(*case) <= STEM_BLOCKS
    assert [_tiles(*c) for c in GPU_CASES_3] == [1, 1, 2, 2 * 3 * 2, 3 * 5 * 2]


def test_provider_methods_check_their_arguments():
    from torchseg_amd import _lib, kernels as K
    kp = K.provider()
    img = torch.zeros(1, 3, 8, 10, dtype=torch.bfloat16)
    assert kp.image_bnact_supported(img, 7) and kp.image_bnact_supported(img, 3)
    assert not kp.image_bnact_supported(img, 5)
    assert not kp.image_bnact_supported(img.float(), 7)
    assert not kp.image_bnact_supported(img[:, :, :, :9], 3)                           # not contiguous
    assert not kp.image_bnact_supported(img[:, :, :, :9].contiguous(), 7)              # W odd
    assert kp.image_bnact_supported(img[:, :, :, :9].contiguous(), 3)
    assert not kp.image_bnact_supported(torch.zeros(1, 4, 8, 10, dtype=torch.bfloat16), 3)
    fp = torch.zeros(3, 64)
    for w in (torch.zeros(64, 3, 5, 5), torch.zeros(64, 3, 7, 3), torch.zeros(32, 3, 3, 3), torch.zeros(64, 4, 3, 3),
              torch.zeros(64, 3, 3, 3, dtype=torch.bfloat16)):
        with pytest.raises(_lib.TsgError, match="image_bnact_pack"):
            kp.image_bnact_pack(w, fp)
    with pytest.raises(_lib.TsgError, match="image_bnact_pack"):
        kp.image_bnact_pack(torch.zeros(64, 3, 3, 3), torch.zeros(3, 32))
    wp3, wp7, ab = torch.zeros(64 * 32, dtype=torch.bfloat16), torch.zeros(64 * 176, dtype=torch.bfloat16), torch.zeros(2, 64)
    with pytest.raises(_lib.TsgError, match="pack"):                                    # the other kernel's filter
        kp.image_bnact_fwd(img, (wp7, ab), 3, True)
    with pytest.raises(_lib.TsgError, match="pack"):
        kp.image_bnact_fwd(img, (wp3, ab), 7, True)
    with pytest.raises(_lib.TsgError, match="pack"):
        kp.image_bnact_fwd(img, (wp3, ab[:1]), 3, True)
    with pytest.raises(_lib.TsgError, match="image"):
        kp.image_bnact_fwd(img.float(), (wp3, ab), 3, True)
    with pytest.raises(_lib.TsgError, match="7x7 or a 3x3"):
        kp.image_bnact_fwd(img, (wp3, ab), 5, True)
    with pytest.raises(_lib.TsgError, match="AMD GPU"):                                 # every check passed: no CPU path
        kp.image_bnact_fwd(img, (wp3, ab), 3, True)


def _one(isa, needle):
    meta = {k: v for k, v in _kernel_meta(isa).items() if needle in k}
    assert len(meta) == 1, (needle, sorted(_kernel_meta(isa)))
    name = next(iter(meta))
    block = [b for b in isa.split("  - .agpr_count:")[1:] if re.search(r"\.name:\s+" + re.escape(name) + r"\s", b)][0]
    regs = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))      # the unified file: VGPRs + AGPRs
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    return name, meta[name], regs, lds


def _waves_per_simd(regs):
    return min(8, 512 // ((regs + 7) // 8 * 8))      # a 512-entry file per SIMD, allocated in granules of 8


@pytest.mark.parametrize("src, new, old, blocks", [("deepstem.hip", "ds_bnact_fwd_k", "ds_fwd_k", 4),
                                                   ("stemconv.hip", "stem_bnact_fwd_k", "stem_fwd_kILb0ELb1E", 3)])
def test_kernels_do_not_spill_and_keep_their_siblings_lds(tmp_path_factory, src, new, old, blocks):
    """No scratch, no spills; static LDS no larger than the unfused sibling's; registers within what `blocks` 4-wave blocks
    per CU (= waves per SIMD) leave each wave: the launch bounds in the sources.  For the 7x7 that is the residency its
    768-block persistent grid assumes, and no fewer than its sibling's; 2 MFMAs per k-step as in the siblings; no atomics."""
    isa = _isa(tmp_path_factory, src)
    name, (spill, scratch), regs, lds = _one(isa, new)
    _, (ospill, oscratch), oregs, olds = _one(isa, old + "E" if old == "ds_fwd_k" else old)
    assert spill == 0 and scratch == 0, (name, spill, scratch)
    assert ospill == 0 and oscratch == 0
    assert lds <= olds and blocks * lds <= 160 * 1024, (lds, olds)
    assert _waves_per_simd(regs) >= blocks, (name, regs)
    if src == "stemconv.hip":
        assert _waves_per_simd(regs) >= _waves_per_simd(oregs) and blocks * 256 >= STEM_BLOCKS, (regs, oregs)
    body = isa[isa.index("\n" + name + ":"):].split("s_endpgm")[0]
    assert len(re.findall(r"\n\s*v_mfma_f32_32x32x16_bf16", body)) == (4 if src == "deepstem.hip" else 22)
    assert "global_atomic" not in body and "buffer_atomic" not in body and "flat_atomic" not in body
    print("%s: %d registers (%d waves per SIMD), %d B of LDS; %s: %d registers" % (new, regs, _waves_per_simd(regs), lds, old, oregs))


def _r50(seed=0, **kw):
    from base_model.resnet import resnet50
    torch.manual_seed(seed)
    return _randomise_bn(resnet50(None, norm_layer=nn.BatchNorm2d, **kw), seed + 1)


def test_installer_counts_and_state_dict():
    from torchseg_amd import stembn
    from torchseg_amd.convbn import _FusedConvBn, install_fused_convbn
    from torchseg_amd.pwbn import install_fused_pointwise
    from torchseg_amd.stembn import _FusedDeepStem, _FusedStem, _FusedStemCbr, install_fused_stem
    for build, n, kind in ((_r18, 1, _FusedStemCbr), (lambda: _r50(deep_stem=True, stem_width=64), 3, _FusedDeepStem),
                           (lambda: _pspnet(50, 21), 3, _FusedDeepStem), (_r50, 0, None)):
        net = build()
        keys = list(net.state_dict().keys())
        others = copy.deepcopy(net)
        counts = (install_fused_convbn(others), install_fused_convbn(others, dilated=True, plain=False),
                  install_fused_convbn(others, strided=True, plain=False), install_fused_pointwise(others))
        assert install_fused_stem(others) == n                      # after the other four, as prepare_inference does
        assert install_fused_stem(net) == n and install_fused_stem(net) == 0
        taken = [m for m in net.modules() if isinstance(m, _FusedStem)]
        assert len(taken) == (1 if n else 0) and all(isinstance(m, kind) for m in taken)
        assert not any(isinstance(m, _FusedConvBn) for m in taken)  # convbn.fused_calls does not see them
        assert list(net.state_dict().keys()) == keys and list(others.state_dict().keys()) == keys
        assert stembn.fused_calls(net) == 0 and stembn.image_fused_calls(net) == 0
        # the other installers find what they found, before or after this one
        assert (install_fused_convbn(net), install_fused_convbn(net, dilated=True, plain=False),
                install_fused_convbn(net, strided=True, plain=False), install_fused_pointwise(net)) == counts
        assert copy.deepcopy(net).state_dict().keys() == net.state_dict().keys()
    r18 = _r18()
    install_fused_stem(r18)
    assert isinstance(r18.spatial_path.conv_7x7, _FusedStemCbr) and r18.spatial_path.conv_7x7.tsg_stem_fused
    assert not isinstance(r18.context_path, _FusedStem)              # ResNet-18's bare 7x7 conv1 + bn1 is out of scope


def test_what_is_not_taken():
    from base_model.resnet import resnet50
    from seg_opr.seg_oprs import ConvBnRelu
    from torchseg_amd.stembn import install_fused_stem

    def deep(**kw):
        return resnet50(None, norm_layer=nn.BatchNorm2d, deep_stem=True, **{"stem_width": 64, **kw})
    assert install_fused_stem(deep()) == 3
    assert install_fused_stem(deep(stem_width=32)) == 0
    assert install_fused_stem(deep(stem_width=128)) == 0
    for first in (nn.Conv2d(3, 64, 3, 2, 1, bias=True), nn.Conv2d(3, 64, 5, 2, 2, bias=False),
                  nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.Conv2d(3, 64, 3, 2, 1, bias=False, padding_mode="reflect")):
        net = deep()
        net.conv1[0] = first
        assert install_fused_stem(net) == 0
    net = deep()
    net.conv1[0] = nn.Conv2d(3, 66, 3, 2, 1, groups=3, bias=False)  # grouped: 64 outputs cannot be split over 3 inputs
    assert install_fused_stem(net) == 0
    net = deep()
    net.conv1 = nn.Sequential(*list(net.conv1)[:6])                  # a Sequential of another length
    assert install_fused_stem(net) == 0
    net = deep()
    net.conv1 = nn.Sequential(*list(net.conv1), nn.Identity())
    assert install_fused_stem(net) == 0
    net = deep()
    net.conv1[3] = nn.Conv2d(64, 64, 3, 1, 1, groups=2, bias=False)
    assert install_fused_stem(net) == 0
    net = deep()
    net.conv1[2] = nn.ReLU6()
    assert install_fused_stem(net) == 0
    for hook_on in (lambda n: n, lambda n: n.conv1[1], lambda n: n.conv1[6], lambda n: n.bn1, lambda n: n.maxpool):
        net = deep()
        hook_on(net).register_forward_hook(lambda *a: None)
        assert install_fused_stem(net) == 0
    # ConvBnRelu-shaped modules
    assert install_fused_stem(ConvBnRelu(3, 64, 7, 2, 3)) == 1
    assert install_fused_stem(ConvBnRelu(3, 64, 7, 2, 3, has_relu=False)) == 1
    for m in (ConvBnRelu(3, 64, 7, 2, 3, has_bias=True), ConvBnRelu(3, 64, 7, 2, 3, has_bn=False),
              ConvBnRelu(3, 64, 7, 1, 3), ConvBnRelu(3, 64, 7, 2, 2), ConvBnRelu(3, 64, 5, 2, 2), ConvBnRelu(3, 64, 3, 2, 1),
              ConvBnRelu(3, 32, 7, 2, 3), ConvBnRelu(4, 64, 7, 2, 3), ConvBnRelu(16, 64, 3, 1, 1)):
        assert install_fused_stem(m) == 0
    hooked = ConvBnRelu(3, 64, 7, 2, 3)
    hooked.conv.register_forward_pre_hook(lambda *a: None)
    assert install_fused_stem(hooked) == 0
    # a module taken earlier declines once a hook appears: the stock method runs, the hook fires
    m = ConvBnRelu(3, 64, 7, 2, 3).eval()
    assert install_fused_stem(m) == 1
    fired = []
    m.bn.register_forward_hook(lambda *a: fired.append(1))
    x = torch.randn(1, 3, 8, 8)
    with torch.no_grad():
        assert torch.equal(m(x), ConvBnRelu.forward(m, x))
    assert fired == [1, 1]


@pytest.mark.parametrize("which", ["r18", "r50-deep", "pspnet", "r18-all"])
def test_reclassed_network_is_the_stock_network_wherever_the_kernels_do_not_apply(which):
    """CPU input in eval mode, train mode, and gradients enabled (every parameter gradient too): bit-identical."""
    from torchseg_amd import stembn
    from torchseg_amd.convbn import install_fused_convbn
    from torchseg_amd.pwbn import install_fused_pointwise
    torch.manual_seed(2)
    stock = {"r18": _r18, "r18-all": _r18, "r50-deep": lambda: _r50(deep_stem=True, stem_width=64),
             "pspnet": lambda: _randomise_bn(_pspnet(50, 21), 5)}[which]()
    ours = copy.deepcopy(stock)
    if which == "r18-all":
        install_fused_convbn(ours, strided=True)
        install_fused_pointwise(ours)
    assert stembn.install_fused_stem(ours) == (1 if which.startswith("r18") else 3)
    assert list(ours.state_dict().keys()) == list(stock.state_dict().keys())
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, 96, generator=g)

    def same(a, b):
        a, b = (a if isinstance(a, (list, tuple)) else [a]), (b if isinstance(b, (list, tuple)) else [b])
        return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))

    def run(net):
        torch.manual_seed(7)                                         # PSPNet's Dropout2d draws in train mode
        return net(x)

    def loss(y):
        return sum(t.square().mean() for t in (y if isinstance(y, (list, tuple)) else [y]))

    stock.eval(), ours.eval()
    with torch.no_grad():
        assert same(run(stock), run(ours))
        with torch.autocast("cpu", dtype=torch.bfloat16):            # bf16 autocast, but not on a GPU
            assert same(run(stock), run(ours))

    stock.train(), ours.train()
    with torch.no_grad():
        assert same(run(stock), run(ours))
    for (k, u), (_, v) in zip(stock.state_dict().items(), ours.state_dict().items()):
        assert torch.equal(u, v), k                                  # the running statistics moved alike

    for mode in (True, False):                                       # gradients enabled, in train and in eval mode
        stock.train(mode), ours.train(mode)
        outs = []
        for net in (stock, ours):
            net.zero_grad(set_to_none=True)
            y = run(net)
            loss(y).backward()
            outs.append([t.detach() for t in (y if isinstance(y, (list, tuple)) else [y])])
        assert same(outs[0], outs[1])
        for (n, p), (_, q) in zip(stock.named_parameters(), ours.named_parameters()):
            assert (p.grad is None) == (q.grad is None), n
            if p.grad is not None:
                assert torch.equal(p.grad, q.grad), n
    assert stembn.fused_calls(ours) == 0 and stembn.image_fused_calls(ours) == 0


def test_cbr_chain_runs_the_module_sequence_behind_a_stem_install_only():
    """seg_oprs.cbr_chain's test names both flags, is off with gradients enabled and in train mode, and a chain without
    an install has neither flag."""
    import inspect
    from seg_opr import seg_oprs
    from torchseg_amd.stembn import install_fused_stem
    from torchseg_amd.workloads.bisenet import SpatialPath
    src = inspect.getsource(seg_oprs.cbr_chain)
    assert "tsg_cbn_strided" in src and "tsg_stem_fused" in src and "not torch.is_grad_enabled()" in src
    sp = SpatialPath(3, 64)
    mods = [sp.conv_7x7, sp.conv_3x3_1, sp.conv_3x3_2, sp.conv_1x1]
    assert not any(getattr(m, "tsg_stem_fused", False) or getattr(m, "tsg_cbn_strided", False) for m in mods)
    assert install_fused_stem(sp) == 1
    assert [getattr(m, "tsg_stem_fused", False) for m in mods] == [True, False, False, False]


def test_prepare_inference_switch_defaults_to_off(monkeypatch):
    """The signature carries the switch with None as its default; then TSG_STEMBN_FUSED decides, and unset means off (no
    GPU: the constructor is not run here, tests/test_stembn_gpu.py covers the effect).  The install comes after the other
    four, the switch is documented with the others, and the DDP side never installs this."""
    import inspect
    from torchseg_amd import convbn, infer, stembn
    import torchseg_amd.ddp as ddp
    for fn in (infer.prepare_inference, infer.InferenceModule.__init__):
        assert inspect.signature(fn).parameters["fuse_stem"].default is None
    src = inspect.getsource(infer.InferenceModule.__init__)
    assert 'ddp._env_flag("TSG_STEMBN_FUSED", False)' in src
    assert "install_fused_stem(self.module)" in src
    for other in ("TSG_SEPCONV_FUSED", "TSG_CONVBN_FUSED", "TSG_DILBN_FUSED", "TSG_S2BN_FUSED", "TSG_PWBN_FUSED"):
        assert src.index(other) < src.index("TSG_STEMBN_FUSED")                          # the install order
    assert "fuse_stem=fuse_stem" in inspect.getsource(infer.prepare_inference)
    monkeypatch.delenv("TSG_STEMBN_FUSED", raising=False)
    assert ddp._env_flag("TSG_STEMBN_FUSED", False) is False
    monkeypatch.setenv("TSG_STEMBN_FUSED", "0")
    assert ddp._env_flag("TSG_STEMBN_FUSED", False) is False
    monkeypatch.setenv("TSG_STEMBN_FUSED", "1")
    assert ddp._env_flag("TSG_STEMBN_FUSED", False) is True
    src = inspect.getsource(ddp)
    assert "install_fused_stem" not in src and "import stembn" not in src
    for doc in (ddp.__doc__, infer.__doc__, stembn.__doc__):
        assert "TSG_STEMBN_FUSED" in doc
    for doc in (ddp.__doc__, infer.__doc__, convbn.__doc__):
        assert "stay unfused" not in " ".join(doc.split())
