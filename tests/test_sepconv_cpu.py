"""The fused separable unit (csrc/sepconv.hip, csrc/sep_geom.h, torchseg_amd/sepconv.py) as far as it can be checked
without a GPU: the C-ABI's support predicate, pack size and argument validation, the host plan under ASan + UBSan
(tests/sep_geom_check.cpp, a stand-alone program run as a child process), the installer's count on BiSeNet-X39 and
BiSeNet-R18, that every call the fused kernel cannot take (CPU input in eval mode, train mode, gradients enabled) is
bit for bit the stock network, and that no kernel of sepconv.hip spills or uses scratch."""
import copy
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn

from test_isa_guards_cpu import _isa, _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (C_in, C_out, stride): the fifteen combinations of Xception39's 51 units
X39_UNITS = [(8, 64, 2), (8, 16, 2), (16, 16, 1), (16, 64, 1), (64, 16, 1),
             (64, 128, 2), (64, 32, 2), (32, 32, 1), (32, 128, 1), (128, 32, 1),
             (128, 256, 2), (128, 64, 2), (64, 64, 1), (64, 256, 1), (256, 64, 1)]


def test_support_predicate_pack_size_and_null_pointers():
    from torchseg_amd import _lib
    lib = _lib.lib()
    for dt in (_lib.BF16, _lib.F32):
        for cin, cout, s in X39_UNITS:
            for H, W in ((1, 1), (13, 19), (96, 192)):
                assert lib.tsg_sepconv_supported(dt, cin, cout, s, H, W) == 1, (dt, cin, cout, s, H, W)
            assert lib.tsg_sepconv_pack_bytes(dt, cin, cout) > 0
        for cin in (4, 12, 264):
            assert lib.tsg_sepconv_supported(dt, cin, 64, 1, 13, 19) == 0, cin
            assert lib.tsg_sepconv_pack_bytes(dt, cin, 64) == 0
        for cout in (8, 24, 272):
            assert lib.tsg_sepconv_supported(dt, 64, cout, 1, 13, 19) == 0, cout
            assert lib.tsg_sepconv_pack_bytes(dt, 64, cout) == 0
        assert lib.tsg_sepconv_supported(dt, 64, 64, 3, 13, 19) == 0
        assert lib.tsg_sepconv_supported(dt, 64, 64, 1, 0, 19) == 0
        assert lib.tsg_sepconv_supported(dt, 64, 64, 1, 13, 0) == 0
        assert lib.tsg_sepconv_fwd(None, None, None, None, dt, 1, 13, 19, 64, 64, 1, 1, None) == -5      # TSG_E_NULL
        assert lib.tsg_sepconv_pack(None, None, None, dt, 64, 64, None, None) == -5
    assert lib.tsg_sepconv_supported(7, 64, 64, 1, 13, 19) == 0 and lib.tsg_sepconv_pack_bytes(7, 64, 64) == 0
    # the sections of csrc/sep_geom.h: filter 36 bytes and a, b 8 bytes per channel, then W_p
    assert lib.tsg_sepconv_pack_bytes(_lib.F32, 64, 32) == 64 * 36 + 32 * 8 + 64 * 32 * 4
    assert lib.tsg_sepconv_pack_bytes(_lib.BF16, 64, 32) == 64 * 36 + 32 * 8 + 32 * 64 * 2
    assert lib.tsg_sepconv_pack_bytes(_lib.BF16, 8, 16) == 8 * 36 + 16 * 8 + 32 * 16 * 2       # padded to one 32 x 16 tile
    # host-side validation comes before any launch: a shape outside the domain, then a misaligned pointer
    assert lib.tsg_sepconv_fwd(16, 16, None, 16, _lib.BF16, 1, 13, 19, 12, 64, 1, 1, None) == -3          # TSG_E_SHAPE
    assert lib.tsg_sepconv_fwd(16, 16, None, 16, _lib.BF16, 1, 13, 19, 64, 64, 3, 1, None) == -3
    assert lib.tsg_sepconv_fwd(16, 16, None, 24, _lib.BF16, 1, 13, 19, 64, 64, 1, 1, None) == -4          # TSG_E_ALIGN
    assert lib.tsg_sepconv_fwd(16, 16, 8, 16, _lib.F32, 1, 13, 19, 64, 64, 1, 1, None) == -4
    assert lib.tsg_sepconv_pack(16, 16, 16, _lib.BF16, 64, 64, 8, None) == -4


def test_host_plan_under_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path / "sep_geom_check"
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "sep_geom_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr


def test_kernels_do_not_spill_or_use_scratch(tmp_path_factory):
    meta = _kernel_meta(_isa(tmp_path_factory, "sepconv.hip"))
    fwd = [k for k in meta if "sep_fwd_bf16_k" in k or "sep_fwd_f32_k" in k]
    assert len(fwd) == 3 and any("sep_pack_k" in k for k in meta), sorted(meta)     # two strip widths + the parity kernel
    for name, (spill, scratch) in meta.items():
        assert spill == 0 and scratch == 0, (name, spill, scratch)


def _x39(seed=0):
    from torchseg_amd.workloads.bisenet_x39 import BiSeNetX39
    torch.manual_seed(seed)
    net = BiSeNetX39(19, False, None, None, pretrained_model=None, norm_layer=nn.BatchNorm2d)
    g = torch.Generator().manual_seed(seed + 1)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(0.1 * torch.randn(m.num_features, generator=g))
            m.running_var.copy_(1.0 + 0.2 * torch.rand(m.num_features, generator=g))
    return net


def test_installer_counts_and_keeps_the_state_dict():
    from torchseg_amd.sepconv import _FusedSeparable, fused_calls, install_fused_separable
    from torchseg_amd.workloads.bisenet import BiSeNet
    net = _x39()
    keys = list(net.state_dict().keys())
    assert install_fused_separable(net) == 51
    assert list(net.state_dict().keys()) == keys
    assert sum(isinstance(m, _FusedSeparable) for m in net.modules()) == 51
    assert install_fused_separable(net) == 0                     # nothing left to take
    assert fused_calls(net) == 0
    assert install_fused_separable(BiSeNet(19, False, None, None, nn.BatchNorm2d)) == 0
    # structure, not class: any module with a depthwise conv1 and a 1x1 ConvBnRelu-like point_wise_cbr; a biased or
    # strided point-wise convolution, a 5x5 depthwise one or a hooked layer is left alone
    from seg_opr.seg_oprs import ConvBnRelu

    class Unit(nn.Module):
        def __init__(self, k=3, pw_stride=1, bias=False):
            super().__init__()
            self.conv1 = nn.Conv2d(16, 16, k, 1, k // 2, groups=16, bias=False)
            self.point_wise_cbr = ConvBnRelu(16, 32, 1, pw_stride, 0, has_bias=bias)

        def forward(self, x):
            return self.point_wise_cbr(self.conv1(x))

    hooked = Unit()
    hooked.point_wise_cbr.bn.register_forward_hook(lambda *a: None)
    pile = nn.Sequential(Unit(), Unit(k=5), Unit(pw_stride=2), Unit(bias=True), hooked)
    assert install_fused_separable(pile) == 1 and isinstance(pile[0], _FusedSeparable) and isinstance(pile[0], Unit)
    x = torch.randn(1, 16, 6, 5)
    pile.eval()
    with torch.no_grad():
        assert torch.equal(pile[0](x), Unit.forward(pile[0], x))


def test_reclassed_network_is_the_stock_network_wherever_the_kernel_does_not_apply():
    """CPU input in eval mode, train mode, and gradients enabled (every parameter gradient too): bit-identical."""
    from torchseg_amd.sepconv import fused_calls, install_fused_separable
    stock = _x39()
    ours = copy.deepcopy(stock)
    assert install_fused_separable(ours.context_path) == 51
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, 96, generator=g)

    stock.eval(), ours.eval()
    with torch.no_grad():
        assert torch.equal(stock(x), ours(x))
        for a, b in zip(stock.context_path(x), ours.context_path(x)):
            assert torch.equal(a, b)

    stock.train(), ours.train()
    with torch.no_grad():
        for a, b in zip(stock.context_path(x), ours.context_path(x)):
            assert torch.equal(a, b)
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


def test_prepare_inference_switch_defaults_to_off(monkeypatch):
    """The signature carries the switch and TSG_SEPCONV_FUSED is read only when it is None (no GPU: the constructor is
    not run here; tests/test_sepconv_gpu.py covers the effect)."""
    import inspect
    from torchseg_amd import infer
    for fn in (infer.prepare_inference, infer.InferenceModule.__init__):
        assert inspect.signature(fn).parameters["fuse_separable"].default is None
    src = inspect.getsource(infer.InferenceModule.__init__)
    assert '_env_flag("TSG_SEPCONV_FUSED", False)' in src
    import torchseg_amd.ddp as ddp
    assert "install_fused_separable" not in inspect.getsource(ddp.install_kernels)
    assert "TSG_SEPCONV_FUSED" in ddp.__doc__
