"""PSPNet's pyramid pooling head without the concatenation (csrc/ppmbn.hip, torchseg_amd/ppmbn.py) as far as it can be
checked without a GPU: the C-ABI's support predicates, workspace query and argument-validation order, the host plan under
sanitizers (tests/ppm_geom_check.cpp), that no kernel spills or uses scratch and that the convolution fits two blocks per
compute unit, the installer's counts, the state-dict keys, that every call the fused chain cannot take (CPU input, train
mode, gradients enabled) is bit for bit the stock module, and the switch's default.

CASES are the GPU test's kernel shapes (B, H, W, C, Cb, Cout, pooled maps), the smallest at which each mechanism can go wrong:
  (1, 6, 7, 16, 16, 64, 1 2 3 6)      below one 8 x 32 tile; H equals the largest scale (identity rows); one chunk
  (2, 8, 32, 32, 16, 64, 1 2 3 6)     an exact tile; two images (a T per image); both buffers of the double buffering
  (1, 9, 33, 48, 32, 128, 1 2 3 6)    ragged both ways; an odd chunk count; two oc tiles; two K steps of the branch MFMA
  (1, 17, 40, 64, 16, 192, 2x3 6x4)   n = 2; rectangular pooled maps; several tiles; three oc tiles
  (1, 72, 256, 16, 16, 512, 1 2 3 6)  a persistent block walks two tiles: cbn_geom gives 72 tiles on 64 slots
EXACT_CASES have H - 1 and W - 1 powers of two, so that every interpolation weight is dyadic."""
import copy
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from test_convbn_cpu import HIPCC, _r18, _randomise_bn
from test_dilbn_cpu import _pspnet
from test_isa_guards_cpu import _isa, _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

STD = ((1, 1), (2, 2), (3, 3), (6, 6))
CASES = [(1, 6, 7, 16, 16, 64, STD), (2, 8, 32, 32, 16, 64, STD), (1, 9, 33, 48, 32, 128, STD),
         (1, 17, 40, 64, 16, 192, ((2, 3), (6, 4))), (1, 72, 256, 16, 16, 512, STD)]
EXACT_CASES = [(1, 9, 17, 16, 16, 64, STD), (2, 9, 33, 32, 16, 128, STD), (1, 17, 33, 16, 32, 64, ((2, 3), (6, 5)))]
# PSPNet's head at B = 1 on ADE's 480 x 480 crop, 768 x 1536 and 1024 x 2048
HEADS = [(1, 60, 60, 2048, 512, 512, STD), (1, 96, 192, 2048, 512, 512, STD), (1, 128, 256, 2048, 512, 512, STD)]
LDS = 69504


def _maps(maps):
    n = len(maps)
    return n, (ctypes.c_int * n)(*[m[0] for m in maps]), (ctypes.c_int * n)(*[m[1] for m in maps])


def test_support_predicates_workspace_and_plan():
    from torchseg_amd import _lib
    lib = _lib.lib()
    plan = (ctypes.c_int64 * 6)()
    for B, H, W, C, Cb, Cout, maps in CASES + EXACT_CASES + HEADS:
        n, sh, sw = _maps(maps)
        assert lib.tsg_ppm_supported(_lib.BF16, B, H, W, n, sh, sw, C, Cb, Cout) == 1
        assert lib.tsg_ppm_supported(_lib.F32, B, H, W, n, sh, sw, C, Cb, Cout) == 0         # the parity mode is not ours
        assert lib.tsg_ppm_taps_supported(_lib.BF16, B, n, sh, sw, Cb, Cout) == 1
        assert lib.tsg_ppm_taps_supported(_lib.F32, B, n, sh, sw, Cb, Cout) == 0
        assert lib.tsg_ppm_addend_supported(B, H, W, n, sh, sw, Cout) == 1
        assert lib.tsg_conv3x3_bnact_add_supported(_lib.BF16, B, H, W, C, Cout) == 1
        assert lib.tsg_conv3x3_bnact_add_supported(_lib.F32, B, H, W, C, Cout) == 0
        assert lib.tsg_ppm_plan(B, H, W, n, sh, sw, Cb, Cout, plan) == 0
        cells, cols, tap_grid, add_grid, e_off, ws = plan
        assert cells == sum(h * w for h, w in maps) and cols == sum(w for _, w in maps)
        assert tap_grid == B * n * 9 * (Cout // 32) and add_grid == B * H * (Cout // 64)
        t_bytes = B * cells * 9 * Cout * 4
        assert t_bytes <= e_off < t_bytes + 256 and e_off % 256 == 0 and ws == e_off + B * H * W * Cout * 4
        assert lib.tsg_ppm_ws_bytes(B, H, W, n, sh, sw, Cb, Cout) == ws
    n, sh, sw = _maps(STD)
    # the standard head's tables: 50 cells of 9 taps of 512 floats per image
    assert lib.tsg_ppm_plan(1, 96, 192, n, sh, sw, 512, 512, plan) == 0 and tuple(plan)[:2] == (50, 12)
    assert plan[4] == 50 * 9 * 512 * 4 and plan[5] == plan[4] + 96 * 192 * 512 * 4
    for bad in ((24, 64), (16, 96), (0, 64), (16, 0), (8, 64)):                              # (Cb, Cout)
        assert lib.tsg_ppm_taps_supported(_lib.BF16, 1, n, sh, sw, *bad) == 0
        assert lib.tsg_ppm_ws_bytes(1, 9, 33, n, sh, sw, *bad) == 0
        assert lib.tsg_ppm_plan(1, 9, 33, n, sh, sw, *bad, plan) == -3                       # TSG_E_SHAPE
    assert lib.tsg_ppm_supported(_lib.BF16, 1, 9, 33, n, sh, sw, 24, 16, 64) == 0            # the convolution's C_in
    assert lib.tsg_ppm_supported(_lib.BF16, 1, 9, 33, 0, sh, sw, 16, 16, 64) == 0
    assert lib.tsg_ppm_supported(_lib.BF16, 1, 9, 33, 5, sh, sw, 16, 16, 64) == 0
    assert lib.tsg_ppm_supported(_lib.BF16, 0, 9, 33, n, sh, sw, 16, 16, 64) == 0
    assert lib.tsg_ppm_supported(_lib.BF16, 1, 0, 33, n, sh, sw, 16, 16, 64) == 0
    assert lib.tsg_ppm_supported(_lib.BF16, 1, 9, 33, n, None, sw, 16, 16, 64) == 0
    _, h9, w9 = _maps(((9, 9),))
    assert lib.tsg_ppm_taps_supported(_lib.BF16, 1, 1, h9, w9, 16, 64) == 0                  # 81 cells
    _, h8, w8 = _maps(((8, 8),))
    assert lib.tsg_ppm_taps_supported(_lib.BF16, 1, 1, h8, w8, 16, 64) == 1                  # 64 cells
    _, hw, ww = _maps(((1, 33),))
    assert lib.tsg_ppm_addend_supported(1, 9, 33, 1, hw, ww, 64) == 0                        # 33 columns
    _, hw, ww = _maps(((2, 16), (2, 16)))
    assert lib.tsg_ppm_addend_supported(1, 9, 33, 2, hw, ww, 64) == 1                        # 32 columns together
    assert lib.tsg_ppm_addend_supported(1, 8192, 8192, n, sh, sw, 64) == 0                   # 2^32 elements per image of E
    assert lib.tsg_ppm_plan(1, 9, 33, n, sh, sw, 16, 64, None) == -5                         # TSG_E_NULL
    assert lib.tsg_ppm_plan(1, 9, 33, n, sh, sw, 24, 64, None) == -5                         # null before shape


def test_argument_checks_null_then_shape_then_alignment():
    """all three before any launch: this runs without a GPU"""
    from torchseg_amd import _lib
    lib = _lib.lib()
    n, sh, sw = _maps(STD)
    ok4 = (16, 16, 16, 16)
    # tsg_ppm_taps_fwd(p0, p1, p2, p3, wb, T, B, n, sh, sw, Cb, Cout, stream)
    for args in (((None, 16, 16, 16), 16, 16, sh, sw), ((16, 16, None, 16), 16, 16, sh, sw), (ok4, None, 16, sh, sw),
                 (ok4, 16, None, sh, sw), (ok4, 16, 16, None, sw), (ok4, 16, 16, sh, None)):
        ps, wb, T, a, b = args
        assert lib.tsg_ppm_taps_fwd(*ps, wb, T, 1, n, a, b, 16, 64, None) == -5
        assert lib.tsg_ppm_taps_fwd(*ps, wb, T, 1, n, a, b, 24, 64, None) == -5               # null before shape
    assert lib.tsg_ppm_taps_fwd(16, 16, None, None, 16, 16, 1, 2, sh, sw, 24, 64, None) == -3  # p_s for s >= n may be NULL
    assert lib.tsg_ppm_taps_fwd(*ok4, 16, 16, 1, n, sh, sw, 24, 64, None) == -3
    assert lib.tsg_ppm_taps_fwd(*ok4, 16, 16, 1, n, sh, sw, 16, 96, None) == -3
    assert lib.tsg_ppm_taps_fwd(*ok4, 16, 16, 0, n, sh, sw, 16, 64, None) == -3
    assert lib.tsg_ppm_taps_fwd(*ok4, 16, 16, 1, 5, sh, sw, 16, 64, None) == -3
    assert lib.tsg_ppm_taps_fwd(*ok4, 24, 16, 1, n, sh, sw, 24, 64, None) == -3               # shape before alignment
    assert lib.tsg_ppm_taps_fwd(*ok4, 24, 16, 1, n, sh, sw, 16, 64, None) == -4               # TSG_E_ALIGN
    assert lib.tsg_ppm_taps_fwd(*ok4, 16, 8, 1, n, sh, sw, 16, 64, None) == -4
    assert lib.tsg_ppm_taps_fwd(16, 16, 16, 24, 16, 16, 1, n, sh, sw, 16, 64, None) == -4
    # tsg_ppm_addend_fwd(T, E, B, H, W, n, sh, sw, Cout, stream)
    for T, E, a, b in ((None, 16, sh, sw), (16, None, sh, sw), (16, 16, None, sw), (16, 16, sh, None)):
        assert lib.tsg_ppm_addend_fwd(T, E, 1, 9, 33, n, a, b, 64, None) == -5
        assert lib.tsg_ppm_addend_fwd(T, E, 1, 9, 33, n, a, b, 96, None) == -5
    assert lib.tsg_ppm_addend_fwd(16, 16, 1, 9, 33, n, sh, sw, 96, None) == -3
    assert lib.tsg_ppm_addend_fwd(16, 16, 1, 0, 33, n, sh, sw, 64, None) == -3
    assert lib.tsg_ppm_addend_fwd(16, 24, 1, 9, 33, n, sh, sw, 96, None) == -3
    assert lib.tsg_ppm_addend_fwd(16, 24, 1, 9, 33, n, sh, sw, 64, None) == -4
    assert lib.tsg_ppm_addend_fwd(8, 16, 1, 9, 33, n, sh, sw, 64, None) == -4
    # tsg_conv3x3_bnact_add_fwd(x, wf, ab, addend, y, B, H, W, Cin, Cout, relu, stream)
    for args in ((None, 16, 16, 16, 16), (16, None, 16, 16, 16), (16, 16, None, 16, 16), (16, 16, 16, None, 16),
                 (16, 16, 16, 16, None)):
        assert lib.tsg_conv3x3_bnact_add_fwd(*args, 1, 9, 33, 16, 64, 1, None) == -5
        assert lib.tsg_conv3x3_bnact_add_fwd(*args, 1, 9, 33, 24, 64, 1, None) == -5
    assert lib.tsg_conv3x3_bnact_add_fwd(16, 16, 16, 16, 16, 1, 9, 33, 24, 64, 1, None) == -3
    assert lib.tsg_conv3x3_bnact_add_fwd(16, 16, 16, 16, 16, 1, 9, 33, 16, 96, 1, None) == -3
    assert lib.tsg_conv3x3_bnact_add_fwd(16, 16, 16, 16, 16, 1, 16384, 8192, 16, 64, 1, None) == -3
    assert lib.tsg_conv3x3_bnact_add_fwd(16, 16, 16, 24, 16, 1, 9, 33, 24, 64, 1, None) == -3
    for k in range(5):
        args = [16] * 5
        args[k] = 24 if k != 2 else 4
        assert lib.tsg_conv3x3_bnact_add_fwd(*args, 1, 9, 33, 16, 64, 1, None) == -4
    plan, ref = (ctypes.c_int * 5)(), (ctypes.c_int * 5)()
    for B, H, W, C, Cb, Cout, maps in CASES + HEADS:
        assert lib.tsg_conv3x3_bnact_add_plan(B, H, W, C, Cout, plan) == 0
        assert lib.tsg_conv3x3_bnact_plan(B, H, W, C, Cout, ref) == 0
        assert tuple(plan) == tuple(ref) and plan[4] == LDS                                   # the sibling's plan and LDS
    assert lib.tsg_conv3x3_bnact_add_plan(1, 9, 33, 24, 64, plan) == -3
    assert lib.tsg_conv3x3_bnact_add_plan(1, 9, 33, 24, 64, None) == -5


def test_the_largest_case_makes_a_block_walk_two_tiles():
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, H, W, C, Cb, Cout, maps = CASES[-1]
    ntiles, nslots, noct, grid, lds = kp.conv3x3_bnact_add_plan(B, H, W, C, Cout)
    assert (ntiles, nslots, noct, grid) == (72, 64, 8, 512) and ntiles > nslots
    for B, H, W, C, Cb, Cout, maps in CASES[:-1]:
        ntiles, nslots, _, _, _ = kp.conv3x3_bnact_add_plan(B, H, W, C, Cout)
        assert ntiles <= nslots


def test_provider_twins_check_their_arguments():
    from torchseg_amd import _lib, kernels as K
    kp = K.provider()
    assert kp.ppm_plan(1, 9, 33, STD, 32, 128)[:4] == (50, 12, 4 * 9 * 4, 9 * 2)
    with pytest.raises(_lib.TsgError):
        kp.ppm_plan(1, 9, 33, STD, 24, 128)
    assert kp.ppm_ws_bytes(1, 9, 33, STD, 24, 128) == 0 and kp.ppm_ws_bytes(1, 9, 33, STD, 32, 128) == kp.ppm_plan(1, 9, 33, STD, 32, 128)[5]
    x = torch.zeros(1, 16, 9, 33, dtype=torch.bfloat16)
    assert not kp.ppm_supported(x, STD, 16, 64)                                          # NCHW
    xc = x.contiguous(memory_format=torch.channels_last)
    assert kp.ppm_supported(xc, STD, 16, 64)
    assert not kp.ppm_supported(xc.float(), STD, 16, 64) and not kp.ppm_supported(xc, STD, 16, 96)
    assert not kp.ppm_supported(xc, STD + ((1, 1),), 16, 64) and not kp.ppm_supported(xc, (), 16, 64)
    T, E = kp.ppm_workspace(xc, STD, 16, 64)
    assert T.shape == (1, 50, 9, 64) and E.shape == (1, 9, 33, 64) and T.dtype == E.dtype == torch.float32
    assert T.data_ptr() % 16 == 0 and E.data_ptr() % 16 == 0 and E.data_ptr() >= T.data_ptr() + T.numel() * 4
    w = torch.arange(64 * 80 * 9, dtype=torch.float32).reshape(64, 80, 3, 3)
    wb = kp.ppm_pack_branches(w, 16, 4)
    assert wb.shape == (4, 9, 64, 16) and wb.dtype == torch.bfloat16 and wb.is_contiguous()
    assert torch.equal(wb[2, 5, 7], w[7, 16 + 2 * 16:16 + 3 * 16, 1, 2].to(torch.bfloat16))
    with pytest.raises(_lib.TsgError):
        kp.ppm_pack_branches(w, 16, 3)                                                   # 64 channels do not split in three
    ps = [torch.zeros(1, 16, s, s, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last) for s in (1, 2, 3, 6)]
    with pytest.raises(_lib.TsgError, match="pooled"):
        kp.ppm_taps_fwd(ps[:3], wb, T)
    with pytest.raises(_lib.TsgError, match="pooled"):
        kp.ppm_taps_fwd([p.float() for p in ps], wb, T)
    with pytest.raises(_lib.TsgError, match="T must"):
        kp.ppm_taps_fwd(ps, wb, T[:, :49])
    with pytest.raises(_lib.TsgError, match="needed"):
        kp.ppm_addend_fwd(T, STD[:3], E)
    wf, ab = torch.zeros(9 * 16 * 64, dtype=torch.bfloat16), torch.zeros(2, 64)
    with pytest.raises(_lib.TsgError, match="pack"):
        kp.conv3x3_bnact_add_fwd(xc, (wf[:-16], ab), 64, E, True)
    with pytest.raises(_lib.TsgError, match="addend"):
        kp.conv3x3_bnact_add_fwd(xc, (wf, ab), 64, E.permute(0, 3, 1, 2), True)
    with pytest.raises(_lib.TsgError, match="addend"):
        kp.conv3x3_bnact_add_fwd(xc, (wf, ab), 64, E.double(), True)


def test_host_plan_under_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path / "ppm_geom_check"
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "ppm_geom_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr


def test_kernels_do_not_spill_and_the_convolution_fits_two_blocks_per_cu(tmp_path_factory):
    """From the code object's metadata only.  Three kernels; no scratch, no spills; the convolution at most 256 VGPRs + AGPRs
    (two 4-wave blocks on a CU's four SIMDs are two waves per SIMD of a 512 register file) and twice its LDS inside the
    CU's 160 KB, one unrolled chunk of 9 taps x 2 channel blocks x 2 rows = 36 MFMAs as its sibling has; the addend kernel's
    row stage is 24,576 B of LDS; the tap kernel uses none; no atomics anywhere."""
    isa = _isa(tmp_path_factory, "ppmbn.hip")
    meta = _kernel_meta(isa)
    names = sorted(meta)
    assert len(names) == 3 and [sum(k in n for n in names) for k in ("ppm_taps_k", "ppm_addend_k", "pab_fwd_k")] == [1, 1, 1], names
    for name, (spill, scratch) in meta.items():
        assert spill == 0 and scratch == 0, (name, spill, scratch)
    blocks = isa.split("  - .agpr_count:")[1:]
    info = {}
    for blk in blocks:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        info[name] = dict(agpr=int(re.match(r"\s+(\d+)", blk).group(1)),
                          vgpr=int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                          lds=int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)),
                          sgpr_spill=int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)))
    by = {k: next(v for n, v in info.items() if k in n) for k in ("ppm_taps_k", "ppm_addend_k", "pab_fwd_k")}
    assert all(v["sgpr_spill"] == 0 for v in by.values()), by
    assert by["pab_fwd_k"]["vgpr"] + by["pab_fwd_k"]["agpr"] <= 256, by
    assert by["pab_fwd_k"]["lds"] == 0 and 2 * LDS <= 160 * 1024                     # dynamic: tsg_conv3x3_bnact_add_plan's LDS
    assert by["ppm_addend_k"]["lds"] == 3 * 32 * 16 * 16 and by["ppm_taps_k"]["lds"] == 0
    sib = _isa(tmp_path_factory, "convbn.hip")
    count = lambda text, name: len(re.findall(r"\n\s*v_mfma_f32_32x32x16_bf16", text[text.index("\n" + name + ":"):].split("s_endpgm")[0]))
    pab = next(n for n in meta if "pab_fwd_k" in n)
    cbn = next(n for n in _kernel_meta(sib) if "cbn_fwd_k" in n)
    assert count(isa, pab) == count(sib, cbn) > 0
    for name in meta:
        body = isa[isa.index("\n" + name + ":"):].split("s_endpgm")[0]
        assert "global_atomic" not in body and "buffer_atomic" not in body and "flat_atomic" not in body and "ds_add" not in body


# ---- the installer -----------------------------------------------------------------------------------------------------
def _head(seed=0, fc_dim=32, scales=(1, 2, 3, 6)):
    from torchseg_amd.workloads.pspnet import PyramidPooling
    torch.manual_seed(seed)
    return _randomise_bn(PyramidPooling("psp", 19, fc_dim=fc_dim, pool_scales=scales), seed + 1)


def test_installer_counts_and_state_dict():
    from torchseg_amd.convbn import _FusedCbr, install_fused_convbn
    from torchseg_amd.ppmbn import _FusedPyramid, eligible, install_fused_pyramid, pyramid_fused_calls
    from torchseg_amd.workloads.fcn import FCN
    from torchseg_amd.workloads.pspnet import PSANet, PyramidPooling
    for depth in (50, 101):
        net = _pspnet(depth)
        keys = list(net.state_dict().keys())
        assert [n for n, m in net.named_modules() if eligible(m)] == ["psp_layer"]
        assert install_fused_pyramid(net) == 1 and install_fused_pyramid(net) == 0
        assert isinstance(net.psp_layer, _FusedPyramid) and isinstance(net.psp_layer, PyramidPooling)
        assert sum(isinstance(m, _FusedPyramid) for m in net.modules()) == 1
        assert list(net.state_dict().keys()) == keys and pyramid_fused_calls(net) == 0
    torch.manual_seed(0)
    for other in (_r18(), PSANet(19, None, None, nn.BatchNorm2d, depth=50), FCN(19, None, True, None, nn.BatchNorm2d)):
        assert install_fused_pyramid(other) == 0 and not any(isinstance(m, _FusedPyramid) for m in other.modules())
    # after install_fused_convbn re-classed conv6[0], and before it: the same head either way
    a = _head()
    assert install_fused_convbn(a) == 1 and isinstance(a.conv6[0], _FusedCbr) and install_fused_pyramid(a) == 1
    b = _head()
    assert install_fused_pyramid(b) == 1 and install_fused_convbn(b) == 1 and isinstance(b, _FusedPyramid)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys()) == list(_head().state_dict().keys())
    assert copy.deepcopy(a).__class__ is a.__class__
    # what is not this head
    assert install_fused_pyramid(_head(scales=(1, 2, 3, 4, 6))) == 0                       # five branches
    assert install_fused_pyramid(_head(scales=(1,))) == 1 and install_fused_pyramid(_head(scales=((2, 3), (6, 4)))) == 1
    for hook_on in (lambda m: m, lambda m: m.conv6, lambda m: m.conv6[0], lambda m: m.conv6[0].bn, lambda m: m.ppm[1],
                    lambda m: m.ppm[2][1].conv):
        hooked = _head()
        hook_on(hooked).register_forward_hook(lambda *a: None)
        assert install_fused_pyramid(hooked) == 0, hook_on
    wrong = _head()
    wrong.conv6[0].conv.stride = (2, 2)
    assert install_fused_pyramid(wrong) == 0
    wrong = _head()
    wrong.ppm[1][1] = nn.Conv2d(32, 512, 1)                                                # not ConvBnRelu-shaped
    assert install_fused_pyramid(wrong) == 0
    wrong = _head()
    wrong.ppm = nn.ModuleList(list(wrong.ppm)[:3])                                         # conv6 expects C + 4 Cb channels
    assert install_fused_pyramid(wrong) == 0
    wrong = _head()
    wrong.conv6[0].has_bn = False
    assert install_fused_pyramid(wrong) == 0
    assert install_fused_pyramid(nn.Sequential(_head(), _head())) == 2


@pytest.mark.parametrize("with_convbn", [False, True], ids=["alone", "after-convbn"])
def test_reclassed_head_is_the_stock_head_wherever_the_chain_does_not_apply(with_convbn):
    """CPU input in eval mode, train mode, and gradients enabled (every parameter gradient too): bit-identical."""
    from torchseg_amd.convbn import install_fused_convbn
    from torchseg_amd.ppmbn import install_fused_pyramid, pyramid_fused_calls
    stock = _head(2)
    ours = copy.deepcopy(stock)
    if with_convbn:
        assert install_fused_convbn(ours) == 1
    assert install_fused_pyramid(ours) == 1
    assert list(ours.state_dict().keys()) == list(stock.state_dict().keys())
    x = torch.randn(2, 32, 8, 16, generator=torch.Generator().manual_seed(5))
    stock.eval(), ours.eval()
    with torch.no_grad():
        assert torch.equal(stock(x), ours(x))
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert torch.equal(stock(x), ours(x))
    stock.train(), ours.train()
    with torch.no_grad():
        outs = []
        for net in (stock, ours):
            torch.manual_seed(9)                                 # Dropout2d draws alike
            outs.append(net(x))
        assert torch.equal(outs[0], outs[1])
    for (k, u), (_, v) in zip(stock.state_dict().items(), ours.state_dict().items()):
        assert torch.equal(u, v), k                              # the running statistics moved alike
    for mode in (True, False):                                   # gradients enabled, in train and in eval mode
        stock.train(mode), ours.train(mode)
        outs = []
        for net in (stock, ours):
            net.zero_grad(set_to_none=True)
            torch.manual_seed(9)                                 # Dropout2d draws alike
            y = net(x)
            y.square().mean().backward()
            outs.append(y.detach())
        assert torch.equal(outs[0], outs[1])
        for (n, p), (_, q) in zip(stock.named_parameters(), ours.named_parameters()):
            assert (p.grad is None) == (q.grad is None), n
            if p.grad is not None:
                assert torch.equal(p.grad, q.grad), n
    assert pyramid_fused_calls(ours) == 0


def test_prepare_inference_switch_defaults_to_off(monkeypatch):
    """The signature carries the switch with None as its default; then TSG_PPMBN_FUSED decides, and unset means off (no GPU:
    the constructor is not run here, tests/test_ppmbn_gpu.py covers the effect).  The switch is documented with the others,
    it is installed after them, and the DDP side never installs this."""
    import inspect
    from torchseg_amd import infer, ppmbn
    import torchseg_amd.ddp as ddp
    for fn in (infer.prepare_inference, infer.InferenceModule.__init__):
        assert inspect.signature(fn).parameters["fuse_pyramid"].default is None
    src = inspect.getsource(infer.InferenceModule.__init__)
    assert 'ddp._env_flag("TSG_PPMBN_FUSED", False)' in src and "install_fused_pyramid(self.module)" in src
    for other in ("TSG_SEPCONV_FUSED", "TSG_CONVBN_FUSED", "TSG_DILBN_FUSED", "TSG_S2BN_FUSED", "TSG_PWBN_FUSED", "TSG_STEMBN_FUSED"):
        assert src.index(other) < src.index("TSG_PPMBN_FUSED")
    monkeypatch.delenv("TSG_PPMBN_FUSED", raising=False)
    assert ddp._env_flag("TSG_PPMBN_FUSED", False) is False
    monkeypatch.setenv("TSG_PPMBN_FUSED", "0")
    assert ddp._env_flag("TSG_PPMBN_FUSED", False) is False
    monkeypatch.setenv("TSG_PPMBN_FUSED", "1")
    assert ddp._env_flag("TSG_PPMBN_FUSED", False) is True
    assert "install_fused_pyramid" not in inspect.getsource(ddp)
    for doc in (infer.__doc__, ppmbn.__doc__):
        assert "TSG_PPMBN_FUSED" in doc
