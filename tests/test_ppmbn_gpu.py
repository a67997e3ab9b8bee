"""GPU: PSPNet's pyramid pooling head without the concatenation (csrc/ppmbn.hip, torchseg_amd/ppmbn.py) against torch's CPU
float64 `F.interpolate(align_corners=True)` + `torch.cat` + `F.conv2d` on the operands the kernels read (x and the pooled
maps already bf16, the weight rounded to bf16).  The reference is never the code under test.

  1. exact data: every intermediate is exact in fp32 in any order, the output must be BIT-equal to float64 rounded once;
  2. random data within a per-element bound derived from the formats (see _ppm_tol), each stage (T, E) against its own
     float64 value as well, so that a failure names its stage;
  3. the bound has teeth, inside the same tests: two float64 variants (pooled channels replicate-padded; the addend
     dropped) exceed 4 x the bound;
  4. operands, workspace and output inside poisoned guard bands, three calls bit-identical, the same result at 16-byte
     aligned offsets inside larger allocations, and tsg_conv3x3_bnact_add_fwd with E = 0 bit-equal to tsg_conv3x3_bnact_fwd;
  5. the module: a PyramidPooling on an 8 x 16 map against the float64 composition evaluated on the device's own pooled
     maps, the counters, untouched operands, the stock path in train mode and with gradients enabled, the pack cache;
  6. PSPNet-R50 through prepare_inference(fuse_pyramid=True): counts, eager against graph replay, the pending tail, the
     distance from the fp32 parity run, the other networks, and the switch's default.

Kernel cases are (B, H, W, C, Cb, Cout, pooled maps): tests/test_ppmbn_cpu.py says what each one catches."""
import copy
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _guard
from test_convbn_cpu import _r18, _randomise_bn
from test_convbn_gpu import BF, CL, U32, _bn_ab, _fused_tol, _gamma, _rel
from test_dilbn_cpu import _pspnet
from test_ppmbn_cpu import CASES, EXACT_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
if FURNACE not in sys.path:
    sys.path.insert(0, FURNACE)

pytestmark = pytest.mark.gpu

_ids = lambda c: "x".join(map(str, c[:6])) + "-" + "_".join("%dx%d" % m for m in c[6])


@pytest.fixture(autouse=True)
def _restore_process_globals(monkeypatch):
    """prepare_inference switches syncbn.PREFER_CHANNELS_LAST_OUTPUT on for the process"""
    from torchseg_amd import syncbn
    monkeypatch.setattr(syncbn, "PREFER_CHANNELS_LAST_OUTPUT", syncbn.PREFER_CHANNELS_LAST_OUTPUT)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", torch.backends.cudnn.benchmark)


@pytest.fixture
def _pin_vendor_library(monkeypatch):
    """The pools' branch convolutions, the classifier and the stock path of a declined call run the vendor library, which
    repeats from call to call only when it is asked for its deterministic kernels (tests/test_convbn_gpu.py says why); the
    kernels of this feature do not read the setting."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


# ---- operands and the float64 reference ----------------------------------------------------------------------------------
def _operands(case, exact, seed=0):
    """CPU operands: x and the pooled maps already rounded to bf16, w fp32 [Cout, C + n Cb, 3, 3], fp32 a, b"""
    B, H, W, C, Cb, Cout, maps = case
    n = len(maps)
    g = torch.Generator().manual_seed(seed + 1000 * C + Cout + 7 * H + Cb)
    if exact:
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
        x = ri(-2, 2, B, C, H, W)
        ps = [ri(-2, 2, B, Cb, sh, sw) for sh, sw in maps]
        w = ri(-1, 1, Cout, C + n * Cb, 3, 3)
        a = torch.pow(2.0, ri(-1, 1, Cout))
        b = ri(-16, 16, Cout) / 4
    else:
        x = torch.randn(B, C, H, W, generator=g)
        ps = [torch.randn(B, Cb, sh, sw, generator=g) for sh, sw in maps]
        w = torch.randn(Cout, C + n * Cb, 3, 3, generator=g) * (2.0 / (9 * (C + n * Cb))) ** 0.5
        a = 0.5 + torch.rand(Cout, generator=g)
        a = a * torch.where(torch.rand(Cout, generator=g) < 0.25, -1.0, 1.0)
        b = torch.randn(Cout, generator=g) * 0.5
    return x.to(BF), [p.to(BF) for p in ps], w, a, b


def _up64(p, H, W):
    return F.interpolate(p, size=(H, W), mode="bilinear", align_corners=True)


def _stages64(x, ps, w, C, H, W):
    """float64, of operands that are float64 already: (u_x, E, T, S_x, M)
      u_x [B,Cout,H,W]  the convolution of x with W[:, :C];   S_x the same of the absolute values
      E   [B,Cout,H,W]  the convolution of cat(up(p_s)) with W[:, C:] (zero padding of the concatenated tensor)
      T   [B,cells,9,Cout]  the tap tables;  S_T the same of the absolute values
      M   [B,Cout,1,1]  sum over branches and taps of the largest S_T of the branch's cells: no path through the staged
                        interpolation (whatever taps its fp32 indices pick) sums to more than M in absolute value"""
    Cb = ps[0].shape[1]
    u_x = F.conv2d(x, w[:, :C], None, 1, 1)
    S_x = F.conv2d(x.abs(), w[:, :C].abs(), None, 1, 1)
    E = F.conv2d(torch.cat([_up64(p, H, W) for p in ps], 1), w[:, C:], None, 1, 1)
    T, M = [], 0.0
    for s, p in enumerate(ps):
        ws = w[:, C + s * Cb:C + (s + 1) * Cb].reshape(w.shape[0], Cb, 9)                       # [oc][cb][tap]
        pc = p.permute(0, 2, 3, 1).reshape(p.shape[0], -1, Cb)                                 # [b][cell][cb]
        T.append(torch.einsum("bnc,oct->bnto", pc, ws))
        M = M + torch.einsum("bnc,oct->bnto", pc.abs(), ws.abs()).amax(dim=1).sum(dim=1)       # [b][oc]
    return u_x, E, torch.cat(T, 1), S_x, M.view(M.shape[0], -1, 1, 1)


_REF = {}


def _ref64(case, exact, seed=0):
    """(operands, stages): computed once per case and shared"""
    key = (case, exact, seed)
    if key not in _REF:
        ops = _operands(case, exact, seed)
        x, ps, w, a, b = ops
        _REF[key] = (ops, _stages64(x.double(), [p.double() for p in ps], w.to(BF).double(), case[3], case[1], case[2]))
    return _REF[key]


def _epilogue64(u, a, b, relu):
    v = a.double().view(1, -1, 1, 1) * u + b.double().view(1, -1, 1, 1)
    return v.clamp_min(0.0) if relu else v


# ---- the bound -------------------------------------------------------------------------------------------------------------
def _lambda_err(maps):
    """Bound of the error of ONE interpolation weight formed in fp32 as tsg_resample.h forms it: scale = fl((in - 1) /
    (out - 1)) and r = fl(scale dst) carry one rounding each, so |r - src| <= 2.01 u src <= 2.01 u (in - 1); l1 = r - i0 is
    exact and l0 = fl(1 - l1) adds u.  Where the fp32 r falls on the other side of an integer than src does, the kernel's
    pair of taps is shifted by one and its weights are within the same distance of (0, 1): the value moves by no more."""
    big = max(max(m) for m in maps)
    return (2.01 * (big - 1) + 1) * U32


def _e_tol(case, M):
    """|E_kernel - E64| per element <= M (gamma_Cb + gamma_40 + 4 dl):
      gamma_Cb  T is an fp32 accumulation of Cb exact products of bf16 values, in any order; the interpolation weights of a
                tap and a branch are non-negative and sum to 1, and over taps and branches the |T| involved sum to <= M
      gamma_40  the staged interpolation in fp32: per tap and branch two products and an addition in the row stage and again
                in the pixel stage, and the running sums over 3 kh and over 3 kw x n <= 4 branches: fewer than 40 roundings
                on any path from a T value to E
      4 dl      each direction's two weights are off by at most dl = _lambda_err each: 2 dl |v| per direction"""
    return M * (_gamma(case[4]) + _gamma(40) + 4 * _lambda_err(case[6]))


def _ppm_tol(case, y64, a, b, S_x, M):
    """_fused_tol of tests/test_convbn_gpu.py with K = 9 (C + n Cb) over the magnitude S_x + M of everything that is summed
    (the convolution's accumulation and T's, in any order), 2.01 u of the magnitudes for the roundings of `acc + E` and of
    the fma, and the extra roundings of the staged interpolation and of the fp32 weights (the gamma_40 + 4 dl part of
    _e_tol) handed in as the error of an operand, scaled by |a|."""
    B, H, W, C, Cb, Cout, maps = case
    aa = a.double().abs().view(1, -1, 1, 1)
    aS = aa * (S_x + M)
    mag = 2 * aS + b.double().abs().view(1, -1, 1, 1)
    extra = aa * M * (_gamma(40) + 4 * _lambda_err(maps))
    return _fused_tol(y64, aS, mag, 9 * (C + len(maps) * Cb), extra)


# ---- running the chain -------------------------------------------------------------------------------------------------------
def _device_operands(ops, dev):
    x, ps, w, a, b = ops
    fp = torch.stack([a, b, torch.zeros_like(a)]).to(dev)
    return (x.to(dev).contiguous(memory_format=CL), [p.to(dev).contiguous(memory_format=CL) for p in ps], w.to(dev), fp)


def _chain(kp, case, xd, pd, wd, fp, relu):
    """the three launches on device operands -> (y, T, E)"""
    B, H, W, C, Cb, Cout, maps = case
    pack = kp.conv3x3_bnact_pack(wd[:, :C], None, fp)
    wb = kp.ppm_pack_branches(wd, C, len(maps))
    T, E = kp.ppm_workspace(xd, maps, Cb, Cout)
    kp.ppm_taps_fwd(list(pd), wb, T)
    kp.ppm_addend_fwd(T, maps, E)
    return kp.conv3x3_bnact_add_fwd(xd, pack, Cout, E, relu), T, E


@pytest.mark.parametrize("case", EXACT_CASES, ids=_ids)
def test_exact_data_is_bit_equal_to_float64(cuda, case):
    """x and p_s integers in [-2, 2], w in {-1, 0, 1}, a in {1/2, 1, 2}, b multiples of 1/4; H - 1 and W - 1 powers of two, so
    every interpolation weight is dyadic and exact in fp32: T is an integer, E a multiple of 2^-9 below 2^8, a (u + E) + b a
    multiple of 2^-10 below 2^12 -- exact in fp32 in any order; the only rounding is the last one."""
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, H, W, C, Cb, Cout, maps = case
    ops, (u_x, E64, T64, _, _) = _ref64(case, True)
    x, ps, w, a, b = ops
    xd, pd, wd, fp = _device_operands(ops, cuda)
    assert kp.ppm_supported(xd, maps, Cb, Cout)
    assert torch.equal(E64 * 512, (E64 * 512).round()) and float((u_x + E64).abs().max()) * 2 + 8 < 2 ** 12
    _teeth(case, True)                                                      # the bound of the random test, on this data too
    for relu in (True, False):
        y, T, E = _chain(kp, case, xd, pd, wd, fp, relu)
        torch.cuda.synchronize()
        assert torch.equal(T.cpu().double(), T64), "stage 1 (T)"
        assert torch.equal(E.cpu().double().permute(0, 3, 1, 2), E64), "stage 2 (E)"
        want = _epilogue64(u_x + E64, a, b, relu)
        assert torch.equal(want, want.float().double())                 # the float64 value is an fp32 number
        want = want.float().to(BF)
        assert y.dtype == BF and y.shape == want.shape and y.is_contiguous(memory_format=CL)
        got = y.cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
            (case, relu, int((got != want).sum()), float((got.float() - want.float()).abs().max()))


def _report(what, err, tol):
    print("ppmbn %s: max err %.3e, max err / tol %.3f" % (what, float(err.max()), float((err / tol).max())))
    bad = ~(err <= tol)
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err - tol).max()))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_random_data_against_float64_stage_by_stage(cuda, case):
    """T within gamma_Cb sum|w||p| per element, E within _e_tol, y within _ppm_tol; see their docstrings."""
    from torchseg_amd import kernels as K
    kp = K.provider()
    B, H, W, C, Cb, Cout, maps = case
    ops, (u_x, E64, T64, S_x, M) = _ref64(case, False)
    x, ps, w, a, b = ops
    xd, pd, wd, fp = _device_operands(ops, cuda)
    keep = [xd.clone()] + [p.clone() for p in pd]
    _teeth(case, False)                                                     # a bound that these variants pass would show nothing
    wq = w.to(BF).double()
    S_T = torch.cat([torch.einsum("bnc,oct->bnto", p.double().permute(0, 2, 3, 1).reshape(B, -1, Cb).abs(),
                                  wq[:, C + s * Cb:C + (s + 1) * Cb].reshape(Cout, Cb, 9).abs()) for s, p in enumerate(ps)], 1)
    for relu in (True, False):
        y, T, E = _chain(kp, case, xd, pd, wd, fp, relu)
        y2, T2, E2 = _chain(kp, case, xd, pd, wd, fp, relu)
        torch.cuda.synchronize()
        for u, v in ((y, y2), (T, T2), (E, E2)):
            assert torch.equal(_guard.raw_bytes(u), _guard.raw_bytes(v))    # bit-identical from launch to launch
        _report("T %s" % (case,), (T.cpu().double() - T64).abs(), _gamma(Cb) * S_T + 1e-300)
        _report("E %s" % (case,), (E.cpu().double().permute(0, 3, 1, 2) - E64).abs(), _e_tol(case, M).expand_as(E64))
        y64 = _epilogue64(u_x + E64, a, b, relu)
        _report("y %s relu=%s" % (case, relu), (y.double().cpu() - y64).abs(), _ppm_tol(case, y64, a, b, S_x, M))
    for t, k in zip([xd] + list(pd), keep):
        assert torch.equal(_guard.raw_bytes(t), _guard.raw_bytes(k))       # the operands are never written


def _teeth(case, exact):
    """On the CPU, in float64: the variant whose pooled channels are replicate-padded instead of zero-padded must exceed
    4 x the bound on at least one element of each of the four border lines and on no interior element; the variant with the
    addend dropped must exceed it on more than half of the elements."""
    B, H, W, C, Cb, Cout, maps = case
    ops, (u_x, E64, T64, S_x, M) = _ref64(case, exact)
    x, ps, w, a, b = ops
    wq = w.to(BF).double()
    y64 = _epilogue64(u_x + E64, a, b, True)
    tol = _ppm_tol(case, y64, a, b, S_x, M)
    up = torch.cat([_up64(p.double(), H, W) for p in ps], 1)
    E_rep = F.conv2d(F.pad(up, (1, 1, 1, 1), mode="replicate"), wq[:, C:], None, 1, 0)
    over = (_epilogue64(u_x + E_rep, a, b, True) - y64).abs() > 4 * tol
    assert not bool(over[:, :, 1:-1, 1:-1].any())
    for name, line in (("top", over[:, :, 0]), ("bottom", over[:, :, -1]), ("left", over[:, :, :, 0]), ("right", over[:, :, :, -1])):
        assert bool(line.any()), (case, exact, name)
    over = (_epilogue64(u_x, a, b, True) - y64).abs() > 4 * tol
    share = float(over.double().mean())
    print("ppmbn teeth %s exact=%s: addend dropped: %.1f %% of the elements beyond 4 x the bound" % (case, exact, 100 * share))
    assert share > 0.5, (case, exact, share)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_inside_guard_bands(cuda, case):
    """Operands in guarded arenas, the packs, the workspace and the output allocated through Guarded(fill) under both fills:
    no guard byte moves and the three results (y, T and E) are bit-identical; then the raw entry points with x, the pooled
    maps, the workspace and y at 16-byte-aligned offsets inside larger poisoned allocations: the same bits, and not a byte
    around y has moved; E = 0 makes tsg_conv3x3_bnact_add_fwd bit-equal to tsg_conv3x3_bnact_fwd."""
    import ctypes
    from torchseg_amd import _lib, kernels as K
    kp = K.provider()
    B, H, W, C, Cb, Cout, maps = case
    n = len(maps)
    ops, (u_x, E64, T64, S_x, M) = _ref64(case, False, seed=3)
    x, ps, w, a, b = ops
    xd, pd, wd, fp = _device_operands(ops, cuda)

    def head(xx, pp, ww, fwd_pack):
        return _chain(kp, case, xx, pp, ww, fwd_pack, True)

    plain, Tp, Ep = _guard.three_calls(head, [xd, tuple(pd), wd, fp])[0]
    y64 = _epilogue64(u_x + E64, a, b, True)
    _report("guarded y %s" % (case,), (plain.double().cpu() - y64).abs(), _ppm_tol(case, y64, a, b, S_x, M))

    def inside(t, off, fill, dtype=BF):
        """t's dense bytes (NHWC for a 4-d bf16 tensor) at element offset `off` of a larger poisoned buffer -> (buffer, view)"""
        numel = t.numel()
        raw = torch.full((numel + 2 * off + 64,), fill, dtype=torch.int16 if dtype == BF else torch.int32, device=cuda)
        buf = raw.view(dtype)
        flat = buf[off:off + numel]
        if dtype == BF:
            return buf, flat.view(t.shape[0], t.shape[2], t.shape[3], t.shape[1]).permute(0, 3, 1, 2)
        return buf, flat.view(t.shape)

    wf, ab = kp.conv3x3_bnact_pack(wd[:, :C], None, fp)
    wb = kp.ppm_pack_branches(wd, C, n)
    bx, vx = inside(xd, 8, -1)
    vx.copy_(xd)
    vps = []
    for s, p in enumerate(pd):
        _, vp = inside(p, 8 * (s + 1), -1)
        vp.copy_(p)
        vps.append(vp)
    bT, vT = inside(Tp, 4, -1, torch.float32)
    bE, vE = inside(Ep, 12, -1, torch.float32)
    by, vy = inside(plain, 24, 0x5a5a)
    assert vx.data_ptr() % 32 == 16 and vT.data_ptr() % 32 == 16 and vE.data_ptr() % 16 == 0 and vy.data_ptr() % 16 == 0
    sh, sw = (ctypes.c_int * n)(*[m[0] for m in maps]), (ctypes.c_int * n)(*[m[1] for m in maps])
    st = _lib.stream_ptr(vx)
    ptrs = [p.data_ptr() for p in vps] + [None] * (4 - n)
    _lib.call(kp.lib.tsg_ppm_taps_fwd, *ptrs, wb.data_ptr(), vT.data_ptr(), B, n, sh, sw, Cb, Cout, st)
    _lib.call(kp.lib.tsg_ppm_addend_fwd, vT.data_ptr(), vE.data_ptr(), B, H, W, n, sh, sw, Cout, st)
    _lib.call(kp.lib.tsg_conv3x3_bnact_add_fwd, vx.data_ptr(), wf.data_ptr(), ab.data_ptr(), vE.data_ptr(), vy.data_ptr(),
              B, H, W, C, Cout, 1, st)
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(vT), _guard.raw_bytes(Tp)) and torch.equal(_guard.raw_bytes(vE), _guard.raw_bytes(Ep))
    assert torch.equal(_guard.raw_bytes(vy), _guard.raw_bytes(plain))
    raw = by.view(torch.int16)
    assert bool((raw[:24] == 0x5a5a).all()) and bool((raw[24 + plain.numel():] == 0x5a5a).all())
    for buf, view, off in ((bT, vT, 4), (bE, vE, 12)):
        r = buf.view(torch.int32)
        assert bool((r[:off] == -1).all()) and bool((r[off + view.numel():] == -1).all())
    # a misaligned operand is refused before any launch
    assert kp.lib.tsg_conv3x3_bnact_add_fwd(vx.data_ptr(), wf.data_ptr(), ab.data_ptr(), vE.data_ptr() + 4, vy.data_ptr(),
                                            B, H, W, C, Cout, 1, st) == -4
    assert kp.lib.tsg_ppm_addend_fwd(vT.data_ptr() + 8, vE.data_ptr(), B, H, W, n, sh, sw, Cout, st) == -4
    assert kp.lib.tsg_ppm_taps_fwd(*ptrs, wb.data_ptr() + 2, vT.data_ptr(), B, n, sh, sw, Cb, Cout, st) == -4
    # E = 0: the sibling kernel's bits
    zero = torch.zeros(B, H, W, Cout, dtype=torch.float32, device=cuda)
    for relu in (True, False):
        ya = kp.conv3x3_bnact_add_fwd(xd, (wf, ab), Cout, zero, relu)
        yb = kp.conv3x3_bnact_fwd(xd, (wf, ab), Cout, None, relu)
        torch.cuda.synchronize()
        assert torch.equal(_guard.raw_bytes(ya), _guard.raw_bytes(yb)), relu


# ---- the module ----------------------------------------------------------------------------------------------------------------
def _head(seed, fc_dim=32, scales=(1, 2, 3, 6)):
    from torchseg_amd.workloads.pspnet import PyramidPooling
    torch.manual_seed(seed)
    return _randomise_bn(PyramidPooling("psp", 19, fc_dim=fc_dim, pool_scales=scales), seed + 1).eval()


def _record(monkeypatch, kp):
    """the pooled maps handed to tsg_ppm_taps_fwd and the output of tsg_conv3x3_bnact_add_fwd, per call"""
    seen = dict(pooled=[], y=[])
    taps, add = kp.ppm_taps_fwd, kp.conv3x3_bnact_add_fwd
    monkeypatch.setattr(kp, "ppm_taps_fwd", lambda pooled, wb, T: seen["pooled"].append([p.clone() for p in pooled]) or taps(pooled, wb, T))

    def add_fwd(*a):
        y = add(*a)
        seen["y"].append(y)
        return y
    monkeypatch.setattr(kp, "conv3x3_bnact_add_fwd", add_fwd)
    return seen


def _head_check(mod, x, seen, dev, what):
    """the fused layer's output of the last call against the float64 composition on the device's own pooled maps"""
    conv, bn = mod.conv6[0].conv, mod.conv6[0].bn
    ps = [p.cpu() for p in seen["pooled"][-1]]
    C, Cb, Cout = x.shape[1], ps[0].shape[1], conv.out_channels
    case = (x.shape[0], x.shape[2], x.shape[3], C, Cb, Cout, tuple(tuple(p.shape[2:]) for p in ps))
    u_x, E64, _, S_x, M = _stages64(x.double(), [p.double() for p in ps], conv.weight.detach().cpu().to(BF).double(), C,
                                    x.shape[2], x.shape[3])
    a, b = _bn_ab(bn, dev)
    y64 = (a * (u_x + E64) + b).clamp_min(0.0)
    _report("module %s" % what, (seen["y"][-1].double().cpu() - y64).abs(),
            _ppm_tol(case, y64, a.view(-1).float(), b.view(-1).float(), S_x, M))


def test_module(cuda, monkeypatch, _pin_vendor_library):
    from torchseg_amd import kernels as K
    from torchseg_amd.infer import prepare_inference
    from torchseg_amd.ppmbn import _FusedPyramid, pyramid_fused_calls
    base = _head(5)
    keys = list(base.state_dict().keys())
    on = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_pyramid=True)
    off = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_pyramid=False)
    assert on.fused_pyramid == 1 and off.fused_pyramid == 0 and isinstance(on.module, _FusedPyramid)
    assert list(on.module.state_dict().keys()) == keys
    seen = _record(monkeypatch, K.provider())
    x = torch.randn(2, 32, 8, 16, generator=torch.Generator().manual_seed(8)).to(BF)
    xd = x.to(cuda).contiguous(memory_format=CL)
    keep = xd.clone()
    out = on(xd)
    torch.cuda.synchronize()
    assert pyramid_fused_calls(on.module) == 1 and len(seen["y"]) == 1 and out.shape == (2, 19, 8, 16)
    assert torch.equal(_guard.raw_bytes(xd), _guard.raw_bytes(keep))
    assert [tuple(p.shape) for p in seen["pooled"][0]] == [(2, 512, s, s) for s in (1, 2, 3, 6)]
    _head_check(on.module, x, seen, cuda, "first call")
    # what follows the fused layer is conv6[1:], as the modules run it
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        rest = on.module.conv6[2](on.module.conv6[1](seen["y"][0]))
    assert torch.equal(_guard.raw_bytes(rest), _guard.raw_bytes(out))
    # train mode, and eval mode with gradients enabled: the stock method, bit for bit; the counter does not move
    stock_cls = type(off.module)

    def run(m, train, grad):
        m.train(train)
        torch.manual_seed(9)                                                # Dropout2d draws alike in train mode
        with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=BF):
            o = m(xd).detach().clone()
        m.eval()
        return o

    for train, grad in ((False, True), (True, False), (True, True)):
        a, b = run(on.module, train, grad), run(off.module, train, grad)
        torch.cuda.synchronize()
        assert pyramid_fused_calls(on.module) == 1 and len(seen["y"]) == 1, (train, grad)
        assert torch.equal(_guard.raw_bytes(a), _guard.raw_bytes(b)), (train, grad)
    assert isinstance(on.module, stock_cls)
    for (k, p), (_, q) in zip(on.module.state_dict().items(), off.module.state_dict().items()):
        assert torch.equal(p, q), k                                         # the running statistics moved alike
    # the pack cache: an in-place write to running_var, then a whole state dict
    before = on(xd).clone()
    with torch.no_grad():
        on.module.conv6[0].bn.running_var.mul_(4.0)
    after = on(xd).clone()
    torch.cuda.synchronize()
    assert pyramid_fused_calls(on.module) == 3 and not torch.equal(before, after)
    _head_check(on.module, x, seen, cuda, "after running_var.mul_(4)")
    on.module.load_state_dict(_head(17).state_dict())
    on(xd)
    torch.cuda.synchronize()
    assert pyramid_fused_calls(on.module) == 4
    _head_check(on.module, x, seen, cuda, "after load_state_dict")
    # a hook on the fused layer: the call is the stock one (the hook fires), the counter does not move
    fired = []
    h = on.module.conv6[0].register_forward_hook(lambda *a: fired.append(1))
    on(xd)
    h.remove()
    assert fired == [1] and pyramid_fused_calls(on.module) == 4
    # a conv6[0] that install_fused_convbn re-classed: a declined call is the replaced method, that layer's own fused
    # forward included (a hook on a branch), or its stock one (gradients enabled)
    from torchseg_amd.convbn import fused_calls
    both = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=True, fuse_pyramid=True)
    only = prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_convbn=True, fuse_pyramid=False)
    assert both.fused_pyramid == 1 and both.fused_convbn == only.fused_convbn == 1
    both(xd)
    assert pyramid_fused_calls(both.module) == 1 and fused_calls(both.module) == 0
    a, b = run(both.module, False, True), run(only.module, False, True)
    assert torch.equal(_guard.raw_bytes(a), _guard.raw_bytes(b)) and pyramid_fused_calls(both.module) == 1
    assert fused_calls(both.module) == 0
    h = both.module.ppm[0].register_forward_hook(lambda *a: None)
    a, b = both(xd).clone(), only(xd).clone()
    h.remove()
    torch.cuda.synchronize()
    assert torch.equal(_guard.raw_bytes(a), _guard.raw_bytes(b))
    # (whether conv6[0]'s own kernel takes the stock head's concatenated tensor is that layer's gate: the same in both)
    assert pyramid_fused_calls(both.module) == 1 and fused_calls(both.module) == fused_calls(only.module)


# ---- PSPNet-R50 --------------------------------------------------------------------------------------------------------------------
ALL_ON = dict(fuse_convbn=True, fuse_pointwise=True, fuse_dilated=True, fuse_strided=True, fuse_stem=True)


def _psp50(seed):
    return _randomise_bn(_pspnet(50, seed), seed + 1).eval()


def test_pspnet_r50_counts_eager_graph_and_pending_tail(cuda, _pin_vendor_library):
    from torchseg_amd import convbn, pwbn, stembn
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import pending_tail, prepare_inference
    from torchseg_amd.ppmbn import pyramid_fused_calls
    net = _psp50(21).to(cuda)
    off = prepare_inference(copy.deepcopy(net), dtype=BF, fuse_pyramid=False, **ALL_ON)
    eager = prepare_inference(copy.deepcopy(net), dtype=BF, fuse_pyramid=True, **ALL_ON)
    graph = prepare_inference(copy.deepcopy(net), dtype=BF, fuse_pyramid=True, graph=True, **ALL_ON)
    assert eager.fused_pyramid == 1 and graph.fused_pyramid == 1 and off.fused_pyramid == 0
    for name in ("fused_convbn", "fused_pointwise", "fused_dilated", "fused_strided", "fused_stem", "fused_separable"):
        assert getattr(eager, name) == getattr(off, name), name
    replays = []
    for k, seed in enumerate((1, 2)):
        x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(seed)).to(cuda)
        out = eager(x)
        tail = pending_tail(out)
        assert tail is not None and tuple(tail[1]) == (64, 128) and tail[0].shape[1] == 19     # still the pending head
        a = materialize(out).clone()
        b = graph(x).clone()
        torch.cuda.synchronize()
        assert a.shape == (1, 19, 64, 128) and bool(torch.isfinite(a).all())
        assert torch.equal(a, b), (seed, float((a - b).abs().max()))
        assert pyramid_fused_calls(eager.module) == k + 1                  # one fused forward per call
        replays.append(b)
    assert not torch.equal(replays[0], replays[1])
    assert pyramid_fused_calls(graph.module) == 2                          # the warm-up and the capture
    materialize(off(x))
    materialize(off(x))
    assert pyramid_fused_calls(off.module) == 0
    # the other installers' launches are what they are with the switch off, but for conv6[0]'s own: the fused head never
    # calls that layer, and the count drops by exactly the launches it made with the switch off.  Measured: that is 0,
    # not the one launch per call the feature's issue assumed -- torch.cat of the channels_last x and up-sampled maps returns
    # an NCHW-contiguous bf16 tensor (strides (524288, 128, 16, 1) here), and convbn._input_ok asks for channels_last, so
    # today's conv6[0] runs on the vendor library even with fuse_convbn=True.  The assertion holds for either
    # outcome (0, or 2 should that layer's gate ever take the tensor); the printed line records which one it was.
    head_off, head_on = off.module.psp_layer.conv6[0], eager.module.psp_layer.conv6[0]
    assert isinstance(head_off, convbn._FusedConvBn) and isinstance(head_on, convbn._FusedConvBn)
    print("ppmbn counts: conv6[0] made %d fused launches in 2 calls with the switch off, %d with it on; convbn.fused_calls "
          "%d off, %d on" % (head_off.tsg_fused_calls, head_on.tsg_fused_calls, convbn.fused_calls(off.module),
                             convbn.fused_calls(eager.module)))
    assert head_on.tsg_fused_calls == 0 and head_off.tsg_fused_calls in (0, 2)
    assert convbn.fused_calls(eager.module) == convbn.fused_calls(off.module) - head_off.tsg_fused_calls
    assert convbn.dil_fused_calls(eager.module) == convbn.dil_fused_calls(off.module)
    assert convbn.s2_fused_calls(eager.module) == convbn.s2_fused_calls(off.module)
    assert pwbn.fused_calls(eager.module) == pwbn.fused_calls(off.module)
    assert stembn.fused_calls(eager.module) == stembn.fused_calls(off.module)


def test_pspnet_r50_logits_against_the_fp32_parity_run(cuda, _pin_vendor_library):
    """With the head fused (every other switch on in every arm) the bf16 log-probabilities are at most 1.25 x as far from the
    fp32 parity run as with the switch off: the project's factor for this comparison.  The ratio printed here is
    profiles/ppmbn_parity.txt."""
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    from torchseg_amd.ppmbn import pyramid_fused_calls
    base = _psp50(11)
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(14)).to(cuda)
    arms = dict(parity=prepare_inference(copy.deepcopy(base).to(cuda), dtype=torch.float32, fuse_pyramid=True, **ALL_ON),
                unfused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_pyramid=False, **ALL_ON),
                fused=prepare_inference(copy.deepcopy(base).to(cuda), dtype=BF, fuse_pyramid=True, **ALL_ON))
    outs = {k: materialize(m(x)).clone() for k, m in arms.items()}
    torch.cuda.synchronize()
    assert pyramid_fused_calls(arms["fused"].module) == 1 and pyramid_fused_calls(arms["unfused"].module) == 0
    assert pyramid_fused_calls(arms["parity"].module) == 0                  # fp32: the parity mode stays on the exact kernels
    u, f = _rel(outs["unfused"], outs["parity"]), _rel(outs["fused"], outs["parity"])
    print("ppmbn parity [PSPNet-R50, 1x3x64x128] log-probabilities: max |d| / max |fp32 parity|: head unfused bf16 %.4e, "
          "head fused bf16 %.4e (ratio %.3f)" % (u, f, f / u if u else float("nan")))
    assert f <= 1.25 * u, (f, u)


def test_other_networks_and_the_switch_unset(cuda, monkeypatch, _pin_vendor_library):
    """BiSeNet-R18 and PSANet hold no such head; unset, or 0, nothing is re-classed and the output is today's, bit for bit."""
    from torchseg_amd.fusion import materialize
    from torchseg_amd.infer import prepare_inference
    from torchseg_amd.ppmbn import _FusedPyramid, pyramid_fused_calls
    from torchseg_amd.workloads.pspnet import PSANet
    assert prepare_inference(_r18(3).eval().to(cuda), dtype=BF, fuse_pyramid=True).fused_pyramid == 0
    torch.manual_seed(4)
    assert prepare_inference(PSANet(19, None, None, nn.BatchNorm2d, depth=50).eval().to(cuda), dtype=BF,
                             fuse_pyramid=True).fused_pyramid == 0
    monkeypatch.delenv("TSG_DTYPE", raising=False)
    monkeypatch.delenv("TSG_PPMBN_FUSED", raising=False)
    net = _psp50(41).to(cuda)
    x = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(42)).to(cuda)
    outs = []
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("TSG_PPMBN_FUSED", env)
        unset = prepare_inference(copy.deepcopy(net), dtype=BF, **ALL_ON)
        off = prepare_inference(copy.deepcopy(net), dtype=BF, fuse_pyramid=False, **ALL_ON)
        for m in (unset, off):
            assert m.fused_pyramid == 0 and not any(isinstance(k, _FusedPyramid) for k in m.modules())
        a, b = materialize(unset(x)).clone(), materialize(off(x)).clone()
        torch.cuda.synchronize()
        assert torch.equal(a, b), env
        outs.append(a)
    assert torch.equal(outs[0], outs[1])
    monkeypatch.setenv("TSG_PPMBN_FUSED", "1")
    on = prepare_inference(copy.deepcopy(net), dtype=BF, **ALL_ON)
    assert on.fused_pyramid == 1
    materialize(on(x))
    assert pyramid_fused_calls(on.module) == 1
