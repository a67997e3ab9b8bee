"""Kernel-level oracles for the evaluator's device path: tsg_resize_bilinear_hp against oracle/evaluator_ref.resize_scores
and torch's float64 F.interpolate, tsg_augment_crop in the form Evaluator.scale_scores calls it (inv_scale given, no
labels, pad_pixel 0.0 / -1.0, all windows of a scale in one call) against the oracle's own statements, and the whole
sliding path with a network that adds no noise (nn.Identity).  tests/test_evaluator_gpu.py judges the same code end to
end through convolutions whose fp32 noise sets its tolerances; every bound here is derived beside it.

Each comparison prints its measured figure before it asserts (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import augment_ref as A
from oracle import evaluator_ref as R

pytestmark = pytest.mark.gpu
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])      # as tests/test_evaluator_gpu.py
EPS = 2.0 ** -23


def _kp():
    from torchseg_amd import kernels as K
    return K.provider()


def _evaluator(class_num, scales, flip):
    from torchseg_amd.workloads import ensure_furnace_on_path
    ensure_furnace_on_path()
    from engine.evaluator import Evaluator
    return Evaluator(None, class_num, MEAN, STD, None, scales, flip, [0])


# ---------------------------------------------------------------------------------------------------------------------
# A. resize_bilinear_hp
RESIZE_CASES = [  # (NC, IH, IW, OH, OW)
    (3, 5, 7, 13, 9),             # non-integer up-sampling, clamped taps on all four borders
    (2, 1, 1, 4, 6),              # one-pixel source: every tap is the pixel, weight 0
    (2, 1, 9, 1, 4),              # one source row, down-sampling in x only
    (5, 2, 3, 7, 2),              # up in y, down in x
    (2, 6, 10, 96, 7),            # large ratio one way, shrink the other
    (7, 52, 68, 70, 90),          # the evaluator's 0.75 scale of 70 x 90 brought back (52 = cvRound(52.5))
    (7, 105, 135, 70, 90),        # the 1.5 scale brought back: down-sampling without antialiasing
    (19, 64, 64, 16, 16),         # factor 4 down: every weight is exactly 0.5
    (4, 33, 47, 33, 47),          # identity
    (3, 100, 150, 800, 1000),     # 2.4 M outputs > 8192 blocks x 256: the grid-stride loop takes a second trip
]
IDENTITY, ONE_PIXEL, FACTOR4 = (4, 33, 47, 33, 47), (2, 1, 1, 4, 6), (19, 64, 64, 16, 16)
DTYPES = [torch.float32, torch.bfloat16]

# |got - want| <= RESIZE_BOUND * max|x| against either oracle, elementwise.  The kernel's weights are the oracle's own
# (double, narrowed to float); it then rounds about eight times in fp32 on values no larger than max|x| (two
# complements, four products, three sums), and oracle 1's cast to float32 adds half an ulp.  An fp32 restatement of the
# kernel's expression in numpy stays within 1.6 * 2^-23 * max|x| of oracle 1 on all ten cases.  The same bound holds for
# bf16 sources: a bf16 value is exact in fp32.
# Measured on an MI355X, largest err / (2^-23 * max|x|) against either oracle, per case in the order of RESIZE_CASES:
#   float32   0.77  0  0.19  0.34  0.56  1.09  0.62  0.29  0  1.05
#   bfloat16  0.57  0  0     0.39  0.63  0.75  0.04  0     0  1.02
# and 1.09 / 0.93 for the sum over the three sources of the accumulation test (its bound is 12).  The library is built
# without contraction, and the figures equal those of the fp32 restatement on the host.
RESIZE_BOUND = 4 * EPS
ORACLES_AGREE = 2 * EPS           # oracle 1's float-narrowed weights and its cast to float32 against float64 throughout


@functools.lru_cache(maxsize=None)
def _resize_case(case, dtype):
    """(x rounded to dtype on the CPU, oracle 1, oracle 2 as float64 [NC, OH, OW], max|x|): computed once per case"""
    NC, IH, IW, OH, OW = case
    g = torch.Generator().manual_seed(1000 * IH + 10 * OW + NC)
    x = (3 * torch.randn(NC, IH, IW, generator=g)).to(dtype)
    xf = x.float()
    o1 = R.resize_scores(np.ascontiguousarray(xf.permute(1, 2, 0).numpy()), OH, OW)
    o1 = torch.from_numpy(np.ascontiguousarray(o1.transpose(2, 0, 1))).double()
    o2 = F.interpolate(xf.double()[None], size=(OH, OW), mode="bilinear", align_corners=False)[0]
    return x, o1, o2, float(xf.abs().max())


@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "bfloat16"])
def test_resize_hp_matches_both_oracles(cuda, dtype, case):
    NC, IH, IW, OH, OW = case
    x, o1, o2, amax = _resize_case(case, dtype)
    agree = float((o1 - o2).abs().max())
    assert agree <= ORACLES_AGREE * amax, ("the two oracles disagree", agree / (EPS * amax))
    got = _kp().resize_bilinear_hp(x.to(cuda), OH, OW)
    assert got.dtype == torch.float32 and tuple(got.shape) == (NC, OH, OW)
    got = got.cpu().double()
    e1, e2 = float((got - o1).abs().max()), float((got - o2).abs().max())
    print("resize_hp %s %s: err / (2^-23 max|x|) = %.3f (resize_scores) %.3f (interpolate float64); oracles apart %.3f"
          % (case, str(dtype).replace("torch.", ""), e1 / (EPS * amax), e2 / (EPS * amax), agree / (EPS * amax)))
    assert e1 <= RESIZE_BOUND * amax, (e1 / (EPS * amax), "against resize_scores")
    assert e2 <= RESIZE_BOUND * amax, (e2 / (EPS * amax), "against F.interpolate in float64")


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "bfloat16"])
def test_resize_hp_exact_cases(cuda, dtype):
    kp = _kp()
    # identity: every weight is 0 and the tap is the pixel itself
    x = _resize_case(IDENTITY, dtype)[0]
    assert torch.equal(kp.resize_bilinear_hp(x.to(cuda), 33, 47).cpu(), x.float())
    # one-pixel source: that pixel everywhere
    x = _resize_case(ONE_PIXEL, dtype)[0]
    assert torch.equal(kp.resize_bilinear_hp(x.to(cuda), 4, 6).cpu(), x.float().expand(2, 4, 6))
    # factor 4 down: src = 4 dst + 1.5, taps 4 dst + 1 and 4 dst + 2 with weight 0.5, every complement exactly 0.5.
    # Scaling by 0.5 is exact, so only the three sums round and a fused multiply-add cannot change them.
    x = _resize_case(FACTOR4, dtype)[0]
    xf = x.float()
    a, b, c, d = xf[:, 1::4, 1::4], xf[:, 1::4, 2::4], xf[:, 2::4, 1::4], xf[:, 2::4, 2::4]
    want = 0.5 * (0.5 * a + 0.5 * b) + 0.5 * (0.5 * c + 0.5 * d)
    assert want.dtype == torch.float32 and tuple(want.shape) == (19, 16, 16)
    assert torch.equal(kp.resize_bilinear_hp(x.to(cuda), 16, 16).cpu(), want)


ACC_SOURCES = [(7, 52, 68, 70, 90), (7, 70, 90, 70, 90), (7, 105, 135, 70, 90)]    # the three scales of sliding_scores


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "bfloat16"])
def test_resize_hp_accumulates_like_sliding_scores(cuda, dtype):
    """The first scale is a plain call, the others add into `total` (out=, accumulate=True).  The kernel forms y[i] + v
    with the v of the plain call, and the sum of a stored value and a computed sum cannot be contracted: bit-equal to a
    torch add of the plain result on the device."""
    kp = _kp()
    xs = [_resize_case(c, dtype) for c in ACC_SOURCES]
    amax = max(c[3] for c in xs)
    total = kp.resize_bilinear_hp(xs[0][0].to(cuda), 70, 90)
    for x, _, _, _ in xs[1:]:
        xd = x.to(cuda)
        plain = kp.resize_bilinear_hp(xd, 70, 90)
        want = total + plain
        assert kp.resize_bilinear_hp(xd, 70, 90, out=total, accumulate=True) is total
        assert torch.equal(total, want), float((total - want).abs().max())
    ref = sum(c[1] for c in xs)
    err = float((total.cpu().double() - ref).abs().max())
    print("resize_hp accumulate %s: err / (2^-23 max|x|) = %.3f of the sum over three sources"
          % (str(dtype).replace("torch.", ""), err / (EPS * amax)))
    assert err <= 3 * RESIZE_BOUND * amax, err / (EPS * amax)
    # accumulate=True without out= has nothing to add to: the plain result
    xd = xs[0][0].to(cuda)
    assert torch.equal(kp.resize_bilinear_hp(xd, 70, 90, accumulate=True), kp.resize_bilinear_hp(xd, 70, 90))


# ---------------------------------------------------------------------------------------------------------------------
# D. the wrapper refuses an `out` the kernel would write past or mis-lay
def test_resize_hp_refuses_a_bad_out(cuda, monkeypatch):
    from torchseg_amd import _lib as L
    kp = _kp()
    launches = []
    real = kp.lib.tsg_resize_bilinear_hp

    def spy(*a):
        launches.append(a)
        return real(*a)

    spy.__name__ = real.__name__
    monkeypatch.setattr(kp.lib, "tsg_resize_bilinear_hp", spy)
    x = torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(0)).to(cuda)
    bad = {
        "dtype": torch.full((2, 3, 13, 9), 7.0, dtype=torch.bfloat16, device=cuda),
        "last dimension": torch.full((2, 3, 13, 8), 7.0, device=cuda),
        "leading dimensions": torch.full((6, 13, 9), 7.0, device=cuda),
        "transposed view": torch.full((2, 3, 9, 13), 7.0, device=cuda).transpose(2, 3),
        "cpu": torch.full((2, 3, 13, 9), 7.0),
    }
    assert tuple(bad["transposed view"].shape) == (2, 3, 13, 9) and not bad["transposed view"].is_contiguous()
    for what, out in bad.items():
        for accumulate in (False, True):
            with pytest.raises(L.TsgError):
                kp.resize_bilinear_hp(x, 13, 9, out=out, accumulate=accumulate)
        assert bool((out == 7.0).all()), what
    with pytest.raises(L.TsgError):                                   # a non-contiguous source, through _require_contiguous
        kp.resize_bilinear_hp(x.transpose(2, 3), 13, 9)
    assert not launches, "a refused call reached the library"
    good = torch.full((2, 3, 13, 9), 7.0, device=cuda)
    assert kp.resize_bilinear_hp(x, 13, 9, out=good) is good and len(launches) == 1
    assert torch.equal(good, kp.resize_bilinear_hp(x, 13, 9))


# ---------------------------------------------------------------------------------------------------------------------
# B. augment_crop as Evaluator.scale_scores calls it
STRIDE_RATE = 2 / 3
EVAL_CASES = [  # (H, W), crop, s
    ((33, 47), 32, 1.25),         # SH / H = 41 / 33 != s; windows slide both ways
    ((33, 47), 32, 1.75),
    ((70, 90), 48, 0.75),         # 70 * 0.75 = 52.5 -> 52 rows, half to even
    ((70, 90), 48, 1.5),
    ((40, 100), 64, 1.0),         # rows padded on the RAW image (crop_y 0, the kernel centres), columns slide
    ((40, 100), 64, 0.5),         # long side below the crop: one window, normalised THEN padded with 0 (pad_pixel -1)
    ((37, 53), 16, 2.0),          # stride 11: 7 x 10 = 70 windows in one call = five launches of at most 16
]
DYADIC = (0.5, 1.0, 2.0)          # every weight a dyadic fraction: all arithmetic on uint8 data is exact in double
ONE_LEVEL = (1.0 / 255.0) / STD   # one grey level in normalised units, per channel
# CLOSE and TIE_SHARE are the bounds of tests/test_augment_gpu.py; an exception must also sit on a near-tie of the oracle.
# Measured on an MI355X: no exception in any case (the kernel interpolates in double, operation for operation as the
# oracle does), 2 % to 7 % of the values of the inexact scales are near-ties, the largest other difference is 4.3e-7.
TIE, CLOSE, TIE_SHARE = 1e-6, 1e-5, 1e-4


def _image(hw, seed):
    return np.random.RandomState(seed).randint(0, 256, size=tuple(hw) + (3,)).astype(np.uint8)


def _pad_value(c):
    """what the library's host code stores for a raw pixel 0: (0 / 255 - mean) * (1 / std) formed in fp32"""
    mean, std = MEAN.astype(np.float32), STD.astype(np.float32)
    return (np.float32(0.0) / np.float32(255.0) - mean[c]) * (np.float32(1.0) / std[c])


def _windows_of(scaled, before, crop, wins, raw_pad):
    """The oracle's statements on one scaled image (evaluator_ref.scale_process): -> per window (input [3,crop,crop],
    the interpolated values before the uint8 rounding laid out the same way, mask of the padded pixels)."""
    out = []
    inside = np.ones(scaled.shape[:2] + (1,), dtype=np.float64)
    if raw_pad:
        raw, _ = R.pad_image_to_shape(scaled, crop, 0)
        bef, _ = R.pad_image_to_shape(before, crop, 0.0)
        ins, _ = R.pad_image_to_shape(inside, crop, 0.0)
        for sy, sx in wins:
            want, _ = R.process_image(raw[sy:sy + crop, sx:sx + crop], MEAN, STD, crop)
            b, _ = R.pad_image_to_shape(bef[sy:sy + crop, sx:sx + crop], crop, 0.0)
            i, _ = R.pad_image_to_shape(ins[sy:sy + crop, sx:sx + crop], crop, 0.0)
            out.append((want, b.transpose(2, 0, 1), np.broadcast_to(i.transpose(2, 0, 1) == 0, want.shape)))
    else:
        want, _ = R.process_image(scaled, MEAN, STD, crop)
        b, _ = R.pad_image_to_shape(before, crop, 0.0)
        i, _ = R.pad_image_to_shape(inside, crop, 0.0)
        out.append((want, b.transpose(2, 0, 1), np.broadcast_to(i.transpose(2, 0, 1) == 0, want.shape)))
    return out


def _eval_call(cuda, img, crop, s, with_inv_scale=True):
    """All windows of one scale in ONE augment_crop call, geom rows formed as Evaluator.scale_scores forms them ->
    (got [n,3,crop,crop] numpy, oracle windows, raw_pad)"""
    ev = _evaluator(3, [s], False)
    H, W = img.shape[0], img.shape[1]
    sh, sw, pad_rows, pad_cols, margin, wins, raw_pad = ev._windows(img, s, crop, STRIDE_RATE)
    scaled = R.resize_image_by_factor(img, s)
    assert scaled.shape[:2] == (sh, sw) and raw_pad == (max(sh, sw) > crop)
    before = A.resize_linear_u8(img, sh, sw, rounded=False, inv_scale=(s, s))
    want = _windows_of(scaled, before, crop, wins, raw_pad)
    geom = np.array([[H, W, sh, sw, 0, max(sy - margin[0], 0) if sh >= crop else 0,
                      max(sx - margin[2], 0) if sw >= crop else 0] for sy, sx in wins], dtype=np.int32)
    img_d = torch.from_numpy(img).to(cuda)
    x, lab = _kp().augment_crop([img_d] * len(wins), None, geom, (crop, crop), ev.image_mean, ev.image_std,
                                pad_pixel=0.0 if raw_pad else -1.0,
                                inv_scale=np.full((len(wins), 2), float(s)) if with_inv_scale else None)
    assert lab is None and tuple(x.shape) == (len(wins), 3, crop, crop) and x.dtype == torch.float32
    return x.cpu().numpy(), want, raw_pad


def _judge(got, want, raw_pad, exact, what):
    """got [n,3,h,w] against the oracle windows: every value within 1e-5, except values exactly one grey level off where
    the oracle's value before rounding lies within 1e-6 of a half-integer, at most 1e-4 of all values (none when every
    weight is dyadic); padded pixels bit for bit.  -> (exceptions, near-ties, values)"""
    assert len(want) == got.shape[0]
    w = np.stack([t[0] for t in want])
    before = np.stack([t[1] for t in want])
    padded = np.stack([t[2] for t in want])
    diff = np.abs(got.astype(np.float64) - w)
    loose = diff > CLOSE
    near_tie = np.abs(before - np.floor(before) - 0.5) <= TIE
    level = ONE_LEVEL[None, :, None, None]
    one_off = np.abs(diff - level) <= CLOSE
    print("augment_crop %s: %d windows, %d values, %d near-ties, %d one-level exceptions, max |d| elsewhere %.2e"
          % (what, got.shape[0], got.size, int(near_tie.sum()), int(loose.sum()),
             float(diff[~loose].max()) if (~loose).any() else 0.0))
    bad = loose & ~(one_off & near_tie & ~padded)
    assert not bad.any(), (what, "first wrong value (window, channel, row, column)", tuple(np.argwhere(bad)[0]),
                           int(bad.sum()), float(diff[bad].max()))
    assert loose.mean() <= TIE_SHARE, (what, int(loose.sum()), got.size)
    if exact:
        assert not loose.any(), (what, int(loose.sum()))
    for c in range(3):
        p = got[:, c][padded[:, c]]
        if raw_pad:                                              # the RAW image is padded with 0, then normalised
            assert (p == _pad_value(c)).all(), (what, c, float(_pad_value(c)), np.unique(p)[:4])
        else:                                                    # normalised, then padded with 0
            assert (p == 0).all(), (what, c, np.unique(p)[:4])
    return int(loose.sum()), int(near_tie.sum()), int(padded.sum())


@pytest.mark.parametrize("case", EVAL_CASES, ids=lambda c: "%dx%d-crop%d-s%s" % (c[0] + c[1:]))
def test_augment_crop_as_the_evaluator_calls_it(cuda, case):
    hw, crop, s = case
    img = _image(hw, 100 * hw[0] + hw[1])
    got, want, raw_pad = _eval_call(cuda, img, crop, s)
    _, ties, padded = _judge(got, want, raw_pad, s in DYADIC, str(case))
    if s not in DYADIC:
        assert ties > 0                                          # the exception mask is not empty: 2 % to 7 % of the values
    if case == ((40, 100), 64, 1.0):
        assert raw_pad and padded == 2 * 3 * 24 * 64             # two windows (stride 43), 12 rows above and below
    if case == ((40, 100), 64, 0.5):
        assert not raw_pad and padded == 3 * (64 * 64 - 20 * 50)
    if case == ((37, 53), 16, 2.0):
        assert got.shape[0] == 70 > 4 * _kp().lib.tsg_augment_max_samples()


def test_augment_crop_without_inv_scale_differs(cuda):
    """the same call without inv_scale (the kernel then derives 41 / 33 and 59 / 47 instead of 1.25) must NOT pass: the
    comparison above can see the argument"""
    hw, crop, s = EVAL_CASES[0]
    got, want, _ = _eval_call(cuda, _image(hw, 100 * hw[0] + hw[1]), crop, s, with_inv_scale=False)
    diff = np.abs(got - np.stack([t[0] for t in want]))
    assert (diff > CLOSE).mean() > TIE_SHARE, (diff > CLOSE).mean()


def test_augment_crop_inv_scale_rows_follow_the_launches(cuda):
    """17 samples = a launch of 16 and a launch of 1: sixteen windows of one image at (1.25, 1.25), then ANOTHER image at
    (fy, fx) = (0.5, 2.0).  The second launch must see row 16 of inv_scale, not row 0."""
    crop = 32
    a, b = _image((33, 47), 1), _image((40, 30), 2)
    sa = R.resize_image_by_factor(a, 1.25)
    assert sa.shape[:2] == (41, 59)
    wins = [(y, x) for y in (0, 3, 6, 9) for x in (0, 9, 18, 27)]
    want = _windows_of(sa, A.resize_linear_u8(a, 41, 59, rounded=False, inv_scale=(1.25, 1.25)), crop, wins, True)
    # cv2.resize(b, None, fx=2.0, fy=0.5): 20 x 60, the rows padded to the crop on the raw image, one window at column 10
    sb = A.resize_linear_u8(b, 20, 60, inv_scale=(0.5, 2.0))
    want += _windows_of(sb, A.resize_linear_u8(b, 20, 60, rounded=False, inv_scale=(0.5, 2.0)), crop, [(0, 10)], True)
    geom = np.array([[33, 47, 41, 59, 0, y, x] for y, x in wins] + [[40, 30, 20, 60, 0, 0, 10]], dtype=np.int32)
    inv = np.array([[1.25, 1.25]] * 16 + [[0.5, 2.0]])
    ad, bd = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)
    assert len(geom) == 17 == _kp().lib.tsg_augment_max_samples() + 1
    x, _ = _kp().augment_crop([ad] * 16 + [bd], None, geom, (crop, crop), MEAN.astype(np.float32), STD.astype(np.float32),
                              pad_pixel=0.0, inv_scale=inv)
    got = x.cpu().numpy()
    _judge(got[:16], want[:16], True, False, "sixteen windows at (1.25, 1.25)")
    _judge(got[16:], want[16:], True, True, "sample 16 at (0.5, 2.0)")


# ---------------------------------------------------------------------------------------------------------------------
# C. the whole device path with a network that adds no noise
# rtol, elementwise, atol 0.  The scores are sums of exp(x) or exp(2x) of the normalised windows, all positive, and a
# relative error survives sums and convex combinations of positive numbers.  The network input differs from the oracle's
# by about 2 ulp of |x| <= 2.7: 5e-7 in exp, 1e-6 with flip; two exp evaluations 1.2e-7 each; up to nine window adds
# 6e-8 each; three scale adds and the resize of part A 5e-7: 2.5e-6 in all, and 1e-5 is a factor of four over it.
# Scales 0.5, 1.0 and 2.0 resize uint8 data exactly, so no tie exceptions.
# Measured on an MI355X: 4.7e-7 without flip, 9.9e-7 with; scale_process 6.1e-7 and 1.1e-6.
IDENTITY_RTOL = 1e-5


def _rel(got, want):
    assert got.shape == want.shape and (want > 0).all()
    return float((np.abs(got.astype(np.float64) - want) / want).max())


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
def test_sliding_scores_of_an_identity_network(cuda, flip, monkeypatch):
    monkeypatch.delenv("TSG_INFER", raising=False)
    scales, crop, hw = [0.5, 1.0, 2.0], 32, (40, 56)
    img = _image(hw, 4056)
    _, want = R.sliding_eval(nn.Identity(), img, 3, scales, crop, STRIDE_RATE, MEAN, STD, flip, return_scores=True)
    ev = _evaluator(3, scales, flip)
    ev.val_func = nn.Identity()
    assert len(ev._windows(img, 2.0, crop, STRIDE_RATE)[5]) == 20
    got = {}
    for wb in (4, 20):
        ev.window_batch = wb
        got[wb] = ev.sliding_scores(img, crop, STRIDE_RATE, 0)
    assert torch.equal(got[4], got[20])                                # eval mode: the batching changes nothing
    rel = _rel(got[4].permute(1, 2, 0).cpu().numpy(), want)
    print("identity network, flip %s: scores %.3g .. %.3g, largest relative error %.3e" % (flip, want.min(), want.max(), rel))
    assert rel <= IDENTITY_RTOL, rel
    ori = (47, 61)
    sp = ev.scale_process(img, ori, crop, STRIDE_RATE, 0)
    want_sp = R.scale_process(nn.Identity(), img, ori, crop, STRIDE_RATE, MEAN, STD, flip)
    rel = _rel(sp, want_sp.astype(np.float64))
    print("identity network, flip %s: scale_process to %s, largest relative error %.3e" % (flip, ori, rel))
    assert rel <= IDENTITY_RTOL, rel
