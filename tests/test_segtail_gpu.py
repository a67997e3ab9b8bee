"""GPU: the fused segmentation head tail (tsg_seg_tail_logprob / tsg_seg_tail_accum) against float64 oracles.

The oracle interpolates in float64 with the tap indices and weights of oracle/upsample_ref.py (the scale and the
fractional weights formed in float32, as aten and tsg_upsample_bilinear_ac_fwd form them), then takes log_softmax in
float64; it runs on the device in float64 only because the 150-class 768x1536 maps are too large for a quick host pass.
"""
import pytest
import torch

from oracle.upsample_ref import interp_matrix

pytestmark = pytest.mark.gpu


def _oracle_logprob(z, H, W):
    """float64 log_softmax(interpolate(z, (H, W), align_corners=True), 1)"""
    dev = z.device
    Wy = torch.from_numpy(interp_matrix(z.shape[-2], H)).to(dev)
    Wx = torch.from_numpy(interp_matrix(z.shape[-1], W)).to(dev)
    v = torch.einsum("oi,ncij,pj->ncop", Wy, z.double(), Wx)
    return torch.log_softmax(v, dim=1)


def _check(out, ref):
    err = (out.double() - ref).abs()
    bound = 4e-6 + 1e-6 * ref.abs()
    bad = (err > bound)
    assert not bad.any(), "max err %.3e at %s (ref %.4f)" % (err.max().item(), bad.nonzero()[0].tolist(),
                                                           ref[tuple(bad.nonzero()[0].tolist())].item())


CASES = [(1, 19, 16, 32, 128, 256), (4, 19, 16, 32, 128, 256), (1, 21, 12, 20, 96, 160), (4, 21, 12, 20, 96, 160),
         (1, 150, 8, 8, 64, 64), (4, 150, 8, 8, 64, 64), (1, 19, 97, 193, 768, 1536), (1, 150, 97, 193, 768, 1536),
         (2, 19, 7, 9, 31, 45), (1, 3, 5, 6, 1, 1)]


@pytest.mark.parametrize("N,C,h,w,H,W", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_logprob_matches_float64(cuda, N, C, h, w, H, W, dtype):
    from torchseg_amd import kernels as K
    g = torch.Generator().manual_seed(N * 1000 + C + h)
    z = (3.0 * torch.randn(N, C, h, w, generator=g)).to(dtype).to(cuda)
    out = K.provider().seg_tail_logprob(z, H, W)
    again = K.provider().seg_tail_logprob(z, H, W)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == (N, C, H, W)
    _check(out, _oracle_logprob(z, H, W))
    assert torch.equal(out, again)


def test_logprob_is_the_stock_chain_in_fp32(cuda):
    """fp32 z: the same values as F.log_softmax(F.interpolate(z)) up to fp32 rounding of the softmax."""
    import torch.nn.functional as F
    from torchseg_amd import kernels as K
    z = torch.randn(2, 19, 32, 64, device=cuda)
    out = K.provider().seg_tail_logprob(z, 256, 512)
    ref = F.log_softmax(F.interpolate(z, size=(256, 512), mode="bilinear", align_corners=True), dim=1)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=2e-5)


def _oracle_accum(z, zf, geom, dst, H, W, accumulate):
    """float64 restatement of the reference's window loop: data[...] += exp(lp + flip(lp_flip)), window by window."""
    lp = _oracle_logprob(z, H, W)
    if zf is not None:
        lp = lp + _oracle_logprob(zf, H, W).flip(-1)
    e = torch.exp(lp)
    out = dst.double().clone()
    written = torch.zeros(dst.shape[1:], dtype=torch.bool, device=dst.device)
    for n, (oy, ox, t, l, rows, cols) in enumerate(geom):
        win = e[n, :, t:t + rows, l:l + cols]
        if accumulate:
            out[:, oy:oy + rows, ox:ox + cols] += win
        else:
            w = written[oy:oy + rows, ox:ox + cols]
            out[:, oy:oy + rows, ox:ox + cols] = torch.where(w, out[:, oy:oy + rows, ox:ox + cols] + win, win)
            written[oy:oy + rows, ox:ox + cols] = True
    return out


# overlapping windows (stride rate 2/3 on a 2-D grid), crop margins, a padded one-window case, odd widths
GEOMS = {
    "grid2x2": ((96, 160), (64, 128), [(0, 0, 0, 0, 64, 128), (0, 32, 0, 0, 64, 128), (32, 0, 0, 0, 64, 128),
                                       (32, 32, 0, 0, 64, 128)]),
    "margins": ((50, 70), (64, 64), [(0, 0, 7, 3, 50, 61), (0, 6, 7, 0, 50, 64)]),
    "one_window_padded": ((41, 57), (64, 64), [(0, 0, 11, 3, 41, 57)]),
    "odd": ((37, 53), (30, 30), [(0, 0, 0, 0, 30, 30), (7, 23, 0, 0, 30, 30), (7, 0, 0, 0, 30, 30),
                                 (0, 20, 0, 0, 30, 30), (3, 11, 0, 0, 30, 30)]),
}


@pytest.mark.parametrize("name", sorted(GEOMS))
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_accum_matches_reference_loop(cuda, name, flip, accumulate, dtype):
    from torchseg_amd import kernels as K
    kp = K.provider()
    (Hd, Wd), (H, W), geom = GEOMS[name]
    N, C = len(geom), 19
    g = torch.Generator().manual_seed(len(name) * 7 + flip)
    z = (2.0 * torch.randn(N, C, (H + 7) // 8, (W + 7) // 8, generator=g)).to(dtype).to(cuda)
    zf = (2.0 * torch.randn(z.shape, generator=g)).to(dtype).to(cuda) if flip else None
    dst0 = torch.rand(C, Hd, Wd, generator=g).to(cuda)
    out = kp.seg_tail_accum(z, zf, geom, dst0.clone(), H, W, accumulate=accumulate)
    again = kp.seg_tail_accum(z, zf, geom, dst0.clone(), H, W, accumulate=accumulate)
    ref = _oracle_accum(z, zf, geom, dst0, H, W, accumulate)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.double(), ref, rtol=2e-5, atol=1e-6)
    assert torch.equal(out, again)
    # the same windows one launch each, in order: bit-equal (one read of dst per pixel adds in window order)
    # accumulate = 0 over a batch == a dst zeroed where the batch covers it, then the windows added one by one
    seq = dst0.clone()
    if not accumulate:
        for (oy, ox, t, l, rows, cols) in geom:
            seq[:, oy:oy + rows, ox:ox + cols] = 0.0
    for n in range(N):
        kp.seg_tail_accum(z[n:n + 1].contiguous(), None if zf is None else zf[n:n + 1].contiguous(), [geom[n]], seq,
                          H, W, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(out, seq)


def test_accum_under_graph_replay(cuda):
    from torchseg_amd import kernels as K
    kp = K.provider()
    (Hd, Wd), (H, W), geom = GEOMS["grid2x2"]
    N, C = len(geom), 19
    z = torch.randn(N, C, H // 8, W // 8, device=cuda).to(torch.bfloat16)
    zf = torch.randn_like(z)
    g_dev = torch.tensor(geom, dtype=torch.int32, device=cuda)
    region = (0, Hd, 0, Wd)
    dst = torch.zeros(C, Hd, Wd, device=cuda)
    kp.seg_tail_accum(z, zf, g_dev, dst, H, W, accumulate=False, region=region)      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kp.seg_tail_accum(z, zf, g_dev, dst, H, W, accumulate=False, region=region)
    eager = kp.seg_tail_accum(z, zf, geom, torch.zeros_like(dst), H, W, accumulate=False)
    dst.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dst, eager)
    z.copy_(torch.randn_like(z))
    graph.replay()
    eager = kp.seg_tail_accum(z, zf, geom, torch.zeros_like(dst), H, W, accumulate=False)
    torch.cuda.synchronize()
    assert torch.equal(dst, eager)


def test_accum_large_window_no_flip_vs_flip(cuda):
    """A 1024x1024 Cityscapes window (19 x 128^2 logits) into a 1024x2048 map, three windows at stride 683."""
    from torchseg_amd import kernels as K
    kp = K.provider()
    geom = [(0, 0, 0, 0, 1024, 1024), (0, 683, 0, 0, 1024, 1024), (0, 1024, 0, 0, 1024, 1024)]
    z = torch.randn(3, 19, 128, 128, device=cuda).to(torch.bfloat16)
    zf = torch.randn_like(z)
    for flip in (None, zf):
        out = kp.seg_tail_accum(z, flip, geom, torch.zeros(19, 1024, 2048, device=cuda), 1024, 1024,
                                accumulate=False)
        ref = _oracle_accum(z, flip, geom, torch.zeros(19, 1024, 2048, device=cuda), 1024, 1024, True)
        torch.cuda.synchronize()
        torch.testing.assert_close(out.double(), ref, rtol=2e-5, atol=1e-6)
        del out, ref
