"""adn_wgrad_multi: batchable k4 weight gradients of either class in one launch, the small-image fast form and the dead
taps of 1x1 images.  bf16, through the C ABI.

The cross-check is adn_wgrad_batch, which keeps running class-1 problems through the GENERAL form of the tap-staged kernel:
the small-image form must stage the same LDS tiles, so dW and the norm partials are compared with torch.equal.  The
independent reference is the float64 autograd dW of tests/test_gpu_k4_rect.py from the bf16-rounded operands, under the
bound that module applies to the tap-staged route (TOL_F32_OUT of max|ref|).  Every dW and every partials buffer starts
as NaN.

Channels are R = 128, C = 128 and the two-source forms C0 = C1 = 128 and R0 = R1 = 128.  One exception, asserted below: an
8x8 image at B = 32 is batchable only from 256 tiles on (fewer tiles make the planner split the pixels more than twice), so
the 8x8 problems of the mixed launch carry the 512 channels they have in unet_256.
"""
import ctypes as C
import functools

import pytest
import torch

from test_gpu_k4_rect import _dw_reference, _wgrad_operands
from test_gpu_kernels import DEV, TOL_F32_OUT, K, rel_err

DTYPE = torch.bfloat16
NAN = float('nan')
# (B, Hs, Ws): half a step, a partial last step, several steps, non-square images, every border tap
SHAPES = [(32, 1, 1), (3, 1, 1), (32, 2, 2), (5, 2, 2), (40, 2, 2), (32, 4, 4), (3, 4, 4), (32, 2, 4), (7, 4, 2), (9, 4, 2)]
ONE, TWO_PLAIN, TWO_GATH = (128, 0, 128, 0), (128, 128, 128, 0), (128, 0, 128, 128)      # R0, R1, C0, C1
WIDE_ONE, WIDE_TWO_PLAIN = (512, 0, 512, 0), (512, 512, 512, 0)


@functools.lru_cache(maxsize=None)
def problem(B, Hs, Ws, chans):
    """(device operands, the same on the CPU, norm partials per launch) of one problem; shared between the tests, never
    modified."""
    R0, R1, C0, C1 = chans
    plain, gath, ops = _wgrad_operands('multi/%dx%dx%d/%d+%d_%d+%d' % ((B, Hs, Ws) + chans), DTYPE, B, Hs, Ws, R0, R1, C0, C1)
    cls, nsq = K().wgrad_batchable(DTYPE, B, Hs, Ws, R0, R1, C0, C1)
    assert cls == (2 if Hs * Ws >= 64 else 1) and nsq == (R0 + R1) // 128 * (16 * (C0 + C1) // 128), (B, Hs, Ws, chans)
    return ops, (plain, gath), nsq


@functools.lru_cache(maxsize=None)
def reference(B, Hs, Ws, chans):
    """float64 dW [R][16][C] from the rounded operands (the 128-channel problems only: seconds on the CPU beyond that)."""
    plain, gath = problem(B, Hs, Ws, chans)[1]
    return _dw_reference('convT' if chans[1] else 'conv', plain, gath)


def launch(entry, B, Hs, Ws, chans, ops=None):
    """One-problem launch into NaN-prefilled buffers: (dW [R][16][C], partials)."""
    dev, _, nsq = problem(B, Hs, Ws, chans)
    p0, p1, g0, g1 = ops or dev
    R, Cc = chans[0] + chans[1], chans[2] + chans[3]
    dw = torch.full((R * 16 * Cc,), NAN, device=DEV)
    sq = torch.full((nsq,), NAN, dtype=torch.float64, device=DEV)
    entry(DTYPE, B, [(Hs, Ws, p0, p1, g0, g1, dw, sq)])
    return dw.view(R, 16, Cc), sq


@pytest.mark.gpu
@pytest.mark.parametrize('B,Hs,Ws', SHAPES)
def test_small_image_form(B, Hs, Ws):
    """One-problem launches through adn_wgrad_multi (small-image form) against the general form of adn_wgrad_batch -- the
    same bits --, against the lone adn_wgrad where that runs unsplit, and against float64."""
    k = K()
    for chans in (ONE, TWO_PLAIN, TWO_GATH):
        (p0, p1, g0, g1), _, nsq = problem(B, Hs, Ws, chans)
        ref = reference(B, Hs, Ws, chans)
        dw, sq = launch(k.wgrad_multi, B, Hs, Ws, chans)
        dw_gen, sq_gen = launch(k.wgrad_batch, B, Hs, Ws, chans)
        assert not bool(torch.isnan(dw).any()) and not bool(torch.isnan(sq).any()), chans
        assert torch.equal(dw, dw_gen) and torch.equal(sq, sq_gen), chans
        if k.wgrad_workspace_bytes(DTYPE, B, Hs, Ws, *chans) == 0:
            assert nsq == k.wgrad_sq_count(DTYPE, B, Hs, Ws, *chans)
            dw_one = torch.full((ref.numel(),), NAN, device=DEV)
            sq_one = torch.full((nsq,), NAN, dtype=torch.float64, device=DEV)
            k.wgrad(DTYPE, B, Hs, Ws, p0, p1, g0, g1, dw_one, torch.empty(4, device=DEV), sq=sq_one)
            assert torch.equal(dw.view(-1), dw_one) and torch.equal(sq, sq_one), chans
        err = rel_err(dw, ref)
        print('%dx%dx%d %s: %.3e' % (B, Hs, Ws, chans, err))
        assert err <= TOL_F32_OUT[DTYPE], (chans, err)
        want = float((dw.double() ** 2).sum())
        assert abs(float(sq.sum()) - want) <= 1e-7 * want, chans


# the small-image levels of a U-Net at B = 32 in the order backward() meets them: the up layers from 8x8 inwards (two plain
# sources: the skip concat), then the down layers from 1x1 outwards
MIXED = [(8, WIDE_TWO_PLAIN), (4, TWO_PLAIN), (2, TWO_PLAIN), (1, TWO_PLAIN), (1, ONE), (2, TWO_GATH), (4, ONE), (8, WIDE_ONE)]


@pytest.mark.gpu
def test_mixed_launch():
    """Eight problems of both classes in one launch, in the engine's order and shuffled: every problem's dW and partials
    equal its one-problem launch."""
    k = K()
    B = 32
    assert k.wgrad_batchable(DTYPE, B, 8, 8, *ONE) == (0, 0)           # (why the 8x8 problems are the wide ones)
    lone = [launch(k.wgrad_multi, B, hs, hs, chans) for hs, chans in MIXED]
    for order in (list(range(8)), [5, 0, 7, 3, 1, 6, 2, 4]):
        probs = []
        for i in order:
            hs, chans = MIXED[i]
            (p0, p1, g0, g1), _, nsq = problem(B, hs, hs, chans)
            probs.append((hs, hs, p0, p1, g0, g1, torch.full((lone[i][0].numel(),), NAN, device=DEV),
                          torch.full((nsq,), NAN, dtype=torch.float64, device=DEV)))
        k.wgrad_multi(DTYPE, B, probs)
        for i, prob in zip(order, probs):
            assert torch.equal(prob[6], lone[i][0].view(-1)) and torch.equal(prob[7], lone[i][1]), (order, MIXED[i])
    for (hs, chans), (dw, _) in zip(MIXED, lone):
        if hs < 8:
            assert rel_err(dw, reference(B, hs, hs, chans)) <= TOL_F32_OUT[DTYPE], (hs, chans)
            continue
        # the class-2 problems: the lone adn_wgrad splits their pixels -- another summation order (as test_gpu_kernels.py)
        p0, p1, g0, g1 = problem(B, hs, hs, chans)[0]
        ws = torch.empty(k.wgrad_workspace_bytes(DTYPE, B, hs, hs, *chans) // 4, device=DEV)
        dw_one = torch.full((dw.numel(),), NAN, device=DEV)
        k.wgrad(DTYPE, B, hs, hs, p0, p1, g0, g1, dw_one, ws)
        assert rel_err(dw.view(-1), dw_one) <= 1e-5, (hs, chans)


@pytest.mark.gpu
@pytest.mark.parametrize('B', [32, 3])
def test_dead_taps(B):
    """1x1 images: every dW element of a tap outside {1,2}^2 is +0.0f, the partials of those column tiles are 0.0, the live
    taps equal the general form.  The dead tiles are not multiplied at all: an infinite operand, which the general form
    turns into NaN there (0 * inf), leaves them zero."""
    k = K()
    live = torch.tensor([ky in (1, 2) and kx in (1, 2) for ky in range(4) for kx in range(4)])
    for chans in (ONE, TWO_PLAIN, TWO_GATH):
        dw, sq = launch(k.wgrad_multi, B, 1, 1, chans)
        dw_gen, sq_gen = launch(k.wgrad_batch, B, 1, 1, chans)
        bits = dw.cpu().view(torch.int32)
        assert bool((bits[:, ~live, :] == 0).all()), chans
        assert torch.equal(dw[:, live, :], dw_gen[:, live, :]), chans
        # partials are [row tile][column tile]; with C a multiple of 128 a column tile lies inside one tap
        per_tap = sq.cpu().view(dw.shape[0] // 128, 16, -1)
        assert bool((per_tap[:, ~live, :] == 0.0).all()) and bool((per_tap[:, live, :] > 0.0).all()), chans
        assert torch.equal(sq, sq_gen), chans
        p0, p1, g0, g1 = problem(B, 1, 1, chans)[0]
        p_inf = p0.clone()
        p_inf[0, 0, 0, 5] = float('inf')
        dw_inf, _ = launch(k.wgrad_multi, B, 1, 1, chans, ops=(p_inf, p1, g0, g1))
        assert bool((dw_inf.cpu().view(torch.int32)[:, ~live, :] == 0).all()), chans
        assert bool(torch.isinf(dw_inf[5, live, :]).all()), chans


def _host_desc(B, Hs, Ws, R0, R1, C0, C1):
    from audio_depth_estimation_amd import _lib
    d = _lib.AdnWgradDesc()
    d.dtype, d.B, d.Hs, d.Ws, d.R0, d.R1, d.C0, d.C1 = _lib.ADN_BF16, B, Hs, Ws, R0, R1, C0, C1
    d.plain0 = d.gath0 = d.dw = 1              # (dummy non-null operands: a refused call returns before any launch)
    d.plain1 = 1 if R1 else None
    d.gath1 = 1 if C1 else None
    return d


def test_refusals():
    """Argument checks of adn_wgrad_multi, on the host: too many problems, a problem that is not batchable, a null operand."""
    from audio_depth_estimation_amd import _lib
    lib = _lib.load()
    good = _host_desc(32, 2, 2, 128, 0, 128, 0)
    assert lib.adn_wgrad_batchable(C.byref(good)) == 1

    def refused(descs, n=None):
        arr = (_lib.AdnWgradDesc * len(descs))(*descs)
        rc = lib.adn_wgrad_multi(arr, len(descs) if n is None else n, None)
        return rc != 0 and lib.adn_last_error().decode()

    ADN_ERR_ARG = lib.adn_wgrad_multi(None, 1, None)
    assert ADN_ERR_ARG != 0
    arr9 = (_lib.AdnWgradDesc * 9)(*[good] * 9)
    assert lib.adn_wgrad_multi(arr9, 9, None) == ADN_ERR_ARG and '1 .. 8 problems' in lib.adn_last_error().decode()
    assert lib.adn_wgrad_multi(arr9, 0, None) == ADN_ERR_ARG
    patch = _host_desc(32, 64, 64, 128, 0, 64, 0)                          # a patch-staged layer
    assert 'problem 1 is not batchable' in refused([good, patch])
    null = _host_desc(32, 2, 2, 128, 0, 128, 0)
    null.gath0 = None
    assert 'problem 0 is not batchable' in refused([null, good])
    for bad in ([good, patch], [null, good]):
        arr = (_lib.AdnWgradDesc * 2)(*bad)
        assert lib.adn_wgrad_multi(arr, 2, None) == ADN_ERR_ARG
