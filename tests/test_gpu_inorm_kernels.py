"""adn_inorm_fwd / adn_inorm_bwd (csrc/inorm.hip) against a float64 restatement, on both forms and both access widths.

Tolerances
  * f32: max|xhat err| <= 2e-5 and max|dz err| <= 2e-4 * max|dz| (the bars of the BatchNorm kernel tests).
  * bf16: the reference is computed in float64 from the SAME bf16-rounded inputs; every output element is within one bf16
    ulp of it (ulp(x) = 2^(floor(log2|x|) - 7)) plus the f32 bar above (an f32 result that close to a rounding boundary may
    round the other way).
  * mean / istd (f32, extras of this file): a 256-thread tree over <= 64 sequential terms per thread carries at most
    (64 + 8) * 2^-24 ~ 4e-6 of the mean absolute deviation -> mean within 2e-5 * max|z - z[0]|, istd within 1e-4 relative.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS = 1e-5
SLOPE = 0.2

# (B, HW, C): 2x2 bottleneck; one 16-byte item; 6x10 with 3 items per row; 3x5 / 4x4 on the plain form (C % 8 != 0);
# a streaming shape with a ragged last slab (50x52 = 2600 rows); the largest level of unet_256 at 256^2
CASES = [(3, 4, 512), (1, 4, 8), (2, 60, 24), (2, 15, 4), (2, 16, 12), (2, 2600, 64), (1, 128 * 128, 64)]
DTYPES = [torch.float32, torch.bfloat16]


def K():
    from audio_depth_estimation_amd import kernels
    return kernels


def lib():
    from audio_depth_estimation_amd import _lib
    return _lib.load()


def switch_hw(C, dtype):
    """First HW the host rule sends to the streaming form (read from adn_inorm_form, not assumed)."""
    lo, hi = 2, 1 << 20
    assert K().inorm_form(lo, C, dtype).startswith('resident') and K().inorm_form(hi, C, dtype).startswith('streaming')
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if K().inorm_form(mid, C, dtype).startswith('resident'):
            lo = mid
        else:
            hi = mid
    return hi


def make_inputs(B, HW, C, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * HW + C)
    off = 3.0 * torch.randn(1, 1, C, generator=g)
    sc = 0.25 + 2.0 * torch.rand(B, 1, C, generator=g)
    z = (torch.randn(B, HW, C, generator=g) * sc + off).to(dtype)
    gr = torch.randn(B, HW, C, generator=g)
    gr = (gr * (torch.rand(B, HW, C, generator=g) > 0.4)).to(dtype)          # already masked by an activation
    return z, gr


def ref_fwd(z):
    z64 = z.double()
    mean = z64.mean(1, keepdim=True)
    var = ((z64 - mean) ** 2).mean(1, keepdim=True)
    istd = (var + EPS).rsqrt()
    return (z64 - mean) * istd, mean[:, 0], istd[:, 0]


def ref_bwd(g, z, gscale):
    xhat, _, istd = ref_fwd(z)
    gp = g.double() * gscale
    return istd[:, None] * (gp - gp.mean(1, keepdim=True) - xhat * (gp * xhat).mean(1, keepdim=True))


def ulp_bf16(ref):
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)


def check(out, ref, dtype, f32_abs, what):
    err = (out.double().cpu() - ref).abs()
    bound = torch.full_like(ref, f32_abs)
    if dtype == torch.bfloat16:
        bound = bound + ulp_bf16(ref)
    bad = err > bound
    assert not bool(bad.any()), f'{what}: max err {float(err.max()):.3e}, {int(bad.sum())} elements over the bound'


def workspace(B, HW, C):
    return torch.empty(max(K().inorm_workspace_bytes(B, HW, C), 16) // 4, dtype=torch.float32, device=DEV)


def run_fwd(z, leaky=True, relu=True, keep=None, scale=1.0):
    B, HW, C = z.shape
    mean = torch.empty(B, C, dtype=torch.float32, device=DEV)
    istd = torch.empty(B, C, dtype=torch.float32, device=DEV)
    ol = torch.full_like(z, float('nan')) if leaky else None
    orl = torch.full_like(z, float('nan')) if relu else None
    K().inorm_fwd(z, B, HW, C, EPS, SLOPE, mean, istd, ol, orl, workspace(B, HW, C), keep=keep, keep_scale=scale)
    return mean, istd, ol, orl


def run_case(B, HW, C, dtype):
    z, g = make_inputs(B, HW, C, dtype)
    xhat, mean64, istd64 = ref_fwd(z)
    ref_l = torch.where(xhat > 0, xhat, xhat * SLOPE)
    ref_r = xhat.clamp_min(0)
    zd = z.to(DEV)
    mean, istd, ol, orl = run_fwd(zd)
    dev = (z.double() - z.double()[:, :1]).abs().max()
    assert float((mean.double().cpu() - mean64).abs().max()) <= 2e-5 * float(dev) + 1e-30
    assert float(((istd.double().cpu() - istd64) / istd64).abs().max()) <= 1e-4
    check(ol, ref_l, dtype, 2e-5, 'leaky')
    check(orl, ref_r, dtype, 2e-5, 'relu')
    # either output alone gives the same bits as both; a second run gives the same bits
    m2, i2, ol2, _ = run_fwd(zd, relu=False)
    m3, i3, _, orl3 = run_fwd(zd, leaky=False)
    for a, b in ((ol2, ol), (orl3, orl), (m2, mean), (m3, mean), (i2, istd), (i3, istd)):
        assert torch.equal(a, b)
    # dropout: keep * 2 * output, bit for bit
    keep = (torch.rand(B, HW, C, generator=torch.Generator().manual_seed(5)) > 0.5).to(torch.uint8).to(DEV)
    _, _, old, ord_ = run_fwd(zd, keep=keep, scale=2.0)
    assert torch.equal(old, (ol.float() * 2.0 * keep).to(dtype))
    assert torch.equal(ord_, (orl.float() * 2.0 * keep).to(dtype))
    # backward from the float64 statistics
    mean_d, istd_d = mean64.float().to(DEV), istd64.float().to(DEV)
    for gscale in (1.0, 2.0):
        ref = ref_bwd(g, z, gscale)
        outs = []
        for _ in range(2):
            gd = g.to(DEV).clone()
            K().inorm_bwd(gd, zd, mean_d, istd_d, B, HW, C, gscale, workspace(B, HW, C))
            outs.append(gd)
        assert torch.equal(outs[0], outs[1])
        check(outs[0], ref, dtype, 2e-4 * float(ref.abs().max()), f'dz gscale={gscale}')


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_inorm_matches_float64(case, dtype):
    run_case(*case, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('C', [16, 12])
def test_both_sides_of_the_form_switch(C, dtype):
    hw = switch_hw(C, dtype)
    assert K().inorm_form(hw - 1, C, dtype).startswith('resident') and K().inorm_form(hw, C, dtype).startswith('streaming')
    assert K().inorm_form(hw, C, dtype).endswith('plain') == (C % 8 != 0)
    run_case(2, hw - 1, C, dtype)
    run_case(2, hw, C, dtype)
    run_case(2, 2 * hw + 1, C, dtype)            # a last slab of ONE row


def test_forms_of_the_unet256_levels():
    """Every level of unet_256 at 256^2 from 2x2 to 32x32 is resident; the two widest are streaming."""
    for dtype in DTYPES:
        for side, C in ((2, 512), (4, 512), (8, 512), (16, 512), (32, 256)):
            assert K().inorm_form(side * side, C, dtype) == 'resident'
        for side, C in ((64, 128), (128, 64)):
            assert K().inorm_form(side * side, C, dtype) == 'streaming'


@pytest.mark.parametrize('HW', [4, 60, 1500])
def test_constant_channel_gives_zero(HW):
    for dtype in DTYPES:
        z = torch.randn(2, HW, 8).to(dtype)
        z[:, :, 3] = 7.25
        z[1, :, 5] = -300.0
        mean, istd, ol, orl = run_fwd(z.to(DEV))
        assert torch.isfinite(ol).all() and torch.isfinite(orl).all()
        assert float(ol[:, :, 3].abs().max()) == 0.0 and float(orl[1, :, 5].abs().max()) == 0.0
        assert float((istd[:, 3].cpu() - EPS ** -0.5).abs().max()) <= 1e-4 * EPS ** -0.5
        assert float(mean[1, 5]) == -300.0


@pytest.mark.parametrize('HW', [16, 900, 4000])
def test_large_mean_small_spread_f32(HW):
    """mean 300, std 0.5: the input's own f32 rounding gives 6e-5 on xhat; a sum-of-squares variance is off by percent."""
    g = torch.Generator().manual_seed(HW)
    z = (300.0 + 0.5 * torch.randn(2, HW, 8, generator=g)).float()
    xhat, _, _ = ref_fwd(z)
    _, _, ol, _ = run_fwd(z.to(DEV), relu=False)
    got = ol.double().cpu()
    got = torch.where(got > 0, got, got / SLOPE)
    assert float((got - xhat).abs().max()) <= 5e-4


def _raw_fwd(z, B, HW, C, ws, ws_bytes, mean, istd, out):
    code = 1 if z.dtype == torch.bfloat16 else 0
    return lib().adn_inorm_fwd(z.data_ptr(), B, HW, C, code, EPS, SLOPE, mean.data_ptr(), istd.data_ptr(), out.data_ptr(),
                               None, None, 1.0, ws.data_ptr(), ws_bytes, None)


def _raw_bwd(g, z, B, HW, C, ws, ws_bytes, mean, istd):
    code = 1 if z.dtype == torch.bfloat16 else 0
    return lib().adn_inorm_bwd(g.data_ptr(), z.data_ptr(), mean.data_ptr(), istd.data_ptr(), B, HW, C, code, 1.0,
                               ws.data_ptr(), ws_bytes, None)


def test_refusals():
    B, HW, C = 2, 16, 8
    z = torch.randn(B, HW, C + 1, device=DEV).flatten()
    out, g = torch.empty_like(z), torch.zeros_like(z)
    mean, istd = torch.zeros(B * C, device=DEV), torch.ones(B * C, device=DEV)
    need = K().inorm_workspace_bytes(B, HW, C)
    ws = torch.empty(need // 4 + 4, dtype=torch.float32, device=DEV)
    assert lib().adn_inorm_workspace_bytes(B, 1, C) < 0
    assert _raw_fwd(z, B, 1, C, ws, need, mean, istd, out) == -1                 # HW = 1
    assert b'spatial' in lib().adn_last_error()
    assert _raw_bwd(g, z, B, 1, C, ws, need, mean, istd) == -1
    assert _raw_fwd(z, B, HW, C, ws, need - 4, mean, istd, out) == -1            # short workspace
    assert b'workspace' in lib().adn_last_error()
    assert _raw_bwd(g, z, B, HW, C, ws, need - 4, mean, istd) == -1
    assert _raw_fwd(z[1:], B, HW, C, ws, need, mean, istd, out) == -1            # 4-byte aligned, 16 needed
    assert b'misaligned' in lib().adn_last_error()
    assert _raw_bwd(g[1:], z, B, HW, C, ws, need, mean, istd) == -1
    assert lib().adn_inorm_fwd(None, B, HW, C, 0, EPS, SLOPE, mean.data_ptr(), istd.data_ptr(), out.data_ptr(), None, None,
                               1.0, ws.data_ptr(), need, None) == -1
    assert _raw_fwd(z, B, HW, C, ws, need, mean, istd, out) == 0                 # the same call with nothing wrong
    assert _raw_bwd(g, z, B, HW, C, ws, need, mean, istd) == 0
    torch.cuda.synchronize()
    assert ctypes.c_int(lib().adn_inorm_form(1, C, 0)).value < 0
