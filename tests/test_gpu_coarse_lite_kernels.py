"""adn_l0_forward_stats (csrc/edge.hip): the thin first layer of CoarseDepthLite in front of a train-mode BatchNorm, against a
float64 convolution of the same f32 operands.

The kernel rounds its two GEMM operands (network input, weight) to bf16 in registers, as every bf16 layer of the engine does,
and accumulates in f32; the bias is added in f32.  The operands here are f32 tensors whose values are bf16-representable, so
the float64 reference multiplies exactly the numbers the kernel multiplies and the bars below measure the kernel's own
arithmetic: 32 exact products summed in f32 (error <= 32 * 2^-24 * sum|terms| < 1e-6 at these magnitudes) and ONE rounding
of z to bf16 (relative 2^-9, half a unit in the last place).
  * z: |err| <= 2^-8 |ref| + 1e-6;
  * the summed partial rows against the float64 sums of the UNROUNDED z and z^2 (the ADN_EPI_Z_STATS convention: the sums are
    taken before the bf16 rounding, epilogue.h): 1e-5 relative per channel.  The bias is +-[0.5, 1.5] and the input is
    zero-centred, so no channel sum is a cancellation;
  * every partial row is written (the buffer starts as NaN) and two launches give identical bits;
  * (3, 5, 64): the same layer through adn_igemm (S2 on the zero-padded NHWC input, EPI_Z_STATS with the bias) -- z equal or
    adjacent bf16 numbers (two correct roundings of f32 sums that differ in their order; adjacent bf16 numbers are at most
    2^-7 apart, relative), batch mean and variance within 1e-4 relative.
Shapes (B, Hs, Ws): (2, 3, 16) -- every output row touches a border; (1, 8, 48) -- Ws / 16 is not a multiple of 4, the other
work-unit split of edge.hip; (3, 5, 64) -- more than one work unit per wave and more than one workgroup.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(2, 3, 16), (1, 8, 48), (3, 5, 64)]
_CACHE = {}


def _case(B, Hs, Ws):
    """Operands, the float64 reference and two launches of the kernel; computed once per shape."""
    key = (B, Hs, Ws)
    if key in _CACHE:
        return _CACHE[key]
    from audio_depth_estimation_amd import kernels as K
    g = torch.Generator().manual_seed(100 * B + Hs + Ws)
    x = (2 * torch.rand(B, 2, 2 * Hs, 2 * Ws, generator=g) - 1).bfloat16().float()
    w = (0.25 * torch.randn(64, 2, 4, 4, generator=g)).bfloat16().float()
    bias = (0.5 + torch.rand(64, generator=g)) * torch.where(torch.rand(64, generator=g) < 0.5, -1.0, 1.0)
    ref = F.conv2d(x.double(), w.double(), bias.double(), stride=2, padding=1).permute(0, 2, 3, 1).contiguous()   # NHWC
    wm = w.permute(0, 2, 3, 1).contiguous().to(DEV)                       # [64][kh][kw][ci]: the parameter's flat storage
    xd, bd = x.to(DEV), bias.to(DEV)
    P = K.l0_forward_stats_num_partials(B, Hs, Ws)
    runs = []
    for _ in range(2):
        z = torch.full((B, Hs, Ws, 64), float('nan'), dtype=torch.bfloat16, device=DEV)
        part = torch.full((P, 2, 64), float('nan'), device=DEV)
        K.l0_forward_stats(xd, wm, bd, B, Hs, Ws, z, part)
        torch.cuda.synchronize()
        runs.append((z.cpu(), part.cpu()))
    _CACHE[key] = dict(x=x, w=w, bias=bias, ref=ref, wm=wm, xd=xd, bd=bd, P=P, runs=runs)
    return _CACHE[key]


@pytest.mark.parametrize('B,Hs,Ws', SHAPES)
def test_z_within_one_bf16_rounding_of_float64(B, Hs, Ws):
    c = _case(B, Hs, Ws)
    z, ref = c['runs'][0][0].double(), c['ref']
    err = (z - ref).abs()
    slack = err - (2.0 ** -8 * ref.abs() + 1e-6)
    print(f'({B},{Hs},{Ws}): max |err| {float(err.max()):.3e}, max err/|ref| {float((err / ref.abs()).max()):.3e}, '
          f'worst slack {float(slack.max()):.3e}')
    assert torch.isfinite(z).all()
    assert bool((slack <= 0).all())


@pytest.mark.parametrize('B,Hs,Ws', SHAPES)
def test_partial_rows_sum_to_the_float64_channel_sums(B, Hs, Ws):
    c = _case(B, Hs, Ws)
    part, ref = c['runs'][0][1], c['ref'].reshape(-1, 64)
    assert tuple(part.shape) == (c['P'], 2, 64) and torch.isfinite(part).all()       # every row was written
    got = part.double().sum(0)
    want = torch.stack([ref.sum(0), (ref * ref).sum(0)])
    rel = ((got - want).abs() / want.abs()).max(dim=1).values
    print(f'({B},{Hs},{Ws}): P {c["P"]} rel sum z {float(rel[0]):.3e} sum z^2 {float(rel[1]):.3e}')
    assert float(rel.max()) <= 1e-5


@pytest.mark.parametrize('B,Hs,Ws', SHAPES)
def test_two_launches_give_identical_bits(B, Hs, Ws):
    (z0, p0), (z1, p1) = _case(B, Hs, Ws)['runs']
    assert torch.equal(z0.view(torch.int16), z1.view(torch.int16))
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))


def test_without_bias():
    from audio_depth_estimation_amd import kernels as K
    B, Hs, Ws = SHAPES[0]
    c = _case(B, Hs, Ws)
    z = torch.empty(B, Hs, Ws, 64, dtype=torch.bfloat16, device=DEV)
    part = torch.empty(c['P'], 2, 64, device=DEV)
    K.l0_forward_stats(c['xd'], c['wm'], None, B, Hs, Ws, z, part)
    ref = c['ref'] - c['bias'].double()
    err = (z.cpu().double() - ref).abs()
    assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-6).all())


def test_thin_route_equals_the_igemm_route_of_the_first_layer():
    from audio_depth_estimation_amd import kernels as K
    from audio_depth_estimation_amd._lib import EPI_Z_STATS, GEMM_S2
    B, Hs, Ws = 3, 5, 64
    c = _case(B, Hs, Ws)
    T = torch.bfloat16
    x8 = torch.empty(B, 2 * Hs, 2 * Ws, 8, dtype=T, device=DEV)
    K.nchw_to_nhwc(c['xd'], x8)                                           # channels 2..7 zero
    w_s2 = torch.zeros(64, 16, 8, dtype=T, device=DEV)
    K.pack_weights(c['wm'].view(-1), 64, 2, T, w_s2, None, y_pad=8)
    P, wsb = K.igemm_query(T, GEMM_S2, B, Hs, Ws, 8, 0, 64, [64], epi=EPI_Z_STATS)
    ws = torch.empty(wsb // 4 + 4, device=DEV)
    z = torch.empty(B, Hs, Ws, 64, dtype=T, device=DEV)
    part = torch.full((P, 2, 64), float('nan'), device=DEV)
    K.igemm(T, GEMM_S2, B, Hs, Ws, x8, None, w_s2, 64, EPI_Z_STATS, [K.Seg(64, out0=z, partials=part, bias=c['bd'])], ws)
    torch.cuda.synchronize()
    zt, pt = c['runs'][0]
    a, b = zt.double(), z.cpu().double()
    diff = (a - b).abs()
    print(f'thin vs igemm: {int((diff > 0).sum())} of {diff.numel()} z differ, max rel {float((diff / b.abs()).max()):.3e}')
    assert bool((diff <= 2.0 ** -7 * b.abs() + 1e-6).all())
    n = B * Hs * Ws
    stats = []
    for p in (pt, part.cpu()):
        s = p.double().sum(0)
        mean = s[0] / n
        stats.append((mean, s[1] / n - mean * mean))
    for (ma, va), (mb, vb) in [(stats[0], stats[1])]:
        print(f'mean rel {float(((ma - mb).abs() / mb.abs()).max()):.3e} var rel {float(((va - vb).abs() / vb).max()):.3e}')
        assert float(((ma - mb).abs() / mb.abs()).max()) <= 1e-4
        assert float(((va - vb).abs() / vb).max()) <= 1e-4
