"""The grid-stride kernels of csrc/elementwise.hip and csrc/dcnet.hip PAST their first grid pass and at the channel counts
whose per-thread state moves between passes (C = 96, 192, 24), each against a float64 restatement computed on the CPU from
the same inputs (already rounded to the storage dtype).  Shapes and the regime each one reaches: tests/streaming_pass_cases.py,
checked on the host by tests/test_streaming_pass_cases.py.  Every output is pre-filled with NaN (0xAA for the fp8 buffers).

Left out on purpose: plain maxpool2_fwd, maxpool2_bwd and upsample2x_bwd past the 8192-block cap need at least 67 M elements
per case.  Their loops are the same code as the tail-fused instantiations tested here; the difference is a null TailStats, and
for maxpool2_fwd a stateless 64-bit index.

Tolerances (u = 2^-24, half a float32 ulp; ulp_bf16(x) = 2^(floor(log2|x|) - 7); EVERY element must be inside its bound)
  elementwise f32 output   (R + 1) * u * (sum of |terms| of that element, from the float64 reference), R = the f32 roundings
                           of the kernel's expression:
      bn_act               z*sc + sh, * slope: R = 3; terms |z sc|, |sh|.  A sign decision that differs from float64 needs
                           |v| below the error of v, and then both branches are inside the bound.
      bn_bwd_apply         sc * (g - c0 - ((z - m) * is) * c1): R = 6; terms |sc g|, |sc c0|, |sc xhat c1|
      upsample2x_fwd       (1-ly)((1-lx)a + lx b) + ly((1-lx)c + lx d): R = 11; terms = the same expression over |taps|.
                           The kernel computes the source coordinate in f32 as torch's f32 path does, f = fl(fl((in-1)/(out-1)) * o):
                           two roundings on a value <= in - 1, so lx (ly) is off by at most 2u(Wi-1) (2u(Hi-1)) from the float64
                           coordinate -- 3e-5 at Hi = 257.  The bound adds 2u(Wi-1)|d out/d lx| + 2u(Hi-1)|d out/d ly|, both
                           derivatives from the float64 taps.  (Bilinear interpolation is continuous across a cell border, so a
                           floor that lands in the neighbouring cell changes nothing beyond this.)
      upsample2x_bwd_tail  old + sum over <= 4 x 4 candidates of (wy wx) g: R = 3 * 16 + 2 = 50; terms |old| + adjoint(|g|).
                           The weight error above gives each candidate's weight an error <= 2u(Hi-1) + 2u(Wi-1); the candidates of
                           source pixel i lie in outputs 2i-2 .. 2i+3, so the bound adds that times the 6 x 6 window sum of |g|
                           (a worst case over all 36: about 1e-3 at 181 x 183 for |g| ~ 1).
      head zpre / act 3    per lane n = V * ceil(C / (lpp V)) products and adds, log2(lpp) shuffle adds, the bias: R = 2n + log2(lpp)
                           + 1; terms |x w|, |b|
      head gx (acts 0, 3)  gout * d is exact (d is 0 or 1), times w: R = 1 (the reference reads the same f32 zpre the kernel reads)
      l1tv grad            c0 s + cx s - cx s + cy s - cy s with three f32 constants: R = 12; terms c0 + 2 cx + 2 cy
  elementwise bf16 output  the f32 bound + ulp_bf16(reference)
  exact                    max-pool routing (+ old on a grid of multiples of 1/8 below 8: the f32 sum and its bf16 rounding are
                           exact), the ReLU mask, every copy kernel, clamp_range
  per-channel sums         (T + 3) * u * (sum of |terms| of the channel), T = f32 additions that feed one partial-row entry =
                           terms per thread x threads per channel group, read from the kernel:
      maxpool2_bwd_tail    4 pixels x ceil(work / (grid * 256)) passes, x 256 / (C / 8) threads
      upsample2x_bwd_tail  ceil(work / (grid * 256)) passes x 256 / (C / 8) threads
      relu_bwd_stats       ceil(rows / rpi) x rpi (rpi = 256 // channel groups of the column pass); scalar path: rows
      head dw / db         ceil(pixels / (grid * gpb)) passes x gpb pixel groups of a block
                           The cross-row sum is float64 (in the test; in colsum_kernel for the head).  bf16 tail sums add the f32
                           value BEFORE storage rounding, so the reference sums use the unrounded float64 gradient.
  head acts 1, 2           (__expf / tanhf) the bars of test_head1x1: 1e-5 of max|ref| (out), 2e-5 (dw, db), TOL_T_OUT (gx).
                           Measured error of a plain f32 torch evaluation of the same expressions on the CPU against float64
                           (the reference, not the kernel), worst over the cases here: zpre / out 3.0e-7, dw / db 2.2e-6
                           (1 - tanh^2 cancels in the saturated range), gx 3.1e-3 in bf16 (the storage rounding), all of
                           max|ref| -- 4x each of them is still inside the bars, so no bar is widened.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import streaming_pass_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
F64 = torch.float64
DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
TOL_T_OUT = {torch.float32: 2e-5, torch.bfloat16: 6e-3}              # of test_gpu_dcnet_kernels.py
SLOPE = 0.2
MAXD = 30.0


def K():
    from audio_depth_estimation_amd import kernels
    return kernels


def expand(cases):
    return [pytest.param(c, DT[d], id=sc.case_id(c) + '-' + d) for c in cases for d in c.dtypes]


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def ulp_bf16(ref):
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)


def inside(out, ref, f32_bound, dtype, what):
    """Every element of ``out`` within ``f32_bound`` (+ one bf16 ulp of the reference) of the float64 ``ref``."""
    got = out.detach().double().cpu().reshape(ref.shape)
    bound = f32_bound + ulp_bf16(ref) if dtype == torch.bfloat16 else f32_bound
    err = (got - ref).abs()
    bad = ~(err <= bound)                                   # a NaN left in the output is bad
    if bool(bad.any()):
        idx = bad.reshape(-1).nonzero()[:4, 0].tolist()
        worst = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float('inf')).max())
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements over the bound, worst {worst:.3g}x, '
                             f'first flat indices {idx}')


def sums_inside(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    assert bool((err <= bound).all()), f'{what}: worst {float((err / bound.clamp_min(1e-300)).max()):.3g}x the bound'


def rel_err(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def nan_like(shape, dtype):
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


def u8(*shape):
    return torch.full(shape, 0xAA, dtype=torch.uint8, device=DEV)


def per_channel(C, lo, hi, k):
    """f32 [C] on the device, clearly different from channel to channel (a low-discrepancy walk over [lo, hi))."""
    mult = (0.6180339887498949, 0.7548776662466927, 0.5698402909980532, 0.4142135623730951, 0.7320508075688772)[k]
    c = torch.arange(1, C + 1, dtype=F64)
    return (lo + (hi - lo) * ((c * mult) % 1.0)).float().to(DEV)


def check_fp8(out_bf16, q8, qs):
    """The ``check`` of test_fused_fp8_copies_equal_quantizing_the_bf16_output: scales and bytes bit-equal to mx8_quantize."""
    C = out_bf16.shape[-1]
    out_bf16, q8, qs = out_bf16.reshape(-1, C), q8.reshape(-1, C), qs.reshape(-1, C // 32)
    rows = out_bf16.shape[0]
    pad = -rows % (128 // math.gcd(C, 128))                  # adn_mx8_quantize wants rows * C % 128 == 0: zero rows appended,
    src = F.pad(out_bf16, [0, 0, 0, pad])                    # (every 32-channel block is quantized on its own)
    want8, wants = u8(rows + pad, C), u8(rows + pad, C // 32)
    K().mx8_quantize(src, want8, wants)
    want8, wants = want8[:rows], wants[:rows]
    assert torch.equal(qs, wants)
    nz = (want8 & 0x7f) != 0
    assert torch.equal(q8[nz], want8[nz]) and not bool(((q8 & 0x7f)[~nz]).any())


# ================================================================================================ BatchNorm apply kernels
def bn_inputs(pixels, C, dtype):
    g = gen(11 + C)
    z = (torch.randn(pixels, C, device=DEV, generator=g) * 2).to(dtype)
    gr = torch.randn(pixels, C, device=DEV, generator=g).to(dtype)
    scale, shift = per_channel(C, 0.5, 2.5, 0), per_channel(C, -2.0, 2.0, 1)
    mean, istd = per_channel(C, -1.0, 1.0, 2), per_channel(C, 0.5, 2.0, 3)
    coef = torch.cat([per_channel(C, -0.5, 0.5, 4), per_channel(C, -0.5, 0.5, 1)])
    return z, gr, scale, shift, mean, istd, coef


@pytest.mark.parametrize('case,dtype', expand(sc.BN))
def test_bn_act_past_one_pass(case, dtype):
    pixels, C = case.shape
    z, _, scale, shift, _, _, _ = bn_inputs(pixels, C, dtype)
    z64, s64, h64 = z.double().cpu(), scale.double().cpu(), shift.double().cpu()
    v = z64 * s64 + h64
    bound = 4 * U * ((z64 * s64).abs() + h64.abs())
    slope = float(torch.tensor(SLOPE, dtype=torch.float32))
    leaky, relu = torch.where(v > 0, v, v * slope), v.clamp_min(0)
    for want_leaky, want_relu in ((True, False), (False, True), (True, True)):
        ol = nan_like((pixels, C), dtype) if want_leaky else None
        orl = nan_like((pixels, C), dtype) if want_relu else None
        K().bn_act(z, pixels, C, scale, shift, SLOPE, ol, orl)
        if want_leaky:
            inside(ol, leaky, bound, dtype, f'leaky ({want_leaky}, {want_relu})')
        if want_relu:
            inside(orl, relu, bound, dtype, f'relu ({want_leaky}, {want_relu})')


@pytest.mark.parametrize('case,dtype', expand(sc.BN))
def test_bn_bwd_apply_past_one_pass(case, dtype):
    pixels, C = case.shape
    z, gr, scale, _, mean, istd, coef = bn_inputs(pixels, C, dtype)
    z64, g64 = z.double().cpu(), gr.double().cpu()
    s64, m64, i64, c64 = (t.double().cpu() for t in (scale, mean, istd, coef))
    xh = (z64 - m64) * i64
    ref = s64 * (g64 - c64[:C] - xh * c64[C:])
    bound = 7 * U * s64.abs() * (g64.abs() + c64[:C].abs() + (xh * c64[C:]).abs())
    K().bn_bwd_apply(gr, z, pixels, C, scale, mean, istd, coef)
    inside(gr, ref, bound, dtype, 'bn_bwd_apply')


@pytest.mark.parametrize('case,dtype', expand(sc.BN_MX8))
def test_bn_mx8_variants_past_one_pass(case, dtype):
    pixels, C = case.shape
    z, gr, scale, shift, mean, istd, coef = bn_inputs(pixels, C, dtype)
    y0, y1 = nan_like((pixels, C), dtype), nan_like((pixels, C), dtype)
    q8, qs = u8(pixels, C), u8(pixels, C // 32)
    K().bn_act(z, pixels, C, scale, shift, 0.0, None, y0)
    K().bn_act_mx8(z, pixels, C, scale, shift, y1, q8, qs)
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
    check_fp8(y1, q8, qs)
    g0, g1 = gr.clone(), gr.clone()
    q8, qs = u8(pixels, C), u8(pixels, C // 32)
    K().bn_bwd_apply(g0, z, pixels, C, scale, mean, istd, coef)
    K().bn_bwd_apply_mx8(g1, z, pixels, C, scale, mean, istd, coef, q8, qs)
    assert torch.equal(g0.view(torch.int16), g1.view(torch.int16))
    check_fp8(g1, q8, qs)


# ================================================================================================ bilinear x2 upsample forward
def up_axis(n_in):
    """float64 source index, neighbour and weight of each of the 2 n_in outputs (align_corners=True)."""
    f = torch.arange(2 * n_in, dtype=F64) * ((n_in - 1) / (2 * n_in - 1))
    i0 = f.floor().clamp(max=n_in - 1).long()
    return i0, (i0 + 1).clamp(max=n_in - 1), f - i0


@functools.lru_cache(maxsize=1)
def upsample_fwd_reference(B, Hi, Wi, C, dtype):
    """(x on the device, float64 reference [B, 2Hi, 2Wi, C], f32 bound) -- shared by the two targets of a dtype."""
    x = torch.randn(B, Hi, Wi, C, device=DEV, generator=gen(21)).to(dtype)
    x64 = x.double().cpu()
    y0, y1, ly = up_axis(Hi)
    x0, x1, lx = up_axis(Wi)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    top, bot = x64[:, y0], x64[:, y1]
    a, b, c, d = top[:, :, x0], top[:, :, x1], bot[:, :, x0], bot[:, :, x1]
    del top, bot
    ref = (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d)
    mag = (1 - ly) * ((1 - lx) * a.abs() + lx * b.abs()) + ly * ((1 - lx) * c.abs() + lx * d.abs())
    dlx = ((1 - ly) * (b - a) + ly * (d - c)).abs()
    dly = ((1 - lx) * (c - a) + lx * (d - b)).abs()
    bound = 12 * U * mag + 2 * U * (Wi - 1) * dlx + 2 * U * (Hi - 1) * dly
    # the restatement above IS float64 F.interpolate(align_corners=True)
    torch_ref = F.interpolate(x64.permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=True).permute(0, 2, 3, 1)
    assert float((torch_ref - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    return x, ref, bound


def pad_to(t, Ho, Wo):
    """F.pad of Up.forward on an NHWC tensor: diff // 2 before, the rest after."""
    dH, dW = Ho - t.shape[1], Wo - t.shape[2]
    return F.pad(t, [0, 0, dW // 2, dW - dW // 2, dH // 2, dH - dH // 2])


UPSAMPLE_FWD_RUNS = sorted(expand(sc.UPSAMPLE_FWD), key=lambda p: str(p.values[1]))       # the two targets of a dtype together


@pytest.mark.parametrize('case,dtype', UPSAMPLE_FWD_RUNS)
def test_upsample2x_fwd_past_one_pass(case, dtype):
    B, Hi, Wi, C, Ho, Wo = case.shape
    x, ref, bound = upsample_fwd_reference(B, Hi, Wi, C, dtype)
    out = nan_like((B, Ho, Wo, C), dtype)
    K().upsample2x_fwd(x, out)
    inside(out, pad_to(ref, Ho, Wo), pad_to(bound, Ho, Wo), dtype, 'upsample2x_fwd')
    if dtype == torch.bfloat16:                             # the fp8 variant: same bf16 bits, fp8 copy = quantizing them
        out1, q8, qs = nan_like((B, Ho, Wo, C), dtype), u8(B, Ho, Wo, C), u8(B, Ho, Wo, C // 32)
        K().upsample2x_fwd_mx8(x, out1, q8, qs)
        assert torch.equal(out.view(torch.int16), out1.view(torch.int16))
        check_fp8(out1, q8, qs)


# ================================================================================================ tail-fused backward kernels
def tail_inputs(B, H, W, C, dtype, seed):
    g = gen(seed)
    # post-ReLU forward output on a coarse grid: zeros and many exact ties inside a 2 x 2 window
    y = ((torch.randn(B, H, W, C, device=DEV, generator=g) * 2).round().clamp(min=0) * 0.5).to(dtype)
    z = torch.randn(B, H, W, C, device=DEV, generator=g).to(dtype)
    old = ((torch.randn(B, H, W, C, device=DEV, generator=g) * 8).round().clamp(-31, 31) / 8).to(dtype)
    return y, z, old, per_channel(C, -1.0, 1.0, 2), per_channel(C, 0.5, 2.0, 3)


def tail_sums_check(part, rows, C, T, g_sum, gx_sum, g_abs, gx_abs, what):
    part = part.view(rows, 2, C)
    assert bool(torch.isfinite(part).all()), what + ': a partial row is not finite'
    got = part.double().sum(0).cpu()
    sums_inside(got[0], g_sum, (T + 3) * U * g_abs, what + ' sum g')
    sums_inside(got[1], gx_sum, (T + 3) * U * gx_abs, what + ' sum g xhat')


@pytest.mark.parametrize('case,dtype', expand(sc.MAXPOOL_TAIL))
def test_maxpool2_bwd_tail_past_one_pass(case, dtype):
    B, H, W, C = case.shape
    Ho, Wo = H // 2, W // 2
    y, z, old, mean, istd = tail_inputs(B, H, W, C, dtype, 31)
    gd = ((torch.randn(B, Ho, Wo, C, device=DEV, generator=gen(32)) * 8).round().clamp(-31, 31) / 8).to(dtype)
    m64, i64 = mean.double().cpu(), istd.double().cpu()
    work = sc.items(case)
    P = K().tail_stats_blocks(work, C)
    assert P == case.cap
    T = 4 * -(-work // (P * 256)) * (256 // (C // 8))
    outs = {}
    for acc in (True, False):
        gx = old.clone() if acc else nan_like((B, H, W, C), dtype)
        part = nan_like((P * 2 * C,), torch.float32)
        K().maxpool2_bwd_tail(gd, y, gx, acc, z, mean, istd, part)
        outs[acc] = (gx.cpu(), part)
    # float64 reference, one image at a time (the largest case holds 34 M elements)
    tot = {acc: [torch.zeros(C, dtype=F64) for _ in range(4)] for acc in outs}
    for b in range(B):
        y64, gd64 = y[b].double().cpu(), gd[b].double().cpu()
        v = [y64[dy:2 * Ho:2, dx:2 * Wo:2] for dy in (0, 1) for dx in (0, 1)]
        m, arg = v[0], torch.zeros(v[0].shape, dtype=torch.int8)
        for q in (1, 2, 3):                                 # the FIRST maximum in scan order: strict >
            gt = v[q] > m
            m, arg = torch.where(gt, v[q], m), torch.where(gt, torch.tensor(q, dtype=torch.int8), arg)
        routed = torch.zeros(H, W, C, dtype=F64)
        for q, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            routed[dy:2 * Ho:2, dx:2 * Wo:2] = torch.where(arg == q, gd64, torch.zeros((), dtype=F64))
        xh = (z[b].double().cpu() - m64) * i64
        for acc, (gx, _) in outs.items():
            ref = (routed + old[b].double().cpu() if acc else routed) * (y64 > 0)
            assert torch.equal(gx[b].double(), ref), f'accumulate={acc}, image {b}: gradient not exact'
            t = tot[acc]
            for k, term in enumerate((ref, ref * xh, ref.abs(), (ref * xh).abs())):
                t[k] += term.sum((0, 1))
    for acc, (_, part) in outs.items():
        tail_sums_check(part, P, C, T, *tot[acc], f'maxpool2_bwd_tail accumulate={acc}')


@pytest.mark.parametrize('case,dtype', expand(sc.UPSAMPLE_TAIL))
def test_upsample2x_bwd_tail_past_one_pass(case, dtype):
    B, Hi, Wi, C, Ho, Wo = case.shape
    y, z, old, mean, istd = tail_inputs(B, Hi, Wi, C, dtype, 41)
    gu = torch.randn(B, Ho, Wo, C, device=DEV, generator=gen(42)).to(dtype)
    work = sc.items(case)
    P = K().tail_stats_blocks(work, C)
    assert P == case.cap
    T = -(-work // (P * 256)) * (256 // (C // 8))
    # float64 adjoint of interpolate + pad, of g and of |g| (the weights are positive)
    padT, padL = (Ho - 2 * Hi) // 2, (Wo - 2 * Wi) // 2
    g64 = gu.double().cpu()[:, padT:padT + 2 * Hi, padL:padL + 2 * Wi].permute(0, 3, 1, 2)
    src = torch.zeros(B, C, Hi, Wi, dtype=F64, requires_grad=True)
    up = F.interpolate(src, scale_factor=2, mode='bilinear', align_corners=True)
    adj = torch.autograd.grad(up, src, g64, retain_graph=True)[0].permute(0, 2, 3, 1)
    adj_abs = torch.autograd.grad(up, src, g64.abs())[0].permute(0, 2, 3, 1)
    window = 36 * F.avg_pool2d(g64.abs(), 6, stride=2, padding=2).permute(0, 2, 3, 1)     # outputs 2i-2 .. 2i+3, both axes
    assert window.shape == adj.shape
    y64, old64 = y.double().cpu(), old.double().cpu()
    xh = (z.double().cpu() - mean.double().cpu()) * istd.double().cpu()
    for acc in (True, False):
        gx = old.clone() if acc else nan_like((B, Hi, Wi, C), dtype)
        part = nan_like((P * 2 * C,), torch.float32)
        K().upsample2x_bwd_tail(gu, gx, acc, y, z, mean, istd, part)
        mask = y64 > 0
        ref = (adj + old64 if acc else adj) * mask
        bound = (51 * U * (adj_abs + (old64.abs() if acc else 0)) + 2 * U * ((Hi - 1) + (Wi - 1)) * window) * mask
        inside(gx, ref, bound, dtype, f'upsample2x_bwd_tail accumulate={acc}')
        tail_sums_check(part, P, C, T, ref.sum((0, 1, 2)), (ref * xh).sum((0, 1, 2)), ref.abs().sum((0, 1, 2)),
                        (ref * xh).abs().sum((0, 1, 2)), f'upsample2x_bwd_tail accumulate={acc}')


# ================================================================================================ relu_bwd_stats
@pytest.mark.parametrize('case,dtype', expand(sc.RELU_STATS))
def test_relu_bwd_stats_rows_and_columns(case, dtype):
    pixels, C = case.shape
    g = gen(51)
    z = torch.randn(pixels, C, device=DEV, generator=g).to(dtype)
    mean, istd = per_channel(C, -1.0, 1.0, 2), per_channel(C, 0.5, 2.0, 3)
    y = torch.relu((z.float() - mean) * istd).to(dtype)
    gr = torch.randn(pixels, C, device=DEV, generator=g).to(dtype)
    P = K().relu_bwd_stats_num_partials(pixels, C)
    rows = -(-pixels // P)
    assert rows == case.claim['rows']
    part = nan_like((P, 2, C), torch.float32)
    g64, y64 = gr.double().cpu(), y.double().cpu()
    xh = (z.double().cpu() - mean.double().cpu()) * istd.double().cpu()
    K().relu_bwd_stats(gr, y, z, mean, istd, pixels, C, part)
    gm = g64 * (y64 > 0)
    assert torch.equal(gr.double().cpu(), gm)                               # the masked gradient is exact
    assert bool(torch.isfinite(part).all())
    empty = [b for b in range(P) if b * rows >= pixels]
    assert len(empty) == case.claim['empty'] and not bool(part[empty].any())  # blocks without rows write zeros
    if C % 8:
        T = torch.full((C,), float(rows), dtype=F64)
    else:
        grp = torch.arange(C) // 8
        span = torch.where(grp < (C // 8) // 256 * 256, torch.tensor(256), torch.tensor((C // 8) % 256 or 256))
        rpi = 256 // span
        T = (-(-rows // rpi) * rpi).double()
    got = part.double().sum(0).cpu()
    sums_inside(got[0], gm.sum(0), (T + 3) * U * gm.abs().sum(0), 'sum g')
    sums_inside(got[1], (gm * xh).sum(0), (T + 3) * U * (gm * xh).abs().sum(0), 'sum g xhat')


# ================================================================================================ 1x1 head
def head_ref(x64, w64, b64, act):
    zz = x64 @ w64 + b64
    if act == 0:
        return zz, zz.clamp(0, MAXD)
    if act == 1:
        return zz, (torch.sigmoid(zz) * MAXD).clamp(0, MAXD)
    return zz, torch.tanh(zz) * MAXD if act == 2 else zz


def zpre_bound(x64, w64, b64, C):
    V, lpp = sc.head_lanes(C)
    n = V * -(-C // (lpp * V))
    return (2 * n + int(math.log2(lpp)) + 1 + 1) * U * (x64.abs() @ w64.abs() + b64.abs())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('act', [2, 3])
@pytest.mark.parametrize('shape', sc.HEAD_SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_head1x1_tanh_and_identity(dtype, act, shape):
    """Acts 2 (tanh * max_depth) and 3 (identity: Head1x1 uses it whenever the output is resized) against float64 autograd of
    conv1x1 + act, at the shapes and bars of test_head1x1; tanh in its linear AND its saturated range."""
    B, C, H, W = shape
    pixels = B * H * W
    g = gen(61 + C)
    x = torch.randn(pixels, C, device=DEV, generator=g).to(dtype)
    w = (torch.randn(C, device=DEV, generator=g) * (2.0 / math.sqrt(C)))
    x[0] = 0                                                 # z = bias: linear range
    x[1] = (3.0 * torch.sign(w) / w.abs().sum()).to(dtype)   # z ~ 3.1: saturated; x[2]: the other side
    x[2] = -x[1]
    b = torch.tensor([0.1], device=DEV)
    gout = torch.randn(pixels, device=DEV, generator=g)
    x64 = x.double().cpu().requires_grad_(True)
    w64, b64 = w.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    conv = F.conv2d(x64.view(B, H, W, C).permute(0, 3, 1, 2), w64.view(1, C, 1, 1), b64)
    ref = torch.tanh(conv) * MAXD if act == 2 else conv
    zz = conv.detach().reshape(-1)
    assert float(zz[0].abs()) < 0.2 and float(zz[1]) > 2.5 and float(zz[2]) < -2.5
    assert bool((zz.abs() < 0.5).any()) and bool((zz.abs() > 2.5).any())
    ref.backward(gout.double().cpu().view(B, 1, H, W))
    zpre, out = nan_like((pixels,), torch.float32), nan_like((pixels,), torch.float32)
    K().head1x1_fwd(x, w, b, act, MAXD, zpre, out)
    assert rel_err(zpre, zz) <= 1e-5 and rel_err(out, ref) <= 1e-5
    gx, dw, db = nan_like((pixels, C), dtype), nan_like((C,), torch.float32), nan_like((1,), torch.float32)
    ws = torch.empty(K().head1x1_bwd_workspace_bytes(pixels, C) // 4, dtype=torch.float32, device=DEV)
    K().head1x1_bwd(gout, zpre, x, w, act, MAXD, gx, dw, db, ws)
    assert rel_err(gx, x64.grad) <= TOL_T_OUT[dtype]
    assert rel_err(dw, w64.grad) <= 2e-5 and rel_err(db, b64.grad) <= 2e-5


def head_inputs(pixels, C, dtype, wstd, bias, wnorm=None):
    g = gen(71 + C)
    x = torch.randn(pixels, C, device=DEV, generator=g).to(dtype)
    w = torch.randn(C, device=DEV, generator=g) * wstd
    if wnorm:
        w = w * (wnorm / w.norm())
    gout = torch.randn(pixels, device=DEV, generator=g)
    return x, w, torch.tensor([bias], device=DEV), gout


@pytest.mark.parametrize('case,dtype', expand(sc.HEAD_FWD))
def test_head1x1_fwd_past_one_pass(case, dtype):
    pixels, C = case.shape
    x, w, b, _ = head_inputs(pixels, C, dtype, 0.3, 0.1)
    x64, w64, b64 = x.double().cpu(), w.double().cpu(), b.double().cpu()
    bound = zpre_bound(x64, w64, b64, C)
    for act in (3, 1):
        zz, ref = head_ref(x64, w64, b64, act)
        zpre, out = nan_like((pixels,), torch.float32), nan_like((pixels,), torch.float32)
        K().head1x1_fwd(x, w, b, act, MAXD, zpre, out)
        inside(zpre, zz, bound, torch.float32, f'zpre act {act}')
        if act == 3:
            assert torch.equal(out, zpre)
        else:
            assert rel_err(out, ref) <= 1e-5


@pytest.mark.parametrize('case,dtype', expand(sc.HEAD_BWD))
def test_head1x1_bwd_past_one_pass(case, dtype):
    pixels, C = case.shape
    x, w, b, gout = head_inputs(pixels, C, dtype, 1.0, 2.0, wnorm=12.0)              # z ~ N(2, 12^2): both clamps of act 0
    x64, w64, b64, go64 = x.double().cpu(), w.double().cpu(), b.double().cpu(), gout.double().cpu()
    zpre, out = nan_like((pixels,), torch.float32), nan_like((pixels,), torch.float32)
    K().head1x1_fwd(x, w, b, 0, MAXD, zpre, out)
    inside(zpre, x64 @ w64 + b64, zpre_bound(x64, w64, b64, C), torch.float32, 'zpre')
    z64 = zpre.double().cpu()                                # the backward reads THIS f32 tensor: its reference does too
    inrange = (z64 >= 0) & (z64 <= MAXD)
    assert 0.3 < float(inrange.double().mean()) < 0.8 and bool((z64 < 0).any()) and bool((z64 > MAXD).any())
    V, lpp = sc.head_lanes(C)
    gpb = 256 // lpp
    nb = K().head1x1_bwd_workspace_bytes(pixels, C) // ((C + 1) * 4)
    T = -(-pixels // (nb * gpb)) * gpb
    ws = torch.empty(nb * (C + 1), dtype=torch.float32, device=DEV)
    for act in (0, 3):
        dz = go64 * inrange if act == 0 else go64
        gx, dw, db = nan_like((pixels, C), dtype), nan_like((C,), torch.float32), nan_like((1,), torch.float32)
        K().head1x1_bwd(gout, zpre, x, w, act, MAXD, gx, dw, db, ws)
        gref = dz[:, None] * w64[None, :]
        inside(gx, gref, 2 * U * gref.abs(), dtype, f'gx act {act}')
        sums_inside(dw, dz @ x64, (T + 3) * U * (dz.abs() @ x64.abs()), f'dw act {act}')
        sums_inside(db, dz.sum().reshape(1), (T + 3) * U * dz.abs().sum().reshape(1), f'db act {act}')


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_head1x1_bwd_refuses_too_many_channels_and_goes_on(dtype):
    pixels = 64
    for C in sc.HEAD_BWD_REFUSED:
        x, w, b, gout = head_inputs(pixels, C, dtype, 0.1, 0.0)
        zpre = torch.zeros(pixels, device=DEV)
        gx, dw, db = nan_like((pixels, C), dtype), nan_like((C,), torch.float32), nan_like((1,), torch.float32)
        ws = nan_like((K().head1x1_bwd_workspace_bytes(pixels, C) // 4,), torch.float32)
        with pytest.raises(RuntimeError, match='too large'):
            K().head1x1_bwd(gout, zpre, x, w, 3, MAXD, gx, dw, db, ws)
        torch.cuda.synchronize()
        for t in (gx, dw, db, ws):
            assert bool(torch.isnan(t).all())                # nothing was written
    C = 250                                                  # scalar path, under its limit of 256
    x, w, b, gout = head_inputs(pixels, C, dtype, 0.1, 0.0)
    zpre = torch.zeros(pixels, device=DEV)
    gx, dw, db = nan_like((pixels, C), dtype), nan_like((C,), torch.float32), nan_like((1,), torch.float32)
    ws = nan_like((K().head1x1_bwd_workspace_bytes(pixels, C) // 4,), torch.float32)
    K().head1x1_bwd(gout, zpre, x, w, 3, MAXD, gx, dw, db, ws)                  # the next valid call succeeds
    go64, x64 = gout.double().cpu(), x.double().cpu()
    sums_inside(dw, go64 @ x64, (pixels + 3) * U * (go64.abs() @ x64.abs()), 'dw after a refusal')
    gref = go64[:, None] * w.double().cpu()[None, :]
    inside(gx, gref, 2 * U * gref.abs(), dtype, 'gx after a refusal')


# ================================================================================================ exact copies
@pytest.mark.parametrize('case,dtype', expand(sc.NHWC_TO_NCHW))
def test_nhwc_to_nchw_past_one_pass(case, dtype):
    B, C, H, W = case.shape
    src = torch.randn(B, H, W, C, device=DEV, generator=gen(81)).to(dtype)
    dst = nan_like((B, C, H, W), torch.float32)
    K().nhwc_to_nchw(src, dst)
    assert torch.equal(dst, src.float().permute(0, 3, 1, 2))


@pytest.mark.parametrize('case,dtype', expand(sc.NCHW_TO_NHWC))
def test_nchw_to_nhwc_every_pixel(case, dtype):
    B, C, H, W, Cpad = case.shape
    src = torch.randn(B, C, H, W, device=DEV, generator=gen(82))
    dst = nan_like((B, H, W, Cpad), dtype)
    K().nchw_to_nhwc(src, dst)
    assert torch.equal(dst[..., :C], src.permute(0, 2, 3, 1).to(dtype))
    assert not bool(dst[..., C:].any())                      # padded channels are zero (and no NaN is left)


@pytest.mark.parametrize('case,dtype', expand(sc.PIXEL_SHUFFLE))
def test_pixel_shuffle2_past_one_pass(case, dtype):
    B, H, W, C = case.shape
    packed = torch.randn(B, H, W, 4 * C, device=DEV, generator=gen(83)).to(dtype)
    spatial = nan_like((B, 2 * H, 2 * W, C), dtype)
    K().pixel_shuffle2(packed, spatial)
    want = packed.view(B, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, C)
    assert torch.equal(spatial, want)
    back = nan_like(tuple(packed.shape), dtype)
    K().pixel_shuffle2(back, spatial, inverse=True)
    assert torch.equal(back, packed)


def test_clamp_range_past_one_pass():
    n = sc.CLAMP[0].shape[0]
    g = gen(84)
    x = 40 * torch.rand(n, device=DEV, generator=g) - 5
    p = sc.CLAMP_PLANT
    x[p:p + 3] = torch.tensor([0.0, 30.0, 30.000002], device=DEV)
    go = torch.randn(n, device=DEV, generator=g)
    out, gx = nan_like((n,), torch.float32), nan_like((n,), torch.float32)
    K().clamp_range(x, 30.0, out)
    K().clamp_range(x, 30.0, gx, g=go)
    x64 = x.double().cpu()
    assert torch.equal(out.double().cpu(), x64.clamp(0, 30.0))
    assert torch.equal(gx.double().cpu(), go.double().cpu() * ((x64 >= 0) & (x64 <= 30.0)))
    assert gx[p:p + 3].tolist() == [float(go[p]), float(go[p + 1]), 0.0]


# ================================================================================================ L1 + TV loss
def test_l1tv_loss_past_one_pass():
    B, H, W = sc.L1TV[0].shape
    g = gen(91)
    pred = (torch.rand(B, 1, H, W, device=DEV, generator=g) * 8).round().div(2)      # coarse grid: sign(0) ties in every pass
    gt = (torch.rand(B, 1, H, W, device=DEV, generator=g) * 8).round().div(2)
    p64 = pred.double().cpu().requires_grad_(True)
    g64 = gt.double().cpu()
    l1w, sw = 1.0, float(torch.tensor(0.1, dtype=torch.float32))
    sm = (p64[..., :, :-1] - p64[..., :, 1:]).abs().mean() + (p64[..., :-1, :] - p64[..., 1:, :]).abs().mean()
    loss = l1w * (p64 - g64).abs().mean() + sw * sm
    loss.backward()
    n = B * H * W
    for lo_, hi_ in ((0, 262144), (262144, 2 * 262144), (8192 * 256, n)):           # ties in the first, second and last pass
        d = (pred.reshape(-1)[lo_:hi_] - gt.reshape(-1)[lo_:hi_])
        assert bool((d == 0).any())
    stats = torch.zeros(4, dtype=F64, device=DEV)
    ws = torch.empty(K().l1tv_workspace_bytes(n) // 8, dtype=F64, device=DEV)
    K().l1tv_stats(pred, gt, stats, ws)
    want = torch.stack([(p64 - g64).abs().sum(), (p64[..., :, :-1] - p64[..., :, 1:]).abs().sum(),
                        (p64[..., :-1, :] - p64[..., 1:, :]).abs().sum()]).detach()
    assert torch.equal(stats[:3].cpu(), want)                # multiples of 1/2 below 2^53: every summation order is exact
    for replicas in (1, 2):
        lo = nan_like((1,), torch.float32)
        grad = nan_like(tuple(pred.shape), torch.float32)
        K().l1tv_finish(pred, gt, stats * replicas, replicas, l1w, 0.1, lo, grad)
        assert abs(float(lo) - loss.item()) <= 1e-6 * abs(loss.item())
        c0, cx, cy = l1w / n, sw / (B * H * (W - 1)), sw / (B * (H - 1) * W)
        bound = torch.full((1,), 13 * U * (c0 + 2 * cx + 2 * cy), dtype=F64)
        inside(grad * replicas, p64.grad, bound, torch.float32, f'l1tv grad, {replicas} replicas')
