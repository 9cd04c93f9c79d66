"""The 4x4 stride-2 kernels ("k4": the S2 / T2 geometries of adn_igemm with the RAW, Z_STATS and BWD epilogues, adn_wgrad,
adn_wgrad_batch and adn_wgrad_patch_batch) on rectangular and non-power-of-two small grids, through the C ABI and against a
float64 reference.

The engine passes Hs and Ws separately to every one of these calls and accepts any image divisible by 2^levels, but the
other modules launch them on squares only.  The planner's tiling rules are not symmetric (tests/k4_rect_cases.py), so every
grid is launched as Hs x Ws and as Ws x Hs; each case asserts the kernel form of its own descriptor before it launches.

Reference: operands are pre-rounded to the storage dtype; the convolution (or, for a weight gradient, torch autograd) runs
in float64 on the CPU from those rounded values, once per shape.  Inputs come from a generator seeded by the case name and
plain randn images are not symmetric under transposition: SWAP_SENTINEL / WGRAD_SENTINEL cases also assert that the result
is NOT within tolerance of the reference of the image with H and W exchanged, so the case can see an Hs / Ws mix-up.
Every output and every partials tensor starts as NaN.

Tolerances are the ones test_gpu_kernels.py states for these kernels on squares: f32 outputs <= TOL_F32_OUT (2e-5 f32, 1e-4
bf16) of max|ref|, outputs in dtype <= TOL_T_OUT (2e-5 / 6e-3), twice that where the launch accumulates; BatchNorm-forward
column sums <= 1e-4 + TOL_F32_OUT, BatchNorm-backward sums <= 1e-3; norm partials 1e-7 of sum(dW^2).
"""
import ctypes as C
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

import k4_rect_cases as kc
from test_gpu_kernels import DEV, TOL_F32_OUT, TOL_T_OUT, K, from_nhwc, nhwc, pack, rel_err, rounded, ws_for

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {kc.F32: torch.float32, kc.BF16: torch.bfloat16}
NAN = float('nan')


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _conv(geom, x, w):
    if geom == kc.S2:
        return F.conv2d(x.double(), w.double(), stride=2, padding=1)
    return F.conv_transpose2d(x.double(), w.double(), stride=2, padding=1)


def _hw_exchanged(t):
    """The NCHW image whose NHWC memory is t's, read with H and W exchanged."""
    B, Cc, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B, W, H, Cc).permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=2)
def operands(key):
    """(x, w, device operands, v): rounded input and weights on the CPU, in0 / in1 / packed weights on the device and the
    convolution in float64, NCHW.  Shared by the epilogues of a shape (consecutive tests), never modified."""
    c = kc.IGEMM[key]
    dtype = TORCH_DTYPE[c['dtype']]
    B, Hs, Ws, C0, C1, N = c['B'], c['Hs'], c['Ws'], c['C0'], c['C1'], sum(c['segs'])
    g = _gen(key)
    if c['geom'] == kc.S2:                          # Conv2d(k4, s2, p1) / dgrad of ConvTranspose2d: out on the small grid
        x = rounded(torch.randn(B, C0 + C1, 2 * Hs, 2 * Ws, generator=g), dtype)
        w = rounded(torch.randn(N, C0 + C1, 4, 4, generator=g) * 0.1, dtype)
        w_op = pack(w, dtype)[0]
    else:                                           # ConvTranspose2d(k4, s2, p1) / dgrad of Conv2d: out on the large grid
        x = rounded(torch.randn(B, C0 + C1, Hs, Ws, generator=g), dtype)
        w = rounded(torch.randn(C0 + C1, N, 4, 4, generator=g) * 0.1, dtype)
        w_op = pack(w, dtype)[1]
    in0 = nhwc(x[:, :C0], dtype)
    in1 = nhwc(x[:, C0:], dtype) if C1 else None
    return x, w, (in0, in1, w_op), _conv(c['geom'], x, w)


def launch(key, epi, segs):
    """Assert the planned form of this very descriptor, then launch it; returns the partial rows of the plan."""
    c = kc.IGEMM[key]
    k = K()
    dtype = TORCH_DTYPE[c['dtype']]
    in0, in1, w_op = operands(key)[2]
    N = sum(c['segs'])
    P, ws = ws_for(dtype, c['geom'], c['B'], c['Hs'], c['Ws'], c['C0'], c['C1'], N, c['segs'], epi=epi)
    from audio_depth_estimation_amd import _lib
    d = k._igemm_desc(dtype, c['geom'], c['B'], c['Hs'], c['Ws'], in0, in1, w_op, N, epi, segs, ws, 0)
    buf = C.create_string_buffer(160)
    assert _lib.load().adn_igemm_describe(C.byref(d), buf, len(buf)) == 0
    import igemm_epilogue_cases
    assert igemm_epilogue_cases.plan_form(buf.value.decode()) == c['forms'][epi], (key, buf.value.decode())
    k.igemm(dtype, c['geom'], c['B'], c['Hs'], c['Ws'], in0, in1, w_op, N, epi, segs, ws)
    torch.cuda.synchronize()
    return P


def seg_slices(key):
    lo = 0
    for ch in kc.IGEMM[key]['segs']:
        yield lo, lo + ch
        lo += ch


def out_shape(key, ch):
    c = kc.IGEMM[key]
    m = 1 if c['geom'] == kc.S2 else 2
    return (c['B'], m * c['Hs'], m * c['Ws'], ch)


def num_partial_rows(key, epi):
    c = kc.IGEMM[key]
    return K().igemm_query(TORCH_DTYPE[c['dtype']], c['geom'], c['B'], c['Hs'], c['Ws'], c['C0'], c['C1'], sum(c['segs']),
                           c['segs'], epi=epi)[0]


GUARD_ROWS = 2              # partial rows behind the plan's own: the kernel must leave them alone


def new_partials(P, ch):
    return torch.full((P + GUARD_ROWS, 2, ch), NAN, dtype=torch.float32, device=DEV)


def check_partials(partials, P, want0, want1, tol, what):
    """Rows [:P] all written (no NaN survives), the rows behind them untouched, both sums against the float64 ones."""
    got = partials.cpu()
    assert not bool(torch.isnan(got[:P]).any()), (what, 'a partial row of the plan was not written')
    assert bool(torch.isnan(got[P:]).all()), (what, 'a partial row beyond the plan was written')
    for name, col, want in (('sum', 0, want0), ('sum2', 1, want1)):
        err = rel_err(got[:P, col].double().sum(0), want)
        print('%s %s: %.3e' % (what, name, err))
        assert err <= tol, (what, name, err)


def check_forward_and_input_gradient(key):
    """RAW epilogue, f32 output: S2 == Conv2d(k4, s2, p1) forward == the input gradient of the transposed conv whose weights
    are these; T2 == ConvTranspose2d(k4, s2, p1) forward == the input gradient of the conv (sets A and C mirror each other)."""
    c = kc.IGEMM[key]
    dtype = TORCH_DTYPE[c['dtype']]
    x, w, _, v = operands(key)
    k = K()
    outs = [torch.full(out_shape(key, hi - lo), NAN, dtype=torch.float32, device=DEV) for lo, hi in seg_slices(key)]
    launch(key, kc.RAW, [k.Seg(o.shape[-1], out0=o) for o in outs])
    got = torch.cat([from_nhwc(o) for o in outs], 1)
    err = rel_err(got, v)
    print('%s: %.3e' % (key, err))
    assert err <= TOL_F32_OUT[dtype], err
    if key in kc.SWAP_SENTINEL:
        # the same memory read as a Ws x Hs image, convolved, and its output memory read back as Hs x Ws
        v_sw = _conv(c['geom'], _hw_exchanged(x), w)
        wrong = _hw_exchanged(v_sw)
        assert wrong.shape == v.shape
        far = rel_err(got, wrong)
        print('%s: %.3e from the H/W-exchanged reference' % (key, far))
        assert far > 100 * TOL_F32_OUT[dtype], far


def check_z_stats(key):
    """Z_STATS: z in dtype and, per segment, the column sums of z and z^2 over the partial rows the query announces."""
    c = kc.IGEMM[key]
    dtype = TORCH_DTYPE[c['dtype']]
    v = operands(key)[3]
    k = K()
    P = num_partial_rows(key, kc.Z_STATS)
    zs = [torch.full(out_shape(key, hi - lo), NAN, dtype=dtype, device=DEV) for lo, hi in seg_slices(key)]
    parts = [new_partials(P, z.shape[-1]) for z in zs]
    assert launch(key, kc.Z_STATS, [k.Seg(z.shape[-1], out0=z, partials=p) for z, p in zip(zs, parts)]) == P
    for si, ((lo, hi), z, p) in enumerate(zip(seg_slices(key), zs, parts)):
        ref = v[:, lo:hi]
        err = rel_err(from_nhwc(z), ref)
        print('%s seg%d z: %.3e' % (key, si, err))
        assert err <= TOL_T_OUT[dtype], (si, err)
        check_partials(p, P, ref.sum((0, 2, 3)), (ref * ref).sum((0, 2, 3)), 1e-4 + TOL_F32_OUT[dtype], '%s seg%d' % (key, si))


def _away_from_zero(z, scale, shift, dtype):
    """z (rounded to dtype) such that act = z * scale + shift is nowhere within 1e-3 of 0: the mask act > 0 is then the
    same in any arithmetic."""
    sc, sh = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    for _ in range(4):
        act = z.double() * sc + sh
        near = act.abs() < 1e-3
        if not bool(near.any()):
            return z, act
        z = torch.where(near, rounded(z + 0.5, dtype), z)
    raise AssertionError('could not move the activations away from 0')


def check_bwd(key):
    """BWD: g = v * (ref > 0 ? 1 : slope) (+ old out0 where the launch accumulates), one or two segments; the last segment
    carries the BatchNorm-backward sums of g and g * xhat.  S2 (the dgrad of a transposed conv) masks by a ReLU, T2 (the
    dgrad of a conv) by a LeakyReLU; in a two-segment launch the first segment takes the other one.  BWD_MASK_FROM_Z cases
    pass the forward's scale / shift with ref = leaky(z * scale + shift), so a kernel may take the mask from z."""
    c = kc.IGEMM[key]
    dtype = TORCH_DTYPE[c['dtype']]
    v = operands(key)[3]
    k = K()
    g = _gen(key + '/bwd')
    accumulate, mask_z = key in kc.BWD_ACCUMULATE, key in kc.BWD_MASK_FROM_Z
    P = num_partial_rows(key, kc.BWD)
    nseg = len(c['segs'])
    segs, checks = [], []
    for si, (lo, hi) in enumerate(seg_slices(key)):
        ch, last = hi - lo, si == nseg - 1
        shape = (c['B'], ch) + out_shape(key, ch)[1:3]                                   # NCHW
        slope = (0.0, 0.2)[(c['geom'] == kc.T2) == last]
        ref_act = rounded(torch.randn(shape, generator=g), dtype)
        mask = ref_act > 0
        kw = {}
        if last:
            zfwd = rounded(torch.randn(shape, generator=g), dtype)
            mean, istd = torch.randn(ch, generator=g) * 0.1, torch.rand(ch, generator=g) + 0.5
            if mask_z:
                slope = 0.2
                scale, shift = torch.randn(ch, generator=g) * 0.5 + 1.0, torch.randn(ch, generator=g) * 0.3
                scale[::7] *= -1.0                                                       # (a negative gamma flips the mask)
                zfwd, act = _away_from_zero(zfwd, scale, shift, dtype)
                mask = act > 0
                ref_act = rounded(F.leaky_relu(act, slope).float(), dtype)
                kw.update(scale=scale.to(DEV), shift=shift.to(DEV))
            partials = new_partials(P, ch)
            kw.update(z=nhwc(zfwd, dtype), mean=mean.to(DEV), istd=istd.to(DEV), partials=partials)
        g_ref = v[:, lo:hi] * torch.where(mask, 1.0, slope).double()
        if accumulate:
            old = rounded(torch.randn(shape, generator=g), dtype)
            g_ref = g_ref + old.double()
            out = nhwc(old, dtype).clone()
        else:
            out = torch.full(out_shape(key, ch), NAN, dtype=dtype, device=DEV)
        segs.append(k.Seg(ch, out0=out, ref=nhwc(ref_act, dtype), slope=slope, accumulate=accumulate, **kw))
        checks.append((out, g_ref, (partials, zfwd, mean, istd) if last else None))
    assert launch(key, kc.BWD, segs) == P
    for si, (out, g_ref, stats) in enumerate(checks):
        err = rel_err(from_nhwc(out), g_ref)
        print('%s seg%d g: %.3e' % (key, si, err))
        assert err <= (2 if accumulate else 1) * TOL_T_OUT[dtype], (si, err)
        if stats is not None:
            partials, zfwd, mean, istd = stats
            xhat = (zfwd.double() - mean.double().view(1, -1, 1, 1)) * istd.double().view(1, -1, 1, 1)
            check_partials(partials, P, g_ref.sum((0, 2, 3)), (g_ref * xhat).sum((0, 2, 3)), 1e-3, '%s seg%d' % (key, si))


EPI_NAME = {kc.RAW: 'raw', kc.Z_STATS: 'z_stats', kc.BWD: 'bwd'}
# shape by shape, so that the epilogues of a shape run back to back and share its operands and its float64 convolution
IGEMM_LAUNCHES = [(key, epi) for key, c in kc.IGEMM.items() for epi in kc.EPIS if c['forms'][epi] is not None]


@pytest.mark.parametrize('key,epi', IGEMM_LAUNCHES, ids=['%s-%s' % (k_, EPI_NAME[e]) for k_, e in IGEMM_LAUNCHES])
def test_igemm(key, epi):
    """Every (shape, epilogue) of tests/k4_rect_cases.py against float64: see the three checks above."""
    {kc.RAW: check_forward_and_input_gradient, kc.Z_STATS: check_z_stats, kc.BWD: check_bwd}[epi](key)


# ---------------------------------------------------------------- weight gradient
def _dw_reference(style, plain, gath):
    """float64 autograd dW, [R][16][C]: conv-style (plain = dZ on the small grid, gathered = the layer input on the large one)
    or convT-style (plain = the layer input on the small grid, gathered = dZ on the large one)."""
    R, Cg = plain.shape[1], gath.shape[1]
    w = torch.zeros(R, Cg, 4, 4, dtype=torch.float64, requires_grad=True)
    if style == 'conv':
        F.conv2d(gath.double(), w, stride=2, padding=1).backward(plain.double())
    else:
        F.conv_transpose2d(plain.double(), w, stride=2, padding=1).backward(gath.double())
    return w.grad.permute(0, 2, 3, 1).reshape(R, 16, Cg)


def _wgrad_operands(name, dtype, B, Hs, Ws, R0, R1, C0, C1):
    g = _gen(name)
    plain = rounded(torch.randn(B, R0 + R1, Hs, Ws, generator=g), dtype)
    gath = rounded(torch.randn(B, C0 + C1, 2 * Hs, 2 * Ws, generator=g), dtype)
    dev = (nhwc(plain[:, :R0], dtype), nhwc(plain[:, R0:], dtype) if R1 else None,
           nhwc(gath[:, :C0], dtype), nhwc(gath[:, C0:], dtype) if C1 else None)
    return plain, gath, dev


@pytest.mark.parametrize('style', ['conv', 'convT'])
@pytest.mark.parametrize('key', list(kc.WGRAD))
def test_wgrad(key, style):
    """adn_wgrad against float64 autograd, the norm partials against the dW that was written."""
    c = kc.WGRAD[key]
    dtype = TORCH_DTYPE[c['dtype']]
    B, Hs, Ws, R0, R1, C0, C1 = (c[n] for n in ('B', 'Hs', 'Ws', 'R0', 'R1', 'C0', 'C1'))
    k = K()
    assert (k.wgrad_workspace_bytes(dtype, B, Hs, Ws, R0, R1, C0, C1), k.wgrad_sq_count(dtype, B, Hs, Ws, R0, R1, C0, C1),
            k.wgrad_batchable(dtype, B, Hs, Ws, R0, R1, C0, C1)[0]) == c['answers']
    plain, gath, (p0, p1, g0, g1) = _wgrad_operands(key + style, dtype, B, Hs, Ws, R0, R1, C0, C1)
    ref = _dw_reference(style, plain, gath)
    n = ref.numel()
    ws = torch.empty(max(c['answers'][0], 16) // 4, dtype=torch.float32, device=DEV)
    dw = torch.full((n,), NAN, dtype=torch.float32, device=DEV)
    k.wgrad(dtype, B, Hs, Ws, p0, p1, g0, g1, dw, ws)
    err = rel_err(dw.view(ref.shape), ref)
    print('%s %s: %.3e' % (key, style, err))
    assert err <= TOL_F32_OUT[dtype], err
    if key in kc.WGRAD_SENTINEL:
        far = rel_err(dw.view(ref.shape), _dw_reference(style, _hw_exchanged(plain), _hw_exchanged(gath)))
        print('%s %s: %.3e from the H/W-exchanged reference' % (key, style, far))
        assert far > 100 * TOL_F32_OUT[dtype], far
    cnt = c['answers'][1]
    sq = torch.full((max(cnt, 1),), NAN, dtype=torch.float64, device=DEV)
    dw2 = torch.full((n,), NAN, dtype=torch.float32, device=DEV)
    k.wgrad(dtype, B, Hs, Ws, p0, p1, g0, g1, dw2, ws, sq=sq)
    assert torch.equal(dw2, dw)
    if cnt == 0:
        assert bool(torch.isnan(sq).all())                       # documented: nothing is written
        return
    want = float((dw.double() ** 2).sum())
    assert abs(float(sq.sum()) - want) <= 1e-7 * want, (float(sq.sum()), want)


def _batch_operands(tag, B, probs):
    """float64 references and device operands of the problems of a batch launch."""
    dtype = torch.bfloat16
    refs, ops = [], []
    for i, (Hs, Ws, R0, R1, Cc) in enumerate(probs):
        plain, gath, (p0, p1, g0, g1) = _wgrad_operands('%s/%d' % (tag, i), dtype, B, Hs, Ws, R0, R1, Cc, 0)
        refs.append(_dw_reference('convT' if R1 else 'conv', plain, gath))
        ops.append((Hs, Ws, p0, p1, g0, g1))
    return refs, ops


@pytest.mark.parametrize('group', range(len(kc.WGRAD_BATCH)))
def test_wgrad_batch(group):
    """adn_wgrad_batch on rectangular small levels: every problem against float64, bit-identical to its lone unsplit launch
    (adn_wgrad where that plans unsplit, else a batch of one: inside a batch every problem runs unsplit) -- dW and the norm
    partials alike -- and within 1e-5 of a lone launch that splits the pixels (another summation order)."""
    B, cls, probs = kc.WGRAD_BATCH[group]
    k = K()
    dtype = torch.bfloat16
    refs, ops = _batch_operands('batch%d' % group, B, probs)
    problems, lone = [], []
    for (Hs, Ws, p0, p1, g0, g1), (_, _, R0, R1, Cc), ref in zip(ops, probs, refs):
        n = ref.numel()
        got_cls, nsq = k.wgrad_batchable(dtype, B, Hs, Ws, R0, R1, Cc, 0)
        assert got_cls == cls and nsq > 0
        nbytes = k.wgrad_workspace_bytes(dtype, B, Hs, Ws, R0, R1, Cc, 0)
        ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=DEV)
        dw_ref = torch.full((n,), NAN, device=DEV)
        k.wgrad(dtype, B, Hs, Ws, p0, p1, g0, g1, dw_ref, ws)
        dw1 = torch.full((n,), NAN, device=DEV)
        sq1 = torch.full((nsq,), NAN, dtype=torch.float64, device=DEV)
        k.wgrad_batch(dtype, B, [(Hs, Ws, p0, p1, g0, g1, dw1, sq1)])
        if nbytes == 0:                                           # the lone launch is unsplit too: the same bits
            assert nsq == k.wgrad_sq_count(dtype, B, Hs, Ws, R0, R1, Cc, 0)
            sq_ref = torch.full((nsq,), NAN, dtype=torch.float64, device=DEV)
            k.wgrad(dtype, B, Hs, Ws, p0, p1, g0, g1, dw1.clone(), ws, sq=sq_ref)
            assert torch.equal(dw1, dw_ref) and torch.equal(sq1, sq_ref), (Hs, Ws)
        else:
            assert rel_err(dw1, dw_ref.cpu()) <= 1e-5, (Hs, Ws)
        lone.append((dw1, sq1))
        problems.append((Hs, Ws, p0, p1, g0, g1, torch.full((n,), NAN, device=DEV),
                         torch.full((nsq,), NAN, dtype=torch.float64, device=DEV)))
    k.wgrad_batch(dtype, B, problems)
    for prob, (dw1, sq1), ref in zip(problems, lone, refs):
        dw, sq = prob[6], prob[7]
        err = rel_err(dw.view(ref.shape), ref)
        print('batch %d, %dx%d: %.3e' % (group, prob[0], prob[1], err))
        assert err <= TOL_F32_OUT[dtype], (prob[:2], err)
        assert torch.equal(dw, dw1) and torch.equal(sq, sq1), prob[:2]
        want = float((dw.double() ** 2).sum())
        assert abs(float(sq.sum()) - want) <= 1e-7 * want, prob[:2]


@pytest.mark.parametrize('group', range(len(kc.WGRAD_PATCH_BATCH)))
def test_wgrad_patch_batch(group):
    """adn_wgrad_patch_batch on rectangular levels: every problem against float64 and within 1e-5 of its lone launch
    (another summation order); the norm partials add up to sum(dW^2) of the dW that was written."""
    probs, nbytes = kc.WGRAD_PATCH_BATCH[group]
    B = kc.PATCH_BATCH_B
    k = K()
    dtype = torch.bfloat16
    assert k.wgrad_patch_batch_workspace_bytes(dtype, B, [(h, w, r0, r1, cc, 0) for h, w, r0, r1, cc in probs]) == nbytes
    refs, ops = _batch_operands('patch_batch%d' % group, B, probs)
    problems, lone = [], []
    for (Hs, Ws, p0, p1, g0, g1), (_, _, R0, R1, Cc), ref in zip(ops, probs, refs):
        n = ref.numel()
        nsq = k.wgrad_sq_count(dtype, B, Hs, Ws, R0, R1, Cc, 0)
        assert nsq > 0
        ws = torch.empty(max(k.wgrad_workspace_bytes(dtype, B, Hs, Ws, R0, R1, Cc, 0), 16) // 4, device=DEV)
        dw_ref = torch.full((n,), NAN, device=DEV)
        k.wgrad(dtype, B, Hs, Ws, p0, p1, g0, g1, dw_ref, ws)
        lone.append(dw_ref)
        problems.append((Hs, Ws, p0, p1, g0, g1, torch.full((n,), NAN, device=DEV),
                         torch.full((nsq,), NAN, dtype=torch.float64, device=DEV)))
    ws = torch.empty(max(nbytes, 16) // 4, device=DEV)
    k.wgrad_patch_batch(dtype, B, problems, ws)
    for prob, dw_ref, ref in zip(problems, lone, refs):
        dw, sq = prob[6], prob[7]
        err = rel_err(dw.view(ref.shape), ref)
        print('patch batch %d, %dx%d: %.3e' % (group, prob[0], prob[1], err))
        assert err <= TOL_F32_OUT[dtype], (prob[:2], err)
        assert rel_err(dw, dw_ref.cpu()) <= 1e-5, prob[:2]
        want = float((dw.double() ** 2).sum())
        assert abs(float(sq.sum()) - want) <= 1e-7 * want, prob[:2]
