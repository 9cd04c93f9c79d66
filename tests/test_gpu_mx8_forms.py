"""adn_conv3x3_mx8 (csrc/mx8.hip) on each of its three kernel forms, with each of its four epilogues, over one and two
output segments, against a float64 reference; tests/mx8_conv_cases.py holds the shapes, variants, cases and data, and
tests/test_mx8_conv_cases.py checks them on the host.

The form depends on the shape alone, so every case names the form it is meant to reach and asserts it against
adn_conv3x3_mx8_describe before it launches (with ADN_MX8_BN set the module fails instead of testing something else).

Two data sets per shape, each convolved once in float64 on the CPU (shared by the variants, never modified):
  * exact: small integers times powers of two, spread over 5 (activations) and 4 (weights) binades of block scale.  MX
    quantisation of it is lossless, every partial sum is a multiple of 2^-8 below 2^24 units, the epilogue operands keep
    f32 exact, so every stored output must be BIT-EQUAL to the float64 result cast to f32, then to bf16 (round to nearest
    even).  One wrong scale byte, tap, channel chunk or border pixel changes bits.  Measured on the MI355X: bit equality
    holds at the full exponent spread (X_EXP -2..2, W_EXP -6..-3) on every case; no narrowing was needed.
  * Gaussian, as tests/test_gpu_mx8.py builds it, quantised on the device; reference = the float64 convolution of the
    oracle's dequantised operands; per element 2^-8 |ref| + 1e-3 max|ref| (Z_STATS, ACT), 2^-7 |ref| + 2e-3 max|ref| (ADD, BWD).

BatchNorm partial rows: their number is adn_conv3x3_mx8_num_partials = pixels / BM of the described form, and EACH row is
compared with the float64 sums over its own tile of the unrounded terms.  Bound: an f32 sum of n <= 256 terms lies within
n 2^-24 sum|terms| of the exact sum, whatever the order (the product inside a term adds one more rounding: 255 + 1); on the
Gaussian data, where the kernel's f32 convolution is only within the output tolerance tol of the reference, the tolerance
carried through the term and summed over the tile is added: sum tol (sums of z, of g), sum (2 |z| + tol) tol (of z^2),
sum tol |xhat| (of g xhat).  On the exact data xhat = (z - mean) istd is exact by construction.

Every output and every partials buffer starts as NaN between sentinel guards that must come back untouched; an output or
a partials buffer that is not passed must come back all sentinel.
"""
import numpy as np
import pytest
import torch

import mx8_conv_cases as cases
from test_gpu_igemm_epilogues import GUARD, SENTINEL, Arena

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_OPERANDS = {}                   # (shape key, data) -> (q0, s0, q1, s1, w8, wsc, v float64 [B][H][W][N]); read-only


def _kernels():
    from audio_depth_estimation_amd import kernels as K
    return K


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def bf16_bits(ref64):
    """float64 -> f32 -> bf16 (both round to nearest even), as int16 bit patterns."""
    return torch.from_numpy(np.ascontiguousarray(ref64)).float().to(torch.bfloat16).view(torch.int16)


def _quant_dev(x_bf16):
    q8 = torch.full(x_bf16.shape, 0xAA, dtype=torch.uint8, device=DEV)
    sc = torch.full(x_bf16.shape[:-1] + (x_bf16.shape[-1] // 32,), 0xAA, dtype=torch.uint8, device=DEV)
    _kernels().mx8_quantize(x_bf16.to(DEV), q8, sc)
    return q8, sc


def operands(key, data):
    """Device operands of a shape (quantised and packed by the library) and its convolution in float64, computed once."""
    if (key, data) in _OPERANDS:
        return _OPERANDS[key, data]
    from oracle import mx8_oracle as mx
    K = _kernels()
    s = cases.SHAPES[key]
    C0, C1, N = s['C0'], s['C1'], sum(s['segs'])
    Cin = C0 + C1
    x, w = cases.exact_data(key) if data == 'exact' else cases.gauss_data(key)
    xb = _bf16(x)
    x0, x1 = xb[..., :C0].contiguous(), (xb[..., C0:].contiguous() if C1 else None)
    if data == 'exact':                                    # lossless in bf16 and in MX e4m3: the data is the operand
        assert np.array_equal(xb.double().numpy(), x)
        v = mx.conv3x3(x, w.transpose(0, 2, 3, 1).reshape(N, 9, Cin).astype(np.float64))
    else:
        xd = np.concatenate([mx.quantize(t.float().numpy())[2] for t in (x0, x1) if t is not None], axis=-1)
        v = mx.conv3x3(xd, mx.pack_weights(w, False)[2])
    q0, s0 = _quant_dev(x0)
    q1, s1 = _quant_dev(x1) if C1 else (None, None)
    s8, ssc = K.mx8_pack_shapes(N, Cin, False)
    w8 = torch.full(s8, 0xAA, dtype=torch.uint8, device=DEV)
    wsc = torch.full(ssc, 0xAA, dtype=torch.uint8, device=DEV)
    K.mx8_pack(torch.from_numpy(np.ascontiguousarray(w.transpose(0, 2, 3, 1))).to(DEV), N, Cin, False, w8, wsc)
    torch.cuda.synchronize()
    v.setflags(write=False)
    _OPERANDS[key, data] = (q0, s0, q1, s1, w8, wsc, v)
    return _OPERANDS[key, data]


class Partials:
    """[P][2][n] f32 partial rows in front of a guard: NaN where the kernel is to write, SENTINEL in the guard -- and all
    over when the buffer is not passed."""

    def __init__(self, P, n, passed):
        self.P, self.n, self.passed = P, n, passed
        self.buf = torch.full((P * 2 * n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        if passed:
            self.buf[:P * 2 * n] = float('nan')

    def tensor(self):
        return self.buf[:self.P * 2 * self.n] if self.passed else None

    def rows(self):
        return self.buf[:self.P * 2 * self.n].cpu().double().numpy().reshape(self.P, 2, self.n)

    def untouched(self):
        keep = self.buf.cpu()[self.P * 2 * self.n if self.passed else 0:]
        return bool((keep == SENTINEL).all())


def out_tol(epi, ref):
    """The project's per-element bounds on the Gaussian data (tests/test_gpu_mx8.py)."""
    if epi in (cases.Z_STATS, cases.ACT):
        return 2.0 ** -8 * np.abs(ref) + 1e-3 * np.abs(ref).max()
    return 2.0 ** -7 * np.abs(ref) + 2e-3 * np.abs(ref).max()


class Segment:
    """One output segment of one case: its kernels.Seg, its Arena, the float64 reference of every passed output, and for the
    statistics the unrounded terms t1 (z resp. g) and t2 (z resp. xhat): partial rows = tile sums of t1 and of t1 * t2."""

    def __init__(self, key, epi, o, v, data, rng, si):
        K = _kernels()
        exact = data == 'exact'
        n, shape = v.shape[-1], v.shape
        vec = lambda name: (cases.exact_vector if exact else cases.gauss_vector)(rng, name, n)
        tensor = lambda relu=False: (cases.grid_tensor(rng, shape, relu) if exact else
                                     _bf16(np.maximum(rng.standard_normal(shape), 0.0) if relu
                                           else rng.standard_normal(shape)).double().numpy())
        s = cases.SHAPES[key]
        self.epi, self.terms, self.refs = epi, None, {}
        P = K.conv3x3_mx8_num_partials(s['B'], s['H'], s['W'], sum(s['segs']), s['C0'], s['C1'])
        self.part = Partials(P, n, bool(o.get('stats')))
        kw = {}
        if epi == cases.Z_STATS:
            z = v.copy()
            if o['bias']:
                kw['bias'] = vec('bias')
                z = z + kw['bias'].astype(np.float64)
            self.refs[0] = z
            self.terms = (z, z)
            self.arena = Arena(shape, torch.bfloat16, [0])
        elif epi == cases.ACT:
            for name in o['p']:
                kw[name] = vec(name)
            y = v * kw['scale'].astype(np.float64) if 'scale' in kw else v.copy()
            b = np.zeros(n, np.float32)                                   # shift + bias, folded in f32 as the kernel folds it
            if 'shift' in kw:
                b = kw['shift']
            if 'bias' in kw:
                b = b + kw['bias']
            y = y + b.astype(np.float64)
            self.refs = {0: np.where(y > 0, y, y * float(o['slope'])), 1: np.maximum(y, 0.0)}
            self.arena = Arena(shape, torch.bfloat16, [int(c) for c in o['outs']])
            self.refs = {i: self.refs[i] for i in self.arena.passed}
            kw['slope'] = o['slope']
        elif epi == cases.ADD:
            g = v.copy()
            if o['bias']:
                kw['bias'] = vec('bias')
                g = g + kw['bias'].astype(np.float64)
            if o['scale'] == 'gate':                                      # ONE scalar: element 0 of a longer tensor whose
                gamma = (0.5, 2.0)[si] if exact else 0.37 + 0.25 * si         # other elements hold another, defined value
                gate = np.full(max(n, 8), 5.0, np.float32)
                gate[0] = gamma
                g = g * float(gate[0])
                self.gate = _f32(gate)
                kw['final_act'] = 1
            elif o['scale'] == 'chan':
                kw['scale'] = vec('scale')
                g = g * kw['scale'].astype(np.float64)
            if o['ref']:
                r = tensor()
                g = g + r
                kw['ref'] = _bf16(r).to(DEV)
            self.arena = Arena(shape, torch.bfloat16, [0])
            if o['accumulate']:
                old = tensor() * 2.0
                g = g + old
                self.arena.fill(0, _bf16(old).to(DEV))
            kw['accumulate'] = o['accumulate']
            self.refs[0] = g
        else:                                                             # BWD
            r = tensor(relu=True)
            g = v * np.where(r > 0, 1.0, float(o['slope']))
            self.arena = Arena(shape, torch.bfloat16, [0])
            if o['accumulate']:
                old = tensor()
                g = g + old
                self.arena.fill(0, _bf16(old).to(DEV))
            kw.update(ref=_bf16(r).to(DEV), slope=o['slope'], accumulate=o['accumulate'])
            if o['stats']:
                zf, mean, istd = tensor(), vec('mean'), vec('istd')
                kw.update(z=_bf16(zf).to(DEV), mean=mean, istd=istd)
                self.terms = (g, (zf - mean.astype(np.float64)) * istd.astype(np.float64))
            self.refs[0] = g
        if not o.get('stats'):
            self.terms = None
        kw = {k: (_f32(t) if isinstance(t, np.ndarray) else t) for k, t in kw.items()}
        if epi == cases.ADD and o['scale'] == 'gate':
            kw['scale'] = self.gate[:1]
        self.seg = K.Seg(n, out0=self.arena.out(0), out1=self.arena.out(1), partials=self.part.tensor(), **kw)

    def check(self, what, exact, bm):
        for i, ref in self.refs.items():
            got = self.arena.out(i).cpu()
            if exact:
                want = bf16_bits(ref)
                same = torch.equal(got.view(torch.int16), want)
                if not same:
                    bad = got.view(torch.int16) != want
                    print('%s out%d: %d of %d elements differ, max |diff| %.4g' % (
                        what, i, int(bad.sum()), bad.numel(), float((got.double() - torch.from_numpy(ref))[bad].abs().max())))
                assert same, (what, i)
            else:
                err, tol = np.abs(got.double().numpy() - ref), out_tol(self.epi, ref)
                print('%s out%d: max err / tol %.3f' % (what, i, float(np.nanmax(err / tol))))
                assert np.isfinite(err).all() and (err <= tol).all(), (what, i)
        assert self.arena.guards_untouched(), what
        assert self.part.untouched(), what
        if self.terms is None:
            return
        t1, t2 = self.terms
        rows = self.part.rows()
        assert rows.shape[0] * bm == t1.shape[0] * t1.shape[1] * t1.shape[2]
        tol = 0.0 if exact else out_tol(self.epi, t1)
        slack1 = tol
        slack2 = (2 * np.abs(t1) + tol) * tol if self.epi == cases.Z_STATS else tol * np.abs(t2)
        for st, (term, slack) in enumerate(((t1, slack1), (t1 * t2, slack2))):
            ref = cases.tile_sums(term, bm)
            bound = cases.SUM_BOUND * cases.tile_sums(np.abs(term), bm)
            if not exact:
                bound = bound + cases.tile_sums(slack, bm)
            err = np.abs(rows[:, st, :] - ref)
            print('%s partials[%d]: %d rows, max err / bound %.3f' % (
                what, st, rows.shape[0], float(np.nanmax(err / np.maximum(bound, 1e-300))) if np.isfinite(err).all() else np.nan))
            assert np.isfinite(err).all() and (err <= bound).all(), (what, st)


@pytest.mark.parametrize('case', cases.CASES, ids=cases.case_id)
def test_conv_form_epilogue(case):
    key, epi, var, data = case
    K = _kernels()
    s = cases.SHAPES[key]
    B, H, W, C0, C1, N = s['B'], s['H'], s['W'], s['C0'], s['C1'], sum(s['segs'])
    q0, s0, q1, s1, w8, wsc, v = operands(key, data)
    segs = [Segment(key, epi, o, v[..., lo:hi], data, cases.rng_for(case, si), si)
            for si, ((lo, hi), o) in enumerate(zip(cases.segment_slices(key), cases.per_segment(key, cases.VARIANTS[epi][var])))]
    line = K.conv3x3_mx8_describe(B, H, W, N, C0, C1)
    assert cases.plan_form(line) == s['form'], (key, line)
    bm = int(s['form'].split('x')[0])
    assert K.conv3x3_mx8_num_partials(B, H, W, N, C0, C1) == B * H * W // bm == cases.plan_tiles(line)[0]
    K.conv3x3_mx8(B, H, W, q0, s0, q1, s1, w8, wsc, N, epi, [g.seg for g in segs])
    torch.cuda.synchronize()
    for si, g in enumerate(segs):
        g.check('%s seg%d' % (cases.case_id(case), si), data == 'exact', bm)


# ---- the quantiser at the widths and sizes nothing else checks --------------------------------------------------------------
def _quantize_against_oracle(xb):
    from oracle import mx8_oracle as mx
    want_bits, want_sc, _ = mx.quantize(xb.float().numpy())
    q8, sc = _quant_dev(xb)
    torch.cuda.synchronize()
    assert np.array_equal(sc.cpu().numpy(), want_sc)
    got = q8.cpu().numpy()
    nz = (want_bits & 0x7f) != 0                          # (sign of a zero: not part of the contract)
    assert np.array_equal(got[nz], want_bits[nz])
    assert not ((got & 0x7f)[~nz]).any()


@pytest.mark.parametrize('Cc', [32, 96])
def test_quantize_bit_exact_at_narrow_widths(Cc):
    """One block per row (C = 32: four threads of a quad span one row) and three (C = 96: the width
    test_fused_fp8_copies_equal_quantizing_the_bf16_output trusts the quantiser at)."""
    rng = np.random.default_rng(Cc)
    rows = 1028
    x = rng.standard_normal((rows, Cc // 32, 32)) * np.exp2(rng.integers(-30, 30, (rows, Cc // 32, 1)))
    x[5] = 0.0                                            # all-zero blocks
    x[6, 0] = 448.0 * 2.0 ** 3                            # exactly the top of a binade
    x[7, -1] = 1.76 * 2.0 ** -3                           # mantissa above 1.75: the scale moves up
    x[8, 0] = np.linspace(-1, 1, 32) * 3e38               # near the top of the bf16 range
    x[9, -1] = np.linspace(-1, 1, 32) * 1e-38             # near the bottom
    _quantize_against_oracle(_bf16(x.reshape(rows, Cc)))


def test_quantize_past_one_grid_pass():
    """2 097 664 eight-channel chunks: 512 more than the 8 192 blocks x 256 threads the launch is capped at, so the last 512
    chunks are a thread's second trip through the grid-stride loop."""
    rows, Cc = 262208, 64
    assert rows * Cc // 8 == 8192 * 256 + 512
    g = torch.Generator().manual_seed(11)
    x = torch.randn(rows, Cc // 32, 32, generator=g) * torch.exp2(torch.randint(-20, 20, (rows, Cc // 32, 1), generator=g).float())
    _quantize_against_oracle(x.reshape(rows, Cc).to(torch.bfloat16))
