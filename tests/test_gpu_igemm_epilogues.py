"""The ACT, FINAL and ADD epilogues of adn_igemm, launched through the C ABI on every kernel form that can carry them, against
a float64 reference.

The three epilogues are written twice in csrc/epilogue.h: epi_scalar runs behind split-K and the direct path (the reduce
kernel), epi_cols_init / epi_vec8 run in the unsplit tile kernel and the three patch kernels (tile_epi_finish).  The plan
depends on the shape, so every case names the kernel form it is meant to reach (tests/igemm_epilogue_cases.py) and asserts it
against adn_igemm_describe of its own descriptor before it launches.

Reference: inputs and weights are pre-rounded to the storage dtype; the convolution is computed in float64 on the CPU from
those rounded values (once per shape, shared by the epilogue variants of that shape and never modified), then the epilogue
in float64, written out plainly.  Tolerances are those of test_gpu_kernels.py: outputs in dtype <= TOL_T_OUT (2e-5 f32,
6e-3 bf16) of max|ref|, the f32 outputs of FINAL <= TOL_F32_OUT (2e-5 / 1e-4).

Every output starts as NaN and sits in one arena per segment, [out0 | guard | out1 | guard]; an output that is not passed is
guard all over.  The guards must come back untouched.
"""
import ctypes as C
import zlib

import pytest
import torch
import torch.nn.functional as F

import igemm_epilogue_cases as cases
from test_gpu_dcnet_kernels import s1_operands
from test_gpu_kernels import DEV, TOL_F32_OUT, TOL_T_OUT, K, nhwc, pack, rounded, ws_for

pytestmark = pytest.mark.gpu

GUARD = 256                      # elements of every guard region
SENTINEL = -7.0                  # exact in bf16
TORCH_DTYPE = {cases.F32: torch.float32, cases.BF16: torch.bfloat16}
_OPERANDS = {}                   # shape key -> (in0, in1, packed weights, v float64 [B][Ho][Wo][N]); read-only


def operands(key):
    """Device operands of a shape and its convolution in float64 (NHWC), computed once."""
    if key in _OPERANDS:
        return _OPERANDS[key]
    s = cases.SHAPES[key]
    dtype = TORCH_DTYPE[s['dtype']]
    B, Hs, Ws, C0, C1, N, ks = s['B'], s['Hs'], s['Ws'], s['C0'], s['C1'], sum(s['segs']), s['ks']
    Cin = C0 + C1
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    if s['geom'] == cases.S2:                       # Conv2d(k4, s2, p1): out on the small grid
        x = rounded(torch.randn(B, Cin, 2 * Hs, 2 * Ws, generator=g), dtype)
        w = rounded(torch.randn(N, Cin, 4, 4, generator=g) * 0.1, dtype)
        v = F.conv2d(x.double(), w.double(), stride=2, padding=1)
        w_op = pack(w, dtype)[0]
    elif s['geom'] == cases.T2:                     # ConvTranspose2d(k4, s2, p1): out on the large grid
        x = rounded(torch.randn(B, Cin, Hs, Ws, generator=g), dtype)
        w = rounded(torch.randn(Cin, N, 4, 4, generator=g) * 0.1, dtype)
        v = F.conv_transpose2d(x.double(), w.double(), stride=2, padding=1)
        w_op = pack(w, dtype)[1]
    else:                                           # Conv2d(ks, padding = ks // 2)
        x = rounded(torch.randn(B, Cin, Hs, Ws, generator=g), dtype)
        w = rounded(torch.randn(N, Cin, ks, ks, generator=g) * 0.1, dtype)
        v = F.conv2d(x.double(), w.double(), padding=ks // 2)
        w_op = s1_operands(w, dtype)[0]
    in0 = nhwc(x[:, :C0], dtype)
    in1 = nhwc(x[:, C0:], dtype) if C1 else None
    _OPERANDS[key] = (in0, in1, w_op, v.permute(0, 2, 3, 1).contiguous())
    return _OPERANDS[key]


def channel_vector(name, n, seed):
    """Distinct, non-constant per-channel f32 vectors: a ramp plus a seeded perturbation; `scale` takes both signs."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = {'scale': (-1.5, 1.5), 'shift': (-0.8, 0.6), 'bias': (0.9, -0.7)}[name]
    ramp = torch.linspace(lo, hi, n) if n > 1 else torch.tensor([hi])
    return (ramp + 0.2 * torch.randn(n, generator=g)).float()


class Arena:
    """[out0 | guard | out1 | guard] of one segment in one allocation; outputs NaN, guards (and outputs not passed) SENTINEL."""

    def __init__(self, shape, dtype, passed):
        self.shape, n = shape, 1
        for d in shape:
            n *= d
        self.n = n
        self.stride = -(-n // 64) * 64 + GUARD                 # (region starts stay 16-byte aligned)
        self.buf = torch.full((2 * self.stride,), SENTINEL, dtype=dtype, device=DEV)
        self.passed = passed
        for i in passed:
            self.buf[i * self.stride:i * self.stride + n] = float('nan')

    def out(self, i):
        return self.buf[i * self.stride:i * self.stride + self.n].view(self.shape) if i in self.passed else None

    def fill(self, i, values):
        self.out(i).copy_(values)

    def guards_untouched(self):
        keep = torch.ones(2 * self.stride, dtype=torch.bool)
        for i in self.passed:
            keep[i * self.stride:i * self.stride + self.n] = False
        return bool((self.buf.cpu()[keep] == SENTINEL).all())


def max_rel_err(got, ref):
    """max|got - ref| / max|ref| in float64; NaN (an element nobody wrote) stays NaN and fails every bound."""
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def launch(key, epi, segs):
    """Assert the planned form of this very descriptor, then launch it."""
    s = cases.SHAPES[key]
    k = K()
    dtype = TORCH_DTYPE[s['dtype']]
    in0, in1, w_op, _ = operands(key)
    N = sum(s['segs'])
    if s['geom'] == cases.S1:
        nbytes = k.igemm_query(dtype, s['geom'], s['B'], s['Hs'], s['Ws'], s['C0'], s['C1'], N, s['segs'], ks=s['ks'], epi=epi)[1]
        ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=DEV)
    else:
        ws = ws_for(dtype, s['geom'], s['B'], s['Hs'], s['Ws'], s['C0'], s['C1'], N, s['segs'], epi=epi)[1]
    from audio_depth_estimation_amd import _lib
    d = k._igemm_desc(dtype, s['geom'], s['B'], s['Hs'], s['Ws'], in0, in1, w_op, N, epi, segs, ws, s['ks'])
    buf = C.create_string_buffer(160)
    assert _lib.load().adn_igemm_describe(C.byref(d), buf, len(buf)) == 0
    assert cases.plan_form(buf.value.decode()) == s['form'], (key, buf.value.decode())
    k.igemm(dtype, s['geom'], s['B'], s['Hs'], s['Ws'], in0, in1, w_op, N, epi, segs, ws, ks=s['ks'])
    torch.cuda.synchronize()


def segment_slices(key):
    lo = 0
    for ch in cases.SHAPES[key]['segs']:
        yield lo, lo + ch
        lo += ch


def per_segment(key, variant):
    segs = cases.SHAPES[key]['segs']
    assert len(variant) in (1, len(segs)), 'a two-segment variant needs a two-segment shape'
    return [variant[i if len(variant) > 1 else 0] for i in range(len(segs))]


def case_id(c):
    key, var = c
    return '%s-%s' % (key, var if isinstance(var, str) else 'act%d_%s' % (var[0], 'bias' if var[1] else 'nobias'))


@pytest.mark.parametrize('case', cases.ACT_CASES, ids=case_id)
def test_epilogue_act(case):
    """ACT: y = v * scale[n] + shift[n] + bias[n]; out0 = leaky(y, slope), out1 = relu(y), each only where it is passed."""
    key, var = case
    dtype = TORCH_DTYPE[cases.SHAPES[key]['dtype']]
    v = operands(key)[3]
    k = K()
    segs, arenas, refs = [], [], []
    for si, ((lo, hi), o) in enumerate(zip(segment_slices(key), per_segment(key, cases.ACT_VARIANTS[var]))):
        vec = {n: channel_vector(n, hi - lo, 100 * si + j) for j, n in enumerate(('scale', 'shift', 'bias')) if n in o['p']}
        y = v[..., lo:hi].clone()
        if 'scale' in vec:
            y = y * vec['scale'].double()
        if 'shift' in vec:
            y = y + vec['shift'].double()
        if 'bias' in vec:
            y = y + vec['bias'].double()
        refs.append({0: torch.where(y > 0, y, y * float(o['slope'])), 1: y.clamp_min(0.0)})
        a = Arena(y.shape, dtype, [int(c) for c in o['outs']])
        arenas.append(a)
        segs.append(k.Seg(hi - lo, out0=a.out(0), out1=a.out(1), slope=o['slope'],
                          **{n: t.to(DEV) for n, t in vec.items()}))
    launch(key, cases.ACT, segs)
    for si, (a, ref) in enumerate(zip(arenas, refs)):
        for i in a.passed:
            err = max_rel_err(a.out(i), ref[i])
            print('%s seg%d out%d: %.3e' % (case_id(case), si, i, err))
            assert err <= TOL_T_OUT[dtype], (si, i, err)
        assert a.guards_untouched(), si


@pytest.mark.parametrize('case', cases.FINAL_CASES, ids=case_id)
def test_epilogue_final(case):
    """FINAL: out0 (always f32) = final_act(v + bias[n]), final_act 0 relu, 1 sigmoid, 2 identity."""
    key, (final_act, has_bias) = case
    dtype = TORCH_DTYPE[cases.SHAPES[key]['dtype']]
    v = operands(key)[3]
    k = K()
    segs, arenas, refs = [], [], []
    for si, (lo, hi) in enumerate(segment_slices(key)):
        y = v[..., lo:hi].clone()
        bias = channel_vector('bias', hi - lo, 300 + si) if has_bias else None
        if has_bias:
            y = y + bias.double()
        refs.append(y.clamp_min(0.0) if final_act == 0 else (torch.sigmoid(y) if final_act == 1 else y))
        a = Arena(y.shape, torch.float32, [0])
        arenas.append(a)
        segs.append(k.Seg(hi - lo, out0=a.out(0), bias=bias.to(DEV) if has_bias else None, final_act=final_act))
    launch(key, cases.FINAL, segs)
    for si, (a, ref) in enumerate(zip(arenas, refs)):
        err = max_rel_err(a.out(0), ref)
        print('%s seg%d: %.3e' % (case_id(case), si, err))
        assert err <= TOL_F32_OUT[dtype], (si, err)
        assert a.guards_untouched(), si


@pytest.mark.parametrize('case', cases.ADD_CASES, ids=case_id)
def test_epilogue_add(case):
    """ADD: out0 = (v + bias[n]) * scale + ref + old out0, every term optional; scale is per channel, or with final_act != 0
    ONE device scalar (the residual gate gamma).  The gate is element 0 of a longer tensor whose other elements hold another
    value, so that a kernel indexing it by channel reads defined, wrong numbers."""
    key, var = case
    dtype = TORCH_DTYPE[cases.SHAPES[key]['dtype']]
    v = operands(key)[3]
    k = K()
    segs, arenas, refs = [], [], []
    for si, ((lo, hi), o) in enumerate(zip(segment_slices(key), per_segment(key, cases.ADD_VARIANTS[var]))):
        n = hi - lo
        g = torch.Generator().manual_seed(500 + si)
        y = v[..., lo:hi].clone()
        bias = channel_vector('bias', n, 400 + si) if o['bias'] else None
        if o['bias']:
            y = y + bias.double()
        scale = None
        if o['scale'] == 'gate':
            gamma = 0.37 + 0.25 * si                         # != 1, != bias[0]
            scale = torch.full((max(n, 8),), 5.0)
            scale[0] = gamma
            y = y * float(scale[0].double())
            scale = scale.to(DEV)[:1]
        elif o['scale'] == 'chan':
            scale = channel_vector('scale', n, 450 + si)
            y = y * scale.double()
            scale = scale.to(DEV)
        ref_t = None
        if o['ref']:
            r = rounded(torch.randn(y.shape, generator=g), dtype)
            y = y + r.double()
            ref_t = r.to(dtype).to(DEV)
        a = Arena(y.shape, dtype, [0])
        old = rounded(torch.randn(y.shape, generator=g) * 2.0, dtype)        # known values where the call accumulates
        if o['accumulate']:
            y = y + old.double()
            a.fill(0, old.to(dtype))
        refs.append(y)
        arenas.append(a)
        segs.append(k.Seg(n, out0=a.out(0), bias=bias.to(DEV) if o['bias'] else None, scale=scale, ref=ref_t,
                          accumulate=o['accumulate'], final_act=1 if o['scale'] == 'gate' else 0))
    launch(key, cases.ADD, segs)
    for si, (a, ref) in enumerate(zip(arenas, refs)):
        err = max_rel_err(a.out(0), ref)
        print('%s seg%d: %.3e' % (case_id(case), si, err))
        assert err <= TOL_T_OUT[dtype], (si, err)
        assert a.guards_untouched(), si
