"""The attention kernels of csrc/attn.hip (generic) and csrc/attn_mfma.hip (bf16 MFMA), channel_sum and gate_bwd through
the C ABI against float64 references written out from the formulas in the header of attn.hip (no autograd):

    S = scale * Q K^T (keys / values of entry (b + shift) % B2),  P = softmax(S),  O = P V,  lse = logsumexp(S)
    D = rowsum(dO * O_in),  dS = P * (dO V^T - D) * scale,  dQ = dS K,  dK = dS^T Q,  dV = P^T dO  (dK, dV of entry (b + shift) % B2)

Cases, operand layouts and the kernel form each case must reach are tests/attn_cases.py; every case asserts
kernels.attn_form (the launches' own dispatch predicate) before it launches, tests/test_host_logic.py does the same without
a GPU.  Inputs are pre-rounded to the storage dtype.  Every operand has a buffer and a row stride of its own (or the
engine's fused q|k|v / dq|dk|dv layout); outputs, lse and the workspace start as NaN; padding columns, GUARD_ROWS rows in
front and a tail behind every buffer hold a sentinel and must come back bit-identical, inputs must come back unchanged.
(The tail is long enough for any operand's rows walked with any other operand's stride.)

Errors are per batch entry, max_b(max|got_b - ref_b| / max|ref_b|).  Bounds are the project's (o 2e-5 f32 / 6e-3 bf16,
gradients 2e-4 / 2e-2, lse 1e-4 absolute) plus two derived terms for large scores: o and the gradients get
4 * eps_f32 * max|S| (a rounding of S passes through exp as a relative error of P), lse gets 1e-6 * max|lse_ref| (about 8
f32 roundings).

Input families: 'soft' q, k = 2 randn; 'peaked' q, k = gain * randn (gain 5; attn_cases.PEAKED_GAIN for the MFMA head dims,
where the test asserts a median effective key count 1 / sum p^2 between 1.2 and 4 from the reference: 1.3 to 1.6 at 16/128,
2.0 to 2.4 at 32/256, 2.3 to 2.9 at 64/512; gain 3 for the rows with three keys, see attn_cases.py); 'offset+' / 'offset-' = peaked with
channel 0 of q set to c and of k to +-c, c^2 scale = 100, so that every score moves by +-100 and the softmax is unchanged in
exact arithmetic; 'neg-scale' = gain 8 with scale = -1 / sqrt(dv), which must run (correctly) on the generic kernels.

The backward is judged alone: it is fed the reference o rounded to the storage dtype and the reference lse rounded to f32,
never the forward kernel's output (test_attention_chained does that, as the engine does).  The offset families are left out
of the backward: with the offset channel the column sums of the bf16-rounded dS no longer cancel against k[:, 0] = c, and a
float64 CPU model of that rounding alone already puts dq at 1.2e-2 to 2.0e-2 of the 2e-2 bound.

Largest errors measured on an MI355X (unmutated library, all cases pass), per form, dtype and family:

    forward            o         lse       | isolated backward   dq        dk        dv        D (rel. to sum|dO O|)
    generic f32 soft   2.3e-6    3.6e-6    | generic f32 soft    3.3e-6    3.0e-6    2.6e-6    1.2e-7
    generic f32 peaked 4.0e-6    3.2e-5    | generic f32 peaked  1.7e-5    1.1e-5    1.3e-5    1.3e-7
    generic f32 off+   2.0e-5    8.0e-5    | generic bf16 soft   3.5e-3    3.4e-3    3.5e-3    1.0e-7
    generic f32 off-   2.9e-5    8.6e-5    | generic bf16 peaked 3.4e-3    3.6e-3    3.2e-3    7.1e-8
    generic bf16 soft  3.1e-3    2.1e-6    | generic bf16 neg    2.3e-3    2.8e-3    2.4e-3    3.1e-8
    generic bf16 peak. 3.4e-3    1.2e-5    | mfma bf16 soft      5.0e-3    4.5e-3    5.2e-3    3.6e-8
    generic bf16 off+- 2.5e-3    4.5e-5    | mfma bf16 peaked    5.7e-3    4.6e-3    3.7e-3    5.1e-8
    generic bf16 neg   3.6e-3    1.2e-5    | chained             o         dq        dk        dv
    mfma bf16 soft     4.0e-3    9.5e-7    | generic f32 peaked  4.0e-6    3.2e-6    3.9e-6    4.4e-6
    mfma bf16 peaked   3.5e-3    5.0e-6    | mfma bf16 peaked    3.0e-3    4.3e-3    3.8e-3    2.8e-3
    mfma bf16 off+-    2.5e-3    2.1e-5    |
    (the conditioned bounds of the f32 offset cases are 6.8e-5 to 1.2e-4 for o and 1.6e-4 to 3.1e-4 for lse; the flat 2e-5 would
    fail them)        channel_sum f32 5.6e-7, bf16 4.4e-8;  gate_bwd dgamma 8.3e-8 / 1.5e-8, t 3.9e-8 / 2.6e-3

What these tests see that test_attention_fwd_bwd (test_gpu_dcnet_kernels.py: kv_shift = B2 / 2, one fused stride, soft inputs)
cannot.  Each one-line mutation was built into a copy of the library and run on the MI355X; test_attention_fwd_bwd passed all
22 of its cases under every one of them:
  1. qb = (kb + p.shift) % p.B2 in attn_bwd_dkv_mfma_kernel: test_attention_backward_isolated, _mfma_with_poisoned_lds and
     _chained fail on every MFMA row with (B2, shift) = (3, 1) or (3, 2) (dk, dv off by factors of 1e3 and more), 19 cases
  2. the same in attn_bwd_dkv_generic: the isolated backward of every generic row with B2 = 3 or 16 and the chained generic
     row fail, 32 cases
  3. p.ld_dq and p.ld_dk exchanged in adn_attn_mfma_bwd: the isolated, poisoned and chained backward of every MFMA row with
     distinct strides fail (rows land at the other operand's stride, NaN is left in dq / dk), 31 cases; the rows with the
     fused layout, where the two strides are equal, pass
  4. m[t] = 0.f in attn_fwd_mfma_kernel and m = 0.f in attn_fwd_generic: test_attention_forward fails on 'offset-' of all
     three MFMA head dims and of ten generic rows (NaN: every probability underflows), 13 cases
  5. N % 256 in the dispatch predicate: only the form assertions fail -- `assert 'generic' == 'mfma'` in all 74 cases of the MFMA
     rows here and in test_attn_cases_reach_the_forms_they_name on the host; the numbers still agree with float64
"""
import zlib

import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = -7.0                  # exact in bf16
EPS_F32 = 2.0 ** -23
TORCH_DTYPE = {ac.F32: torch.float32, ac.BF16: torch.bfloat16}
TOL_O = {ac.F32: 2e-5, ac.BF16: 6e-3}
TOL_GRAD = {ac.F32: 2e-4, ac.BF16: 2e-2}
_REF = {}                        # (row, family) -> inputs and float64 results; computed once, read-only


def K():
    from audio_depth_estimation_amd import kernels
    return kernels


def rounded(x, dtype):
    return x.to(dtype).double()


def reference(name, family):
    """Inputs (pre-rounded, float64 [B2][N][*]) and the float64 forward and backward of one case, one batch entry at a time."""
    if (name, family) in _REF:
        return _REF[(name, family)]
    row = ac.ROWS[name]
    dtype = TORCH_DTYPE[row['dtype']]
    B2, N, dqk, dv, shift = row['B2'], row['N'], row['dqk'], row['dv'], row['kv_shift']
    scale = ac.scale_of(row, family)
    g = torch.Generator().manual_seed(zlib.crc32(('%s/%s' % (name, family)).encode()))
    gain = {'soft': 2.0, 'neg-scale': ac.NEG_SCALE_GAIN}.get(family, row['gain'])
    q = torch.randn(B2, N, dqk, generator=g, dtype=torch.float64) * gain
    k = torch.randn(B2, N, dqk, generator=g, dtype=torch.float64) * gain
    if family in ('offset+', 'offset-'):
        c = (ac.OFFSET_SCORE / abs(scale)) ** 0.5
        q[:, :, 0] = c
        k[:, :, 0] = c if family == 'offset+' else -c
    q, k = rounded(q, dtype), rounded(k, dtype)
    v = rounded(torch.randn(B2, N, dv, generator=g, dtype=torch.float64), dtype)
    dout = rounded(torch.randn(B2, N, dv, generator=g, dtype=torch.float64), dtype)
    r = dict(q=q, k=k, v=v, dout=dout, scale=scale, o=torch.empty(B2, N, dv, dtype=torch.float64),
             lse=torch.empty(B2, N, dtype=torch.float64), dsum=torch.empty(B2, N, dtype=torch.float64),
             dsum_abs=torch.empty(B2, N, dtype=torch.float64), dq=torch.empty_like(q), dk=torch.empty_like(k),
             dv=torch.empty_like(v))
    smax, eff = 0.0, []
    for b in range(B2):
        kb = (b + shift) % B2
        S = (q[b] @ k[kb].t()) * scale
        m = S.max(-1, keepdim=True).values
        E = torch.exp(S - m)
        P = E / E.sum(-1, keepdim=True)
        r['o'][b] = P @ v[kb]
        r['lse'][b] = m[:, 0] + torch.log(E.sum(-1))
        smax = max(smax, float(S.abs().max()))
        eff.append(1.0 / (P * P).sum(-1))
        # backward from the STORED forward results: o in the storage dtype, lse in f32
        o_in = rounded(r['o'][b], dtype)
        P_in = torch.exp(S - r['lse'][b].float().double()[:, None])
        D = (dout[b] * o_in).sum(-1)
        r['dsum'][b] = D
        r['dsum_abs'][b] = (dout[b] * o_in).abs().sum(-1)
        dS = P_in * (dout[b] @ v[kb].t() - D[:, None]) * scale
        r['dq'][b] = dS @ k[kb]
        r['dk'][kb] = dS.t() @ q[b]
        r['dv'][kb] = P_in.t() @ dout[b]
    r['smax'] = smax
    r['eff_keys'] = float(torch.cat(eff).median())
    r['o_in'] = rounded(r['o'], dtype)
    r['lse_in'] = r['lse'].float()
    _REF[(name, family)] = r
    return r


class Arena:
    """The operands of one case on the device, laid out by attn_cases.layout.  A buffer is [GUARD_ROWS rows | B2 N rows |
    tail], SENTINEL everywhere except in the views; lse and the workspace are f32 [guard | B2 N | guard]."""

    def __init__(self, name):
        row = ac.ROWS[name]
        self.row, self.dtype = row, TORCH_DTYPE[row['dtype']]
        B2, N = row['B2'], row['N']
        rows = B2 * N
        bufs, ops = ac.layout(row)
        reach = (rows + 1) * max(bufs.values())               # any operand's rows walked with any operand's stride
        self.buf = {b: torch.full((2 * ac.GUARD_ROWS * ld + reach,), SENTINEL, dtype=self.dtype, device=DEV)
                    for b, ld in bufs.items()}
        self.where = ac.view_offsets(row)
        self.view, self.given = {}, {}
        for op, (b, off, ld) in self.where.items():
            assert self.buf[b].data_ptr() % 256 == 0
            self.view[op] = torch.as_strided(self.buf[b], (B2, N, ac.width_of(row, op)), (N * ld, ld, 1), off)
        G = ac.GUARD_F32
        self.f32 = {n: torch.full((rows + 2 * G,), SENTINEL, dtype=torch.float32, device=DEV) for n in ('lse', 'ws')}
        self.lse = self.f32['lse'][G:G + rows].view(B2, N)
        self.ws = self.f32['ws'][G:G + rows]
        for t in (self.lse, self.ws):
            t.fill_(float('nan'))

    def give(self, **tensors):
        """Inputs (float64, already rounded) into their views; remembered bit for bit."""
        for op, t in tensors.items():
            dst = self.lse if op == 'lse' else self.view[op]
            dst.copy_(t.to(dst.dtype))
            self.given[op] = dst.clone()

    def poison(self, *ops):
        for op in ops:
            self.view[op].fill_(float('nan'))

    def fwd_args(self, scale):
        v = self.view
        return (v['q'], v['k'], v['v'], v['o'], self.lse, self.row['dqk'], self.row['dv'], self.row['kv_shift'], scale)

    def bwd_args(self, scale):
        v = self.view
        return self.fwd_args(scale) + (v['dout'], v['dq'], v['dk'], v['dv'], self.ws)

    def got(self, op):
        t = {'lse': self.lse, 'ws': self.ws.view(self.row['B2'], self.row['N'])}.get(op)
        return (self.view[op] if t is None else t).detach().cpu().double()

    def assert_untouched(self):
        """Inputs unchanged; with every view blanked, every buffer is SENTINEL bit for bit."""
        for op, t in self.given.items():
            assert torch.equal(self.lse if op == 'lse' else self.view[op], t), 'input %s was modified' % op
        row = self.row
        for b, buf in self.buf.items():
            c = buf.clone()
            for op, (bb, off, ld) in self.where.items():
                if bb == b:
                    torch.as_strided(c, (row['B2'] * row['N'], ac.width_of(row, op)), (ld, 1), off).fill_(SENTINEL)
            assert torch.equal(c, torch.full_like(c, SENTINEL)), 'padding or guard rows of buffer %s were written' % b
        G = ac.GUARD_F32
        for n, buf in self.f32.items():
            assert bool((buf[:G] == SENTINEL).all()) and bool((buf[-G:] == SENTINEL).all()), 'guard of %s was written' % n


def batch_err(got, ref):
    """max over batch entries of max|got_b - ref_b| / max|ref_b|; NaN (an element nobody wrote) stays NaN and fails every bound."""
    errs = []
    for b in range(ref.shape[0]):
        num, den = (got[b] - ref[b]).abs().max(), ref[b].abs().max()
        if float(den) == 0:                        # an all-zero reference entry (one key: dq = dk = 0) must be met exactly
            den = torch.tensor(1.0 if float(num) == 0 else 0.0, dtype=torch.float64)
        errs.append(num / den)
    return float(torch.stack(errs).max())          # (torch's max propagates NaN)


def bounds(row, ref):
    cond = 4 * EPS_F32 * ref['smax']
    return dict(o=TOL_O[row['dtype']] + cond, grad=TOL_GRAD[row['dtype']] + cond,
                lse=1e-4 + 1e-6 * float(ref['lse'].abs().max()))


def report(kind, name, family, form, **errs):
    print('ATTN %s %s %s %s %s' % (kind, form, 'bf16' if ac.ROWS[name]['dtype'] else 'f32', family, name),
          ' '.join('%s=%.3e' % kv for kv in errs.items()))


def check_peaked(name, family, ref):
    """A condition on the INPUTS of the peaked families at the MFMA head dims: the softmax is sharp but not one-hot."""
    row = ac.ROWS[name]
    if family == 'peaked' and (row['dqk'], row['dv']) in ac.PEAKED_GAIN:
        assert 1.2 <= ref['eff_keys'] <= 4.0, ref['eff_keys']


def run_forward(name, family):
    row, ref = ac.ROWS[name], reference(name, family)
    check_peaked(name, family, ref)
    a = Arena(name)
    a.give(q=ref['q'], k=ref['k'], v=ref['v'])
    a.poison('o')
    form = ac.form_of(row, family, False)
    assert K().attn_form(*a.fwd_args(ref['scale'])) == form
    K().attn_fwd(*a.fwd_args(ref['scale']))
    torch.cuda.synchronize()
    eo = batch_err(a.got('o'), ref['o'])
    el = float((a.got('lse') - ref['lse']).abs().max())
    report('fwd', name, family, form, o=eo, lse=el)
    bd = bounds(row, ref)
    assert eo <= bd['o'], (eo, bd['o'])
    assert el <= bd['lse'], (el, bd['lse'])
    a.assert_untouched()


def check_grads(kind, a, name, family, form, ref):
    row = ac.ROWS[name]
    errs = {g: batch_err(a.got(g), ref[g]) for g in ('dq', 'dk', 'dv')}
    # D = rowsum(dO * O_in) in the workspace: f32 products, 16 sequential and 6 tree additions per row
    ed = float(((a.got('ws') - ref['dsum']).abs() / ref['dsum_abs'].clamp_min(1e-300)).max())
    report(kind, name, family, form, dsum=ed, **errs)
    bd = bounds(row, ref)
    for g, e in errs.items():
        assert e <= bd['grad'], (g, e, bd['grad'])
    assert ed <= 24 * EPS_F32 / 2, ed
    a.assert_untouched()


def run_backward(name, family):
    row, ref = ac.ROWS[name], reference(name, family)
    a = Arena(name)
    a.give(q=ref['q'], k=ref['k'], v=ref['v'], dout=ref['dout'], o=ref['o_in'], lse=ref['lse_in'])
    a.poison('dq', 'dk', 'dv')
    form = ac.form_of(row, family, True)
    assert K().attn_form(*a.bwd_args(ref['scale'])) == form
    K().attn_bwd(*a.bwd_args(ref['scale']))
    torch.cuda.synchronize()
    check_grads('bwd', a, name, family, form, ref)


FWD_CASES = [(n, f) for n, r in ac.ROWS.items() for f in r['families']] + [(n, f) for n in ac.OFFSET_ROWS for f in ('offset+', 'offset-')]
BWD_CASES = [(n, f) for n, r in ac.ROWS.items() for f in r['families']]
case_id = lambda c: '%s-%s' % c


@pytest.mark.parametrize('case', FWD_CASES, ids=case_id)
def test_attention_forward(case):
    """o and lse of every row with its families, and of one row per head-dim pair and form with every score moved by +-100
    (a missing max subtraction overflows, a running maximum that starts at 0 underflows)."""
    run_forward(*case)


@pytest.mark.parametrize('case', BWD_CASES, ids=case_id)
def test_attention_backward_isolated(case):
    """dq, dk, dv (and D in the workspace) from the REFERENCE o (rounded to the storage dtype) and lse (rounded to f32), so
    that no forward error can cancel a backward one.  Families soft, peaked and neg-scale; the offset families are left
    out: with the offset channel the column sums of the bf16-rounded dS no longer cancel against k[:, 0] = c, and a float64
    CPU model of that rounding alone puts dq at 1.2e-2 to 2.0e-2 of the 2e-2 bound."""
    run_backward(*case)


@pytest.mark.parametrize('name', ac.CHAINED_ROWS)
def test_attention_chained(name):
    """Forward, then the backward on the kernel's own o and lse, as the engine runs them; one row per form."""
    family = 'peaked'
    row, ref = ac.ROWS[name], reference(name, family)
    a = Arena(name)
    a.give(q=ref['q'], k=ref['k'], v=ref['v'], dout=ref['dout'])
    a.poison('o', 'dq', 'dk', 'dv')
    k = K()
    assert k.attn_form(*a.fwd_args(ref['scale'])) == row['form'][0] and k.attn_form(*a.bwd_args(ref['scale'])) == row['form'][1]
    k.attn_fwd(*a.fwd_args(ref['scale']))
    k.attn_bwd(*a.bwd_args(ref['scale']))
    torch.cuda.synchronize()
    bd = bounds(row, ref)
    errs = {g: batch_err(a.got(g), ref[g]) for g in ('o', 'dq', 'dk', 'dv')}
    report('chained', name, family, row['form'][1], **errs)
    assert errs.pop('o') <= bd['o']
    for g, e in errs.items():
        assert e <= bd['grad'], (g, e, bd['grad'])
    a.assert_untouched()


@pytest.mark.parametrize('name', ac.MFMA_ROWS)
def test_attention_mfma_with_poisoned_lds(name, monkeypatch):
    """The MFMA rows once more with every CU's LDS filled with 0xFFFFFFFF in front of each launch (adn_debug_poison_lds):
    a tile read before its DMA has landed, or a slot nobody staged, is NaN instead of the previous launch's values."""
    from audio_depth_estimation_amd import _lib
    monkeypatch.setattr(_lib, '_POISON', True)
    run_forward(name, 'peaked')
    run_backward(name, 'peaked')


# ---- channel_sum -------------------------------------------------------------------------------------------------------
def guarded(n, dtype=torch.float32):
    """n NaN elements between two guards of SENTINEL: (whole buffer, the view)."""
    G = ac.GUARD_F32
    buf = torch.full((n + 2 * G,), SENTINEL, dtype=dtype, device=DEV)
    buf[G:G + n] = float('nan')
    return buf, buf[G:G + n]


def guards_ok(buf):
    G = ac.GUARD_F32
    return bool((buf[:G] == SENTINEL).all()) and bool((buf[-G:] == SENTINEL).all())


CHANNEL_SUM_CASES = ac.CHANNEL_SUM_VECTOR + ac.CHANNEL_SUM_SCALAR + [ac.CHANNEL_SUM_CAPPED]


@pytest.mark.parametrize('dtype', [ac.F32, ac.BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', CHANNEL_SUM_CASES, ids=lambda c: '%dx%d_ld%d' % c)
def test_channel_sum(case, dtype):
    """Column sums of x [rows][ld] against float64: the 8-channel vector path (one and two 2048-column chunks, 1 to 256 rows
    per pass), the scalar path (C or ld no multiple of 8), and more than 1024 * 256 rows (P capped, empty trailing row
    blocks).  The padding columns hold 8192, out and the workspace start as NaN."""
    rows, C, ld = case
    tdt = TORCH_DTYPE[dtype]
    g = torch.Generator().manual_seed(rows * 4099 + C)
    x = torch.full((rows, ld), 8192.0, dtype=torch.float64)
    x[:, :C] = rounded(torch.randn(rows, C, generator=g, dtype=torch.float64), tdt)
    ref = x[:, :C].sum(0)
    k = K()
    obuf, out = guarded(C)
    wbuf, ws = guarded(k.channel_sum_workspace_bytes(rows, C) // 4)
    xd = x.to(tdt).to(DEV)
    k.channel_sum(xd, rows, C, ld, out, ws)
    torch.cuda.synchronize()
    err = float((out.cpu().double() - ref).abs().max() / ref.abs().max())
    print('CHANNEL_SUM %s %dx%d ld %d: %.3e' % ('bf16' if dtype else 'f32', rows, C, ld, err))
    assert err <= 1e-5, err
    assert guards_ok(obuf) and guards_ok(wbuf)
    assert torch.equal(xd.cpu().double(), x)


# ---- gate_bwd ------------------------------------------------------------------------------------------------------------
GATE_CASES = [('no-bias', 1000, 24), ('no-dbias', 1000, 24), ('no-dw', 1000, 24), ('big',) + ac.GATE_BIG]


@pytest.mark.parametrize('dtype', [ac.F32, ac.BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', GATE_CASES, ids=lambda c: c[0])
def test_gate_bwd(case, dtype):
    """dgamma = sum(t att) + sum_c bias[c] gsum[c], t <- gamma t, dbias = gamma gsum, dw <- gamma dw in float64, with bias,
    dbias or dw (and nw = 0) left out -- the other outputs must still match -- and with more elements than one pass of the
    capped grid covers (1024 blocks * 256 threads * 8).  Bounds: t in dtype <= 2e-5 / 6e-3; the f32 results <= 1e-5 (f32
    products, float64 sums)."""
    variant, rows, C = case
    tdt = TORCH_DTYPE[dtype]
    g = torch.Generator().manual_seed(rows + C + len(variant))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    t, att = rounded(rnd(rows, C), tdt), rounded(rnd(rows, C), tdt)
    gamma, gsum, bias, dw = 0.37, rnd(C).float().double(), rnd(C).float().double(), rnd(C * C).float().double()
    has_bias, has_dbias, has_dw = variant != 'no-bias', variant != 'no-dbias', variant != 'no-dw'
    gamma = float(torch.tensor(gamma).float())
    ref_dgamma = (t * att).sum() + ((bias * gsum).sum() if has_bias else 0.0)
    k = K()
    td = t.to(tdt).to(DEV)
    attd = att.to(tdt).to(DEV)
    gbuf, dgamma = guarded(1)
    bbuf, dbias = guarded(C)
    wbuf, dwd = guarded(C * C)
    dwd.copy_(dw.float())
    ws = torch.full((1024,), float('nan'), dtype=torch.float64, device=DEV)
    k.gate_bwd(td, attd, torch.tensor([gamma, 5.0], device=DEV)[:1], gsum.float().to(DEV), bias.float().to(DEV) if has_bias else None,
               C, dgamma, dbias if has_dbias else None, dwd if has_dw else None, ws)
    torch.cuda.synchronize()
    rel = lambda got, ref: float((got.cpu().double() - ref).abs().max() / ref.abs().max())
    e_g, e_t = rel(dgamma, ref_dgamma.reshape(1)), rel(td, t * gamma)
    print('GATE %s %s: dgamma %.3e t %.3e' % (variant, 'bf16' if dtype else 'f32', e_g, e_t))
    assert e_g <= 1e-5, e_g
    assert e_t <= TOL_O[dtype], e_t
    if has_dbias:
        assert rel(dbias, gsum * gamma) <= 1e-5
    else:
        assert bool(torch.isnan(dbias).all())
    if has_dw:
        assert rel(dwd, dw * gamma) <= 1e-5
    else:
        assert torch.equal(dwd.cpu().double(), dw)
    assert guards_ok(gbuf) and guards_ok(bbuf) and guards_ok(wbuf)
    assert torch.equal(attd.cpu().double(), att)
