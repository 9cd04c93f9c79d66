"""The shapes, cases and exact data of tests/test_gpu_mx8_forms.py, checked on the host: every shape reaches the kernel form
it is named for (adn_conv3x3_mx8_describe: validate() and the plan rule, no launch), validate() refuses what it should with
the message that says why, the exact data meets the conditions the bit-for-bit comparison rests on, and the case list covers
every (form, epilogue) pair and every variant."""
import ctypes as C

import numpy as np
import pytest

import mx8_conv_cases as cases
from oracle import mx8_oracle as mx


def _desc(B=1, H=8, W=16, C0=64, C1=0, N=64, epi=cases.Z_STATS, segs=(64,)):
    """A descriptor validate() accepts (dummy non-null operands: nothing here launches)."""
    from audio_depth_estimation_amd import _lib
    d = _lib.AdnMx8ConvDesc()
    d.B, d.H, d.W, d.C0, d.C1, d.N = B, H, W, C0, C1, N
    d.in0 = d.sc0 = d.w = d.wsc = 16
    d.in1 = d.sc1 = 16 if C1 else None
    d.epi = epi
    for i, c in enumerate(segs):
        d.seg[i].channels = c
        d.seg[i].out0 = d.seg[i].ref = 16
    return d


def _describe(d):
    from audio_depth_estimation_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(128)
    rc = lib.adn_conv3x3_mx8_describe(C.byref(d), buf, len(buf))
    return rc, buf.value.decode(), lib.adn_last_error().decode()


@pytest.mark.parametrize('key', list(cases.SHAPES))
def test_every_shape_reaches_its_form(key):
    from audio_depth_estimation_amd import kernels as K
    s = cases.SHAPES[key]
    N, pix = sum(s['segs']), s['B'] * s['H'] * s['W']
    line = K.conv3x3_mx8_describe(s['B'], s['H'], s['W'], N, s['C0'], s['C1'])
    assert cases.plan_form(line) == s['form'], line
    bm, bn = (int(t) for t in s['form'].split('x'))
    assert cases.plan_tiles(line) == (pix // bm, N // bn), line
    assert K.conv3x3_mx8_num_partials(s['B'], s['H'], s['W'], N, s['C0'], s['C1']) == pix // bm
    assert pix <= 32768 and pix % bm == 0
    # the same answer from a descriptor with both segments and every epilogue: the form depends on the shape alone
    for epi in (cases.Z_STATS, cases.ACT, cases.ADD, cases.BWD):
        rc, text, err = _describe(_desc(s['B'], s['H'], s['W'], s['C0'], s['C1'], N, epi, s['segs']))
        assert rc == 0 and text == line, (epi, text, err)


def test_plan_rule_edges():
    from audio_depth_estimation_amd import kernels as K
    for (B, H, W, C0, C1, N), form in cases.PINS:
        line = K.conv3x3_mx8_describe(B, H, W, N, C0, C1)
        assert cases.plan_form(line) == form, line
        bm = int(form.split('x')[0])
        assert K.conv3x3_mx8_num_partials(B, H, W, N, C0, C1) == B * H * W // bm
    # the table's own edges: c_n256 sits exactly at the tall threshold, b_window exactly at the start of the t128 window
    s = cases.SHAPES['c_n256']
    assert s['B'] * s['H'] * s['W'] // 256 * (sum(s['segs']) // 64) == 512
    s = cases.SHAPES['b_window']
    assert s['B'] * s['H'] * s['W'] // 128 * (sum(s['segs']) // 128) == 256
    s = cases.SHAPES['a_wide']
    assert (s['B'] * s['H'] * s['W'] // 128 * (sum(s['segs']) // 128)) % 8 == 4       # the XCD remap has a remainder


def test_describe_needs_a_buffer():
    from audio_depth_estimation_amd import _lib
    lib = _lib.load()
    assert lib.adn_conv3x3_mx8_describe(C.byref(_desc()), None, 0) == -1
    assert b'adn_conv3x3_mx8_describe: no buffer' in lib.adn_last_error()
    assert lib.adn_conv3x3_mx8_describe(None, C.create_string_buffer(8), 8) == -1
    assert b'null descriptor' in lib.adn_last_error()
    short = C.create_string_buffer(8)                                   # a short buffer is filled, terminated, not overrun
    assert lib.adn_conv3x3_mx8_describe(C.byref(_desc()), short, 8) == 0 and short.value == b'mx bm=1'


def _refusals():
    def bwd(**seg0):
        d = _desc(epi=cases.BWD)
        for k, v in seg0.items():
            setattr(d.seg[0], k, v)
        return d

    act = _desc(epi=cases.ACT)
    act.seg[0].out0 = None
    null_sc1 = _desc(C1=64)
    null_sc1.sc1 = None
    return [
        ('H % 8', _desc(H=12), 'the image must tile by 8 x 16 output pixels (B=1 H=12 W=16)'),
        ('W % 16', _desc(W=24), 'the image must tile by 8 x 16 output pixels (B=1 H=8 W=24)'),
        ('C0 % 64', _desc(C0=96), 'channels must be multiples of 64 (C0=96 C1=0 N=64)'),
        ('C1 % 64', _desc(C1=32), 'channels must be multiples of 64 (C0=64 C1=32 N=64)'),
        ('N % 64', _desc(N=96, segs=(96,)), 'channels must be multiples of 64 (C0=64 C1=0 N=96)'),
        ('segments short of N', _desc(N=128, segs=(64,)), 'segment channels 64+0 != N=128'),
        ('segments past N', _desc(N=128, segs=(64, 128)), 'segment channels 64+128 != N=128'),
        ('segment % 64', _desc(N=128, segs=(96, 32)), 'segment channels 96+32 != N=128'),
        ('BWD without ref', bwd(ref=None), 'seg 0 BWD needs ref'),
        ('BWD partials without z', bwd(partials=16, mean=16, istd=16), 'seg 0 BWD stats need z/mean/istd'),
        ('BWD partials without mean', bwd(partials=16, z=16, istd=16), 'seg 0 BWD stats need z/mean/istd'),
        ('BWD partials without istd', bwd(partials=16, z=16, mean=16), 'seg 0 BWD stats need z/mean/istd'),
        ('ACT without output', act, 'seg 0 has no output'),
        ('RAW', _desc(epi=cases.RAW), 'epilogue 0 not supported'),
        ('FINAL', _desc(epi=cases.FINAL), 'epilogue 4 not supported'),
        ('null scales of source 1', null_sc1, 'null operand'),
    ]


@pytest.mark.parametrize('what,d,message', _refusals(), ids=[r[0] for r in _refusals()])
def test_validate_refuses_with_its_message(what, d, message):
    from audio_depth_estimation_amd import _lib
    rc, text, err = _describe(d)
    assert rc == -1 and text == '', (rc, text)
    assert err.startswith('adn_conv3x3_mx8: ') and message in err, err
    assert _lib.load().adn_conv3x3_mx8_num_partials(C.byref(d)) == -1


def test_validate_accepts_the_neighbours_of_its_refusals():
    """BWD with ref and no partials, BWD with partials and z / mean / istd, ACT with out1 alone, a second source with its
    scales: each is the refused descriptor plus the one operand it lacked."""
    d = _desc(epi=cases.BWD)
    assert _describe(d)[0] == 0
    d.seg[0].partials = d.seg[0].z = d.seg[0].mean = d.seg[0].istd = 16
    assert _describe(d)[0] == 0
    d = _desc(epi=cases.ACT)
    d.seg[0].out0, d.seg[0].out1 = None, 16
    assert _describe(d)[0] == 0
    assert _describe(_desc(C1=64))[0] == 0


@pytest.mark.parametrize('key', list(cases.SHAPES))
def test_exact_data_is_exact(key):
    """The conditions under which an f32 accumulator holds the exact convolution in any order, and under which what the
    kernel is given IS the data: exact in bf16, lossless under MX quantisation (activations, and the weights of both packs),
    everything on the grid, sum of |products| below 2^24 units."""
    x, w = cases.exact_data(key)
    s = cases.SHAPES[key]
    N, Cin = sum(s['segs']), s['C0'] + s['C1']
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x) and not (x32.view(np.uint32) & 0xFFFF).any()     # bf16 holds it
    ux, uw = 2.0 ** cases.X_EXP[0], 2.0 ** cases.W_EXP[0]
    assert np.array_equal(np.rint(x / ux) * ux, x) and np.array_equal(np.rint(w / uw) * uw, w.astype(np.float64))
    assert ux * uw == cases.UNIT
    assert np.abs(x).max() == 7 * 2.0 ** cases.X_EXP[1] and np.abs(w).max() == 7 * 2.0 ** cases.W_EXP[1]
    xs = (x[..., :s['C0']], x[..., s['C0']:]) if s['C1'] else (x,)
    for part in xs:                                                      # each source is quantised on its own
        bits, sc, deq = mx.quantize(part.astype(np.float32))
        assert np.array_equal(deq, part)
        assert len(np.unique(sc)) >= 5                                   # the block scales really differ
    m = w.transpose(0, 2, 3, 1).reshape(N, 9, Cin).astype(np.float64)
    _, wsc, deq = mx.pack_weights(w, False)
    assert np.array_equal(deq, m) and len(np.unique(wsc)) >= 4
    _, _, deq_t = mx.pack_weights(w, True)
    assert np.array_equal(deq_t, m[:, ::-1, :].transpose(2, 1, 0))
    worst = float(mx.conv3x3(np.abs(x), np.abs(m)).max()) / cases.UNIT
    print('%s: max sum|products| = %.3e units (2^%.1f)' % (key, worst, np.log2(worst)))
    assert worst < cases.EXACT_LIMIT
    if s['B'] * s['H'] * s['W'] <= 2304:                                 # and the convolution itself sits on the grid
        v = mx.conv3x3(x, m)
        assert np.array_equal(np.rint(v / cases.UNIT) * cases.UNIT, v)
        assert np.mean(np.abs(v) >= 512 * cases.UNIT) > 0.9       # more than 8 bits above the unit: the bf16 store does round


def test_exact_epilogue_operands_keep_float32_exact():
    rng = cases.rng_for('host')
    for name in ('bias', 'shift'):
        v = cases.exact_vector(rng, name, 256).astype(np.float64)
        assert np.array_equal(np.rint(v / cases.UNIT) * cases.UNIT, v) and len(np.unique(v)) > 100
    for name in ('scale', 'istd'):
        v = np.abs(cases.exact_vector(rng, name, 256).astype(np.float64))
        assert np.array_equal(np.exp2(np.rint(np.log2(v))), v) and len(np.unique(v)) >= 3
    assert (cases.exact_vector(rng, 'scale', 256) < 0).any()
    for relu in (False, True):
        t = cases.grid_tensor(rng, (64, 64), relu)
        t32 = t.astype(np.float32)
        assert not (t32.view(np.uint32) & 0xFFFF).any() and np.array_equal(np.rint(t * 16) / 16, t)     # bf16, on the grid
        assert (t == 0).any() and (t > 0).any() and (relu or (t < 0).any())
    m = cases.exact_vector(rng, 'mean', 64).astype(np.float64)
    assert np.array_equal(np.rint(m * 16) / 16, m)


def test_tile_sums_follow_the_kernel_order():
    t = np.zeros((2, 16, 32, 1))
    t[1, 9, 17, 0] = 1.0
    assert np.flatnonzero(cases.tile_sums(t, 128)[:, 0]).tolist() == [4 + 2 + 1]       # image 1, tile row 1, tile column 1
    assert np.flatnonzero(cases.tile_sums(t, 256)[:, 0]).tolist() == [2 + 1]           # 16 x 16 tiles: image 1, column 1
    assert cases.tile_sums(np.ones((2, 16, 32, 3)), 256).tolist() == [[256.0] * 3] * 4


def test_case_list_covers_every_form_epilogue_and_variant():
    assert 60 <= len(cases.CASES) <= 80 and len(set(cases.CASES)) == len(cases.CASES)
    for data, want_all_variants in (('exact', True), ('gauss', False)):
        rows = [c for c in cases.CASES if c[3] == data]
        pairs = {(cases.SHAPES[k]['form'], e) for k, e, _, _ in rows}
        assert pairs == {(f, e) for f in cases.FORMS for e in cases.VARIANTS}, (data, pairs)
        if want_all_variants:
            for e, table in cases.VARIANTS.items():
                for name, sets in table.items():
                    forms = {cases.SHAPES[k]['form'] for k, ee, n, _ in rows if (ee, n) == (e, name)}
                    assert forms == set(cases.FORMS), (e, name, forms)          # every variant on every form
                    if len(sets) == 2:
                        keys = {k for k, ee, n, _ in rows if (ee, n) == (e, name)}
                        assert keys == set(cases.TWO_SEGMENT_SHAPES), (e, name, keys)
    for key, e, name, _ in cases.CASES:
        cases.per_segment(key, cases.VARIANTS[e][name])                          # a two-set variant sits on a two-segment shape
    assert {k for k, _, _, _ in cases.CASES} == set(cases.SHAPES)
    assert len({cases.case_id(c) for c in cases.CASES}) == len(cases.CASES)
