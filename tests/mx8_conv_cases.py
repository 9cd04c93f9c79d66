"""Shapes, epilogue variants, cases and input data of tests/test_gpu_mx8_forms.py: adn_conv3x3_mx8 (csrc/mx8.hip) on each
of its three kernel forms, with each of its four epilogues, over one and two output segments.  Kept free of torch and of the
GPU so that tests/test_mx8_conv_cases.py reads the same literals on the host: it checks every form against
adn_conv3x3_mx8_describe, and the conditions the GPU module's exact comparison rests on against oracle/mx8_oracle.py.

A shape is (B, H, W, C0, C1, output segments) and the form mx8_bn() / mx8_rows() pick for it, 'BMxBN' = output pixels x
output columns per workgroup: '128x128' (8 x 16 pixels, 2 x 2 waves), '128x64', '256x64' (the tall form, 16 x 16 pixels).
Nothing is larger than 32 768 pixels.

Epilogue formulas (include/adn.h, csrc/epilogue.h epi_cols_init / epi_vec8), v = the convolution, n = the channel inside its
segment; every optional operand that is not passed drops out of the formula:
  Z_STATS  z = v + bias[n];  out0 = z;  partials[t][0][n] = sum over the pixels of m-tile t of z, [t][1][n] of z * z
  ACT      y = v * scale[n] + (shift[n] + bias[n]);  out0 = y > 0 ? y : y * slope;  out1 = max(y, 0)
  ADD      out0 = (v + bias[n]) * scale + ref + old out0     (scale per channel; with final_act != 0 ONE device scalar)
  BWD      g = v * (ref > 0 ? 1 : slope) + old out0;  out0 = g;
           partials[t][0][n] = sum g, [t][1][n] = sum g * ((z - mean[n]) * istd[n])
The m-tiles run image by image, then by tile row, then by tile column, BM / 16 x 16 pixels each.
"""
import re
import zlib

import numpy as np

Z_STATS, ACT, BWD, ADD = 1, 2, 3, 5                  # ADN_EPI_* of include/adn.h
RAW, FINAL = 0, 4                                    # the two the fp8 kernel does not carry
EPI_NAME = {Z_STATS: 'z_stats', ACT: 'act', BWD: 'bwd', ADD: 'add'}
FORMS = ('128x128', '128x64', '256x64')


def _shape(B, H, W, C0, C1, segs, form):
    return dict(B=B, H=H, W=W, C0=C0, C1=C1, segs=list(segs), form=form)


SHAPES = {
    'a_one': _shape(1, 8, 16, 64, 0, [128], '128x128'),             # one workgroup, every row on a border
    'a_straddle': _shape(2, 16, 32, 128, 64, [64, 64], '128x128'),  # a tile straddles the segments; two sources, coff = 64
    'a_wide': _shape(3, 8, 32, 64, 0, [128, 128], '128x128'),       # 2 column tiles, 12 workgroups (XCD remap remainder)
    'b_n64': _shape(2, 16, 32, 64, 0, [64], '128x64'),              # H % 16 == 0 but too few tiles for the tall form
    'b_n192': _shape(2, 24, 48, 64, 64, [64, 128], '128x64'),       # H % 16 != 0, 3 column tiles, 54 workgroups
    'b_c128': _shape(1, 8, 16, 128, 0, [64], '128x64'),             # coff = 64 inside one source
    'b_window': _shape(2, 128, 128, 64, 0, [64, 64], '128x64'),     # t128 = 256: 128 columns on 64-column tiles, P = pix/128
    'c_n256': _shape(8, 64, 64, 64, 0, [128, 128], '256x64'),       # tall, 4 column tiles, exactly 512 workgroups
    'c_strip': _shape(32, 16, 64, 64, 64, [64, 192], '256x64'),     # tall, every tile on the top and bottom border
}
# edges of the plan rule that need no launch: (B, H, W, C0, C1, N) -> form
PINS = [
    ((7, 64, 64, 64, 0, 256), '128x64'),              # 448 tiles: below the tall threshold, inside the t128 window
    ((8, 64, 64, 64, 0, 256), '256x64'),
    ((2, 256, 256, 64, 0, 128), '128x128'),           # t128 = 1024: past the window, and 128 columns never go tall
]
TWO_SEGMENT_SHAPES = ('a_straddle', 'b_n192', 'b_window', 'c_n256', 'c_strip')

# One option set per segment; a single set serves both segments of a two-segment shape (each with its own slice of the
# vectors and its own tensors).
Z_VARIANTS = {
    'bias': [dict(bias=True, stats=True)],
    'nobias': [dict(bias=False, stats=True)],
    'seg1_only': [dict(bias=True, stats=False), dict(bias=True, stats=True)],
    'nostats': [dict(bias=True, stats=False)],
}
ACT_VARIANTS = {
    'eval': [dict(p=('scale', 'shift'), slope=0.0, outs='1')],                       # the engine's eval path
    'full': [dict(p=('scale', 'shift', 'bias'), slope=0.25, outs='01')],
    'none': [dict(p=(), slope=0.0, outs='01')],
    'disagree': [dict(p=('scale', 'shift'), slope=0.25, outs='01'), dict(p=('bias',), slope=0.0, outs='1')],
}
ADD_VARIANTS = {
    'plain': [dict(bias=False, scale=None, ref=False, accumulate=False)],
    'acc': [dict(bias=False, scale=None, ref=False, accumulate=True)],
    'mixed': [dict(bias=False, scale=None, ref=False, accumulate=True),              # the engine's: segment 0 accumulates
              dict(bias=False, scale=None, ref=False, accumulate=False)],
    'chan': [dict(bias=True, scale='chan', ref=True, accumulate=False)],
    'gate': [dict(bias=True, scale='gate', ref=True, accumulate=False)],             # final_act = 1, one device scalar
}
BWD_VARIANTS = {
    'stats': [dict(stats=True, slope=0.0, accumulate=False)],
    'acc_stats': [dict(stats=True, slope=0.0, accumulate=True)],                     # the engine's skip case
    'nostats': [dict(stats=False, slope=0.25, accumulate=False)],
    'mixed': [dict(stats=True, slope=0.0, accumulate=False), dict(stats=False, slope=0.0, accumulate=False)],
}
VARIANTS = {Z_STATS: Z_VARIANTS, ACT: ACT_VARIANTS, ADD: ADD_VARIANTS, BWD: BWD_VARIANTS}
TWO_SEGMENT_VARIANTS = [(e, n) for e in (Z_STATS, ACT, ADD, BWD) for n, v in VARIANTS[e].items() if len(v) == 2]

# (shape, epilogue, variant) on the exact data: every single-set variant on every form, the two-segment variants on every
# two-segment shape of TWO_SEGMENT_SHAPES.
EXACT_CASES = [
    ('a_one', Z_STATS, 'bias'), ('b_n64', Z_STATS, 'bias'), ('b_c128', Z_STATS, 'bias'), ('b_window', Z_STATS, 'bias'),
    ('c_n256', Z_STATS, 'bias'),
    ('a_straddle', Z_STATS, 'nobias'), ('a_wide', Z_STATS, 'nobias'), ('b_n192', Z_STATS, 'nobias'), ('c_strip', Z_STATS, 'nobias'),
    ('a_straddle', Z_STATS, 'nostats'), ('b_c128', Z_STATS, 'nostats'), ('c_n256', Z_STATS, 'nostats'),
    ('a_one', ACT, 'eval'), ('a_straddle', ACT, 'eval'), ('b_c128', ACT, 'eval'), ('b_window', ACT, 'eval'), ('c_strip', ACT, 'eval'),
    ('a_wide', ACT, 'full'), ('b_n64', ACT, 'full'), ('b_n192', ACT, 'full'), ('c_n256', ACT, 'full'),
    ('a_one', ACT, 'none'), ('b_n64', ACT, 'none'), ('c_strip', ACT, 'none'),
    ('a_one', ADD, 'plain'), ('b_c128', ADD, 'plain'), ('c_n256', ADD, 'plain'),
    ('a_wide', ADD, 'acc'), ('b_n64', ADD, 'acc'), ('c_strip', ADD, 'acc'),
    ('a_straddle', ADD, 'chan'), ('b_n192', ADD, 'chan'), ('c_n256', ADD, 'chan'),
    ('a_wide', ADD, 'gate'), ('b_window', ADD, 'gate'), ('c_strip', ADD, 'gate'),
    ('a_one', BWD, 'stats'), ('a_wide', BWD, 'stats'), ('b_n64', BWD, 'stats'), ('b_window', BWD, 'stats'), ('c_n256', BWD, 'stats'),
    ('a_straddle', BWD, 'acc_stats'), ('b_n192', BWD, 'acc_stats'), ('b_c128', BWD, 'acc_stats'), ('c_strip', BWD, 'acc_stats'),
    ('a_wide', BWD, 'nostats'), ('b_c128', BWD, 'nostats'), ('c_n256', BWD, 'nostats'),
] + [(key, e, n) for e, n in TWO_SEGMENT_VARIANTS for key in TWO_SEGMENT_SHAPES]
# on the Gaussian data: one case per (form, epilogue), on three shapes so that three references serve them all
GAUSS_CASES = [(key, e, n) for key in ('a_straddle', 'b_n192', 'c_strip')
               for e, n in ((Z_STATS, 'seg1_only'), (ACT, 'full'), (ADD, 'mixed'), (BWD, 'acc_stats'))]
CASES = [c + ('exact',) for c in EXACT_CASES] + [c + ('gauss',) for c in GAUSS_CASES]


def case_id(c):
    return '%s-%s-%s-%s' % (c[0], EPI_NAME[c[1]], c[2], c[3])


def plan_form(line):
    """'mx bm=128 bn=64 tiles_m=256 tiles_n=2' (adn_conv3x3_mx8_describe) -> '128x64'."""
    m = re.match(r'mx bm=(\d+) bn=(\d+) tiles_m=(\d+) tiles_n=(\d+)$', line)
    return '%dx%d' % (int(m.group(1)), int(m.group(2)))


def plan_tiles(line):
    """-> (tiles_m, tiles_n) of the same line."""
    m = re.match(r'mx bm=(\d+) bn=(\d+) tiles_m=(\d+) tiles_n=(\d+)$', line)
    return int(m.group(3)), int(m.group(4))


def per_segment(key, variant):
    segs = SHAPES[key]['segs']
    assert len(variant) in (1, len(segs)), 'a two-segment variant needs a two-segment shape'
    return [variant[i if len(variant) > 1 else 0] for i in range(len(segs))]


def segment_slices(key):
    lo = 0
    for ch in SHAPES[key]['segs']:
        yield lo, lo + ch
        lo += ch


def rng_for(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


# ---- exact data -----------------------------------------------------------------------------------------------------------
# Activations: integers in [-7, 7] times 2^e, e per (pixel, 32-channel block) from X_EXP; weights: integers in [-7, 7] times
# 2^e, e per (output channel, 32-input-channel block) from W_EXP.  Such data is exact in bf16 and in MX e4m3 (3 mantissa bits
# hold 7; a block's elements span at most 7 * 2^4 against its scale), every product and every partial sum is an integer
# multiple of UNIT = 2^-8, and the sum of |products| of one output stays below 2^24 units (tests/test_mx8_conv_cases.py
# asserts all of it): an f32 accumulator holds the exact convolution whatever the order of its additions.
X_EXP = (-2, 2)
W_EXP = (-6, -3)
UNIT = 2.0 ** (X_EXP[0] + W_EXP[0])
EXACT_LIMIT = 2.0 ** 24                              # units


def exact_data(key):
    """(x float64 [B][H][W][C0 + C1], w float32 [N][C0 + C1][3][3]) of a shape."""
    s = SHAPES[key]
    B, H, W, Cin, N = s['B'], s['H'], s['W'], s['C0'] + s['C1'], sum(s['segs'])
    rng = rng_for('exact', key)
    xe = rng.integers(X_EXP[0], X_EXP[1] + 1, (B, H, W, Cin // 32, 1))
    x = rng.integers(-7, 8, (B, H, W, Cin // 32, 32)) * np.exp2(xe)
    we = rng.integers(W_EXP[0], W_EXP[1] + 1, (N, Cin // 32, 1, 1, 1))
    w = rng.integers(-7, 8, (N, Cin // 32, 32, 3, 3)) * np.exp2(we)
    return x.reshape(B, H, W, Cin), w.reshape(N, Cin, 3, 3).astype(np.float32)


def gauss_data(key):
    """Gaussian operands whose block scales spread over binades (as tests/test_gpu_mx8.py builds them); x is float64 and
    still to be rounded to bf16."""
    s = SHAPES[key]
    B, H, W, Cin, N = s['B'], s['H'], s['W'], s['C0'] + s['C1'], sum(s['segs'])
    rng = rng_for('gauss', key)
    x = rng.standard_normal((B, H, W, Cin)) * np.exp2(rng.integers(-3, 4, (B, H, W, 1)))
    w = (rng.standard_normal((N, Cin, 3, 3)) * 0.05 * np.exp2(rng.integers(-2, 3, (N, 1, 1, 1)))).astype(np.float32)
    return x, w


def grid_tensor(rng, shape, relu=False):
    """A bf16-exact tensor on the exact grid: integers in [-100, 100] times 2^-4 (old out0, ref, z of the exact cases)."""
    t = rng.integers(-100, 101, shape).astype(np.float64)
    return (np.maximum(t, 0.0) if relu else t) * 2.0 ** -4


def exact_vector(rng, name, n):
    """Per-channel f32 operands that keep f32 exact on the exact data: bias / shift / mean integer multiples of the unit
    resp. of 2^-4, scales and istd +-2^k."""
    if name in ('bias', 'shift'):
        return (rng.integers(-512, 513, n) * UNIT).astype(np.float32)
    if name == 'mean':
        return (rng.integers(-32, 33, n) * 2.0 ** -4).astype(np.float32)
    if name == 'istd':
        return np.exp2(rng.integers(-1, 2, n)).astype(np.float32)
    assert name == 'scale'
    return (rng.choice([-1.0, 1.0], n) * np.exp2(rng.integers(-2, 2, n))).astype(np.float32)


def gauss_vector(rng, name, n):
    if name == 'scale':
        return (rng.choice([-1.0, 1.0], n) * (0.5 + rng.random(n))).astype(np.float32)
    if name == 'istd':
        return (1.0 + rng.random(n)).astype(np.float32)
    return rng.standard_normal(n).astype(np.float32)


def tile_sums(t, bm):
    """t float64 [B][H][W][n] -> [P][n]: the sum over the pixels of every m-tile, tiles in the kernel's order."""
    B, H, W, n = t.shape
    th = bm // 16
    return t.reshape(B, H // th, th, W // 16, 16, n).sum(axis=(2, 4)).reshape(-1, n)


SUM_BOUND = 256 * 2.0 ** -24         # an f32 sum of n <= 256 terms is within n * 2^-24 * sum|terms| of the exact sum
