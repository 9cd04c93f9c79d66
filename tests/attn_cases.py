"""Cases of tests/test_gpu_attention.py: shapes, shifts, operand layouts, input families and the kernel form (csrc/attn.hip
generic, csrc/attn_mfma.hip MFMA) every case has to reach.  Kept free of torch and of the GPU so that tests/test_host_logic.py
reads the same literals and holds adn_attn_form to them (test_attn_cases_reach_the_forms_they_name).

A row is B2, N, dqk, dv, kv_shift, dtype, a stride recipe, the input families it runs with and the pair (forward form,
backward form) for a positive scale; the 'neg-scale' family has a negative scale and is generic whatever the row says.

Stride recipes (operands q k v o dout dq dk dv; GUARD_ROWS sentinel rows in front of and behind every buffer):
  aligned    every operand in a buffer of its own, eight distinct row strides, all multiples of 8 (what the MFMA form needs)
  ragged     the same with eight distinct strides that are no multiple of 8 (mostly odd): generic rows
  fused      the engine's layout: q | k | v are column slices of one buffer of width 2 dqk + dv + 8, dq | dk | dv of another
             of width 2 dqk + dv + 16; o and dout are contiguous
  ldq+4      aligned, but ld_q is 4 more: not a multiple of 8
  k+4        aligned, but the k view starts 4 elements into its rows (8-byte aligned)
  dout+4     aligned, but the dout view starts 4 elements into its rows: only the backward leaves the MFMA form
"""
F32, BF16 = 0, 1
ESIZE = {F32: 4, BF16: 2}
MFMA, GENERIC = 'mfma', 'generic'
OPERANDS = ('q', 'k', 'v', 'o', 'dout', 'dq', 'dk', 'dv')
GUARD_ROWS = 2
GUARD_F32 = 64                  # guard elements around lse and the workspace (keeps them 16-byte aligned)

MFMA_DIMS = ((16, 128), (32, 256), (64, 512))
GENERIC_DIMS = ((1, 1), (2, 16), (3, 5), (63, 65), (64, 64), (65, 576), (128, 1024))
SHIFTS = ((2, 1), (3, 1), (3, 2), (2, 0), (1, 0))          # (B2, kv_shift)

# gain of q and k in the 'peaked' family per MFMA head-dim pair (the score's standard deviation is gain^2 sqrt(dqk / dv) =
# gain^2 / sqrt(8) for all three); everything else takes 5.  test_gpu_attention.py asserts the effective key count they give.
PEAKED_GAIN = {(16, 128): 5.0, (32, 256): 4.0, (64, 512): 3.5}
NEG_SCALE_GAIN = 8.0
OFFSET_SCORE = 100.0            # |shift of every score| in the offset families: c^2 * scale

ROWS = {}


def _row(name, B2, N, dqk, dv, shift, dtype, recipe, form, families=('soft', 'peaked'), gain=None):
    assert name not in ROWS, name
    ROWS[name] = dict(B2=B2, N=N, dqk=dqk, dv=dv, kv_shift=shift, dtype=dtype, recipe=recipe, families=tuple(families),
                      form=(form, form) if isinstance(form, str) else tuple(form),
                      gain=PEAKED_GAIN.get((dqk, dv), 5.0) if gain is None else gain)


# ---- MFMA rows: bf16, the three full-width head-dim pairs, the smallest N of the form and an odd tile count --------------
_row('m16-128-b3s1', 3, 128, 16, 128, 1, BF16, 'aligned', MFMA)
_row('m16-128-b3s2', 3, 128, 16, 128, 2, BF16, 'aligned', MFMA)
_row('m16-384-b2s1', 2, 384, 16, 128, 1, BF16, 'fused', MFMA)
_row('m16-128-b2s0', 2, 128, 16, 128, 0, BF16, 'aligned', MFMA)
_row('m16-384-b1s0', 1, 384, 16, 128, 0, BF16, 'aligned', MFMA)
_row('m32-128-b3s1', 3, 128, 32, 256, 1, BF16, 'aligned', MFMA)
_row('m32-384-b3s2', 3, 384, 32, 256, 2, BF16, 'aligned', MFMA)
_row('m32-128-b2s1', 2, 128, 32, 256, 1, BF16, 'fused', MFMA)
_row('m32-128-b1s0', 1, 128, 32, 256, 0, BF16, 'aligned', MFMA)
_row('m64-64-b3s1', 3, 64, 64, 512, 1, BF16, 'aligned', MFMA)
_row('m64-192-b3s2', 3, 192, 64, 512, 2, BF16, 'aligned', MFMA)
_row('m64-192-b2s1', 2, 192, 64, 512, 1, BF16, 'fused', MFMA)
_row('m64-64-b2s0', 2, 64, 64, 512, 0, BF16, 'aligned', MFMA)
# ---- fallback rows: an MFMA row (m16-128-b3s1) with ONE thing changed, which must reach the generic kernels -----------------
FALLBACK_OF = 'm16-128-b3s1'
_row('f16-192-n', 3, 192, 16, 128, 1, BF16, 'aligned', GENERIC)                 # N % 128 != 0
_row('f16-128-ldq', 3, 128, 16, 128, 1, BF16, 'ldq+4', GENERIC)
_row('f16-128-koff', 3, 128, 16, 128, 1, BF16, 'k+4', GENERIC)
_row('f16-128-dooff', 3, 128, 16, 128, 1, BF16, 'dout+4', (MFMA, GENERIC))
# scale < 0 on every MFMA head-dim pair (the MFMA softmax scales the maximum of the raw scores: positive scales only)
_row('f16-128-neg', 3, 128, 16, 128, 1, BF16, 'aligned', GENERIC, families=('neg-scale',))
_row('f32-128-neg', 3, 128, 32, 256, 1, BF16, 'aligned', GENERIC, families=('neg-scale',))
_row('f64-64-neg', 3, 64, 64, 512, 1, BF16, 'aligned', GENERIC, families=('neg-scale',))
# ---- generic rows, f32 and bf16: N % 4 in {1, 2, 3} (3, 2, 1 dead waves in the last workgroup), both dqk lane slots, dv that
# is no multiple of 64, dqk = dv = 1 and the limits 128 / 1024 ------------------------------------------------------------------
for _dt, _t in ((F32, 'f32'), (BF16, 'bf16')):
    _row('g1-1-%s' % _t, 1, 1, 1, 1, 0, _dt, 'ragged', GENERIC)
    # (three keys: at gain 5 all six softmax rows of the bf16 case are one-hot, dq and dk are 4e-6 and a float32 model of the
    # reference arithmetic alone is 2.4e-1 / 3.1e-1 away from them -- summation order of dP - D; gain 3 keeps them O(1))
    _row('g2-3-%s' % _t, 2, 3, 2, 16, 1, _dt, 'ragged', GENERIC, gain=3.0)
    _row('g3-5-%s' % _t, 3, 5, 3, 5, 1, _dt, 'ragged', GENERIC)
    _row('g63-63-%s' % _t, 3, 63, 63, 65, 2, _dt, 'ragged', GENERIC)
    _row('g64-65-%s' % _t, 2, 65, 64, 64, 0, _dt, 'ragged', GENERIC)
    _row('g65-130-%s' % _t, 2, 130, 65, 576, 1, _dt, 'fused', GENERIC)
    _row('g128-16-%s' % _t, 2, 16, 128, 1024, 1, _dt, 'ragged', GENERIC)
    _row('g128-70-%s' % _t, 3, 70, 128, 1024, 2, _dt, 'ragged', GENERIC)
    _row('g2-130-%s' % _t, 3, 130, 2, 16, 1, _dt, 'ragged', GENERIC)
    # B2 * N = 16480 rows > 4096 workgroups * 4 waves: the stride loop of attn_rowdot
    _row('g2-1030-%s' % _t, 16, 1030, 2, 8, 1, _dt, 'ragged', GENERIC)

MFMA_ROWS = [n for n, r in ROWS.items() if r['form'] == (MFMA, MFMA)]
# one row per head-dim pair and form for the offset families, and the rows of the chained test
OFFSET_ROWS = (['m16-128-b3s1', 'm32-128-b3s1', 'm64-64-b3s1']
               + ['%s-%s' % (n, t) for t in ('f32', 'bf16')
                  for n in ('g1-1', 'g2-3', 'g3-5', 'g63-63', 'g64-65', 'g65-130', 'g128-70')])
CHAINED_ROWS = ('m32-384-b3s2', 'g63-63-f32')


def scale_of(row, family):
    s = 1.0 / float(row['dv']) ** 0.5
    return -s if family == 'neg-scale' else s


def form_of(row, family, bwd):
    return GENERIC if family == 'neg-scale' else row['form'][int(bool(bwd))]


def width_of(row, op):
    return row['dqk'] if op in ('q', 'k', 'dq', 'dk') else row['dv']


def layout(row):
    """-> (buffers {name: row stride}, operands {op: (buffer, first column, row stride)})."""
    dqk, dv, recipe = row['dqk'], row['dv'], row['recipe']
    if recipe == 'fused':
        bufs = {'qkv': 2 * dqk + dv + 8, 'dqkv': 2 * dqk + dv + 16, 'o': dv, 'dout': dv}
        ops = {'q': ('qkv', 0), 'k': ('qkv', dqk), 'v': ('qkv', 2 * dqk), 'o': ('o', 0), 'dout': ('dout', 0),
               'dq': ('dqkv', 0), 'dk': ('dqkv', dqk), 'dv': ('dqkv', 2 * dqk)}
        return bufs, {op: (b, c, bufs[b]) for op, (b, c) in ops.items()}
    step, pad = (2, 1) if recipe == 'ragged' else (8, 8)
    bufs, ops, used = {}, {}, set()
    for op in OPERANDS:
        ld = width_of(row, op) + pad
        while ld in used or (recipe == 'ragged' and ld % 8 == 0):
            ld += step
        pad += step
        if recipe == 'ldq+4' and op == 'q':
            ld += 4
        used.add(ld)
        bufs[op] = ld
        ops[op] = (op, 4 if recipe == op + '+4' else 0, ld)
    return bufs, ops


def view_offsets(row):
    """{op: (buffer, element offset of the view's first element in its buffer, row stride)}: the one place that decides the
    alignment of every operand, read by the GPU test (views) and by the host test (fake pointers)."""
    return {op: (b, GUARD_ROWS * ld + c, ld) for op, (b, c, ld) in layout(row)[1].items()}


# ---- channel_sum and gate_bwd (csrc/attn.hip) ----------------------------------------------------------------------------
# (rows, C, ld): the 8-channel vector path needs C % 8 == 0 and ld % 8 == 0; 2048-column chunks; 256 / (C / 8) rows per pass
CHANNEL_SUM_VECTOR = [(1000, 8, 8), (257, 8, 16), (255, 24, 24), (1000, 24, 32), (257, 1024, 1024), (1, 1024, 1032),
                      (255, 2048, 2048), (257, 2048, 2056), (1, 2056, 2056), (255, 2056, 2064)]
CHANNEL_SUM_SCALAR = [(1000, 5, 5), (257, 257, 260), (255, 8, 12), (1, 5, 5)]
CHANNEL_SUM_CAPPED = (262400, 8, 8)      # cdiv(rows, 256) = 1025 > 1024 row blocks, 257 rows each: the last two are empty
GATE_BIG = (262400, 8)                   # (rows, C): n = 2 099 200 elements > 1024 blocks * 256 threads * 8
