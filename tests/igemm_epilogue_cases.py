"""Shapes and cases of tests/test_gpu_igemm_epilogues.py: the ACT, FINAL and ADD epilogues of adn_igemm on every kernel form
that can carry them.  Kept free of torch and of the GPU so that the host tests read the same literals:
test_gpu_kernels.igemm_launches() / IGEMM_FORMS take the S2 / T2 launches (tests/golden/igemm_plans.json pins their plans),
tests/test_host_logic.py checks the S1 ones against adn_igemm_describe.

A shape is (dtype, geometry, ks, B, Hs, Ws, C0, C1, output segments) and the kernel form the planner picks for it with a
non-ring epilogue, in the words of IGEMM_FORMS: 'direct', 'tile BMxBN', 'tile BMxBN split' (split-K + reduce kernel),
'patch BMxBN', 'patch-tall 256x64', 'patch-pair 128x128'.  Split-K and direct run the scalar epilogue (epi_scalar in the
reduce kernel); unsplit tiles and the patch kernels run the 8-channel vector epilogue (tile_epi_finish).  Nothing is larger
than 16 x 64 x 64 small-grid pixels.
"""
import re

F32, BF16 = 0, 1
S2, T2, S1 = 0, 1, 2
ACT, FINAL, ADD = 2, 4, 5
EPI_TAG = {ACT: 'epi_act', FINAL: 'epi_final', ADD: 'epi_add'}


def _shape(dtype, geom, B, Hs, Ws, C0, C1, segs, form, ks=0):
    return dict(dtype=dtype, geom=geom, ks=ks, B=B, Hs=Hs, Ws=Ws, C0=C0, C1=C1, segs=list(segs), form=form)


SHAPES = {
    # ---- bf16 ----
    'direct_s2': _shape(BF16, S2, 2, 4, 4, 6, 0, [10], 'direct'),
    'direct_t2_n1': _shape(BF16, T2, 1, 5, 5, 3, 5, [1], 'direct'),                 # Cout = 1, two sources, odd size
    'direct_s1': _shape(BF16, S1, 2, 5, 5, 6, 0, [10], 'direct', ks=3),
    'split_s2': _shape(BF16, S2, 2, 16, 16, 64, 0, [64, 64], 'tile 128x128 split'),     # nsplit 8, one tile holds both segments
    'split_t2': _shape(BF16, T2, 2, 16, 16, 64, 0, [64, 64], 'tile 128x64 split'),
    'split_t2_n64': _shape(BF16, T2, 2, 16, 16, 64, 64, [64], 'tile 128x64 split'),
    'split_s1': _shape(BF16, S1, 2, 16, 16, 64, 0, [64, 64], 'tile 128x128 split', ks=3),
    'split_s1_npow2': _shape(BF16, S1, 2, 6, 10, 64, 0, [128], 'tile 128x128 split', ks=3),   # one tile, mostly beyond M
    'narrow_s1': _shape(BF16, S1, 2, 16, 16, 8, 0, [64], 'tile 128x64', ks=3),          # narrow loader, unsplit
    'onepx_t2': _shape(BF16, T2, 32, 1, 1, 128, 0, [128], 'tile 128x64'),               # one-pixel form, unsplit, M = 32 of 128 rows
    'onepx_s2': _shape(BF16, S2, 32, 1, 1, 128, 0, [128], 'tile 128x128 split'),
    'k1_n192': _shape(BF16, S1, 2, 16, 16, 64, 0, [192], 'tile 128x64', ks=1),          # one K-step, three column tiles
    'k1_gate': _shape(BF16, S1, 8, 32, 32, 64, 0, [128], 'tile 128x128', ks=1),         # the attention block's out projection
    'k1_2k': _shape(BF16, S1, 8, 32, 32, 128, 0, [64], 'tile 128x64', ks=1),
    'k1_bm256': _shape(BF16, S1, 16, 64, 64, 64, 0, [64], 'tile 256x64', ks=1),
    'patch_s2_bn64': _shape(BF16, S2, 8, 64, 64, 64, 0, [64, 64], 'patch 128x64'),
    'patch_s2_bn128': _shape(BF16, S2, 16, 64, 64, 64, 0, [64, 64], 'patch 128x128'),   # a tile straddles the two segments
    'patch_t2': _shape(BF16, T2, 8, 32, 32, 64, 64, [64, 64], 'patch 128x64'),
    'tall_t2': _shape(BF16, T2, 8, 64, 64, 64, 0, [64], 'patch-tall 256x64'),
    'tall_t2_two_src': _shape(BF16, T2, 8, 64, 64, 64, 64, [64], 'patch-tall 256x64'),
    'pair_t2': _shape(BF16, T2, 32, 8, 8, 128, 0, [128, 128], 'patch-pair 128x128'),
    'patch_s1': _shape(BF16, S1, 8, 64, 64, 64, 64, [64], 'patch 128x64', ks=3),
    'tall_s1': _shape(BF16, S1, 16, 64, 64, 64, 0, [64, 64], 'patch-tall 256x64', ks=3),
    'patch_s1_bn128': _shape(BF16, S1, 256, 8, 16, 64, 0, [128, 128], 'patch 128x128', ks=3),
    # ---- f32: the tile kernel or the direct path ----
    'f32_direct_s2': _shape(F32, S2, 2, 4, 4, 6, 0, [10], 'direct'),
    'f32_direct_t2_n1': _shape(F32, T2, 1, 5, 5, 3, 5, [1], 'direct'),
    'f32_direct_s1': _shape(F32, S1, 2, 5, 5, 6, 0, [10], 'direct', ks=3),
    'f32_split_s2': _shape(F32, S2, 2, 16, 16, 64, 0, [64, 64], 'tile 128x128 split'),
    'f32_split_t2': _shape(F32, T2, 2, 16, 16, 64, 0, [128], 'tile 128x128 split'),
    'f32_split_s1': _shape(F32, S1, 2, 16, 16, 64, 0, [64, 64], 'tile 128x128 split', ks=3),
    'f32_tile_s2': _shape(F32, S2, 8, 64, 64, 64, 0, [64, 64], 'tile 128x128'),
    'f32_tile_s2_bm256': _shape(F32, S2, 16, 64, 64, 64, 0, [64, 64], 'tile 256x128'),
    'f32_tile_t2_bm256': _shape(F32, T2, 16, 32, 32, 64, 64, [64], 'tile 256x64'),
    'f32_k1': _shape(F32, S1, 2, 16, 16, 64, 0, [64, 64], 'tile 128x128', ks=1),
}

# ---- ACT: y = v * scale[n] + shift[n] + bias[n]; out0 = leaky(y, slope), out1 = relu(y).  One option set per segment (a
# single set serves both segments of a two-segment shape, each with its own slice of the vectors and its own tensors):
# p = the per-channel vectors that are given, outs = which outputs are passed.
ACT_VARIANTS = {
    'full': [dict(p=('scale', 'shift', 'bias'), slope=0.2, outs='01')],
    'scale': [dict(p=('scale',), slope=1.0, outs='0')],
    'bias': [dict(p=('bias',), slope=0.2, outs='1')],
    'none': [dict(p=(), slope=0.0, outs='01')],
    'qkv': [dict(p=('bias',), slope=1.0, outs='0')],                    # the fused q|k|v projection: linear + bias
    'disagree': [dict(p=('scale', 'shift'), slope=0.2, outs='01'), dict(p=('bias',), slope=0.2, outs='1')],
    'slopes': [dict(p=('scale', 'shift'), slope=0.2, outs='0'), dict(p=('bias',), slope=0.0, outs='01')],
}
ACT_CASES = [
    ('direct_s2', 'full'), ('direct_s2', 'scale'), ('direct_s2', 'bias'), ('direct_s2', 'none'),
    ('direct_s1', 'full'), ('f32_direct_s2', 'full'), ('f32_direct_s2', 'scale'), ('f32_direct_s1', 'bias'),
    ('split_s2', 'full'), ('split_s2', 'scale'), ('split_s2', 'bias'), ('split_s2', 'none'), ('split_s2', 'disagree'),
    ('split_s2', 'slopes'), ('split_t2', 'full'), ('split_t2', 'disagree'), ('split_s1', 'full'), ('split_s1', 'slopes'),
    ('split_s1_npow2', 'full'), ('onepx_s2', 'full'),
    ('f32_split_s2', 'full'), ('f32_split_s2', 'disagree'), ('f32_split_s2', 'slopes'), ('f32_split_s1', 'scale'),
    ('narrow_s1', 'full'), ('narrow_s1', 'bias'), ('onepx_t2', 'full'), ('onepx_t2', 'scale'),
    ('k1_n192', 'qkv'), ('k1_n192', 'full'), ('k1_2k', 'qkv'), ('k1_bm256', 'full'),
    ('patch_s2_bn64', 'full'), ('patch_s2_bn64', 'scale'), ('patch_s2_bn64', 'disagree'),
    ('patch_s2_bn128', 'full'), ('patch_s2_bn128', 'bias'), ('patch_s2_bn128', 'none'), ('patch_s2_bn128', 'disagree'),
    ('patch_s2_bn128', 'slopes'),
    ('patch_t2', 'full'), ('patch_t2', 'slopes'), ('tall_t2', 'full'), ('tall_t2', 'scale'), ('tall_t2_two_src', 'bias'),
    ('pair_t2', 'full'), ('pair_t2', 'disagree'), ('patch_s1', 'full'), ('patch_s1', 'scale'),
    ('tall_s1', 'disagree'), ('patch_s1_bn128', 'slopes'),
    ('f32_tile_s2', 'full'), ('f32_tile_s2', 'disagree'), ('f32_tile_s2', 'slopes'), ('f32_tile_s2', 'scale'),
    ('f32_tile_s2_bm256', 'full'), ('f32_tile_s2_bm256', 'bias'), ('f32_tile_t2_bm256', 'full'), ('f32_tile_t2_bm256', 'none'),
    ('f32_k1', 'disagree'),
]

# ---- FINAL: out0 (f32) = final_act(v + bias[n]); variant = (final_act, bias given) ----
_FINAL_ALL = [(0, True), (1, True), (2, True), (0, False), (1, False), (2, False)]
_FINAL_SOME = [(0, True), (1, True), (2, True), (1, False)]
FINAL_CASES = (
    [('direct_t2_n1', v) for v in _FINAL_ALL] + [('direct_s2', v) for v in _FINAL_SOME] +
    [('f32_direct_t2_n1', v) for v in _FINAL_SOME] +
    [('split_t2_n64', v) for v in _FINAL_ALL] + [('split_s2', v) for v in _FINAL_SOME] +
    [('f32_split_t2', v) for v in _FINAL_SOME] +
    [('onepx_t2', v) for v in _FINAL_SOME] + [('f32_tile_t2_bm256', v) for v in _FINAL_ALL] +
    [('f32_tile_s2', v) for v in _FINAL_SOME] +
    [('tall_t2_two_src', v) for v in _FINAL_ALL] + [('tall_t2', v) for v in _FINAL_SOME] +
    [('patch_t2', v) for v in _FINAL_SOME] + [('patch_s2_bn128', v) for v in _FINAL_SOME])

# ---- ADD: out0 = (v + bias[n]) * scale + ref + old out0.  gate: final_act = 1, scale is ONE device scalar ----
ADD_VARIANTS = {
    'gate': [dict(bias=True, scale='gate', ref=True, accumulate=False)],          # x + gamma * (proj(att) + bias)
    'chan': [dict(bias=True, scale='chan', ref=False, accumulate=False)],
    'acc': [dict(bias=False, scale=None, ref=True, accumulate=True)],
    'mixed': [dict(bias=False, scale=None, ref=True, accumulate=True), dict(bias=False, scale=None, ref=False, accumulate=False)],
    'gate_chan': [dict(bias=True, scale='gate', ref=True, accumulate=False), dict(bias=True, scale='chan', ref=False, accumulate=True)],
}
ADD_CASES = [
    ('direct_s2', 'gate'), ('direct_s2', 'chan'), ('direct_s2', 'acc'), ('direct_s1', 'gate'), ('f32_direct_s1', 'gate'),
    ('f32_direct_s1', 'chan'), ('f32_direct_s2', 'acc'),
    ('split_s1', 'gate'), ('split_s1', 'chan'), ('split_s1', 'acc'), ('split_s1', 'mixed'), ('split_s1', 'gate_chan'),
    ('split_s2', 'gate'), ('split_s2', 'mixed'), ('split_t2', 'chan'), ('split_s1_npow2', 'gate'),
    ('f32_split_s1', 'gate'), ('f32_split_s1', 'mixed'), ('f32_split_s2', 'chan'), ('f32_split_t2', 'acc'),
    ('k1_gate', 'gate'), ('k1_gate', 'chan'), ('k1_gate', 'acc'), ('k1_n192', 'gate'), ('k1_n192', 'chan'),
    ('k1_2k', 'gate'), ('k1_2k', 'acc'), ('k1_bm256', 'gate'), ('k1_bm256', 'chan'), ('narrow_s1', 'acc'),
    ('onepx_t2', 'gate'),
    ('f32_k1', 'gate'), ('f32_k1', 'mixed'), ('f32_k1', 'gate_chan'), ('f32_tile_s2', 'chan'), ('f32_tile_t2_bm256', 'gate'),
    ('f32_tile_t2_bm256', 'acc'),
    ('patch_s1', 'gate'), ('patch_s1', 'chan'), ('patch_s1', 'acc'), ('patch_s2_bn64', 'mixed'), ('patch_s2_bn128', 'mixed'),
    ('patch_s2_bn128', 'gate_chan'), ('patch_t2', 'gate'), ('patch_t2', 'mixed'), ('tall_t2', 'chan'), ('pair_t2', 'mixed'),
]

CASES = {ACT: ACT_CASES, FINAL: FINAL_CASES, ADD: ADD_CASES}


def plan_form(plan):
    """'patch bm=128 bn=64 nsplit=1 ...' (adn_igemm_describe) -> 'patch 128x64'; direct: 'direct'; split-K: '... split'."""
    m = re.match(r'(\S+) bm=(\d+) bn=(\d+) nsplit=(\d+) ', plan)
    kind, bm, bn, ns = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
    return 'direct' if kind == 'direct' else '%s %dx%d%s' % (kind, bm, bn, ' split' if ns > 1 else '')


def launch_rows(s1):
    """One row per (epilogue, shape) that the module launches, in the form of tools/igemm_plan_table.py, with the expected
    form beside it.  s1 = False: the S2 / T2 launches (names as test_gpu_kernels.igemm_launches() builds them); True: the S1
    ones."""
    rows, seen = [], set()
    for epi in (ACT, FINAL, ADD):
        for key, _ in CASES[epi]:
            s = SHAPES[key]
            if (epi, key) in seen or (s['geom'] == S1) != s1:
                continue
            seen.add((epi, key))
            geom = 'S1k%d' % s['ks'] if s1 else 'ST'[s['geom']] + '2'
            shape = '%dx%dx%d_%d+%d_%d' % (s['B'], s['Hs'], s['Ws'], s['C0'], s['C1'], sum(s['segs']))
            name = '%s/%s/%s/%s' % (EPI_TAG[epi], geom, shape, 'bf16' if s['dtype'] else 'f32')
            rows.append(dict(name=name, dtype=s['dtype'], geom=s['geom'], B=s['B'], Hs=s['Hs'], Ws=s['Ws'], C0=s['C0'],
                             C1=s['C1'], N=sum(s['segs']), epi=epi, segs=list(s['segs']), ks=s['ks'], form=s['form']))
    names = [r['name'] for r in rows]
    assert len(set(names)) == len(names), 'two shapes of one epilogue share a descriptor'
    return rows
