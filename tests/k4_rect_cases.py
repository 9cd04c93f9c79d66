"""Shapes and cases of tests/test_gpu_k4_rect.py: the 4x4 stride-2 pair ("k4": the S2 / T2 geometries of adn_igemm and the k4
weight gradient) on rectangular and non-power-of-two small grids.  Kept free of torch and of the GPU so that
tests/test_host_logic.py reads the same literals and checks them against adn_igemm_describe and the weight-gradient plan
queries (test_k4_rect_cases_reach_the_forms_they_name).

The planner's tiling rules are not symmetric in Hs and Ws (patch: Hs % 8 == 0 and Ws % 16 == 0; ring and patch-tall: 16 on
both sides; patch-staged wgrad: 8 on both sides), so every rectangular grid appears as Hs x Ws AND as Ws x Hs, with the same
channels, and each orientation names its own form.  Nothing is larger than 16 x 56 x 40 small-grid pixels or 64 on a side.

An igemm case is (dtype, geometry, B, Hs, Ws, channel set) and the kernel form the planner picks for the RAW, the Z_STATS
and the BWD epilogue, in the words of test_gpu_kernels.IGEMM_FORMS ('direct', 'tile BMxBN', 'tile BMxBN split', 'patch BMxBN',
'patch-tall 256x64', 'ring BMxBN'); None = this epilogue is not launched on this shape.  A and C are each other's input
gradient (the forward of 64 -> 128 is the dgrad of 128 -> 64), so a forward case of one is the dgrad case of the other.

A weight-gradient case is (dtype, B, Hs, Ws, R0 + R1 plain channels, C0 + C1 gathered channels), the route it takes and
what adn_wgrad_workspace_bytes, adn_wgrad_sq_count and adn_wgrad_batchable answer for it.
"""
F32, BF16 = 0, 1
S2, T2 = 0, 1
RAW, Z_STATS, BWD = 0, 1, 3
EPIS = (RAW, Z_STATS, BWD)

# channel sets: C0 + C1 gathered channels -> output segments
SETS = {
    'A': (64, 0, [128]),
    'B': (64, 64, [64]),                # two gathered sources (virtual concat)
    'C': (128, 0, [64]),
    'D': (128, 0, [128, 128]),          # two output segments, one 128-column tile each (or both in one 256-row tile's N)
    'E': (128, 0, [128]),
    'A2': (64, 0, [64, 64]),            # two segments inside one 128-column tile
    'B2': (64, 64, [32, 32]),           # B's 64 channels in two segments: 32-channel segments only run the direct path
    'X': (6, 0, [10]),                  # direct path
    'Y': (3, 5, [1]),                   # direct path, two sources, one output channel
}

SPLIT128, SPLIT64 = 'tile 128x128 split', 'tile 128x64 split'
T128x128, T128x64, T256x64, T256x128 = 'tile 128x128', 'tile 128x64', 'tile 256x64', 'tile 256x128'
P64, P128, TALL = 'patch 128x64', 'patch 128x128', 'patch-tall 256x64'
R64, R128 = 'ring 256x64', 'ring 256x128'
DIRECT = 'direct'

IGEMM = {}


def _forms(f):
    """One form for all three epilogues, or (RAW, Z_STATS, BWD); None = the shape is not launched in this geometry."""
    if f is None:
        return None
    return dict(zip(EPIS, (f, f, f) if isinstance(f, str) else f))


def _pair(dtype, B, Hs, Ws, cset, s2, t2, s2_t=None, t2_t=None):
    """Hs x Ws with forms (s2, t2) and its transpose Ws x Hs with forms (s2_t, t2_t; default: the same)."""
    for h, w, f in ((Hs, Ws, (s2, t2)), (Ws, Hs, (s2 if s2_t is None else s2_t, t2 if t2_t is None else t2_t))):
        for geom in (S2, T2):
            forms = _forms(f[geom])
            if forms is None:
                continue
            C0, C1, segs = SETS[cset]
            key = '%s/%s/%dx%dx%d/%s' % ('bf16' if dtype else 'f32', 'ST'[geom] + '2', B, h, w, cset)
            assert key not in IGEMM, key
            IGEMM[key] = dict(dtype=dtype, geom=geom, B=B, Hs=h, Ws=w, cset=cset, C0=C0, C1=C1, segs=list(segs), forms=forms)


# ---- bf16: small grids, split-K + reduce (the tile kernel's pixel decode: power of two / not) ----
_pair(BF16, 2, 8, 16, 'A', SPLIT128, SPLIT64)
_pair(BF16, 2, 8, 16, 'B', SPLIT64, SPLIT64)
_pair(BF16, 2, 8, 16, 'A2', (None, None, SPLIT128), None)           # BWD, two segments behind the reduce kernel
_pair(BF16, 2, 6, 10, 'A', SPLIT128, SPLIT64)
_pair(BF16, 2, 6, 10, 'B', SPLIT64, SPLIT64)
_pair(BF16, 2, 6, 10, 'D', (None, None, SPLIT128), (None, None, SPLIT64))
_pair(BF16, 3, 2, 4, 'E', SPLIT128, SPLIT64)                        # one tile, mostly beyond M
_pair(BF16, 32, 1, 2, 'A', SPLIT128, SPLIT64)                       # innermost level of a 1:2 image: NOT the one-pixel form
_pair(BF16, 32, 1, 2, 'E', SPLIT128, SPLIT64)
_pair(BF16, 32, 1, 3, 'E', SPLIT128, SPLIT64)                       # innermost level of a 1:3 image
# ---- direct path ----
_pair(BF16, 2, 3, 5, 'X', DIRECT, DIRECT)
_pair(BF16, 1, 5, 4, 'Y', DIRECT, DIRECT)
_pair(BF16, 2, 2, 4, 'X', DIRECT, DIRECT)                           # a power-of-two rectangle
_pair(BF16, 2, 6, 10, 'B2', (None, None, DIRECT), (None, None, DIRECT))     # two segments on the direct path
# ---- T2 plans unsplit from fewer pixels than S2: one patch tile per 8 x 16 image; 16 x 8 cannot be patch-tiled ----
_pair(BF16, 32, 8, 16, 'A', SPLIT128, P64, SPLIT128, T128x64)
_pair(BF16, 8, 24, 48, 'A', SPLIT128, P64, SPLIT128, T128x64)
_pair(BF16, 8, 24, 48, 'B', None, P64, None, T128x64)
_pair(BF16, 8, 24, 48, 'C', SPLIT64, P64, SPLIT64, T128x64)
# ---- S2 plans unsplit from 32768 pixels: 16 x 16-tileable images (patch / patch-tall for RAW, ring for Z_STATS and BWD) ----
_pair(BF16, 16, 32, 64, 'A', (P64, R64, R64), TALL)
_pair(BF16, 16, 32, 64, 'B', None, (TALL, R64, R64))
_pair(BF16, 16, 32, 64, 'C', (None, R64, R64), (None, R64, R64))
_pair(BF16, 16, 32, 64, 'D', (P128, R128, R128), (TALL, R128, R128))
_pair(BF16, 11, 48, 64, 'A', (P64, R64, R64), TALL)                 # 33792 pixels, not a power of two
_pair(BF16, 11, 48, 64, 'B', None, (TALL, R64, R64))
_pair(BF16, 11, 48, 64, 'D', (P128, R128, R128), (None, R128, R128))
# ---- 8 x 16-tileable but not 16 x 16: the patch kernel carries Z_STATS and BWD itself; the transposes run unsplit tiles ----
_pair(BF16, 64, 8, 64, 'A', P64, P64, T128x64, T128x64)
_pair(BF16, 64, 8, 64, 'C', None, P64, None, T256x64)
_pair(BF16, 64, 8, 64, 'D', P128, None, T256x128, None)
_pair(BF16, 13, 40, 64, 'A', P64, P64, T128x64, T128x64)            # 33280 pixels, not a power of two
_pair(BF16, 13, 40, 64, 'D', P128, None, T256x128, None)
# ---- not tileable by any patch: the unsplit tile kernel at bf16 ----
_pair(BF16, 16, 40, 56, 'A', T128x64, T128x64)
_pair(BF16, 16, 40, 56, 'C', T128x64, T256x64)
_pair(BF16, 16, 40, 56, 'D', T256x128, (None, None, T128x64))

# ---- f32: the tile kernel or the direct path ----
_pair(F32, 2, 8, 16, 'A', SPLIT128, SPLIT128)
_pair(F32, 2, 6, 10, 'A', SPLIT128, SPLIT128)
_pair(F32, 2, 6, 10, 'B', SPLIT64, SPLIT64)
_pair(F32, 2, 6, 10, 'D', (None, None, SPLIT128), None)
_pair(F32, 32, 1, 2, 'A', SPLIT128, SPLIT128)
_pair(F32, 32, 1, 3, 'C', SPLIT64, SPLIT64)
_pair(F32, 2, 3, 5, 'X', DIRECT, DIRECT)
_pair(F32, 1, 5, 4, 'Y', DIRECT, DIRECT)
_pair(F32, 2, 2, 4, 'X', DIRECT, DIRECT)
_pair(F32, 8, 24, 48, 'A', None, T128x128)
_pair(F32, 8, 24, 48, 'B', None, T128x64)
_pair(F32, 16, 32, 64, 'A', T128x128, None)
_pair(F32, 16, 32, 64, 'B', T128x64, T256x64)
_pair(F32, 16, 32, 64, 'D', T256x128, None)
_pair(F32, 11, 48, 64, 'A', T128x128, None)
_pair(F32, 11, 48, 64, 'C', None, T256x64)
_pair(F32, 16, 40, 56, 'D', T256x128, None)
_pair(F32, 16, 40, 56, 'B', T128x64, None)

# One BWD launch per kernel form accumulates into out0 (bound 2 x TOL_T_OUT) ...
BWD_ACCUMULATE = {
    'bf16/S2/2x6x10/B2', 'bf16/T2/1x4x5/Y', 'bf16/S2/2x10x6/A', 'bf16/T2/2x16x8/B', 'bf16/S2/2x8x16/A2',
    'bf16/T2/32x16x8/A', 'bf16/S2/64x64x8/A', 'bf16/T2/16x40x56/C', 'bf16/S2/16x56x40/D', 'bf16/S2/64x8x64/A',
    'bf16/T2/8x24x48/B', 'bf16/S2/13x40x64/D', 'bf16/T2/16x64x32/A', 'bf16/S2/16x64x32/A', 'bf16/T2/11x64x48/B',
    'bf16/S2/11x48x64/D', 'bf16/T2/16x32x64/D',
    'f32/S2/2x10x6/A', 'f32/T2/2x6x10/B', 'f32/S2/1x4x5/Y', 'f32/S2/16x64x32/A', 'f32/T2/8x48x24/B', 'f32/T2/11x64x48/C',
    'f32/S2/16x56x40/D',
}
# ... and these take the mask from z (scale / shift passed along): ring cases and patch cases, both geometries
BWD_MASK_FROM_Z = {'bf16/S2/16x32x64/A', 'bf16/T2/16x64x32/C', 'bf16/S2/11x64x48/D', 'bf16/T2/32x8x16/A', 'bf16/S2/13x40x64/A'}
# One case per kernel form whose result must NOT match the reference of the transposed image (it can see an Hs / Ws mix-up)
SWAP_SENTINEL = {
    'bf16/S2/2x3x5/X', 'bf16/T2/2x3x5/X', 'bf16/S2/2x6x10/A', 'bf16/T2/2x6x10/A', 'bf16/S2/2x8x16/B', 'bf16/T2/32x16x8/A',
    'bf16/S2/16x40x56/A', 'bf16/T2/16x40x56/C', 'bf16/S2/16x40x56/D', 'bf16/T2/32x8x16/A', 'bf16/S2/64x8x64/A',
    'bf16/S2/13x40x64/D', 'bf16/T2/16x32x64/A', 'bf16/S2/16x32x64/A', 'bf16/T2/16x32x64/D', 'bf16/S2/11x48x64/D',
    'bf16/T2/11x48x64/B', 'f32/S2/16x32x64/A', 'f32/T2/16x32x64/B', 'f32/S2/2x6x10/A',
}


def igemm_row(key, epi):
    """The planner's view of one launch, in the form of tools/igemm_plan_table.py."""
    c = IGEMM[key]
    return dict(name='%s/epi%d' % (key, epi), dtype=c['dtype'], geom=c['geom'], B=c['B'], Hs=c['Hs'], Ws=c['Ws'], C0=c['C0'],
                C1=c['C1'], N=sum(c['segs']), epi=epi, segs=list(c['segs']), ks=0)


def igemm_cases(epi):
    return [k for k, c in IGEMM.items() if c['forms'][epi] is not None]


# ---------------------------------------------------------------- weight gradient
# channel sets: (R0, R1, C0, C1)
W1 = (128, 0, 64, 0)
W2 = (128, 128, 128, 0)              # two plain sources
W3 = (128, 0, 128, 128)              # two gathered sources, every 128-column tile inside one of them
W4 = (128, 0, 64, 64)                # two gathered sources that a column tile straddles: never the fast form
W5 = (64, 128, 96, 0)                # 96 gathered channels: direct when small, tap-staged split or patch-staged when large
W6 = (8, 0, 6, 0)                    # direct

# route -> what the three queries must say; the literal answers are (workspace bytes, sq count, batchable)
ROUTES = ('fast', 'general', 'direct', 'split', 'patch', 'f32 unsplit', 'f32 split')
WGRAD = {}


def _wpair(route, dtype, B, Hs, Ws, chans, answers):
    for h, w in ((Hs, Ws), (Ws, Hs)):
        key = '%s/%dx%dx%d/%d+%d_%d+%d' % (('bf16' if dtype else 'f32', B, h, w) + chans)
        assert key not in WGRAD, key
        WGRAD[key] = dict(route=route, dtype=dtype, B=B, Hs=h, Ws=w, R0=chans[0], R1=chans[1], C0=chans[2], C1=chans[3],
                          answers=answers, patch=route == 'patch')


# tap-staged MFMA kernel, fast form: power-of-two image, every column tile in one gathered source (batch class 2)
for _b, _h, _w in ((2, 8, 16), (2, 4, 16)):
    _wpair('fast', BF16, _b, _h, _w, W1, (0, 8, 2))
    _wpair('fast', BF16, _b, _h, _w, W2, (0, 32, 2))
    _wpair('fast', BF16, _b, _h, _w, W3, (0, 32, 2))
    _wpair('general', BF16, _b, _h, _w, W4, (0, 16, 1))
# general form: non-power-of-two images (and 2 x 4 at B = 32: unsplit, batch class 1)
for _b, _h, _w, _sets in ((2, 6, 10, (W1, W2, W3, W4)), (3, 3, 5, (W1, W3)), (32, 1, 2, (W1, W2)), (32, 2, 4, (W1, W4)),
                          (32, 1, 3, (W2,))):
    for _s in _sets:
        _wpair('general', BF16, _b, _h, _w, _s, (0, (_s[0] + _s[1]) // 128 * (16 * (_s[2] + _s[3]) // 128), 1))
# direct kernel: channels the MFMA forms do not take
_wpair('direct', BF16, 2, 8, 16, W5, (0, 0, 0))
_wpair('direct', BF16, 2, 8, 16, W6, (0, 0, 0))
_wpair('direct', BF16, 2, 6, 10, W5, (0, 0, 0))
_wpair('direct', BF16, 3, 3, 5, W6, (0, 0, 0))
# pixel split + slab sum, tap-staged (4 x 8: too small for the patch kernel; 24 x 40: not a multiple of 8 x 8 ... of 16)
_wpair('split', BF16, 32, 4, 8, W1, (2097152, 128, 0))
_wpair('split', BF16, 4, 24, 40, W1, (7864320, 128, 0))
_wpair('split', BF16, 4, 24, 40, W5, (2359296, 288, 0))
# patch-staged kernel + slab sum
_wpair('patch', BF16, 8, 16, 32, W1, (8388608, 128, 0))
_wpair('patch', BF16, 8, 16, 32, W2, (33554432, 512, 0))
_wpair('patch', BF16, 8, 16, 32, W5, (18874368, 288, 0))
_wpair('patch', BF16, 8, 16, 32, W4, (16777216, 256, 0))
_wpair('patch', BF16, 4, 24, 48, W1, (9437184, 128, 0))
_wpair('patch', BF16, 4, 24, 48, W5, (21233664, 288, 0))
_wpair('patch', BF16, 4, 24, 48, W4, (18874368, 256, 0))
_wpair('patch', BF16, 2, 64, 32, W1, (8388608, 128, 0))
_wpair('patch', BF16, 2, 64, 32, W2, (33554432, 512, 0))
# f32: the same small shapes run the MFMA kernel unsplit; larger ones split the pixels
_wpair('f32 unsplit', F32, 2, 4, 16, W1, (0, 8, 0))
_wpair('f32 unsplit', F32, 2, 4, 16, W2, (0, 32, 0))
_wpair('f32 unsplit', F32, 2, 6, 10, W1, (0, 8, 0))
_wpair('f32 unsplit', F32, 2, 6, 10, W3, (0, 32, 0))
_wpair('f32 unsplit', F32, 3, 3, 5, W4, (0, 16, 0))
_wpair('f32 unsplit', F32, 32, 1, 2, W1, (0, 8, 0))
_wpair('direct', F32, 2, 8, 16, W5, (0, 0, 0))
_wpair('direct', F32, 2, 6, 10, W6, (0, 0, 0))
_wpair('f32 split', F32, 2, 8, 16, W1, (1048576, 128, 0))
_wpair('f32 split', F32, 8, 16, 32, W1, (16777216, 128, 0))
_wpair('f32 split', F32, 4, 24, 48, W5, (3538944, 288, 0))

# adn_wgrad_batch: (B, class, [(Hs, Ws, R0, R1, C)]); every group beside its transpose
WGRAD_BATCH = [
    (32, 1, [(1, 2, 512, 0, 512), (2, 4, 512, 512, 512), (1, 3, 512, 0, 512), (2, 6, 512, 512, 512)]),
    (32, 1, [(2, 1, 512, 0, 512), (4, 2, 512, 512, 512), (3, 1, 512, 0, 512), (6, 2, 512, 512, 512)]),
    (8, 2, [(8, 16, 512, 0, 512), (16, 8, 512, 512, 512)]),
    (8, 2, [(16, 8, 512, 0, 512), (8, 16, 512, 512, 512)]),
]
# adn_wgrad_patch_batch at B = 8: ([(Hs, Ws, R0, R1, C)], workspace bytes); every group beside its transpose
WGRAD_PATCH_BATCH = [
    ([(32, 16, 128, 0, 64), (16, 32, 256, 0, 128), (24, 48, 64, 128, 96)], 27262976),
    ([(16, 32, 128, 0, 64), (32, 16, 256, 0, 128), (48, 24, 64, 128, 96)], 27262976),
    ([(32, 16, 128, 0, 64), (16, 32, 256, 256, 128), (24, 48, 128, 128, 64), (48, 24, 64, 0, 32)], 29491200),
    ([(16, 32, 128, 0, 64), (32, 16, 256, 256, 128), (48, 24, 128, 128, 64), (24, 48, 64, 0, 32)], 29491200),
]
PATCH_BATCH_B = 8


# One case per route whose dW must NOT match the reference of the transposed images
WGRAD_SENTINEL = {
    'bf16/2x8x16/128+0_128+128', 'bf16/2x6x10/128+0_64+64', 'bf16/2x8x16/64+128_96+0', 'bf16/4x24x40/128+0_64+0',
    'bf16/8x16x32/128+128_128+0', 'bf16/4x24x48/64+128_96+0', 'f32/2x6x10/128+0_128+128', 'f32/2x8x16/128+0_64+0',
}


def wgrad_row(c):
    """The plan tools' view of one weight gradient, in the form of tools/wgrad_plan_table.py."""
    return dict(name='', dtype=c['dtype'], B=c['B'], Hs=c['Hs'], Ws=c['Ws'], R0=c['R0'], R1=c['R1'], C0=c['C0'], C1=c['C1'],
                c_valid=0, ks=0)


def batch_row(B, prob):
    Hs, Ws, R0, R1, Cc = prob
    return dict(name='', dtype=BF16, B=B, Hs=Hs, Ws=Ws, R0=R0, R1=R1, C0=Cc, C1=0, c_valid=0, ks=0)
