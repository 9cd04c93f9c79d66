"""Shapes of tests/test_gpu_streaming_passes.py: the grid-stride kernels of csrc/elementwise.hip and csrc/dcnet.hip past
their first grid pass, and at the channel counts (96, 192, 24) whose channel-group walk moves from pass to pass.  No GPU is
touched here; tests/test_streaming_pass_cases.py recomputes every claim below from the caps and, where the library answers
a grid size itself, holds the cap against the library.

A case is (kernel, dtypes, shape, cap, per_block, claim, why):
  kernel      the kernels.py entry point (or a family name: 'bn' = bn_act and bn_bwd_apply, 'bn_mx8' their fp8 variants)
  dtypes      storage dtypes the GPU test runs, as names ('f32', 'bf16')
  shape       what the GPU test builds; ``items(case)`` turns it into the kernel's count of thread items
  cap         the largest grid the launcher asks for, in blocks
  per_block   thread items one block takes per pass (256 threads; the head kernels: 256 / lanes per pixel)
  claim       dict: passes >= claim['passes']; 'ragged': the last pass is neither empty nor full; 'walk': 'moving' /
              'fixed' (BatchNorm apply: step = (cap * 256) % (C / 8)); 'one_pass': the case is NOT there for a second pass
  why         what the case is there for
"""
from collections import namedtuple

# ---- caps the library cannot be asked for ------------------------------------------------------------------------------
BN_BLOCKS = 1024          # csrc/elementwise.hip, bn_blocks_for(): `... atoi(getenv("ADN_BN_BLOCKS")) : 1024;`
EW_MAX_BLOCKS = 4096      # csrc/elementwise.hip: `constexpr int kMaxBlocks = 4096;`
DC_MAX_BLOCKS = 8192      # csrc/dcnet.hip: `constexpr int kMaxBlocks = 8192;`
# ---- caps the library answers (held against it by the host test) -------------------------------------------------------
TAIL_BLOCKS = 2048        # adn_tail_stats_blocks
RELU_STATS_BLOCKS = 2048  # adn_relu_bwd_stats_num_partials
HEAD_BWD_BLOCKS = 1024    # adn_head1x1_bwd_workspace_bytes / ((C + 1) * 4)
L1TV_STATS_BLOCKS = 1024  # adn_l1tv_workspace_bytes / 24; a block takes 256 * 8 elements before the cap binds
HEAD_IT = 4               # csrc/dcnet.hip: `constexpr int kHeadIt = 4;` (head1x1_bwd: C <= lpp * V * kHeadIt)

Case = namedtuple('Case', 'kernel dtypes shape cap per_block claim why')
BOTH, BF16, F32 = ('f32', 'bf16'), ('bf16',), ('f32',)


def head_lanes(C):
    """(V, lanes per pixel) of the 1x1 head kernels: head_lpp() of csrc/dcnet.hip."""
    V = 8 if C % 8 == 0 else 1
    groups = -(-C // V)
    lpp = 1
    while lpp < groups:
        lpp *= 2
    return V, min(lpp, 64)


def head_bwd_max_channels(C):
    V, lpp = head_lanes(C)
    return lpp * V * HEAD_IT


def _vec(C):
    return C // 8 if C % 8 == 0 else C


def items(case):
    """Thread items (the loop bound the kernel strides over) of a case."""
    k, s = case.kernel, case.shape
    if k in ('bn', 'bn_mx8'):
        pixels, C = s
        return pixels * _vec(C)
    if k in ('upsample2x_fwd', 'upsample2x_fwd_mx8'):
        B, Hi, Wi, C, Ho, Wo = s
        return B * Ho * Wo * _vec(C)
    if k == 'maxpool2_bwd_tail':
        B, H, W, C = s
        return B * ((H + 1) // 2) * ((W + 1) // 2) * (C // 8)
    if k == 'upsample2x_bwd_tail':
        B, Hi, Wi, C, Ho, Wo = s
        return B * Hi * Wi * (C // 8)
    if k in ('head1x1_fwd', 'head1x1_bwd', 'relu_bwd_stats'):
        return s[0]                                   # pixels
    if k == 'nchw_to_nhwc':
        B, C, H, W = s[:4]
        return B * H * W                              # one thread per pixel
    if k == 'nhwc_to_nchw':
        B, C, H, W = s
        return B * C * H * W                          # one thread per element
    if k == 'pixel_shuffle2':
        B, H, W, C = s
        return B * H * W * 4 * _vec(C)
    if k in ('clamp_range', 'l1tv_stats', 'l1tv_finish'):
        n = 1
        for d in s:
            n *= d
        return n
    raise KeyError(k)


def passes(case):
    """(full passes, items in the ragged last pass): the kernel runs ``full + (ragged > 0)`` passes."""
    per_pass = case.cap * case.per_block
    return items(case) // per_pass, items(case) % per_pass


def bn_step(case):
    pixels, C = case.shape
    return (case.cap * 256) % (C // 8) if C % 8 == 0 else None


# ---- BatchNorm apply: bn_act (leaky, relu, both) and bn_bwd_apply ---------------------------------------------------------
BN = [
    Case('bn', BOTH, (32771, 192), BN_BLOCKS, 256, dict(passes=3, ragged=True, walk='moving', step=16),
         'AdaBins C = 192: 24 channel groups, the thread moves 16 groups per pass'),
    Case('bn', BOTH, (65543, 96), BN_BLOCKS, 256, dict(passes=3, ragged=True, walk='moving', step=4),
         'AdaBins C = 96: 12 channel groups, step 4'),
    Case('bn', BOTH, (262147, 24), BN_BLOCKS, 256, dict(passes=3, ragged=True, walk='moving', step=1),
         'C = 24: 3 channel groups, step 1 (every pass wraps somewhere)'),
    Case('bn', BOTH, (98317, 64), BN_BLOCKS, 256, dict(passes=3, ragged=True, walk='fixed', step=0),
         'power-of-two C: coefficients loaded once and kept over three passes'),
    Case('bn', BOTH, (43703, 12), BN_BLOCKS, 256, dict(passes=2, ragged=True),
         'C % 8 != 0: the scalar path, second pass'),
]
BN_MX8 = [
    Case('bn_mx8', BF16, (32771, 192), BN_BLOCKS, 256, dict(passes=3, ragged=True, walk='moving', step=16),
         'fp8 bytes and scale bytes written from inside the moving loop'),
    Case('bn_mx8', BF16, (98317, 64), BN_BLOCKS, 256, dict(passes=3, ragged=True, walk='fixed', step=0),
         'fp8 bytes and scale bytes written from inside the fixed loop'),
]

# ---- bilinear x2 upsample forward (+ fp8 copy): (B, Hi, Wi, C, Ho, Wo) --------------------------------------------------
UPSAMPLE_FWD = [
    Case('upsample2x_fwd', BOTH, (2, 257, 256, 32, 514, 512), DC_MAX_BLOCKS, 256, dict(passes=1, ragged=True),
         '2 105 344 items: 8 192 past one pass'),
    Case('upsample2x_fwd', BOTH, (2, 257, 256, 32, 515, 514), DC_MAX_BLOCKS, 256, dict(passes=1, ragged=True),
         'the padded target of Up.forward (one row, two columns)'),
]
UPSAMPLE_FWD_MX8 = [c._replace(kernel='upsample2x_fwd_mx8', dtypes=BF16) for c in UPSAMPLE_FWD]

# ---- tail-fused backward kernels: mean / istd loaded once per thread -----------------------------------------------------
MAXPOOL_TAIL = [
    Case('maxpool2_bwd_tail', BOTH, (2, 363, 365, 64), TAIL_BLOCKS, 256, dict(passes=1, ragged=True),
         'odd H and W (trailing row and column), 1.02 passes'),
    Case('maxpool2_bwd_tail', BF16, (3, 149, 151, 256), TAIL_BLOCKS, 256, dict(passes=1, ragged=True),
         '32 channel groups, 8 threads per group in the block reduction'),
    Case('maxpool2_bwd_tail', BF16, (4, 363, 365, 64), TAIL_BLOCKS, 256, dict(passes=2, ragged=True),
         '2.03 passes: a thread carries its sums and constants into a third pass'),
]
UPSAMPLE_TAIL = [
    Case('upsample2x_bwd_tail', BOTH, (2, 181, 183, 64, 363, 368), TAIL_BLOCKS, 256, dict(passes=1, ragged=True),
         'padded target (one row, two columns), 1.01 passes'),
    Case('upsample2x_bwd_tail', BF16, (2, 91, 93, 256, 183, 188), TAIL_BLOCKS, 256, dict(passes=1, ragged=True),
         '32 channel groups, 1.03 passes'),
]

# ---- relu_bwd_stats: (pixels, C); a block owns ceil(pixels / grid) rows --------------------------------------------------
# claim: rows = rows per block, rpi = rows per iteration (256 // channel groups; None on the scalar path), idle = idle threads,
# empty = trailing blocks that own no row, col_passes = column passes of 256 channel groups
RELU_STATS = [
    Case('relu_bwd_stats', BOTH, (524289, 8), RELU_STATS_BLOCKS, 257, dict(rows=257, rpi=256, idle=0, empty=7, col_passes=1),
         '257 rows per block: a second trip of the row loop; 7 trailing blocks own nothing'),
    Case('relu_bwd_stats', BOTH, (3001, 192), RELU_STATS_BLOCKS, 251, dict(rows=251, rpi=10, idle=16, empty=0, col_passes=1),
         'C = 192: 24 groups, 10 rows per iteration, 16 idle threads'),
    Case('relu_bwd_stats', BOTH, (1537, 96), RELU_STATS_BLOCKS, 220, dict(rows=220, rpi=21, idle=4, empty=0, col_passes=1),
         'C = 96: 12 groups, 21 rows per iteration, 4 idle threads'),
    Case('relu_bwd_stats', BOTH, (700, 2056), RELU_STATS_BLOCKS, 234, dict(rows=234, rpi=1, idle=0, empty=0, col_passes=2),
         'C > 2048: a second column pass of ONE channel group (256 rows per iteration there)'),
    Case('relu_bwd_stats', BOTH, (1031, 12), RELU_STATS_BLOCKS, 207, dict(rows=207, rpi=None, empty=0, col_passes=1),
         'scalar path, 12 of 256 threads busy'),
    Case('relu_bwd_stats', BOTH, (1031, 20), RELU_STATS_BLOCKS, 207, dict(rows=207, rpi=None, empty=0, col_passes=1),
         'scalar path, C % 8 == 4'),
]

# ---- 1x1 head: (pixels, C); per_block = 256 / lanes per pixel ----------------------------------------------------------
HEAD_FWD = [
    Case('head1x1_fwd', BOTH, (262181, 64), DC_MAX_BLOCKS, 32, dict(passes=1, ragged=True), '8 lanes per pixel'),
    Case('head1x1_fwd', BOTH, (262181, 5), DC_MAX_BLOCKS, 32, dict(passes=1, ragged=True), 'scalar loads, 3 of 8 lanes idle'),
    Case('head1x1_fwd', BF16, (2097189, 8), DC_MAX_BLOCKS, 256, dict(passes=1, ragged=True), 'one lane per pixel'),
    Case('head1x1_fwd', BOTH, (70001, 24), DC_MAX_BLOCKS, 64, dict(one_pass=True),
         '3 channel groups on 4 lanes: one idle lane per pixel group (stays inside one pass)'),
]
HEAD_BWD = [
    Case('head1x1_bwd', BOTH, (98315, 64), HEAD_BWD_BLOCKS, 32, dict(passes=3, ragged=True), 'acc[] kept over four passes'),
    Case('head1x1_bwd', BOTH, (98315, 5), HEAD_BWD_BLOCKS, 32, dict(passes=3, ragged=True), 'scalar path'),
    Case('head1x1_bwd', BOTH, (20011, 2048), HEAD_BWD_BLOCKS, 4, dict(passes=4, ragged=True),
         'the channel limit with V = 8: all four channel passes of all 64 lanes'),
    Case('head1x1_bwd', BOTH, (1037, 250), HEAD_BWD_BLOCKS, 4, dict(one_pass=True),
         'scalar path six channels under its limit of 256: the fourth channel pass is ragged'),
]
HEAD_BWD_REFUSED = (2056, 257)        # one 16-byte group / one channel past the limit
HEAD_SMALL = [(2, 64, 16, 16), (2, 8, 5, 7), (1, 5, 4, 4), (2, 256, 4, 4)]      # (B, C, H, W) of test_head1x1

# ---- exact copies ---------------------------------------------------------------------------------------------------------
# nhwc_to_nchw walks ELEMENTS, nchw_to_nhwc walks PIXELS: the two NCHW shapes below take the former past one pass and are
# converted both ways; the third (with its padded channel count) takes the per-pixel kernel past 4096 * 256 pixels.
NHWC_TO_NCHW = [
    Case('nhwc_to_nchw', BOTH, (2, 64, 96, 97), EW_MAX_BLOCKS, 256, dict(passes=1, ragged=True), '1.14 passes'),
    Case('nhwc_to_nchw', BOTH, (3, 5, 301, 233), EW_MAX_BLOCKS, 256, dict(passes=1, ragged=True), 'odd C, 1.003 passes'),
]
NCHW_TO_NHWC = [
    Case('nchw_to_nhwc', BOTH, (2, 64, 96, 97, 64), EW_MAX_BLOCKS, 256, dict(one_pass=True), 'inverse of the case above'),
    Case('nchw_to_nhwc', BOTH, (3, 5, 301, 233, 5), EW_MAX_BLOCKS, 256, dict(one_pass=True), 'inverse of the case above'),
    Case('nchw_to_nhwc', BOTH, (1, 3, 1031, 1021, 8), EW_MAX_BLOCKS, 256, dict(passes=1, ragged=True),
         '1 052 651 pixels: the per-pixel loop past one pass, 3 channels padded to 8'),
]
PIXEL_SHUFFLE = [
    Case('pixel_shuffle2', BF16, (2, 257, 256, 32), DC_MAX_BLOCKS, 256, dict(passes=1, ragged=True), '16-byte path'),
    Case('pixel_shuffle2', F32, (1, 301, 291, 6), DC_MAX_BLOCKS, 256, dict(passes=1, ragged=True),
         'scalar path (W = 290 stays 2 192 items short of a second pass)'),
]
CLAMP = [Case('clamp_range', F32, (2097152 + 4099,), DC_MAX_BLOCKS, 256, dict(passes=1, ragged=True),
              'boundary values planted in the second pass')]
CLAMP_PLANT = 2097152 + 4000          # where the GPU test plants 0, max_depth and the float after it

# ---- L1 + TV loss: (B, H, W) ----------------------------------------------------------------------------------------------
L1TV = [
    Case('l1tv_stats', F32, (2, 1031, 1019), L1TV_STATS_BLOCKS, 256, dict(passes=8, ragged=True), 'nine passes of 1024 blocks'),
    Case('l1tv_finish', F32, (2, 1031, 1019), DC_MAX_BLOCKS, 256, dict(passes=1, ragged=True), '4 026 pixels past one pass'),
]

ALL = (BN + BN_MX8 + UPSAMPLE_FWD + UPSAMPLE_FWD_MX8 + MAXPOOL_TAIL + UPSAMPLE_TAIL + RELU_STATS + HEAD_FWD + HEAD_BWD +
       NHWC_TO_NCHW + NCHW_TO_NHWC + PIXEL_SHUFFLE + CLAMP + L1TV)


def case_id(case):
    return case.kernel + '-' + 'x'.join(str(d) for d in case.shape)
