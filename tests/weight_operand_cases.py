"""Host-side references of the weight-operand chain (tests/test_gpu_weight_operands.py), plain enough to be read against
the kernels they stand for and exercised without a GPU (tests/test_weight_operand_cases.py):

  * ``optimizer_reference``: one AdamW / Adam (L2) / SGD update in float64, the formulas ``adam_elem`` documents
    (csrc/loss_optim.hip) -- torch.optim's, with the clip coefficient folded into the gradient;
  * ``t2_reference`` / ``s2_reference``: the T2 and S2 GEMM operand layouts as index permutations of a master
    [X][kh][kw][Y] -- the (phase, tap) map ``test_pack_weights_layout`` writes out;
  * ``t2_table``: the layer table of adn_pack_t2_multi as UNetEngine._prepare builds it;
  * ``bf16_rne_bits``: round-to-nearest-even f32 -> bf16 on bit patterns, and ``EDGE_BITS``, the patterns where a cast
    that truncates, rounds half away from zero or mishandles the exponent edge gives other bits.
"""
import numpy as np
import torch

ALIGN = 8                   # flat._align: every parameter starts at a multiple of 8 elements
KINDS = ((0, 0.1), (1, 0.0), (1, 0.1), (2, 0.0))        # (kind, weight decay): AdamW, Adam, Adam + L2, SGD
KIND_NAME = {(0, 0.1): 'AdamW', (1, 0.0): 'Adam', (1, 0.1): 'Adam+L2', (2, 0.0): 'SGD'}
OPT_RTOL, OPT_ATOL = 2e-5, 2e-6                          # the suite's optimizer bar against float64 (test_gpu_aux.py)

# kernel row of phase p, tap t (k4 s2 p1): output row 2*i + p reads kernel rows KH[p, 0], KH[p, 1]
KH = {(0, 0): 1, (0, 1): 3, (1, 0): 0, (1, 1): 2}

# (X, Y) of the layers packed in ONE adn_pack_t2_multi launch: scalar form ((X | Y) & 7 != 0) and vector form mixed, so that
# the blockIdx -> layer scan crosses both; partial 64 x 64 tiles in x, in y and in both; several tiles each way
T2_LAYERS = ((64, 2), (16, 1), (6, 10), (4, 8), (64, 64), (72, 40), (136, 8), (128, 256), (72, 64), (64, 40))

EDGE_BITS = {
    'tie_to_even_down': 0x3F808000,      # exactly between 0x3F80 and 0x3F81: even is below
    'tie_to_even_up': 0x3F818000,        # exactly between 0x3F81 and 0x3F82: even is above
    'below_tie': 0x3F807FFF,
    'above_tie': 0x3F808001,
    'minus_zero': 0x80000000,
    'denormal': 0x00012345,
    'max_finite': 0x7F7FFFFF,            # rounds up to bf16 infinity
    'plus_inf': 0x7F800000,
    'minus_inf': 0xFF800000,
    'nan': 0x7FC00000,
}
EDGE_BF16 = {
    'tie_to_even_down': 0x3F80, 'tie_to_even_up': 0x3F82, 'below_tie': 0x3F80, 'above_tie': 0x3F81, 'minus_zero': 0x8000,
    'denormal': 0x0001, 'max_finite': 0x7F80, 'plus_inf': 0x7F80, 'minus_inf': 0xFF80,
}


def f32r(x):
    """A Python float rounded to f32 and back: what a ``float`` argument of the C ABI holds (0.999f is 3e-5 of
    1 - beta2 away from 0.999)."""
    return float(np.float32(x))


def bf16_rne_bits(bits):
    """uint32 f32 bit patterns -> uint16 bf16 bit patterns, round to nearest even (NaN -> a quiet NaN)."""
    b = np.asarray(bits, dtype=np.uint64)
    rounded = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
    return np.where(nan, 0x7FC0, rounded).astype(np.uint16)


def f32_from_bits(bits, device='cpu'):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy()).to(device)


def optimizer_reference(p, g, m, v, kind, lr, b1, b2, eps, wd, coef, t):
    """Step ``t`` (1-based) of torch.optim.AdamW (kind 0) / Adam with L2 decay (1) / SGD (2) on float64 tensors, the
    gradient scaled by ``coef`` first.  Hyper-parameters as the kernel receives them (see f32r).  -> (p, m, v)."""
    p, g, m, v = p.double(), g.double() * coef, m.double(), v.double()
    if kind == 2:
        return p - lr * g, m, v
    if kind == 0:
        p = p * (1.0 - lr * wd)
    elif wd != 0.0:
        g = g + wd * p
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = v.sqrt() / (bc2 ** 0.5) + eps
    return p - (lr / bc1) * (m / denom), m, v


def t2_reference(master):
    """master [X, 16, Y] (= [X][kh][kw][Y]) -> t2 [4, Y, 4, X] with t2[ph*2+pw, y, ty*2+tx, x] = w[x, y, kh, kw],
    kh = KH[ph, ty], kw = KH[pw, tx].  Pure indexing: the values keep their bits."""
    X, taps, Y = master.shape
    assert taps == 16
    w = master.reshape(X, 4, 4, Y)
    out = torch.empty(4, Y, 4, X, dtype=master.dtype, device=master.device)
    for ph in range(2):
        for pw in range(2):
            for ty in range(2):
                for tx in range(2):
                    out[ph * 2 + pw, :, ty * 2 + tx, :] = w[:, KH[(ph, ty)], KH[(pw, tx)], :].t()
    return out


def s2_reference(master, y_pad):
    """master [X, 16, Y] -> s2 [X, 16, y_pad]: the master itself, channels Y..y_pad zero."""
    X, taps, Y = master.shape
    out = torch.zeros(X, taps, y_pad, dtype=master.dtype, device=master.device)
    out[:, :, :Y] = master
    return out


def _align(n, a=ALIGN):
    return (n + a - 1) // a * a


def t2_table(layers=T2_LAYERS):
    """The table of adn_pack_t2_multi for ``layers`` = [(X, Y)], laid out as the engine lays a model out: masters at
    8-element-aligned offsets of one flat buffer, each followed by a bias-sized parameter of X elements padded to the
    alignment (16 * X * Y is itself aligned: what lies between two conv weights of a model are its other parameters and
    their padding; the pack must read none of it), T2 outputs back to back, 16 taps x 64 x 64 tiles of blocks per layer.
    -> (rows [master_off, X, Y, t2_off, first_block], master elements, t2 elements, total blocks)."""
    rows, m_off, t2_off, blk = [], 0, 0, 0
    for X, Y in layers:
        rows.append([m_off, X, Y, t2_off, blk])
        m_off += _align(16 * X * Y) + _align(X)
        t2_off += 16 * X * Y
        blk += ((X + 63) // 64) * ((Y + 63) // 64) * 16
    return rows, m_off, t2_off, blk


def bits(t):
    """Integer view of a float tensor: comparisons that see -0.0, NaN payloads and every rounding bit."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
