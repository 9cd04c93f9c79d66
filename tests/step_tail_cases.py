"""Seeded cases, float64 references and error bars of the kernels every training step ends in (csrc/loss_optim.hip,
metrics.hip, edgeloss.hip), for tests/test_gpu_step_tail.py; exercised without a GPU by tests/test_step_tail_cases.py.

The kernels DECIDE in float32 (which pixels are valid, the sign of a difference, a clamp, a threshold), so every generator
here draws inputs on which float32 and float64 must decide alike, and the host test asserts that they do:

  * masked loss: pred / gt are multiples of 1/64 (p * scale, g * scale and p - g are exact in float32);
  * edge loss: multiples of 1/4 (Sobel responses and their squares are exact; two radicands are equal or 1/16 apart);
  * metrics: random float32, any pixel near a threshold or an epsilon redrawn;
  * gradient norm: multiples of 1/1024 below 2 (squares and their pair sums are exact in float32);
  * optimizer: gradients and moments exactly 0 or at least 1e-6 in magnitude.

A reference takes scale, eps, the loss weights, lr, the betas ... as the float32 VALUES the kernel receives (``f32r``) and
from there on works in float64 on the float32 inputs, on top of oracle/{loss,optim,metrics,edge_loss}_oracle.py.

Error bars are formulas over a case's own float64 magnitudes, u = 2^-24 (half a float32 ulp, relative):
  counts                                        exact
  sums of exactly representable terms           n * 2^-52 * sum |term|           (only the f64 summation order differs)
  sum d, sum d^2 (d = logf p - logf g)          4u * sum (|log p| + |log g|),  4u * sum 2 |d| (|log p| + |log g|)
  loss value                                    the above through the closed form, + u |loss| for the cast to float32
  per-element outputs                           16u * (sum of the magnitudes of the terms added to make it) + 1e-30
Each ``*_f32`` function restates a kernel's formula elementwise in float32 numpy (float64 sums); the host test requires it
to sit inside every bar with 4x room, so that a bar that is too tight shows up there and not as a GPU failure.
"""
import numpy as np
import torch

from oracle import edge_loss_oracle, loss_oracle, metrics_oracle, optim_oracle

U = 2.0 ** -24
TINY = 1e-30
D52 = 2.0 ** -52


def f32r(x):
    """A Python float rounded to float32 and back: what a ``float`` argument of the C ABI holds."""
    return float(np.float32(x))


# =========================================================================================================== masked loss
EPS = f32r(1e-6)
EPS_BELOW = float(np.nextafter(np.float32(1e-6), np.float32(0.0)))
MASK_NAME = {0: 'ne0', 1: 'gt0', 2: 'all'}
CRIT_NAME = {0: 'L1', 1: 'SIlog', 2: 'Combined', 4: 'MSE'}
L1W, SW, LAM = f32r(0.237), f32r(0.637), f32r(0.869)
LOSS_N = (1, 63, 257, 2049)                         # one thread; part of a block; a second block; a tail past 8 blocks
LOSS_N_FINISH_CAP = 4096 * 256 + 1                  # loss_finish / final_act_bwd: one element into the second grid pass
LOSS_N_RED_CAP = 1024 * 2048 + 1                    # red_blocks: 1024 blocks x 2048 elements, one element past
SCALES = (1.0, 30.0)


def loss_case(n, scale, seed=0):
    """(pred, gt) float32 [n], multiples of 1/64: in (-2, 30) at scale 1, in (-0.25, 1) otherwise.  About 5 % negative and
    10 % zero gt, pred <= 0 on some pixels and pred == gt on some valid ones; at scale 1 (n >= 8) pixel 1 predicts exactly
    the float32 eps and pixel n - 2 the float32 just below it, both over a positive gt."""
    rng = np.random.default_rng(1000 * seed + n % 99991 + int(scale))
    lo, hi = (-127, 1920) if scale == 1.0 else (-15, 64)
    gt = rng.integers(1, hi, n)
    r = rng.random(n)
    gt = np.where(r < 0.05, rng.integers(lo, 0, n), np.where(r < 0.15, 0, gt))
    pred = rng.integers(lo, hi, n)
    same = rng.random(n) < 0.1
    pred = np.where(same, gt, pred)
    if n >= 8:                      # every kind of pixel, whatever the draw
        gt[0], pred[0] = 5, 5                         # pred == gt, valid
        gt[2], pred[2] = lo + 1, 7                    # negative gt
        gt[3], pred[3] = 0, 9                         # zero gt
        gt[4], pred[4] = 11, lo + 2                   # pred < 0
        gt[5], pred[5] = 13, 0                        # pred == 0
    else:                           # a pixel or two: valid, pred != gt, both positive (d != 0, so var = (1 - lam) d^2 > 0)
        gt[:], pred[:] = 32, 16
    pred = (pred / 64.0).astype(np.float32)
    gt = (gt / 64.0).astype(np.float32)
    if scale == 1.0 and n >= 8:
        pred[1], pred[n - 2] = np.float32(EPS), np.float32(EPS_BELOW)
        gt[1], gt[n - 2] = 0.5, 0.25
    return pred, gt


def empty_mask_case(n, mode):
    """No valid pixel under ``mode`` (0: all zero; 1: zero and negative)."""
    pred, gt = loss_case(n, 1.0, seed=3)
    gt = np.where(gt > 0, 0.0 if mode == 0 else -gt, gt).astype(np.float32)
    if mode == 0:
        gt[:] = 0.0
    return pred, gt


def var0_cases():
    """name -> (pred, gt): SIlog variance exactly zero at lambda = 1, in float32 and float64 alike.
    'two_px': pred = 2 gt on the only two valid pixels (d is one number d0 on both; N d0, N d0^2 and their quotients by
    N = 2 are exact in binary, so var = d0^2 - d0^2 = 0 whatever logf returned); 'equal': pred == gt everywhere (d = 0)."""
    n = 63
    gt = np.zeros(n, np.float32)
    pred = np.full(n, 3.0, np.float32)
    gt[[5, 60]] = 4.0
    pred[[5, 60]] = 8.0
    _, g2 = loss_case(257, 1.0, seed=5)
    return {'two_px': (pred, gt), 'equal': (g2.copy(), g2)}


def _sums(x):
    return float(np.sum(x, dtype=np.float64))


def loss_reference(pred, gt, scale, mode, crit, final_act=None, l1w=L1W, sw=SW, lam=LAM, eps=EPS):
    """Float64 reference of adn_loss_stats + adn_loss_finish(_dz) on float32 inputs, with the error bar of every output.
    -> dict(stats[4], stats_bar[4], loss, loss_bar, grad, grad_bar, bias, bias_bar, var, var_bar, n_inexact)."""
    mm, cn = MASK_NAME[mode & 3], CRIT_NAME[crit]
    assert (crit == 4) == bool(mode & 4)
    p64, g64 = pred.astype(np.float64), gt.astype(np.float64)
    tp, tg = torch.from_numpy(p64), torch.from_numpy(g64)
    stats = [float(s) for s in loss_oracle.loss_stats(tp, tg, scale, mm, eps, squared=crit == 4)]
    loss = float(loss_oracle.masked_loss(tp, tg, cn, l1w, sw, lam, scale, mm, eps))
    grad = loss_oracle.masked_loss_grad_numpy(pred, gt, cn, l1w, sw, lam, scale, mm, eps)

    mask = loss_oracle.valid_mask(gt, mm)
    n, N = pred.size, stats[0]
    p, g = p64 * scale, g64 * scale
    t = (p - g)[mask]
    exact = (t.astype(np.float32).astype(np.float64) == t)            # p - g representable: float32 subtracts exactly
    term = t * t if crit == 4 else np.abs(t)
    # exact terms: only the order of the f64 sum differs; an inexact difference (the two eps pixels) is one float32
    # rounding, u of it (2u of its square), with the factor 4 the logf bars below leave as well
    bar_a = n * D52 * _sums(term) + (2 if crit == 4 else 1) * 4 * U * _sums(term[~exact])
    lp, lg = np.log(np.maximum(p, eps))[mask], np.log(np.maximum(g, eps))[mask]
    d = lp - lg
    la = np.abs(lp) + np.abs(lg)
    # d is the difference of two float32 logf values: each within ~1 ulp = 2u of the true log (the factor 4 leaves room
    # for a 1-2 ulp device logf and the rounding of the difference); d^2 moves by 2 |d| times that
    bar_d = 4 * U * _sums(la) + n * D52 * _sums(np.abs(d))
    bar_d2 = 4 * U * _sums(2 * np.abs(d) * la) + n * D52 * _sums(d * d)
    out = dict(stats=stats, stats_bar=[0.0, bar_a, bar_d, bar_d2], n_inexact=int((~exact).sum()), N=N)

    w1 = {0: 1.0, 1: 0.0, 2: l1w, 4: l1w}[crit]
    w2 = {0: 0.0, 1: 1.0, 2: sw, 4: 0.0}[crit]
    if N == 0:
        out.update(loss=float('nan'), loss_bar=0.0, grad=grad, grad_bar=np.zeros(n), var=0.0, var_bar=0.0)
    else:
        l1, mean = stats[1] / N, stats[2] / N
        var = stats[3] / N - lam * mean * mean
        bar_l1 = bar_a / N + D52 * abs(l1)
        bar_mean = bar_d / N
        bar_var = bar_d2 / N + lam * (2 * abs(mean) * bar_mean + bar_mean ** 2)
        silog = np.sqrt(max(var, 0.0))
        # sqrt is concave: the larger excursion is downwards
        bar_silog = silog - np.sqrt(max(var - bar_var, 0.0)) if var > 0 else 0.0
        # + the cast of the f64 value to float32; and never looser than the suite's 1e-5 on the loss (a lone pixel's
        # var = (1 - lam) d^2 cancels enough for the propagated bar to pass it)
        out.update(loss=loss, var=var, var_bar=bar_var,
                   loss_bar=min(w1 * bar_l1 + w2 * bar_silog + U * abs(loss), 1e-5 * abs(loss)))
        if crit == 4:
            c = 2.0 * w1 * scale / N
            T = np.where(mask, abs(c) * (np.abs(p) + np.abs(g)), 0.0)
        else:
            # the element is c1 sign(p - g) + c2 (log p - log g - lam mean_d) / p: four terms
            c1 = w1 * scale / N
            c2 = w2 * scale / (N * silog) if var > 0 else 0.0
            gate = mask & (p >= eps)
            lpf, lgf = np.log(np.maximum(p, eps)), np.log(np.maximum(g, eps))
            T = np.where(mask, c1 * np.abs(np.sign(p - g)), 0.0)
            T = T + np.where(gate, abs(c2) / np.maximum(p, eps) * (np.abs(lpf) + np.abs(lgf) + abs(lam * mean)), 0.0)
        out.update(grad=grad, grad_bar=16 * U * T + TINY)
    if final_act is not None:
        f = loss_oracle.final_act_factor(pred, final_act)
        out['grad'] = out['grad'] * f
        out['grad_bar'] = (out['grad_bar'] - TINY) * np.abs(f) + TINY
        out['bias'] = loss_oracle.bias_grad_sum(out['grad'])
        # the bias gradient is the sum of every term of every element, then one cast to float32
        out['bias_bar'] = _sums(out['grad_bar']) + U * abs(out['bias']) + TINY
    return out


def _act_f32(o, kind):
    o = o.astype(np.float32)
    one = np.float32(1.0)
    return (o * (one - o)) if kind == 1 else (np.ones_like(o) if kind == 2 else (o > 0).astype(np.float32))


def loss_f32(pred, gt, scale, mode, crit, final_act=None, l1w=L1W, sw=SW, lam=LAM, eps=EPS):
    """The kernels' formulas (loss_stats_partial_kernel, loss_finish_kernel) elementwise in float32 numpy, sums in float64.
    -> (stats[4], loss, grad float32, bias); loss and bias before their cast to float32 (one rounding, u, that the bars
    carry as a term of its own)."""
    f = np.float32
    sc, e = f(scale), f(eps)
    m = mode & 3
    valid = (gt != 0) if m == 0 else ((gt > 0) if m == 1 else np.ones(gt.shape, bool))
    p, g = pred * sc, gt * sc
    d = np.log(np.maximum(p, e)) - np.log(np.maximum(g, e))
    assert p.dtype == np.float32 and d.dtype == np.float32
    diff = p - g
    a = diff.astype(np.float64) ** 2 if mode & 4 else np.abs(diff).astype(np.float64)
    d64 = d.astype(np.float64)
    N = float(valid.sum())
    stats = [N, _sums(a[valid]), _sums(d64[valid]), _sums((d64 * d64)[valid])]
    w1 = {0: 1.0, 1: 0.0, 2: l1w, 4: l1w}[crit]
    w2 = {0: 0.0, 1: 1.0, 2: sw, 4: 0.0}[crit]
    if N == 0:
        return stats, float('nan'), np.zeros_like(pred), 0.0
    l1, mean = stats[1] / N, stats[2] / N
    var = stats[3] / N - lam * mean * mean
    silog = np.sqrt(var) if var > 0 else 0.0
    if crit == 4:
        loss = w1 * stats[1] / N
        gr = np.where(valid, f(2.0 * w1 * scale / N) * diff, f(0))
    else:
        loss = w1 * l1 + w2 * silog
        c1 = f(w1 * scale / N)
        c2 = f(w2 * scale / (N * silog)) if silog > 0 else f(0)
        lm = f(lam * mean)
        gr = c1 * np.sign(diff)
        with np.errstate(divide='ignore', invalid='ignore'):
            dd = np.log(p) - np.log(np.maximum(g, e))
            s = c2 * (dd - lm) / p
        gr = gr + np.where((c2 != 0) & (p >= e), s, f(0))
        gr = np.where(valid, gr, f(0))
    gr = gr.astype(f)
    bias = 0.0
    if final_act is not None:
        gr = gr * _act_f32(pred, final_act)
        bias = _sums(gr.astype(np.float64))
    return stats, loss, gr, bias


# ------------------------------------------------------------------------------------------- final_act_bwd, sum_to_scalar
FINAL_ACT_N = (1, 257, LOSS_N_FINISH_CAP)
SUM_N = (1, 63, 257, 2049, LOSS_N_RED_CAP)


def final_act_case(n, seed=0):
    """(gout random float32, out multiples of 1/64 in (-2, 30)): act'(out) is exact in float32 (out (1 - out) has at most
    22 significant bits), so gout * act' is ONE float32 rounding of a product float64 holds exactly."""
    rng = np.random.default_rng(77 + seed + n % 9973)
    out = (rng.integers(-127, 1920, n) / 64.0).astype(np.float32)
    out[rng.random(n) < 0.2] = 0.0
    return rng.standard_normal(n).astype(np.float32), out


def final_act_reference(gout, out, kind):
    """float64 product and the float32 it must round to (the product is exact in float64: 24 + 22 bits)."""
    ref = gout.astype(np.float64) * loss_oracle.final_act_factor(out, kind)
    return ref, ref.astype(np.float32)


def sum_case(n, seed=0):
    rng = np.random.default_rng(99 + seed + n % 9973)
    return (rng.standard_normal(n) * 3.0).astype(np.float32)


def sum_reference(x):
    """(sum, bar): the terms are exact in float64, so the order of the sum (n 2^-52 sum|x|) and the cast to float32."""
    x = np.asarray(x, dtype=np.float64)
    s = _sums(x)
    return s, x.size * D52 * _sums(np.abs(x)) + U * abs(s) + TINY


# ================================================================================================= gradient norm and clip
NORM_N = (1, 2, 3, 4, 5, 7, 1023, 2049, 1024 * 2048 + 3)
ROW_MAX = 8192


def norm_case(n, seed=0):
    """Multiples of 1/1024 in (-2, 2): g^2 (22 bits) and g0^2 + g1^2 are exact in float32, so the partial sums are sums of
    exactly representable terms."""
    rng = np.random.default_rng(555 + seed + n % 9973)
    g = rng.integers(-2047, 2048, n)
    if n >= 4:
        g[0] = 0
    return (g / 1024.0).astype(np.float32)


def split_rows(n4, row=ROW_MAX):
    """(offset, length) rows covering [0, n4), n4 a multiple of 4, each at most ``row`` long."""
    return [(o, min(row, n4 - o)) for o in range(0, n4, row)]


def max_norms(total):
    """(a max_norm that clips, one that does not): coef = max_norm / (total + 1e-6) is 1/2 or, before the clamp, 2."""
    return f32r(0.5 * (total + 1e-6)), f32r(2.0 * (total + 1e-6))


def norm_reference(grads, ranges=(), extra=(), max_norm=1.0, n_terms=None):
    """-> (total, coef, total_bar, coef_bar) of clip_grad_norm_ over rows of ``grads`` and ready-made sums of squares.
    The sum of squares is a sum of exact terms (n 2^-52 of it); sqrt halves the relative error and rounds once, the
    quotient rounds twice more."""
    total, coef = optim_oracle.clip_coef_ranges(grads, ranges, extra, max_norm)
    n = (sum(r[1] for r in ranges) + len(extra)) if n_terms is None else n_terms
    rel = 0.5 * n * D52 + 2 * D52
    return total, coef, rel * total + TINY, (rel + 2 * D52) * coef + TINY


# ============================================================================================================== optimizer
LR, B1, B2, OPT_EPS = f32r(1e-2), f32r(0.9), f32r(0.999), f32r(1e-8)
OPT_KINDS = ((0, 0.0), (0, 0.01), (1, 0.0), (1, 0.01), (2, 0.0))      # (kind, weight decay): AdamW x2, Adam, Adam + L2, SGD
OPT_N = (1, 3, 5, 1027)
OPT_N_CAP = 8192 * 1024 + 3                          # 8192 blocks x 256 threads x 4 and a 3-element tail: the grid is capped
OPT_N_CAP_NEXT = OPT_N_CAP + 4                       # ... and one more group of four: thread 0 strides a second time
OPT_COEF = 0.37
OPT_RTOL, OPT_ATOL = 2e-5, 2e-6                      # the suite's bar on parameters: no bar here may be looser


def opt_case(n, seed=0):
    """(p, g, m, v) float32: v >= m^2 as the moments of one gradient stream have it; gradients and moments are exactly 0
    (a tenth of them) or at least 1e-6 in magnitude."""
    rng = np.random.default_rng(4242 + seed + n % 9973)
    r = lambda: rng.standard_normal(n).astype(np.float32)
    snap = lambda x: np.where(np.abs(x) < 1e-6, np.float32(0), x).astype(np.float32)
    p, g, m = r(), snap(r()), snap(np.float32(0.1) * r())
    g[rng.random(n) < 0.1] = 0
    m[rng.random(n) < 0.1] = 0
    v = (m * m + (np.float32(0.1) * r()) ** 2).astype(np.float32)
    small = (v < 1e-6) | ((rng.random(n) < 0.1) & (m == 0))
    v[small], m[small] = 0, 0
    return p, g, m, v


def opt_state_reference(t):
    """state[0..2] after the step that makes the count ``t``, with bars: pow() within a few ulp of float64 and one
    subtraction (8 ulp of the two terms 1 and beta^t)."""
    s = [float(t), 1.0 - B1 ** t, 1.0 - B2 ** t]
    return s, [0.0, 8 * D52 * (1 + B1 ** t), 8 * D52 * (1 + B2 ** t)]


def opt_reference(p, g, m, v, kind, wd, coef, t, lr=LR):
    """One update in float64 (optim_oracle) -> (p, m, v, p_bar, m_bar, v_bar).  ``wd`` and ``coef`` as float32 values."""
    p64, g64, m64, v64 = (x.astype(np.float64) for x in (p, g, m, v))
    gs = np.abs(g64 * coef)
    if kind == 2:
        pn = optim_oracle.sgd_step(p, g, lr, coef)
        return pn, m64, v64, 16 * U * (np.abs(p64) + lr * gs) + TINY, np.zeros_like(p64), np.zeros_like(p64)
    pn, mn, vn = optim_oracle.adamw_step(p, g, m, v, t, lr, B1, B2, OPT_EPS, wd, decoupled=kind == 0, grad_scale=coef)
    if kind == 1 and wd != 0.0:
        gs = gs + np.abs(wd * p64)                           # the L2 term joins the gradient
    mt = np.abs(m64) + (1.0 - B1) * (gs + np.abs(m64))       # m + (g - m)(1 - b1): three terms
    vt = np.abs(v64) * B2 + (1.0 - B2) * gs * gs
    denom = np.sqrt(vn) / np.sqrt(1.0 - B2 ** t) + OPT_EPS
    step = lr / (1.0 - B1 ** t)
    # p (1 - lr wd) - step m' / denom: p, its decay, and the update, whose numerator m' is itself the three terms above
    pt = np.abs(p64) + (lr * wd * np.abs(p64) if kind == 0 else 0.0) + step * mt / denom
    return pn, mn, vn, 16 * U * pt + TINY, 16 * U * mt + TINY, 16 * U * vt + TINY


def opt_f32(p, g, m, v, kind, wd, coef, t, lr=LR):
    """adam_elem / the SGD line elementwise in float32 numpy."""
    f = np.float32
    lr_, b1, b2, e, wd_, c = f(lr), f(B1), f(B2), f(OPT_EPS), f(wd), f(coef)
    g = g * c
    if kind == 2:
        return p - lr_ * g, m, v
    step = f(lr / (1.0 - B1 ** t))
    isb = f(1.0 / np.sqrt(1.0 - B2 ** t))
    if kind == 0:
        p = p * (f(1) - lr_ * wd_)
    elif wd != 0.0:
        g = g + wd_ * p
    m = m + (g - m) * (f(1) - b1)
    v = v * b2 + (f(1) - b2) * g * g
    p = p - step * (m / (np.sqrt(v) * isb + e))
    assert p.dtype == np.float32
    return p, m, v


# ================================================================================================================ metrics
METRIC_PIXELS = (1, 63, 1023, 1025, 5000)
METRIC_KINDS = ('empty', 'gt_le_eps', 'pred_le_0', 'fallback', 'metres', 'normalised', 'negative_gt', 'eps2_mode0',
                'eps2_mode1')
METRIC_BRANCH = {'empty': 'empty', 'gt_le_eps': 'gt_le_eps', 'pred_le_0': 'pred_le_0', 'fallback': 'fallback',
                 'metres': 'normal', 'normalised': 'normal', 'negative_gt': 'normal', 'eps2_mode0': 'normal',
                 'eps2_mode1': 'fallback'}
METRIC_RTOL, METRIC_ATOL = 2e-5, 1e-6
NEAR = 1e-5
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
EPSILONS = (1e-3, 1e-6)


def metric_kinds(pixels):
    """The kinds a sample of ``pixels`` pixels can be: the eps2 kinds and a negative gt beside a kept one need two."""
    if pixels >= 2:
        return METRIC_KINDS
    return tuple(k for k in METRIC_KINDS if not k.startswith('eps2') and k != 'negative_gt')


def near_decision(gt, pred):
    """Pixels on which float32 rounding could decide otherwise than exact arithmetic: gt or pred within 1e-5 (relative) of
    an epsilon, or max(g/p, p/g) within 1e-5 of a power of 1.25 (with pred clamped at either epsilon)."""
    g, p = gt.astype(np.float64), pred.astype(np.float64)
    bad = np.zeros(g.shape, bool)
    for e in EPSILONS:
        bad |= (np.abs(g - e) <= NEAR * e) | (np.abs(p - e) <= NEAR * e)
    with np.errstate(divide='ignore', invalid='ignore'):
        for e in EPSILONS:
            pc = np.maximum(p, e)
            th = np.maximum(g / pc, pc / g)
            for c in THRESHOLDS:
                bad |= (g > 0) & (np.abs(th - c) <= NEAR * c)
    return bad


def _draw_metric(kind, n, rng):
    f = np.float32
    uni = lambda a, b: rng.uniform(a, b, n).astype(f)
    if kind == 'empty':
        return np.zeros(n, f), uni(0.1, 30.0)
    if kind == 'gt_le_eps':                        # max gt <= 1 -> eps 1e-6, and no gt above it
        return uni(1e-8, 5e-7), uni(0.1, 1.0)
    if kind == 'pred_le_0':
        p = -uni(0.0, 5.0)
        p[rng.random(n) < 0.3] = 0.0
        return uni(0.5, 30.0) if n > 1 else np.array([7.5], f), p
    if kind == 'fallback':                         # gt in metres -> eps 1e-3; every pred in (0, eps): keep = gt > eps & pred > 0
        g = uni(1.5, 30.0)
        p = uni(1e-5, 9e-4)
        if n > 2:
            p[rng.random(n) < 0.2] = -1.0
            p[0] = 5e-4
        return g, p
    if kind in ('metres', 'normalised', 'negative_gt'):
        g = uni(0.5, 30.0) if kind != 'normalised' else uni(0.02, 1.0)
        p = (g * np.exp(rng.normal(0.0, 0.3, n))).astype(f)
        if n > 4:
            g[rng.random(n) < 0.15] = 0.0
            p[rng.random(n) < 0.05] = 0.0
            p[rng.random(n) < 0.05] = -0.5
            g[0], p[0] = (20.0, 21.0) if kind != 'normalised' else (0.5, 0.55)
        if kind == 'negative_gt':
            g[rng.random(n) < 0.2] *= -1.0
            g[n - 1] = -3.0
            if n > 1:
                g[0] = 20.0
        return g, p
    if kind == 'eps2_mode0':     # the only gt above 1 sits where pred is dropped: eps 1e-3, eps2 1e-6, pred > eps kept
        g = uni(0.02, 1.0)
        p = (g * np.exp(rng.normal(0.0, 0.3, n))).astype(f)
        g[n - 1], p[n - 1] = 5.0, 0.0
        return g, p
    if kind == 'eps2_mode1':     # the same, no pred above eps: fallback, and pred (1e-5 .. 9e-4) is clamped at eps2 = 1e-6
        g = uni(0.02, 1.0)
        p = uni(1e-5, 9e-4)
        g[n - 1], p[n - 1] = 5.0, -1.0
        return g, p
    raise ValueError(kind)


def metric_sample(kind, pixels, seed=0):
    """(gt, pred) float32 [pixels] of one kind; pixels near a decision are redrawn (judged by the reference alone)."""
    rng = np.random.default_rng(31 * seed + 7 * METRIC_KINDS.index(kind) + pixels)
    g, p = _draw_metric(kind, pixels, rng)
    for _ in range(20):
        bad = near_decision(g, p)
        if not bad.any():
            break
        g2, p2 = _draw_metric(kind, pixels, rng)
        fixed = np.zeros(pixels, bool)             # the hand-placed pixels stay
        fixed[[0, pixels - 1]] = True
        take = bad & ~fixed
        g[take], p[take] = g2[take], p2[take]
    return g, p


def metric_batch(pixels, seed=0):
    """-> (kinds, gt [S, pixels], pred [S, pixels]): one sample of every kind ``pixels`` allows."""
    kinds = metric_kinds(pixels)
    gp = [metric_sample(k, pixels, seed) for k in kinds]
    return kinds, np.stack([x[0] for x in gp]), np.stack([x[1] for x in gp])


def metric_reference(gt, pred):
    """metrics_oracle.compute_errors of one sample (float32 numpy by construction) and how it went."""
    out, info = metrics_oracle.compute_errors_traced(gt, pred)
    return np.array([float(x) for x in out], dtype=np.float64), info


# ============================================================================================================== edge loss
EDGE_SHAPES = ((1, 1, 1), (2, 1, 7), (2, 7, 1), (3, 2, 2), (3, 5, 7), (2, 40, 56), (1, 363, 363))
EDGE_LAMBDAS = ((f32r(1.0), f32r(0.2), f32r(0.1)), (f32r(0.3), f32r(1.7), f32r(0.9)))
EDGE_EPS = f32r(1e-6)
EDGE_PATCHED = 5 * 7             # from this many pixels per image on, every patch below is non-empty
EDGE_INTERIOR = 40 * 56          # ... and has pixels whose whole 3x3 neighbourhood lies inside it


def _rect(H, W, y0, y1, x0, x1):
    return slice(int(H * y0), max(int(H * y1), int(H * y0) + (H >= 5))), slice(int(W * x0), max(int(W * x1), int(W * x0) + (W >= 5)))


def edge_case(B, H, W, seed=0):
    """(pred, gt) float32 [B, 1, H, W], multiples of 1/4 in [0, 32) (gt: one patch of -1/4 multiples).  Per image: two zero
    gt patches, a negative gt patch, a patch where pred == gt (a ramp of 1/4 per two columns: Sobel magnitude 1), a patch
    where both are constant.  Images too small for patches get zero / negative gt on single pixels by chance."""
    rng = np.random.default_rng(808 + seed + 131 * B + 17 * H + W)
    pred = rng.integers(0, 128, (B, 1, H, W)).astype(np.float64)
    gt = rng.integers(1, 128, (B, 1, H, W)).astype(np.float64)
    r = rng.random((B, 1, H, W))
    gt = np.where(r < 0.1, 0, np.where(r < 0.15, -gt, gt))
    if H * W >= EDGE_PATCHED:
        ys, xs = _rect(H, W, 0.0, 0.3, 0.0, 0.3)
        gt[:, :, ys, xs] = 0
        ys, xs = _rect(H, W, 0.7, 1.0, 0.5, 0.8)
        gt[:, :, ys, xs] = 0
        ys, xs = _rect(H, W, 0.0, 0.3, 0.6, 1.0)
        gt[:, :, ys, xs] = -np.abs(gt[:, :, ys, xs]) - 1
        ys, xs = _rect(H, W, 0.35, 0.65, 0.0, 0.45)
        ramp = 40 + ((np.arange(W) // 2) % 80)[None, None, None, :] + np.zeros((B, 1, H, W))
        gt[:, :, ys, xs] = ramp[:, :, ys, xs]
        pred[:, :, ys, xs] = gt[:, :, ys, xs]
        ys, xs = _rect(H, W, 0.35, 0.65, 0.55, 1.0)
        gt[:, :, ys, xs] = 36
        pred[:, :, ys, xs] = 20
    return (pred / 4.0).astype(np.float32), (gt / 4.0).astype(np.float32)


def _sobel_np(x):
    x = torch.from_numpy(np.ascontiguousarray(x))
    sx, sy = edge_loss_oracle._sobel(x)
    return sx.numpy(), sy.numpy()


def edge_reference(pred, gt, lambdas, eps=EDGE_EPS):
    """Float64 autograd of edge_loss_oracle.edge_loss on the float32 inputs.
    -> dict(terms[4], terms_bar, stats[5], stats_bar, grad, grad_bar, radicand_gap)."""
    lr, le, ls = lambdas
    p = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    g = torch.from_numpy(gt.astype(np.float64))
    total, (recon, edge, smooth) = edge_loss_oracle.edge_loss(p, g, lr, le, ls, eps)
    total.backward()
    grad = p.grad.numpy()
    stats = [float(s) for s in edge_loss_oracle.edge_sums(p.detach(), g, eps)]
    terms = [float(x.detach()) for x in (recon, edge, smooth, total)]

    p64, g64 = pred.astype(np.float64), gt.astype(np.float64)
    n = pred.size
    v = (g64 > 0).astype(np.float64)
    ve = torch.nn.functional.max_pool2d(torch.from_numpy(v), 3, 1, 1).numpy()
    px, py = _sobel_np(p64)
    gx, gy = _sobel_np(g64)
    rp, rg = px * px + py * py, gx * gx + gy * gy
    pm, gm = np.sqrt(rp + eps), np.sqrt(rg + eps)
    gap = np.abs(rp - rg)[ve > 0]
    gap = float(gap[gap > 0].min()) if (gap > 0).any() else float('inf')
    sm = (np.abs(px) + np.abs(py)) * np.exp(-gm) * v
    # stats[1]: exact terms.  stats[3]: each magnitude is a rounded radicand (u) under a rounded sqrt (u, halved and one
    # more): within 2u of itself, twice for the difference.  stats[4]: exp(-gmag) turns the 2u of gmag into 2u gmag, expf
    # and the two products add a few u; a result below the smallest normal float32 (2^-126) may be flushed, times <= 256.
    bar = [0.0, n * D52 * stats[1], 0.0,
           4 * U * _sums(ve * (pm + gm)) + n * D52 * stats[3],
           8 * U * _sums((1 + gm) * sm) + n * 256 * 2.0 ** -126 + n * D52 * stats[4]]
    N, ND = stats[0], stats[2]
    q = [stats[1] / (N + 1e-6) if N > 0 else 0.0, stats[3] / (ND + 1e-6) if ND > 0 else 0.0,
         stats[4] / (N + 1e-6) if N > 0 else 0.0]
    qbar = [bar[1] / (N + 1e-6) if N > 0 else 0.0, bar[3] / (ND + 1e-6) if ND > 0 else 0.0,
            bar[4] / (N + 1e-6) if N > 0 else 0.0]
    tbar = [qbar[i] + 2 * D52 * abs(q[i]) + U * abs(q[i]) + TINY for i in range(3)]       # quotient, then the cast
    tbar.append(lr * qbar[0] + le * qbar[1] + ls * qbar[2] + U * abs(terms[3]) + TINY)

    # gradient: c_R sign(p - g) + sum over the 3x3 neighbours q of fx(q) kx + fy(q) ky, fx = a sx / pmag + b sign(sx)
    cR = lr / (N + 1e-6) if N > 0 else 0.0
    cE = le / (ND + 1e-6) if ND > 0 else 0.0
    cS = ls / (N + 1e-6) if N > 0 else 0.0
    a = cE * ve * np.abs(np.sign(pm * ve - gm * ve))
    b = cS * np.exp(-gm) * v
    fx = a * np.abs(px) / pm + b * np.abs(np.sign(px))
    fy = a * np.abs(py) / pm + b * np.abs(np.sign(py))
    ak = torch.tensor([[1, 0, 1], [2, 0, 2], [1, 0, 1]], dtype=torch.float64).view(1, 1, 3, 3)
    conv = lambda x, k: torch.nn.functional.conv2d(torch.from_numpy(x), k, padding=1).numpy()
    T = cR * v * np.abs(np.sign(p64 - g64)) + conv(fx, ak) + conv(fy, ak.transpose(2, 3).contiguous())
    return dict(terms=terms, terms_bar=tbar, stats=stats, stats_bar=bar, grad=grad, grad_bar=16 * U * T + TINY,
                radicand_gap=gap, n_equal=int(((rp == rg) & (ve > 0)).sum()))


def edge_f32(pred, gt, lambdas, eps=EDGE_EPS):
    """The same loss in float32 torch autograd (elementwise float32), the five sums taken in float64.
    -> (terms[4] before their cast to float32, stats[5], grad)."""
    f = np.float32
    p = torch.from_numpy(pred.copy()).requires_grad_(True)
    g = torch.from_numpy(gt.copy())
    valid = (g > 0).float()
    px, py = edge_loss_oracle._sobel(p)
    gx, gy = edge_loss_oracle._sobel(g)
    pm = torch.sqrt(px * px + py * py + f(eps))
    gm = torch.sqrt(gx * gx + gy * gy + f(eps))
    dil = torch.nn.functional.max_pool2d(valid, 3, 1, 1)
    s = [valid.double().sum(), ((p - g).abs() * valid).double().sum(), dil.double().sum(),
         ((pm * dil - gm * dil).abs()).double().sum(), ((px.abs() + py.abs()) * torch.exp(-gm) * valid).double().sum()]
    N, ND = float(s[0]), float(s[2])
    zero = s[1] * 0
    recon = s[1] / (N + 1e-6) if N > 0 else zero
    edge = s[3] / (ND + 1e-6) if ND > 0 else zero
    smooth = s[4] / (N + 1e-6) if N > 0 else zero
    total = lambdas[0] * recon + lambdas[1] * edge + lambdas[2] * smooth
    if total.requires_grad:
        total.backward()
    grad = p.grad.numpy() if p.grad is not None else np.zeros_like(pred)
    return [float(x.detach()) for x in (recon, edge, smooth, total)], [float(x.detach()) for x in s], grad
