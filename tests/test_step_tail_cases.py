"""The cases and references of tests/test_gpu_step_tail.py, checked on the CPU with the references alone: every generator
meets the conditions the GPU tests rely on (float32 and float64 decide alike, no redrawn sample left, margins), every named
case reaches the branch it is named for, and a float32 restatement of each kernel formula sits inside each error bar with at
least 4x room -- a bar that this file cannot hold is a wrong bar, not a wrong kernel."""
import numpy as np
import pytest

import step_tail_cases as sc
from oracle import loss_oracle

ROOM = 4.0


def _inside(got, ref, bar, what, room=ROOM):
    got, ref, bar = (np.asarray(x, dtype=np.float64) for x in (got, ref, bar))
    err = np.abs(got - ref)
    worst = float(np.max(err * room - bar))
    assert worst <= 0.0, (what, float(np.max(err / np.maximum(bar, 1e-300))))


def _f32_exact(x64):
    return bool((x64.astype(np.float32).astype(np.float64) == x64).all())


# =========================================================================================================== masked loss
@pytest.mark.parametrize('scale', sc.SCALES)
@pytest.mark.parametrize('n', sc.LOSS_N + (sc.LOSS_N_FINISH_CAP,))
def test_loss_inputs_decide_alike_in_float32_and_float64(n, scale):
    pred, gt = sc.loss_case(n, scale)
    p64, g64 = pred.astype(np.float64), gt.astype(np.float64)
    dyadic = (p64 * 64 == np.round(p64 * 64))
    assert (g64 * 64 == np.round(g64 * 64)).all()
    assert (~dyadic).sum() == (2 if scale == 1.0 and n >= 8 else 0)          # the two eps pixels
    lo, hi = (-2, 30) if scale == 1.0 else (-0.25, 1)
    assert lo < p64.min() and p64.max() < hi and lo < g64.min() and g64.max() < hi
    assert _f32_exact(p64 * scale) and _f32_exact(g64 * scale)             # p * scale, g * scale: no rounding
    assert _f32_exact((p64 * scale - g64 * scale)[dyadic])                   # p - g neither
    if n >= 8:
        assert (gt < 0).any() and (gt == 0).any() and (pred <= 0).any() and (pred < 0).any()
        assert ((pred == gt) & (gt > 0)).any()
    if n >= 257:
        assert 0.02 < (gt < 0).mean() < 0.09 and 0.06 < (gt == 0).mean() < 0.15
    if scale == 1.0 and n >= 8:
        e = np.float32(sc.EPS)
        assert pred[1] == e and pred[n - 2] < e and np.nextafter(pred[n - 2], np.float32(1)) == e
        assert gt[1] > 0 and gt[n - 2] > 0
        assert float(pred[1]) >= sc.EPS > float(pred[n - 2])                 # the float64 gate decides as the float32 one
    # Sum |p - g| on the dyadic pixels: float32 reproduces it exactly
    d32 = np.abs(pred * np.float32(scale) - gt * np.float32(scale))[dyadic].astype(np.float64)
    assert d32.sum() == np.abs(p64 * scale - g64 * scale)[dyadic].sum()


def _loss_configs():
    for n in sc.LOSS_N:
        for scale in sc.SCALES:
            for mode in (0, 1, 2):
                for crit in (0, 1, 2, 4):
                    yield n, scale, mode, crit


def test_loss_bars_hold_the_float32_restatement_with_room():
    worst_rel = 0.0
    for n, scale, mode, crit in _loss_configs():
        pred, gt = sc.loss_case(n, scale)
        m = mode | (4 if crit == 4 else 0)
        for fa in (None, 0, 1, 2) if crit != 4 else (None,):
            ref = sc.loss_reference(pred, gt, scale, m, crit, fa)
            stats, loss, grad, bias = sc.loss_f32(pred, gt, scale, m, crit, fa)
            what = (n, scale, mode, crit, fa)
            assert stats[0] == ref['stats'][0] == float(loss_oracle.valid_mask(gt, sc.MASK_NAME[mode]).sum()), what
            assert ref['n_inexact'] <= 2 and (scale == 1.0 or ref['n_inexact'] == 0), what
            for k in (1, 2, 3):
                _inside(stats[k], ref['stats'][k], ref['stats_bar'][k], what + ('stat', k))
            if ref['N'] == 0:
                assert np.isnan(loss) and np.isnan(ref['loss']) and not grad.any() and not ref['grad'].any(), what
                continue
            if crit in (1, 2):
                assert ref['var'] > 100 * ref['var_bar'], what               # var > 0 is no close call
            _inside(loss, ref['loss'], ref['loss_bar'], what + ('loss',))
            assert ref['loss_bar'] <= 1e-5 * abs(ref['loss']) + 1e-12, what  # no looser than the suite's bar on the loss
            worst_rel = max(worst_rel, ref['loss_bar'] / max(abs(ref['loss']), 1e-300))
            _inside(grad, ref['grad'], ref['grad_bar'], what + ('grad',))
            if fa is not None:
                _inside(bias, ref['bias'], ref['bias_bar'], what + ('bias',))
    assert 0 < worst_rel <= 1e-5


@pytest.mark.parametrize('n', (sc.LOSS_N_FINISH_CAP, sc.LOSS_N_RED_CAP))
def test_loss_bars_hold_at_the_large_sizes(n):
    pred, gt = sc.loss_case(n, 1.0)
    ref = sc.loss_reference(pred, gt, 1.0, 0, 2, 0)
    stats, loss, grad, bias = sc.loss_f32(pred, gt, 1.0, 0, 2, 0)
    assert stats[0] == ref['stats'][0]
    for k in (1, 2, 3):
        _inside(stats[k], ref['stats'][k], ref['stats_bar'][k], ('stat', k))
    _inside(loss, ref['loss'], ref['loss_bar'], 'loss')
    assert ref['loss_bar'] <= 1e-5 * abs(ref['loss'])
    _inside(grad, ref['grad'], ref['grad_bar'], 'grad')
    _inside(bias, ref['bias'], ref['bias_bar'], 'bias')


def test_loss_named_cases_reach_their_branches():
    for mode in (0, 1):                                              # empty mask
        pred, gt = sc.empty_mask_case(257, mode)
        ref = sc.loss_reference(pred, gt, 1.0, mode, 2)
        assert ref['N'] == 0 and np.isnan(ref['loss']) and not ref['grad'].any()
    pred, gt = sc.empty_mask_case(257, 1)                            # modes 0 and 1 part on negative gt
    n0 = sc.loss_reference(pred, gt, 1.0, 0, 2)['N']
    assert n0 == float((gt < 0).sum()) > 0
    pred, gt = sc.loss_case(257, 1.0)
    N = [sc.loss_reference(pred, gt, 1.0, m, 2)['N'] for m in (0, 1, 2)]
    assert N[1] < N[0] < N[2] == 257 and N[0] - N[1] == float((gt < 0).sum())
    lam1 = 1.0
    for name, (pred, gt) in sc.var0_cases().items():                 # var <= 0, in float64 and in float32
        for crit in (1, 2):
            ref = sc.loss_reference(pred, gt, 1.0, 0, crit, lam=lam1)
            stats, loss, grad, _ = sc.loss_f32(pred, gt, 1.0, 0, crit, lam=lam1)
            assert ref['N'] >= 2 and ref['var'] == 0.0, (name, ref['var'])
            assert stats[3] / stats[0] - lam1 * (stats[2] / stats[0]) ** 2 == 0.0, name
            want = sc.L1W * ref['stats'][1] / ref['N'] if crit == 2 else 0.0
            assert abs(ref['loss'] - want) <= 1e-15 and abs(loss - want) <= 1e-15
            l1_only = sc.loss_reference(pred, gt, 1.0, 0, 0)['grad'] * (sc.L1W if crit == 2 else 0.0)
            assert np.array_equal(ref['grad'], l1_only) and np.array_equal(grad.astype(np.float64) != 0, l1_only != 0)
        if name == 'two_px':
            assert ref['stats'][2] != 0.0 and l1_only.any()           # d is not zero: lambda = 1 alone makes var vanish
        else:
            assert not l1_only.any()                                  # pred == gt: the sign-0 branch, no gradient at all
    # the gate p >= eps: the pixel AT eps carries a SIlog gradient, the one just below it only the L1 one
    pred, gt = sc.loss_case(63, 1.0)
    g1 = sc.loss_reference(pred, gt, 1.0, 0, 1)['grad']
    assert g1[1] != 0.0 and g1[61] == 0.0 and g1[4] == 0.0 and g1[5] == 0.0 and g1[0] != 0.0
    g0 = sc.loss_reference(pred, gt, 1.0, 0, 0)['grad']
    assert g0[0] == 0.0 and g0[61] < 0.0 and g0[3] == 0.0 and g0[2] != 0.0
    assert sc.loss_reference(pred, gt, 1.0, 1, 0)['grad'][2] == 0.0   # negative gt: valid in mode 0 only


def test_final_act_and_sum_references():
    for n in sc.FINAL_ACT_N[:2] + (4099,):
        gout, out = sc.final_act_case(n)
        assert (out == 0).any() or n == 1
        for kind in (0, 1, 2):
            ref64, ref32 = sc.final_act_reference(gout, out, kind)
            f = loss_oracle.final_act_factor(out, kind)
            assert _f32_exact(f)                                     # act' itself is exact in float32 ...
            got = gout * sc._act_f32(out, kind)
            assert got.dtype == np.float32 and np.array_equal(got, ref32)          # ... so float32 gives THE rounding
            _inside(got, ref64, 16 * sc.U * np.abs(ref64) + sc.TINY, ('final_act', n, kind))
    for n in sc.SUM_N:
        x = sc.sum_case(n)
        s, bar = sc.sum_reference(x)
        got = float(np.sum(x[::-1].astype(np.float64)))                            # another order
        _inside(got, s, bar, ('sum', n))
        xb = x.view(np.uint32) & np.uint32(0xFFFF0000)                            # bf16 values are float32 values
        assert _f32_exact(xb.view(np.float32).astype(np.float64))


# ================================================================================================= gradient norm and clip
@pytest.mark.parametrize('n', sc.NORM_N)
def test_norm_cases_are_exact_in_float32_and_clip_as_named(n):
    g = sc.norm_case(n)
    g64 = g.astype(np.float64)
    assert (g64 * 1024 == np.round(g64 * 1024)).all() and np.abs(g64).max() < 2
    sq32 = g * g
    assert np.array_equal(sq32.astype(np.float64), g64 * g64)                     # g^2 exact in float32
    if n >= 2:
        pair = sq32[0:n - n % 2:2] + sq32[1:n - n % 2 + 1:2]
        assert np.array_equal(pair.astype(np.float64), (g64 * g64)[0:n - n % 2:2] + (g64 * g64)[1:n - n % 2 + 1:2])
    total, _, tbar, _ = sc.norm_reference(g, [(0, n)], (), 1.0)
    assert total > 0
    clip, free = sc.max_norms(total)
    t1, c1, _, cb1 = sc.norm_reference(g, [(0, n)], (), clip)
    t2, c2, _, cb2 = sc.norm_reference(g, [(0, n)], (), free)
    assert abs(c1 - 0.5) < 1e-6 and c2 == 1.0 and free / (t2 + 1e-6) > 1.9        # coef < 1, and coef == 1 by the clamp
    assert tbar <= 1e-5 * total and cb1 <= 1e-5 * c1                              # no looser than the suite's 1e-5 on the norm
    rows = sc.split_rows(n - n % 4)
    assert all(o % 4 == 0 and 0 < ln <= sc.ROW_MAX and ln % 4 == 0 for o, ln in rows)
    assert sum(ln for _, ln in rows) == n - n % 4
    # the routes agree in the reference itself
    t3, _, _, _ = sc.norm_reference(g, rows, [float((g64[n - n % 4:] ** 2).sum())], clip)
    assert abs(t3 - t1) <= 4 * tbar


# ============================================================================================================== optimizer
def test_opt_cases_and_bars():
    for n in sc.OPT_N + (1024 * 1024 + 3,):                  # the GPU test's sizes (its largest: AdamW alone, as here)
        p, g, m, v = sc.opt_case(n)
        for x in (g, m, v):
            assert ((x == 0) | (np.abs(x) >= 1e-6)).all()
        assert (v >= 0).all() and (v.astype(np.float64) >= 0.99 * m.astype(np.float64) ** 2).all()
        if n >= 1027:
            assert (g == 0).any() and (m == 0).any() and (v == 0).any()
        for kind, wd in sc.OPT_KINDS if n in sc.OPT_N else ((0, 0.01),):
            for coef in (sc.f32r(sc.OPT_COEF), 1.0):
                for t in (1, 2, 1000):
                    pr, mr, vr, pb, mb, vb = sc.opt_reference(p, g, m, v, kind, sc.f32r(wd), coef, t)
                    pf, mf, vf = sc.opt_f32(p, g, m, v, kind, sc.f32r(wd), coef, t)
                    what = (n, kind, wd, coef, t)
                    _inside(pf, pr, pb, what + ('p',))
                    assert (pb <= sc.OPT_ATOL + sc.OPT_RTOL * np.abs(pr)).all(), what      # never looser than the suite's
                    if kind != 2:
                        _inside(mf, mr, mb, what + ('m',))
                        _inside(vf, vr, vb, what + ('v',))
                        assert (mb <= sc.OPT_ATOL + sc.OPT_RTOL * np.abs(mr)).all(), what
                        assert (vb <= sc.OPT_ATOL + sc.OPT_RTOL * np.abs(vr)).all(), what
    for t in (1, 2, 1000):
        s, b = sc.opt_state_reference(t)
        assert s[0] == t and 0 < s[1] <= 1 and 0 < s[2] <= 1 and max(b) < 1e-14


def test_opt_three_steps_chain_in_the_reference():
    """Three reference steps fed their own float32-rounded results stay inside the bars of the float32 restatement: the
    GPU test chains the kernel's outputs the same way (each step is judged from the kernel's own previous state)."""
    p, g, m, v = sc.opt_case(5)
    for t in (1, 2, 3):
        pr, mr, vr, pb, mb, vb = sc.opt_reference(p, g, m, v, 0, sc.f32r(0.01), 1.0, t)
        pf, mf, vf = sc.opt_f32(p, g, m, v, 0, sc.f32r(0.01), 1.0, t)
        _inside(pf, pr, pb, ('chain', t))
        p, m, v = pf, mf, vf


# ================================================================================================================ metrics
@pytest.mark.parametrize('pixels', sc.METRIC_PIXELS)
def test_metric_samples_reach_their_branches_with_nothing_near_a_decision(pixels):
    kinds, gt, pred = sc.metric_batch(pixels)
    assert len(kinds) >= (8 if pixels >= 2 else 6) and len(set(kinds)) == len(kinds)
    for k, g, p in zip(kinds, gt, pred):
        assert g.dtype == np.float32 and p.dtype == np.float32
        assert not sc.near_decision(g, p).any(), k                                 # no redrawn sample left
        out, info = sc.metric_reference(g, p)
        assert info['branch'] == sc.METRIC_BRANCH[k], (k, info['branch'])
        if k in ('empty', 'gt_le_eps'):
            assert not out.any()
        if k == 'empty':
            assert not g.any()
        if k == 'gt_le_eps':
            assert g.any() and info['eps'] == 1e-6
        if k == 'pred_le_0':
            assert list(out) == [1.0, float(g.max()), 0.0, 0.0, 0.0, 1.0, float(g.max())] and (p <= 0).all()
        if k == 'fallback':
            assert info['eps'] == info['eps2'] == 1e-3 and info['kept'] > 0 and (p <= 1e-3).all()
        if k == 'metres':
            assert info['eps'] == info['eps2'] == 1e-3 and out[2] > 0
        if k == 'normalised':
            assert info['eps'] == info['eps2'] == 1e-6 and out[2] > 0
        if k == 'negative_gt':
            assert (g < 0).any() and (g > 0).any() and info['kept'] > 0
        if k.startswith('eps2'):
            assert info['eps'] == 1e-3 and info['eps2'] == 1e-6 and info['kept'] == pixels - 1
        if k == 'eps2_mode1':                                                      # here the second epsilon changes log_10
            g2 = g.copy()
            g2[0] = 4.0                                                            # a kept gt above 1: eps2 = eps = 1e-3
            out2, info2 = sc.metric_reference(g2, p)
            assert info2['eps2'] == 1e-3 and info2['branch'] == 'fallback'
            pk, gk = info['p'].astype(np.float64), info['g'].astype(np.float64)
            with_eps1 = np.abs(np.log10(gk) - np.log10(np.maximum(pk, 1e-3))).mean()
            assert abs(with_eps1 - out[5]) > 100 * (sc.METRIC_RTOL * out[5] + sc.METRIC_ATOL)
        if info['branch'] in ('normal', 'fallback') and pixels >= 63 and k in ('metres', 'normalised', 'negative_gt'):
            assert 0 < out[2] < out[4] <= 1                                        # the a's discriminate


# ============================================================================================================== edge loss
@pytest.mark.parametrize('shape', sc.EDGE_SHAPES)
def test_edge_cases_margins_and_bars(shape):
    B, H, W = shape
    pred, gt = sc.edge_case(B, H, W)
    for x in (pred, gt):
        x64 = x.astype(np.float64)
        assert (x64 * 4 == np.round(x64 * 4)).all() and np.abs(x64).max() <= 32
    assert pred.min() >= 0
    if H * W >= sc.EDGE_PATCHED:
        assert (gt == 0).any() and (gt < 0).any() and ((pred == gt) & (gt > 0)).any()
    for lam in sc.EDGE_LAMBDAS:
        ref = sc.edge_reference(pred, gt, lam)
        assert ref['radicand_gap'] >= 1.0 / 16                        # unequal radicands are far apart: the sign is safe
        if H * W >= sc.EDGE_INTERIOR:
            assert ref['n_equal'] >= 2 * B                            # and equal ones exist: the sign-0 branch
        terms, stats, grad = sc.edge_f32(pred, gt, lam)
        assert stats[0] == ref['stats'][0] == float((gt > 0).sum()) and stats[2] == ref['stats'][2]
        for k in (1, 3, 4):
            _inside(stats[k], ref['stats'][k], ref['stats_bar'][k], (shape, 'stat', k))
        for k in range(4):
            _inside(terms[k], ref['terms'][k], ref['terms_bar'][k], (shape, 'term', k))
        _inside(grad, ref['grad'], ref['grad_bar'], (shape, 'grad'))
    ref = sc.edge_reference(pred, -np.abs(gt), sc.EDGE_LAMBDAS[0])    # all invalid
    assert ref['terms'] == [0.0] * 4 and not ref['grad'].any() and ref['stats'][0] == 0 and ref['stats'][2] == 0
