"""The kernels every training step ends in -- csrc/loss_optim.hip (masked loss and its gradient, final-activation
backward, scalar sum, gradient norm and clip coefficient, optimizer step with the bf16 mirror), metrics.hip
(compute_errors) and edgeloss.hip -- through the C ABI (kernels.py) against float64, at the sizes where their launch code
changes path: one thread, part of a block, a second block, the n & 3 tails, one element past every grid cap.

Cases, references and error bars: tests/step_tail_cases.py (its docstring has the bar formulas and their reasons;
tests/test_step_tail_cases.py holds each of them on the CPU with 4x room).  Inputs are drawn so that float32 and float64
decide alike (validity, signs, clamps, thresholds), every comparison keeps every element, and the deliberate corner
behaviours are pinned by name: empty mask -> NaN loss and zero gradient; var <= 0 -> SIlog 0 with zero gradient; all-invalid
edge loss -> zero terms; compute_errors without a valid pixel -> seven zeros.

Measured on an MI355X, the largest error as a fraction of its bar over all cases: loss statistics 0.27, loss gradient and
dz 0.33, bias gradient 0.10, optimizer p / m / v 0.21 / 0.15 / 0.26, edge-loss sums, terms and gradient at most 0.65, the
gradient norm and clip coefficient below 0.001.  The scalar outputs that end in a cast to float32 (loss value, edge terms,
scalar sum) come as close as 0.85: their bar is mostly that one rounding, u |value|, which a cast can use up.  The module
prints these figures when run with -s.
"""
import functools

import numpy as np
import pytest
import torch

import step_tail_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
PAD = 8                      # guard elements after every output
GUARD = -7.25


def K():
    from audio_depth_estimation_amd import kernels
    return kernels


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().double().cpu().numpy()


_worst = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    """After the module: the largest error met per quantity, as a fraction of its bar (shown with -s)."""
    yield
    print('\nworst error / bar: ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(_worst.items())))


def within(got, ref, bar, what):
    """|got - ref| <= bar on EVERY element; the bar is the case's own formula (step_tail_cases)."""
    got, ref, bar = (np.asarray(x, dtype=np.float64) for x in (got, ref, bar))
    assert got.shape == ref.shape, what
    err = np.abs(got - ref)
    ok = err <= bar
    key = ' '.join(str(w) for w in what if isinstance(w, str)) or 'other'
    _worst[key] = max(_worst.get(key, 0.0), float(np.max(np.where(bar > 0, err / np.maximum(bar, 1e-300), 0.0))))
    assert ok.all(), (what, 'worst error / bar', float(np.max(err / np.maximum(bar, 1e-300))), 'at', int(np.argmax(err - bar)))


def guarded(n, dtype=F32, fill=GUARD):
    """(buffer of n + PAD elements filled with a guard value, the view of its first n)."""
    buf = torch.full((n + PAD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def guard_intact(buf, n, fill=GUARD):
    return bool((buf[n:] == fill).all())


# =========================================================================================================== masked loss
@functools.lru_cache(maxsize=None)
def _loss_inputs(n, scale):
    pred, gt = sc.loss_case(n, scale)
    return pred, gt, dev(pred), dev(gt)


def _loss_ws():
    return torch.empty(4096 + 8, dtype=F64, device=DEV)


def _check_loss(pred, gt, p, g, scale, mode, crit, lam=sc.LAM, what=()):
    """adn_loss_stats + adn_loss_finish (with and without a gradient) against the reference -> (ref, stats tensor)."""
    n = pred.size
    ref = sc.loss_reference(pred, gt, scale, mode, crit, lam=lam)
    stats = torch.full((4,), GUARD, dtype=F64, device=DEV)
    K().loss_stats(p, g, scale, mode, sc.EPS, stats, _loss_ws())
    st = host(stats)
    assert st[0] == ref['stats'][0], what + ('N', st[0], ref['stats'][0])                      # a count: exact
    for k in (1, 2, 3):
        within(st[k], ref['stats'][k], ref['stats_bar'][k], what + ('stat', k))
    loss = torch.full((1,), GUARD, device=DEV)
    gbuf, grad = guarded(n)
    K().loss_finish(p, g, scale, mode, sc.EPS, stats, crit, sc.L1W, sc.SW, lam, loss, grad)
    loss_only = torch.full((1,), GUARD, device=DEV)
    K().loss_finish(p, g, scale, mode, sc.EPS, stats, crit, sc.L1W, sc.SW, lam, loss_only, None)
    assert guard_intact(gbuf, n), what
    assert torch.equal(loss.view(torch.int32), loss_only.view(torch.int32)), what            # the loss-only call: same bits
    if ref['N'] == 0:
        assert bool(torch.isnan(loss).all()) and not bool(grad.any()), what
    else:
        within(host(loss)[0], ref['loss'], ref['loss_bar'], what + ('loss',))
        within(host(grad), ref['grad'], ref['grad_bar'], what + ('grad',))
    return ref, stats


def _check_dz(pred, gt, p, g, scale, mode, crit, stats, fa, with_bias, lam=sc.LAM, what=()):
    n = pred.size
    ref = sc.loss_reference(pred, gt, scale, mode, crit, fa, lam=lam)
    loss = torch.full((1,), GUARD, device=DEV)
    zbuf, dz = guarded(n)
    bias = torch.full((1 + PAD,), GUARD, device=DEV)
    K().loss_finish_dz(p, g, scale, mode, sc.EPS, stats, crit, sc.L1W, sc.SW, lam, loss, dz, fa,
                       bias[:1] if with_bias else None, _loss_ws())
    assert guard_intact(zbuf, n) and guard_intact(bias, 1), what
    if ref['N'] == 0:
        assert bool(torch.isnan(loss).all()) and not bool(dz.any()), what
        if with_bias:
            assert float(bias[0]) == 0.0, what
        return
    within(host(loss)[0], ref['loss'], ref['loss_bar'], what + ('loss',))
    within(host(dz), ref['grad'], ref['grad_bar'], what + ('dz',))
    if with_bias:
        within(host(bias)[0], ref['bias'], ref['bias_bar'], what + ('bias',))
    else:
        assert float(bias[0]) == GUARD, what


@pytest.mark.parametrize('scale', sc.SCALES)
@pytest.mark.parametrize('n', sc.LOSS_N)
def test_masked_loss_and_gradient_against_float64(n, scale):
    """Every mask mode x criterion (L1, SIlog, Combined; masked MSE through loss_finish) at one size and scale; the fused
    dz form over every final activation, with and without the bias gradient."""
    pred, gt, p, g = _loss_inputs(n, scale)
    for mode in (0, 1, 2):
        for crit in (0, 1, 2, 4):
            m = mode | (4 if crit == 4 else 0)
            what = (n, scale, mode, crit)
            _, stats = _check_loss(pred, gt, p, g, scale, m, crit, what=what)
            if crit == 4:
                continue
            for fa in (0, 1, 2):
                for with_bias in (True, False):
                    _check_dz(pred, gt, p, g, scale, mode, crit, stats, fa, with_bias, what=what + (fa, with_bias))


def test_masked_loss_past_the_finish_grid_cap():
    """n = 4096 * 256 + 1: the second pass of loss_finish's grid-stride loop (and 513 blocks of the reduction)."""
    n = sc.LOSS_N_FINISH_CAP
    pred, gt = sc.loss_case(n, 1.0)
    p, g = dev(pred), dev(gt)
    _, stats = _check_loss(pred, gt, p, g, 1.0, 0, 2, what=(n,))
    _check_dz(pred, gt, p, g, 1.0, 0, 2, stats, 0, True, what=(n, 'dz'))


def test_masked_loss_past_the_reduction_grid_cap():
    """n = 1024 * 2048 + 1: the capped grid of loss_stats strides a ninth time for one element."""
    n = sc.LOSS_N_RED_CAP
    pred, gt = sc.loss_case(n, 1.0)
    _check_loss(pred, gt, dev(pred), dev(gt), 1.0, 0, 2, what=(n,))


@pytest.mark.parametrize('mode', (0, 1))
def test_empty_mask_gives_nan_loss_and_zero_gradient(mode):
    pred, gt = sc.empty_mask_case(257, mode)
    p, g = dev(pred), dev(gt)
    for crit in (0, 1, 2):
        ref, stats = _check_loss(pred, gt, p, g, 1.0, mode, crit, what=('empty', mode, crit))
        assert ref['N'] == 0 and host(stats)[0] == 0
        _check_dz(pred, gt, p, g, 1.0, mode, crit, stats, 1, True, what=('empty dz', mode, crit))
    ref, _ = _check_loss(pred, gt, p, g, 1.0, mode | 4, 4, what=('empty', mode, 4))
    assert ref['N'] == 0


@pytest.mark.parametrize('name', ('two_px', 'equal'))
def test_nonpositive_variance_gives_zero_silog_and_zero_silog_gradient(name):
    """lambda = 1 and pred = c gt: var is exactly 0 (step_tail_cases.var0_cases says why, in float32 too).  The SIlog term is
    0 and adds no gradient -- torch's sqrt would hand back NaN gradients here; the kernel's var > 0 branch does not."""
    pred, gt = sc.var0_cases()[name]
    p, g = dev(pred), dev(gt)
    n = pred.size
    for crit in (1, 2):
        ref, stats = _check_loss(pred, gt, p, g, 1.0, 0, crit, lam=1.0, what=(name, crit))
        assert ref['var'] == 0.0
        st = host(stats)
        assert st[3] / st[0] - (st[2] / st[0]) ** 2 == 0.0                    # the kernel's own statistics give var == 0
        loss = torch.full((1,), GUARD, device=DEV)
        grad = torch.full((n,), GUARD, device=DEV)
        K().loss_finish(p, g, 1.0, 0, sc.EPS, stats, crit, sc.L1W, sc.SW, 1.0, loss, grad)
        l1 = sc.loss_reference(pred, gt, 1.0, 0, 0)
        w = sc.L1W if crit == 2 else 0.0
        assert float(loss) == float(np.float32(w * l1['stats'][1] / l1['N']))          # the SIlog term is exactly 0
        within(host(grad), w * l1['grad'], 16 * sc.U * np.abs(w * l1['grad']) + sc.TINY, (name, crit, 'grad'))
        if crit == 1 or name == 'equal':
            assert not bool(grad.any())


def test_mask_modes_part_on_negative_ground_truth():
    """gt != 0 (mode 0), gt > 0 (mode 1) and every pixel (mode 2) count different N on the same data, each its own."""
    pred, gt, p, g = _loss_inputs(257, 1.0)
    N = []
    for mode in (0, 1, 2):
        stats = torch.zeros(4, dtype=F64, device=DEV)
        K().loss_stats(p, g, 1.0, mode, sc.EPS, stats, _loss_ws())
        N.append(float(stats[0]))
    assert N == [float((gt != 0).sum()), float((gt > 0).sum()), 257.0] and N[1] < N[0] < N[2]
    pred, gt = sc.empty_mask_case(257, 1)                    # zero and negative gt only: empty in mode 1, not in mode 0
    stats = torch.zeros(4, dtype=F64, device=DEV)
    K().loss_stats(dev(pred), dev(gt), 1.0, 0, sc.EPS, stats, _loss_ws())
    assert float(stats[0]) == float((gt < 0).sum()) > 0


# ------------------------------------------------------------------------------------------- final_act_bwd, sum_to_scalar
@pytest.mark.parametrize('n', sc.FINAL_ACT_N)
def test_final_act_bwd_is_the_rounded_product_and_pads_with_zeros(n):
    """gout * act'(out): act' is exact in float32 on these inputs, so channel 0 must be THE float32 rounding of the float64
    product (tighter than 16u |product|, which is asserted as well), its bf16 form the round-to-nearest-even cast of that;
    the padded channels exactly zero, nothing past n * c_pad."""
    gout, out = sc.final_act_case(n)
    go, o = dev(gout), dev(out)
    for kind in (0, 1, 2):
        ref64, ref32 = sc.final_act_reference(gout, out, kind)
        for dtype in (F32, BF16):
            for c_pad in ((1, 8) if n < sc.LOSS_N_FINISH_CAP else (1,)):
                buf = torch.full((n * c_pad + PAD,), GUARD, dtype=dtype, device=DEV)
                dz = buf[:n * c_pad].view(n, c_pad)
                K().final_act_bwd(go, o, kind, dz)
                what = (n, kind, dtype, c_pad)
                assert guard_intact(buf, n * c_pad), what
                assert not bool(dz[:, 1:].any()) and not bool(torch.isnan(dz[:, 1:]).any()), what
                want = dev(ref32)
                if dtype == F32:
                    within(host(dz[:, 0]), ref64, 16 * sc.U * np.abs(ref64) + sc.TINY, what)
                else:
                    want = want.to(BF16)
                assert torch.equal(dz[:, 0], want), what


@pytest.mark.parametrize('n', sc.SUM_N)
def test_sum_to_scalar_against_float64(n):
    x = sc.sum_case(n)
    ws = torch.empty(1024 + 8, dtype=F64, device=DEV)
    for dtype in (F32, BF16):
        xd = dev(x, dtype)
        s, bar = sc.sum_reference(host(xd))
        out = torch.full((1 + PAD,), GUARD, device=DEV)
        K().sum_to_scalar(xd, out[:1], ws)
        assert guard_intact(out, 1)
        within(host(out)[0], s, bar, (n, dtype))


# ================================================================================================= gradient norm and clip
def _state():
    return torch.full((8,), GUARD, dtype=F64, device=DEV)


def _check_state(state, total, coef, tbar, cbar, what):
    st = host(state)
    within(st[3], total, tbar, what + ('norm',))
    within(st[4], coef, cbar, what + ('coef',))
    assert (st[[0, 1, 2, 5, 6, 7]] == GUARD).all(), what
    return st


@pytest.mark.parametrize('n', sc.NORM_N)
def test_grad_norm_three_routes_against_float64(n):
    """adn_grad_norm; adn_grad_sqsum_partials + adn_grad_norm_ranges(extras only); ranges over the multiple-of-4 prefix +
    the partials of the tail: the same state[3] (norm) and state[4] (clip coefficient) as the reference, with a max_norm
    that clips (coef 1/2) and one that does not (coef == 1 exactly)."""
    k = K()
    g = sc.norm_case(n)
    gd = dev(g)
    ref_sq = float((g.astype(np.float64) ** 2).sum())
    count = k.grad_sqsum_count(n)
    assert count == min(-(-n // 2048), 1024)
    pbuf, partials = guarded(count, F64)
    k.grad_sqsum_partials(gd, partials)
    assert guard_intact(pbuf, count), n                                   # exactly grad_sqsum_count(n) doubles
    within(float(partials.sum()), ref_sq, n * sc.D52 * ref_sq + sc.TINY, (n, 'partials'))       # exact terms: order only
    total0 = float(np.sqrt(ref_sq))
    ws = torch.empty(max(count, 1024) + 8, dtype=F64, device=DEV)
    n4 = n - n % 4
    rows = sc.split_rows(n4)
    for max_norm in sc.max_norms(total0):
        total, coef, tbar, cbar = sc.norm_reference(g, [(0, n)], (), max_norm)
        assert (coef == 1.0) == (max_norm > total0)
        st = _state()
        k.grad_norm(gd, max_norm, st, ws)
        a = _check_state(st, total, coef, tbar, cbar, (n, max_norm, 'grad_norm'))
        st = _state()
        k.grad_norm_ranges(gd, None, partials, max_norm, st, ws)
        b = _check_state(st, total, coef, tbar, cbar, (n, max_norm, 'extras only'))
        assert (coef == 1.0) == (a[4] == 1.0) == (b[4] == 1.0)
        if rows:
            extra = None
            if n % 4:
                extra = torch.empty(k.grad_sqsum_count(n % 4), dtype=F64, device=DEV)
                k.grad_sqsum_partials(gd[n4:], extra)
            st = _state()
            k.grad_norm_ranges(gd, dev(np.array(rows, dtype=np.int64)), extra, max_norm, st, ws)
            c = _check_state(st, total, coef, tbar, cbar, (n, max_norm, 'ranges + tail'))
            assert (coef == 1.0) == (c[4] == 1.0)


@pytest.mark.parametrize('case', ('rows_4_and_8192', 'rows_1500', 'extras_3000', 'both'))
def test_grad_norm_ranges_rows_and_extras(case):
    """Rows of the shortest (4) and the longest (8192) length at scattered offsets; 1500 rows and 3000 extras, past the 1024
    threads of the final kernel (its stride loop); ranges alone (n_extra == 0), extras alone (ranges None), both."""
    k = K()
    rng = np.random.default_rng(17)
    n = 6 * 8192
    g = sc.norm_case(n, seed=3)
    gd = dev(g)
    if case == 'rows_4_and_8192':
        rows = [(8, 4), (16, 8192), (8192 + 32, 4), (2 * 8192, 8192), (n - 4, 4)]
    elif case == 'extras_3000':
        rows = []
    else:
        rows = [(4 * int(i), 4) for i in rng.permutation(6000)[:1496]]              # scattered over [0, 24000)
        rows += [(3 * 8192, 8192), (4 * 8192, 8192), (5 * 8192, 4096), (n - 4, 4)]
        assert len(rows) == 1500
    assert all(o % 4 == 0 and ln % 4 == 0 and 0 < ln <= sc.ROW_MAX and o + ln <= n for o, ln in rows)
    extra = None
    if case in ('extras_3000', 'both'):
        extra = rng.integers(0, 1 << 20, 3000) / 1024.0
        extra[::7] = 0.0
    terms = sum(ln for _, ln in rows) + (0 if extra is None else extra.size)
    total0, _, _, _ = sc.norm_reference(g, rows, () if extra is None else extra, 1.0)
    ws = torch.empty(max(len(rows), 1) + PAD, dtype=F64, device=DEV)
    ws[:] = GUARD
    for max_norm in sc.max_norms(total0):
        total, coef, tbar, cbar = sc.norm_reference(g, rows, () if extra is None else extra, max_norm, n_terms=terms)
        st = _state()
        k.grad_norm_ranges(gd, dev(np.array(rows, dtype=np.int64).reshape(-1, 2)) if rows else None,
                           None if extra is None else dev(extra), max_norm, st, ws[:max(len(rows), 1)])
        got = _check_state(st, total, coef, tbar, cbar, (case, max_norm))
        assert (coef == 1.0) == (got[4] == 1.0) == (max_norm > total0)
        assert guard_intact(ws, max(len(rows), 1)), case                  # one double per row, no more
        if not rows:
            assert bool((ws == GUARD).all())


# ============================================================================================================== optimizer
P_G, M_G, V_G, W_G = -7.25, 3.5, 11.0, 0x5A5A


@functools.lru_cache(maxsize=None)
def _opt_inputs(n):
    return sc.opt_case(n)


def _opt_step(p, g, m, v, kind, wd, use_clip, t0, mirror, coef=sc.OPT_COEF):
    """One adn_optimizer_step on guarded copies, state[0] = t0 before the call -> numpy (p, m, v), w16 (int16 tensor or
    None), state after; guards checked."""
    n = p.size
    bufs = [guarded(n, F32, f) for f in (P_G, M_G, V_G)]
    for (_, view), x in zip(bufs, (p, m, v)):
        view.copy_(dev(x))
    wbuf = torch.full((n + PAD,), W_G, dtype=torch.int16, device=DEV)
    state = torch.zeros(8, dtype=F64, device=DEV)
    state[0], state[1], state[2], state[3] = t0, 0.123, 0.456, GUARD          # [1], [2]: stale, the kernel recomputes them
    state[4] = coef if use_clip else float('nan')                            # use_clip = 0 must not read it
    K().optimizer_step(bufs[0][1], dev(g), bufs[1][1], bufs[2][1], kind, sc.LR, sc.B1, sc.B2, sc.OPT_EPS, wd, use_clip, state,
                       bf16_copy=wbuf[:n].view(BF16) if mirror else None)
    for (buf, _), f in zip(bufs, (P_G, M_G, V_G)):
        assert guard_intact(buf, n, f), (n, kind)
    assert guard_intact(wbuf, n, W_G), (n, kind)
    if not mirror:
        assert bool((wbuf == W_G).all())
    return [b[1] for b in bufs], (wbuf[:n] if mirror else None), host(state)


def _check_opt(n, kind, wd, use_clip, t0, mirror, inputs=None):
    p, g, m, v = inputs or _opt_inputs(n)
    (pd, md, vd), w, st = _opt_step(p, g, m, v, kind, wd, use_clip, t0, mirror)
    t = t0 + 1
    what = (n, kind, wd, use_clip, t0, mirror)
    sref, sbar = sc.opt_state_reference(t)
    assert st[0] == t, what                                                  # a count: exact
    within(st[1:3], sref[1:], sbar[1:], what + ('bias corrections',))
    assert st[3] == GUARD and (np.isnan(st[4]) if not use_clip else st[4] == sc.OPT_COEF), what
    coef = sc.f32r(sc.OPT_COEF) if use_clip else 1.0
    pr, mr, vr, pb, mb, vb = sc.opt_reference(p, g, m, v, kind, sc.f32r(wd), coef, t)
    within(host(pd), pr, pb, what + ('p',))
    if kind == 2:
        assert np.array_equal(host(md), m.astype(np.float64)) and np.array_equal(host(vd), v.astype(np.float64)), what
    else:
        within(host(md), mr, mb, what + ('m',))
        within(host(vd), vr, vb, what + ('v',))
    if mirror:      # round-to-nearest-even bf16 of the kernel's own new float32 parameter, bit for bit, tail included
        assert torch.equal(w, pd.to(BF16).view(torch.int16)), what
    return pd.cpu().numpy(), md.cpu().numpy(), vd.cpu().numpy()


@pytest.mark.parametrize('kind,wd', sc.OPT_KINDS, ids=['AdamW', 'AdamW+wd', 'Adam', 'Adam+L2', 'SGD'])
def test_optimizer_step_against_float64(kind, wd):
    for n in sc.OPT_N:
        for use_clip in (1, 0):
            for t0 in (0, 999):
                for mirror in (True, False):
                    _check_opt(n, kind, wd, use_clip, t0, mirror)


@pytest.mark.parametrize('n', (sc.OPT_N_CAP, sc.OPT_N_CAP_NEXT))
def test_optimizer_step_past_the_grid_cap(n):
    """AdamW at n = 8192 * 1024 + 3: the grid is capped at 8192 blocks, whose threads take exactly one group of four each,
    block 0 the three-element tail.  Four elements more and thread 0 takes a second group: the grid stride."""
    assert (sc.OPT_N_CAP >> 2) == 8192 * 256 and (n >> 2) - 8192 * 256 == (n - sc.OPT_N_CAP) // 4 and n & 3 == 3
    _check_opt(n, 0, 0.01, 1, 0, True)


@pytest.mark.parametrize('kind,wd', ((0, 0.01), (1, 0.01), (2, 0.0)), ids=['AdamW+wd', 'Adam+L2', 'SGD'])
def test_optimizer_three_consecutive_steps(kind, wd):
    """Each step starts from the kernel's own previous float32 state and is judged against one float64 step from there."""
    p, g, m, v = _opt_inputs(5)
    for t0 in (0, 1, 2):
        p, m, v = _check_opt(5, kind, wd, 1, t0, True, inputs=(p, g, m, v))


# ================================================================================================================ metrics
def _errors(gt, pred):
    S = gt.shape[0]
    out = torch.full((S + 1, 7), GUARD, device=DEV)
    K().compute_errors(dev(gt), dev(pred), out[:S])
    assert bool((out[S] == GUARD).all())
    return out[:S]


@pytest.mark.parametrize('pixels', sc.METRIC_PIXELS)
def test_compute_errors_every_branch_in_one_launch(pixels):
    """One launch whose samples leave compute_errors_kernel by different branches (step_tail_cases.METRIC_KINDS), each row
    against metrics_oracle.compute_errors (float32 numpy, the reference's own code path) at the suite's rtol 2e-5 /
    atol 1e-6; the counts behind a1..a3 exactly."""
    kinds, gt, pred = sc.metric_batch(pixels)
    got = _errors(gt, pred).cpu().numpy()
    for i, kind in enumerate(kinds):
        ref, info = sc.metric_reference(gt[i], pred[i])
        assert info['branch'] == sc.METRIC_BRANCH[kind]
        if info['branch'] in ('empty', 'gt_le_eps'):
            assert not got[i].any(), (pixels, kind)                                   # no valid pixel: seven zeros
        elif info['branch'] == 'pred_le_0':
            assert np.array_equal(got[i].astype(np.float64), ref), (pixels, kind)
        else:
            err = np.abs(got[i].astype(np.float64) - ref)
            assert (err <= sc.METRIC_ATOL + sc.METRIC_RTOL * np.abs(ref)).all(), (pixels, kind, got[i], ref)
            for a, c in zip((2, 3, 4), sc.THRESHOLDS):                                # the numerators of a1..a3: exact
                count = int((info['thresh'] < np.float32(c)).sum())
                assert got[i][a] == np.float32(count / info['kept']), (pixels, kind, a)


def test_compute_errors_rows_follow_their_samples():
    _, gt, pred = sc.metric_batch(1025)
    i, j = sc.METRIC_KINDS.index('metres'), sc.METRIC_KINDS.index('eps2_mode1')
    ab = _errors(gt[[i, j]], pred[[i, j]])
    ba = _errors(gt[[j, i]], pred[[j, i]])
    assert torch.equal(ab[0], ba[1]) and torch.equal(ab[1], ba[0]) and not torch.equal(ab[0], ab[1])


# ============================================================================================================== edge loss
def _edge_run(pred, gt, lam):
    k = K()
    B, _, H, W = pred.shape
    n = pred.size
    nbytes = k.edge_loss_workspace_bytes(B, H, W)
    assert nbytes == 512 * 5 * 8 + n * 2 * 4 + 64
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    stats = torch.full((5 + PAD,), GUARD, dtype=F64, device=DEV)
    terms = torch.full((4 + PAD,), GUARD, device=DEV)
    gbuf, grad = guarded(n)
    k.edge_loss(dev(pred), dev(gt), lam, stats[:5], terms[:4], grad.view(B, 1, H, W), ws[:nbytes])
    assert bool((ws[nbytes:] == 0xA5).all()), 'written past edge_loss_workspace_bytes'
    assert guard_intact(gbuf, n) and guard_intact(stats, 5) and guard_intact(terms, 4)
    # without a gradient: the same terms and sums
    stats2, terms2 = torch.zeros(5, dtype=F64, device=DEV), torch.zeros(4, device=DEV)
    k.edge_loss(dev(pred), dev(gt), lam, stats2, terms2, None, ws[:nbytes])
    assert torch.equal(stats2, stats[:5]) and torch.equal(terms2, terms[:4])
    return host(stats[:5]), host(terms[:4]), host(grad).reshape(pred.shape)


@pytest.mark.parametrize('lam', sc.EDGE_LAMBDAS, ids=['lambdas0', 'lambdas1'])
@pytest.mark.parametrize('shape', sc.EDGE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_edge_loss_against_float64_autograd(shape, lam):
    """H or W of 1 and 2 (every Sobel tap but the centre in the padding), several images in one 256-thread block (the
    per-image base of the gather), and 363 x 363: past the 512-block cap of the statistics kernel."""
    pred, gt = sc.edge_case(*shape)
    ref = sc.edge_reference(pred, gt, lam)
    stats, terms, grad = _edge_run(pred, gt, lam)
    what = (shape, lam)
    assert stats[0] == ref['stats'][0] and stats[2] == ref['stats'][2], what                   # counts: exact
    for i in (1, 3, 4):
        within(stats[i], ref['stats'][i], ref['stats_bar'][i], what + ('stat', i))
    within(terms, ref['terms'], ref['terms_bar'], what + ('terms',))
    within(grad, ref['grad'], ref['grad_bar'], what + ('grad',))


def test_edge_loss_without_a_valid_pixel_is_zero():
    pred, gt = sc.edge_case(3, 5, 7)
    stats, terms, grad = _edge_run(pred, -np.abs(gt), sc.EDGE_LAMBDAS[0])
    assert stats[0] == 0 and stats[2] == 0 and not terms.any() and not grad.any()
