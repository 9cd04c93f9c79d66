"""Outermost level without a materialised D1 activation: the rewrites give the bits of the launches they replace.

  * readers of ru[1] = ReLU(BN(zu[1])) given zu[1] + scale / shift (last transposed conv, its weight gradient, the mask
    of its input gradient) == the same call given the buffer adn_bn_act wrote;
  * engine level: forward + backward, a graphed trainer and a train / eval / train sequence with the new form == with
    ADN_D1_MATERIALISED (the launches of before); dropout and instance-norm engines keep those.
Everything here is torch.equal on raw outputs: the reference is the materialised path, run in the same process.
"""
from types import SimpleNamespace

import pytest
import torch

from test_gpu_kernels import DEV, K
from test_gpu_outer_level import _leaky_relu_copies, _signed_operand

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
I16 = torch.int16


def _bits(t):
    return t.view(I16) if t.dtype == BF else t


def _bn_operand(k, shape, seed):
    """z (bf16 NHWC, 64 channels: half negative, exact +-0, +-1e-40), scale (some negative, three channels 0), shift
    (0 on those three), and ru = what adn_bn_act's relu copy holds for them."""
    B, Hs, Ws = shape
    z = _signed_operand((B, Hs, Ws, 64), BF, seed).to(DEV)
    g = torch.Generator().manual_seed(seed + 1000)
    scale = torch.randn(64, generator=g)
    shift = torch.randn(64, generator=g) * 0.5
    scale[[3, 17, 40]] = 0.0
    shift[[3, 17, 40]] = 0.0
    shift[[5, 50]] = 0.0                               # z = +-0 / +-1e-40 then decide the mask on their own
    assert int((scale < 0).sum()) >= 8
    scale, shift = scale.to(DEV), shift.to(DEV)
    ru = torch.full((B, Hs, Ws, 64), float('nan'), dtype=BF, device=DEV)
    k.bn_act(z, B * Hs * Ws, 64, scale, shift, 0.0, None, ru)
    assert not torch.isnan(ru.float()).any()
    frac = float((ru.float() > 0).float().mean())
    assert 0.3 < frac < 0.7, frac
    return z, scale, shift, ru


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 16, 32), (3, 7, 16), (2, 10, 32)])
@pytest.mark.parametrize('two_launch', [False, True])
def test_convt_n1_applies_bn_relu_on_load(shape, two_launch):
    k = K()
    B, Hs, Ws = shape
    z, scale, shift, ru = _bn_operand(k, shape, 41)
    leaky, relu = _leaky_relu_copies(_signed_operand((B, Hs, Ws, 64), BF, 42), BF)
    torch.manual_seed(43)
    w = (torch.randn(128, 16) * 0.05).to(BF).float().view(-1).to(DEV)
    ws = torch.empty(k.convt_n1_workspace_bytes(B, Hs, Ws) // 4, dtype=torch.float32, device=DEV)

    def run(a0, a1, bias, fa, **kw):
        out = torch.full((B, 2 * Hs, 2 * Ws), float('nan'), dtype=torch.float32, device=DEV)
        k.convt_n1_forward(BF, B, Hs, Ws, a0, a1, w, bias, fa, out, ws, two_launch=two_launch, **kw)
        return out
    for fa in (0, 1):
        for bias in (None, torch.tensor([0.3], device=DEV)):
            for a0, relu_in0 in ((relu.to(DEV), False), (leaky.to(DEV), True)):
                ref = run(a0, ru, bias, fa, relu_in0=relu_in0)
                out = run(a0, z, bias, fa, relu_in0=relu_in0, bn1=(scale, shift))
                assert not torch.isnan(ref).any()
                assert torch.equal(out, ref), (fa, bias is not None, relu_in0)
    with pytest.raises(RuntimeError, match='scale1'):
        k.convt_n1_forward(torch.float32, B, Hs, Ws, relu.float().to(DEV), z.float(), w, None, 0,
                           torch.empty(B, 2 * Hs, 2 * Ws, device=DEV), ws, bn1=(scale, shift))


@pytest.mark.parametrize('shape', [(2, 16, 32), (3, 8, 64)])
@pytest.mark.parametrize('relu_plain0', [False, True])
def test_thin_wgrad_applies_bn_relu_on_load(shape, relu_plain0):
    k = K()
    B, Hs, Ws = shape
    z, scale, shift, ru = _bn_operand(k, shape, 44)
    leaky, relu = _leaky_relu_copies(_signed_operand((B, Hs, Ws, 64), BF, 45), BF)
    p0 = (leaky if relu_plain0 else relu).to(DEV)
    torch.manual_seed(46)
    dz = torch.randn(B, 1, 2 * Hs, 2 * Ws, device=DEV)
    ws = torch.empty(k.thin_wgrad_workspace_bytes(B, Hs, Ws, 1, 64, 64) // 4, device=DEV)
    ref = torch.full((128, 16), float('nan'), device=DEV)
    out = torch.full((128, 16), float('nan'), device=DEV)
    k.thin_wgrad(dz, p0, ru, B, Hs, Ws, ref, ws, relu_plain0=relu_plain0)
    k.thin_wgrad(dz, p0, z, B, Hs, Ws, out, ws, relu_plain0=relu_plain0, bn1=(scale, shift))
    assert not torch.isnan(ref).any() and float(ref[64:].abs().max()) > 0
    assert torch.equal(out, ref)


# (2, 16, 32): 2 pixel groups per row, work unit = 1 group; (3, 8, 64): work unit = 4 groups; (8, 64, 208): 6656 work units
# on the launcher's cap of 768 workgroups x 4 waves, more than two per wave
@pytest.mark.parametrize('shape', [(2, 16, 32), (3, 8, 64), (8, 64, 208)])
@pytest.mark.parametrize('stats', [True, False])
def test_d0_dgrad_masks_by_z(shape, stats):
    k = K()
    B, Hs, Ws = shape
    z, scale, shift, ru = _bn_operand(k, shape, 47)
    skip = _leaky_relu_copies(_signed_operand((B, Hs, Ws, 64), BF, 48), BF)[0].to(DEV)
    g = torch.Generator().manual_seed(49)
    dz = torch.randn(B, 1, 2 * Hs, 2 * Ws, generator=g).to(DEV)
    w = (torch.randn(128, 16, generator=g) * 0.05).view(-1).to(DEV)
    mean = (torch.randn(64, generator=g) * 0.1).to(DEV)
    istd = (torch.rand(64, generator=g) + 0.5).to(DEV)
    P = k.d0_dgrad_num_partials(B, Hs, Ws)
    if shape == (8, 64, 208):
        assert P == 768 and B * Hs * (Ws // 16) > 2 * 4 * P
    res = []
    for ref in (ru, None):                              # the two mask sources: by ref, by z / scale / shift
        gd = torch.full((B, Hs, Ws, 64), float('nan'), dtype=BF, device=DEV)
        gu = torch.full((B, Hs, Ws, 64), float('nan'), dtype=BF, device=DEV)
        part = torch.full((P * 2 * 64,), float('nan'), device=DEV)
        k.d0_dgrad(dz, w, B, Hs, Ws, k.Seg(64, out0=gd, ref=skip, slope=0.0),
                   k.Seg(64, out0=gu, ref=ref, slope=0.0, z=z, mean=mean, istd=istd, scale=scale, shift=shift,
                         partials=part if stats else None))
        res.append((gd, gu, part))
    (gd0, gu0, part0), (gd1, gu1, part1) = res
    assert not torch.isnan(gd0.float()).any() and not torch.isnan(gu0.float()).any()
    assert float(gu0.float().abs().max()) > 0 and bool((gu0.view(I16) == 0).any())
    assert torch.equal(_bits(gd1), _bits(gd0)) and torch.equal(_bits(gu1), _bits(gu0))
    if stats:
        assert not torch.isnan(part0).any() and torch.equal(part1, part0)
    else:
        assert bool(torch.isnan(part1).all())
    with pytest.raises(RuntimeError, match='seg 1'):    # neither ref nor the coefficients to mask by
        k.d0_dgrad(dz, w, B, Hs, Ws, k.Seg(64, out0=gd0, ref=skip), k.Seg(64, out0=gu0, z=z, scale=scale))


# ---------------------------------------------------------------------------------------------------------------------
KNOBS = ('ADN_D1_MATERIALISED',)
CFG = SimpleNamespace(dataset=SimpleNamespace(depth_norm=False, max_depth=30.0))


def _engine(monkeypatch, knobs, **kw):
    from audio_depth_estimation_amd.models.unetbaseline_model import define_G
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name in knobs:
        monkeypatch.setenv(name, '1')
    torch.manual_seed(0)
    m = define_G(CFG, 2, 1, 64, 'unet_128', **kw)
    m.compute_dtype = BF
    return m.to(DEV).train().engine()


def _inputs():
    g = torch.Generator().manual_seed(1234)
    audio = torch.rand(2, 2, 128, 128, generator=g).to(DEV)
    up = (torch.randn(2, 1, 128, 128, generator=g) / (2 * 128 * 128)).to(DEV)
    return audio, up


def _train_pass(eng, audio, up):
    pred = eng.forward(audio, True).clone()
    eng.backward(up, fused_norm=True)
    torch.cuda.synchronize()
    bn = eng.levels[1]['u'].bn
    return dict(pred=pred, flat_g=eng.flat_g.clone(), sq_all=eng.sq_all.clone(), rm=bn.running_mean.clone(),
                rv=bn.running_var.clone(), nbt=bn.num_batches_tracked.clone())


def _assert_same(a, b, what):
    for key in a:
        assert torch.equal(a[key], b[key]), (what, key)


@pytest.fixture(scope='module')
def old_form():
    """One training pass and the train / eval / train sequence with ADN_D1_MATERIALISED: the launches of before."""
    mp = pytest.MonkeyPatch()
    try:
        eng = _engine(mp, KNOBS)
        audio, up = _inputs()
        first = _train_pass(eng, audio, up)
        assert not eng.ru1_virtual_ok
        assert not torch.isnan(first['flat_g']).any() and float(first['flat_g'].abs().max()) > 0
        ev = eng.forward(audio, False).clone()
        second = _train_pass(eng, audio, up)
    finally:
        mp.undo()
    return first, ev, second


def test_engine_equals_the_old_form(old_form, monkeypatch):
    knobs = ()
    eng = _engine(monkeypatch, knobs)
    audio, up = _inputs()
    _assert_same(_train_pass(eng, audio, up), old_form[0], knobs)
    assert eng.edge_path and eng.ru1_virtual_ok and eng._ru1_virtual
    # train forward -> eval forward -> train forward + backward: the eval forward writes ru[1], backward follows the
    # forward that fed it
    ev = eng.forward(audio, False).clone()
    assert torch.equal(ev, old_form[1]) and not eng._ru1_virtual
    _assert_same(_train_pass(eng, audio, up), old_form[2], knobs)


def test_graphed_trainer_equals_the_old_form(monkeypatch):
    from audio_depth_estimation_amd.engine import FusedTrainer
    g = torch.Generator().manual_seed(7)
    audio = torch.rand(2, 2, 128, 128, generator=g).to(DEV)
    gt = (30 * torch.rand(2, 1, 128, 128, generator=g)).to(DEV)
    res = []
    for knobs in ((), KNOBS):
        eng = _engine(monkeypatch, knobs)
        tr = FusedTrainer(eng, 'Combined', 0.237, 0.637, 0.869, max_depth=30.0, optimizer='AdamW', lr=0.002, clip_norm=1.0)
        tr.enable_graph(after_steps=1)
        for _ in range(3):
            tr.step(audio, gt)
        torch.cuda.synchronize()
        assert tr._graph is not None
        res.append(eng.flat_p.clone())
    assert not torch.isnan(res[0]).any()
    assert torch.equal(res[0], res[1])


@pytest.mark.parametrize('kw', [dict(use_dropout=True), dict(norm='instance')])
def test_other_configurations_keep_their_launches(kw, monkeypatch):
    from audio_depth_estimation_amd import _lib
    eng = _engine(monkeypatch, (), **kw)
    audio, up = _inputs()
    _lib.RECORD = []
    try:
        eng.forward(audio, True)
        eng.backward(up)
        names = [name for _, _, name, _ in _lib.RECORD]
    finally:
        _lib.RECORD = None
    torch.cuda.synchronize()
    assert not eng.ru1_virtual_ok
    assert not {'adn_convt_n1_forward_bn', 'adn_thin_wgrad_bn'} & set(names)
    assert 'adn_convt_n1_forward_ex' in names


def test_new_form_launch_plan(monkeypatch):
    """The default engine: no apply launch of D1's forward BatchNorm, everything else as in the old form."""
    from audio_depth_estimation_amd import _lib
    plans = []
    for knobs in ((), KNOBS):
        eng = _engine(monkeypatch, knobs)
        audio, up = _inputs()
        _lib.RECORD = []
        try:
            eng.forward(audio, True)
            eng.backward(up)
            plans.append([name for _, _, name, _ in _lib.RECORD])
        finally:
            _lib.RECORD = None
        torch.cuda.synchronize()
    new, old = plans
    assert 'adn_convt_n1_forward_bn' in new and 'adn_thin_wgrad_bn' in new and new.count('adn_d0_dgrad') == 1
    assert 'adn_convt_n1_forward_bn' not in old and 'adn_thin_wgrad_bn' not in old
    count = lambda plan, *names: sum(plan.count(n) for n in names)
    # D1 of unet_128 at B = 2 is small enough for the one-launch BatchNorm kernels in the old form
    assert count(new, 'adn_bn_act', 'adn_bn_fwd_fused') == count(old, 'adn_bn_act', 'adn_bn_fwd_fused') - 1
    assert count(new, 'adn_bn_bwd_apply', 'adn_bn_bwd_fused') == count(old, 'adn_bn_bwd_apply', 'adn_bn_bwd_fused')
    assert len(new) == len(old)                         # (bn_fwd_fused of D1 became bn_fwd_finalize)
