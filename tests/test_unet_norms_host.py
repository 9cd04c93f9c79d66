"""CPU-only: the host side of norm='instance' / 'none' / use_dropout=True (module layout, command line, bindings, refusals)
and the float64 oracle of tests/unet_norm_oracle.py against the reference's fixtures."""
from types import SimpleNamespace

import pytest
import torch

import unet_norm_oracle as O


def _cfg(depth_norm=False, max_depth=30.0):
    return SimpleNamespace(dataset=SimpleNamespace(depth_norm=depth_norm, max_depth=max_depth))


def _model(netG, norm, use_dropout=False, ngf=4):
    from audio_depth_estimation_amd.models.unetbaseline_model import define_G
    return define_G(_cfg(), 2, 1, ngf, netG, norm=norm, use_dropout=use_dropout)


FIXTURES = [('unet128_ngf4_instance', 'unet_128', 'instance', 7, 28), ('unet256_ngf4_instance_b1', 'unet_256', 'instance', 8, 32),
            ('unet128_ngf4_none', 'unet_128', 'none', 7, 15)]


@pytest.mark.parametrize('name,netG,norm,n,nkeys', FIXTURES, ids=[f[0] for f in FIXTURES])
def test_keys_and_parameter_counts_match_the_reference(name, netG, norm, n, nkeys):
    z = O.load_fixture(name)
    ref = {k[4:]: z[k] for k in z if k.startswith('sd0/')}
    for use_dropout in (False, True):                      # nn.Dropout has no state: the same keys
        sd = _model(netG, norm, use_dropout).state_dict()
        assert list(sd.keys()) == list(ref.keys()) and len(sd) == nkeys
        assert all(tuple(sd[k].shape) == ref[k].shape for k in sd)
    m = _model(netG, norm)
    assert sum(p.numel() for p in m.parameters()) == sum(v.size for v in ref.values())     # no buffers in either
    assert [k for k, _ in m.named_parameters()] == O.param_keys(ref)
    # a bias on every conv under instance, only on the last layer under none (use_bias of the reference)
    biases = [k for k in ref if k.endswith('.bias')]
    assert len(biases) == (2 * n if norm == 'instance' else 1)


@pytest.mark.parametrize('norm,use_dropout', [('instance', False), ('none', False), ('batch', True), ('instance', True)])
def test_engine_levels_record_norm_kind_and_dropout(norm, use_dropout):
    m = _model('unet_256', norm, use_dropout)
    eng = m.engine()
    L = eng.levels
    assert len(L) == 8 and not eng.batch_only and eng.uses_dropout == use_dropout
    assert [lv['drop'] for lv in L] == [False] * 4 + [use_dropout] * 3 + [False]          # the num_downs - 5 blocks
    for i, lv in enumerate(L):
        has_d, has_u = 0 < i < 7, i > 0
        assert lv['in_d'] == (norm == 'instance' and has_d) and lv['in_u'] == (norm == 'instance' and has_u)
        assert (lv['bn_d'] is not None) == (norm == 'batch' and has_d)
        assert (lv['bn_u'] is not None) == (norm == 'batch' and has_u)
    plain = _model('unet_256', 'batch').engine()
    assert plain.batch_only and not plain.uses_dropout


def test_data_parallel_refuses_the_new_modes():
    from audio_depth_estimation_amd.engine import FusedTrainer
    for norm, drop in (('instance', False), ('none', False), ('batch', True)):
        with pytest.raises(NotImplementedError, match='data-parallel'):
            FusedTrainer(_model('unet_128', norm, drop).engine(), ddp=object())


def test_cvae_factory_still_refuses():
    from audio_depth_estimation_amd.models.unet_cvae_model import define_G_cvae
    with pytest.raises(NotImplementedError):
        define_G_cvae(_cfg(), 2, 1, 4, 'unet_256', norm='instance')
    with pytest.raises(NotImplementedError):
        define_G_cvae(_cfg(), 2, 1, 4, 'unet_256', use_dropout=True)


def test_command_line_flags_and_experiment_names():
    from audio_depth_estimation_amd import test as test_cli
    from audio_depth_estimation_amd import train
    cfg = SimpleNamespace(model=SimpleNamespace(generator='unet_256'), dataset=SimpleNamespace(name='batvisionv2'),
                          mode=SimpleNamespace(batch_size=32, learning_rate=0.002, optimizer='AdamW', experiment_name='default'))
    p = train.build_parser()
    a = p.parse_args([])
    assert a.norm == 'batch' and a.use_dropout is False
    base = train.experiment_name(cfg, a)
    assert base == 'unet_256_batvisionv2_BS32_Lr0.002_AdamW_default'            # unchanged for the defaults
    assert train.experiment_name(cfg, p.parse_args(['--norm', 'instance'])) == base.replace('_default', '_instance_default')
    assert train.experiment_name(cfg, p.parse_args(['--norm', 'none'])) == base.replace('_default', '_none_default')
    assert train.experiment_name(cfg, p.parse_args(['--use_dropout'])) == base.replace('_default', '_drop_default')
    assert train.experiment_name(cfg, p.parse_args(['--norm', 'instance', '--use_dropout'])) == \
        base.replace('_default', '_instance_drop_default')
    with pytest.raises(SystemExit):
        p.parse_args(['--norm', 'layer'])
    t = test_cli.build_parser()
    assert t.parse_args([]).norm == 'batch' and t.parse_args(['--norm', 'instance']).norm == 'instance'
    with pytest.raises(SystemExit):
        t.parse_args(['--use_dropout'])                     # evaluation never drops


def test_new_symbols_are_bound_and_refuse_on_the_host():
    from audio_depth_estimation_amd import _lib
    from audio_depth_estimation_amd import kernels as K
    names = _lib.symbol_names()
    for sym in ('adn_inorm_fwd', 'adn_inorm_bwd', 'adn_inorm_workspace_bytes', 'adn_inorm_form', 'adn_dropout_apply'):
        assert sym in names
    lib = _lib.load()
    assert lib.adn_version() == 3
    assert K.inorm_workspace_bytes(32, 128 * 128, 64) >= 32 * 2 * 64 * 4
    assert lib.adn_inorm_workspace_bytes(2, 1, 8) == -1
    assert lib.adn_inorm_form(1, 8, 0) == -1 and b'adn_inorm_form' in lib.adn_last_error()
    assert K.inorm_form(4, 512, torch.bfloat16) == 'resident' and K.inorm_form(4, 12, torch.float32) == 'resident-plain'
    assert K.inorm_form(128 * 128, 64, torch.bfloat16) == 'streaming'
    # HW = 1 and a short workspace are refused before any pointer is looked at or anything is launched
    assert lib.adn_inorm_fwd(16, 2, 1, 8, 0, 1e-5, 0.2, 16, 16, 16, None, None, 1.0, 16, 1 << 20, None) == -1
    assert b'spatial' in lib.adn_last_error()
    assert lib.adn_inorm_bwd(16, 16, 16, 16, 2, 1, 8, 0, 1.0, 16, 1 << 20, None) == -1
    need = K.inorm_workspace_bytes(2, 16, 8)
    assert lib.adn_inorm_fwd(16, 2, 16, 8, 0, 1e-5, 0.2, 16, 16, 16, None, None, 1.0, 16, need - 1, None) == -1
    assert b'workspace' in lib.adn_last_error()
    assert lib.adn_inorm_bwd(16, 16, 16, 16, 2, 16, 8, 0, 1.0, 16, need - 1, None) == -1
    assert lib.adn_inorm_fwd(24, 2, 16, 8, 0, 1e-5, 0.2, 16, 16, 16, None, None, 1.0, 16, need, None) == -1     # z at 8 mod 16
    assert b'misaligned' in lib.adn_last_error()


def test_dropout_levels_of_the_oracle():
    assert O.dropout_levels(7) == [4, 5] and O.dropout_levels(8) == [4, 5, 6]


@pytest.mark.parametrize('name,netG,norm,n,nkeys', FIXTURES[::2], ids=[f[0] for f in FIXTURES[::2]])
def test_oracle_reproduces_the_reference_fixtures(name, netG, norm, n, nkeys):
    """The float64 restatement against the reference's own f32 run: prediction 1e-6 (the issue measured 4e-8), weight
    gradients 1e-4 of the tensor maximum (measured there: 4.3e-5 worst), biases in front of an InstanceNorm2d ~ 0."""
    z = O.load_fixture(name)
    ngf, S, depth_norm, B = [int(v) for v in z['meta']]
    lr, max_depth, l1w, sw, lam = [float(v) for v in z['hyper']]
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z if k.startswith('sd0/')}
    pred, loss, grads = O.step(sd, torch.from_numpy(z['audio']), torch.from_numpy(z['gt']), n, bool(depth_norm), norm,
                               (l1w, sw, lam, max_depth))
    ref = torch.from_numpy(z['pred_train']).double()
    assert float((pred - ref).abs().sum() / ref.abs().sum()) <= 1e-6
    assert abs(loss - float(z['loss'])) <= 1e-6 * abs(float(z['loss']))
    zero_bias = O.normed_bias_keys(n, norm)
    assert len(zero_bias) == (2 * n - 3 if norm == 'instance' else 0)
    for k, g in grads.items():
        r = torch.from_numpy(z['grad/' + k]).double()
        if k in zero_bias:                                    # mathematically zero: rounding noise in both
            wmax = float(grads[zero_bias[k]].abs().max())
            assert float(g.abs().max()) <= 1e-12 * wmax and float(r.abs().max()) <= 1e-5 * wmax, k
        else:
            assert float((g - r).abs().max() / r.abs().max()) <= 1e-4, k
