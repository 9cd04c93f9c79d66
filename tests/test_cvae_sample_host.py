"""CPU-only checks of cVAE multi-hypothesis inference: test_cvae command line, the model surface, and the argument
checks of adn_vae_sample / adn_sample_stats (rejected on the host before any launch)."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(**kw):
    from audio_depth_estimation_amd.models.unet_cvae_model import define_G_cvae
    torch.manual_seed(0)
    cfg = SimpleNamespace(dataset=SimpleNamespace(depth_norm=False, max_depth=30.0))
    return define_G_cvae(cfg, 2, 1, 4, 'unet_128', latent_dim=16, **kw)


def test_test_cvae_parser_flags_and_defaults():
    from audio_depth_estimation_amd import test as adn_test
    from audio_depth_estimation_amd import test_cvae
    a = test_cvae.build_parser().parse_args([])
    assert a.n_samples == 8 and a.decode == 'sample' and a.latent_dim == 128 and a.seed is None
    base = adn_test.build_parser().parse_args([])
    for k, v in vars(base).items():                       # test.py's flags, with test.py's defaults
        assert getattr(a, k) == v, k
    a = test_cvae.build_parser().parse_args(['--n_samples', '3', '--decode', 'mean', '--latent_dim', '64', '--synthetic', '4'])
    assert (a.n_samples, a.decode, a.latent_dim, a.synthetic) == (3, 'mean', 64, 4)
    with pytest.raises(SystemExit):
        test_cvae.build_parser().parse_args(['--decode', 'mode'])
    flags = set(re.findall(r'--[a-z_0-9]+', test_cvae.build_parser().format_help()))
    for f in ('--dataset', '--experiment_name', '--checkpoint_path', '--checkpoints', '--eval_on', '--visualize',
              '--output_dir', '--vis_batch_size', '--precision', '--synthetic', '--batch_size', '--latent_dim',
              '--n_samples', '--decode'):
        assert f in flags, f
    with pytest.raises(ValueError, match='n_samples'):
        test_cvae.main(['--n_samples', '0'])


def test_sample_on_model_and_dataparallel_stand_in(monkeypatch):
    from audio_depth_estimation_amd.cvae_engine import CVAEEngine, SampleResult
    m = _build()
    assert callable(m.sample) and callable(CVAEEngine.sample)
    assert SampleResult._fields[:6] == ('samples', 'mean', 'std', 'mu', 'logvar', 'kl')
    with pytest.raises(RuntimeError, match='no CPU path'):          # a CPU input is refused, in eval mode too
        m.eval().sample(torch.zeros(1, 2, 128, 128), 2)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.nn.Module, 'to', lambda self, *a, **k: self)
    dp = _build(gpu_ids=[0])
    assert next(iter(dp.state_dict())).startswith('module.')
    assert callable(dp.sample)
    with pytest.raises(RuntimeError, match='no CPU path'):          # reaches the generator's own sample()
        dp.sample(torch.zeros(1, 2, 128, 128), 2)


def test_abi_lists_sample_symbols():
    from audio_depth_estimation_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'adn.h')).read()
    for name in ('adn_vae_sample', 'adn_sample_stats'):
        assert re.search(r'\bint ' + name + r'\(', text)
        assert name in _lib.symbol_names()
    assert _lib.load().adn_version() == 3


def _vae_sample_args(B=2, C=8, L=4, K=3, mode=0, dtype=0, **null):
    """Positional arguments of adn_vae_sample with dummy non-null operands (16); ``null``: operands passed as NULL."""
    ops = dict.fromkeys(('h', 'w_mu', 'b_mu', 'w_lv', 'b_lv', 'w_dec', 'b_dec', 'eps_in', 'mu', 'logvar', 'eps', 'z',
                         'kl_img', 'kl', 'out_relu'), 16)
    ops.update(null)
    o = ops
    return (o['h'], B, C, L, K, mode, o['w_mu'], o['b_mu'], o['w_lv'], o['b_lv'], o['w_dec'], o['b_dec'], 7, o['eps_in'],
            o['mu'], o['logvar'], o['eps'], o['z'], o['kl_img'], o['kl'], dtype, o['out_relu'], None)


def test_vae_sample_argument_checks_without_gpu():
    from audio_depth_estimation_amd import _lib
    lib = _lib.load()
    err = lambda: lib.adn_last_error()
    for missing in ('h', 'w_mu', 'b_mu', 'w_lv', 'b_lv', 'w_dec', 'b_dec', 'mu', 'logvar', 'eps', 'z', 'kl_img', 'kl',
                    'out_relu'):                                   # every operand but the optional eps_in is required
        assert lib.adn_vae_sample(*_vae_sample_args(**{missing: None})) == -1, missing
        assert b'adn_vae_sample: null pointer' in err(), missing
    for kw, what in ((dict(K=0), b'K 0'), (dict(K=-3), b'K -3'), (dict(K=2, mode=1), b'mean decode'),
                     (dict(mode=2), b'bad mode'), (dict(B=0), b'B 0'), (dict(C=12), b'C 12'), (dict(L=1025), b'L 1025'),
                     (dict(L=0), b'L 0'), (dict(dtype=5), b'bad dtype'),
                     (dict(B=1 << 20, K=1 << 20), b'decode grid'),           # K * B rows past int32
                     (dict(B=1 << 24, K=64, C=512), b'decode grid')):        # channel x row-group waves past int32
        assert lib.adn_vae_sample(*_vae_sample_args(**kw)) == -1, kw
        assert b'adn_vae_sample' in err() and what in err(), (kw, err())


def test_sample_stats_argument_checks_without_gpu():
    from audio_depth_estimation_amd import _lib
    lib = _lib.load()
    for args, what in (((None, 2, 8, 16, 16, None), b'null pointer'), ((16, 2, 8, None, 16, None), b'null pointer'),
                       ((16, 2, 8, 16, None, None), b'null pointer'), ((16, 0, 8, 16, 16, None), b'K 0'),
                       ((16, -1, 8, 16, 16, None), b'K -1'), ((16, 2, 0, 16, 16, None), b'N 0')):
        assert lib.adn_sample_stats(*args) == -1, args
        assert b'adn_sample_stats' in lib.adn_last_error() and what in lib.adn_last_error(), args
