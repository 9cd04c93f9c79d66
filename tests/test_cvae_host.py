"""CPU-only checks of the U-Net cVAE family: module mirror, train_cvae command line, ABI listing."""
import hashlib
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CASES = (('cvae256_ngf4.npz', 'unet_256', False, 128), ('cvae128_ngf4_dn.npz', 'unet_128', True, 100))


def _cfg(depth_norm):
    return SimpleNamespace(dataset=SimpleNamespace(depth_norm=depth_norm, max_depth=30.0))


def _build(netG, depth_norm, latent, **kw):
    from audio_depth_estimation_amd.models.unet_cvae_model import define_G_cvae
    torch.manual_seed(0)
    return define_G_cvae(_cfg(depth_norm), 2, 1, 4, netG, latent_dim=latent, **kw)


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize('fixture,netG,depth_norm,latent', CASES)
def test_initial_state_dict_matches_reference_bits(fixture, netG, depth_norm, latent):
    ref = np.load(os.path.join(GOLDEN, fixture))
    sd = _build(netG, depth_norm, latent).state_dict()
    assert list(sd) == [str(k) for k in ref['sd_init_keys']]
    assert [_sha(v) for v in sd.values()] == [str(h) for h in ref['sd_init_sha']]


def test_dataparallel_prefix_with_gpu_ids(monkeypatch):
    """gpu_ids set: the key-compatible DataParallel stand-in prefixes every key with 'module.' (same bits)."""
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.nn.Module, 'to', lambda self, *a, **k: self)
    ref = np.load(os.path.join(GOLDEN, 'cvae256_ngf4.npz'))
    sd = _build('unet_256', False, 128, gpu_ids=[0]).state_dict()
    assert list(sd) == ['module.' + str(k) for k in ref['sd_init_keys']]
    assert [_sha(v) for v in sd.values()] == [str(h) for h in ref['sd_init_sha']]


def test_parameter_order_innermost_first_and_unused_norms():
    m = _build('unet_256', False, 128)
    names = [n for n, _ in m.named_parameters()]
    inner = 'model.' + 'submodule.' * 7
    assert names[0] == inner + 'downconv.weight'
    assert names[-2:] == ['model.upconv.weight', 'model.upconv.bias']
    assert inner + 'vae.fc_mu.weight' in names
    unused = m.unused_norms()
    assert unused == [m.model.downnorm, m.model.upnorm, m.model.submodule.submodule.submodule.submodule.submodule
                      .submodule.submodule.downnorm]
    assert unused[1].num_features == 1
    # level n-2: inner_nc input channels (no skip concat), every other intermediate level 2 * inner_nc
    assert m.model.submodule.submodule.submodule.submodule.submodule.submodule.upconv.weight.shape[0] == 32
    assert m.model.submodule.submodule.submodule.submodule.submodule.upconv.weight.shape[0] == 64
    # head: ReLU without depth_norm, identity (no final_relu, no Sigmoid) with it
    assert m.model.use_final_relu and isinstance(m.model.final_relu, torch.nn.ReLU)
    dn = _build('unet_256', True, 128)
    assert not dn.model.use_final_relu and not hasattr(dn.model, 'final_relu')
    assert not any(isinstance(x, torch.nn.Sigmoid) for x in dn.modules())


def test_refusals():
    from audio_depth_estimation_amd.models.unet_cvae_model import define_G_cvae
    with pytest.raises(NotImplementedError):
        define_G_cvae(_cfg(False), 2, 1, 4, 'unet_256', use_dropout=True)
    with pytest.raises(NotImplementedError):
        define_G_cvae(_cfg(False), 2, 1, 4, 'unet_256', norm='instance')
    with pytest.raises(NotImplementedError):
        define_G_cvae(_cfg(False), 2, 1, 4, 'unet_64')
    m = _build('unet_128', False, 128)
    with pytest.raises(RuntimeError, match='1x1'):
        m(torch.zeros(1, 2, 256, 256))                    # 2x2 bottleneck: the reference's view(B, C) fails too


def test_train_cvae_parser_and_name(monkeypatch):
    from audio_depth_estimation_amd import train_cvae
    a = train_cvae.build_parser().parse_args([])
    assert a.kl_weight == 1e-4 and a.latent_dim == 128 and a.experiment_name == 'cvae' and a.dataset == 'batvisionv2'
    assert a.precision == 'bf16' and a.graph is False
    flags = set(re.findall(r'--[a-z_0-9]+', train_cvae.build_parser().format_help()))
    for f in ('--dataset', '--experiment_name', '--checkpoints', '--batch_size', '--learning_rate', '--use_wandb',
              '--wandb_project', '--wandb_entity', '--wandb_mode', '--criterion', '--optimizer', '--silog_lambda',
              '--l1_weight', '--silog_weight', '--audio_format', '--validation', '--validation_iter', '--kl_weight',
              '--latent_dim', '--precision', '--graph'):
        assert f in flags, f
    cfg = SimpleNamespace(model=SimpleNamespace(generator='unet_256'), dataset=SimpleNamespace(name='batvisionv2'),
                          mode=SimpleNamespace(batch_size=32, learning_rate=0.002, optimizer='AdamW',
                                               experiment_name='cvae_cvae'))
    assert train_cvae.experiment_name(cfg) == 'unet_256_batvisionv2_BS32_Lr0.002_AdamW_cvae_cvae_cvae'
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit, match='multi-GPU'):
        train_cvae.main([])


def test_abi_lists_vae_symbols():
    from audio_depth_estimation_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'adn.h')).read()
    for name in ('adn_vae_fwd', 'adn_vae_bwd'):
        assert re.search(r'\bint ' + name + r'\(', text)
        assert name in _lib.symbol_names()
