"""CPU-only checks of CoarseDepthLite (model_type 'lite' of the coarse-depth family): module mirror against the reference's
bits, the fixture's conditioning, refusals, the command line, the ABI of the thin first-layer kernel and the kernel forms
adn_igemm plans for the base-64 network."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from audio_depth_estimation_amd import kernels as K
from audio_depth_estimation_amd._lib import EPI_ACT, EPI_ADD, EPI_BWD, EPI_Z_STATS, GEMM_S1, GEMM_S2, GEMM_T2
from audio_depth_estimation_amd.coarse_engine import CoarseLiteEngine
from audio_depth_estimation_amd.models.coarse_depth_model import CoarseDepthLite, init_net, init_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'coarse_lite64_bc64.npz')
CASES = ('sq', 'rect', 'b48')


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()


def _build(case='sq'):
    z = np.load(GOLDEN)
    nb, base, H, W, B, seed = [int(v) for v in z[case + '/meta']]
    torch.manual_seed(seed)
    m = CoarseDepthLite(2, nb, base, W)
    init_weights(m, 'kaiming')
    return m, z


@pytest.mark.parametrize('case', CASES)
def test_initial_state_dict_matches_reference_bits(case):
    m, z = _build(case)
    sd = m.state_dict()
    assert len(sd) == 73 and list(sd)[:4] == ['bin_centers', 'encoder.0.weight', 'encoder.0.bias', 'encoder.1.weight']
    assert list(sd) == [str(k) for k in z[case + '/sd_init_keys']]
    assert [_sha(v) for v in sd.values()] == [str(h) for h in z[case + '/sd_init_sha']]
    assert m.get_num_params() == int(z[case + '/num_params'])


def test_init_net_is_the_factory_path():
    """init_net(CoarseDepthLite(...), 'kaiming') is what the reference's factory does for 'lite': same bits as the fixture."""
    z = np.load(GOLDEN)
    nb, base, H, W, B, seed = [int(v) for v in z['sq/meta']]
    torch.manual_seed(seed)
    m = init_net(CoarseDepthLite(2, nb, base, W), 'kaiming')
    assert [_sha(v) for v in m.state_dict().values()] == [str(h) for h in z['sq/sd_init_sha']]


def test_surface_and_parameter_counts():
    m = CoarseDepthLite()
    assert [n for n, _ in m.named_children()] == ['encoder', 'decoder', 'head']
    assert (m.n_bins, m.output_size, m.head.in_channels) == (128, 256, 48)
    assert len(m.encoder) == 15 and len(m.decoder) == 15 and m.head.kernel_size == (3, 3)
    assert isinstance(m.encoder[2], torch.nn.LeakyReLU) and m.encoder[2].negative_slope == 0.2
    assert isinstance(m.decoder[0], torch.nn.ConvTranspose2d) and isinstance(m.decoder[2], torch.nn.ReLU)
    assert not hasattr(m, 'predict_depth')
    assert CoarseDepthLite(2, 128, 64, 256).get_num_params() == 14042560
    assert CoarseDepthLite(2, 16, 48, 256).get_num_params() == 7866112


@pytest.mark.parametrize('case', CASES)
def test_fixture_is_well_conditioned(case):
    """No activation unit on which the reference's own f32 and float64 runs disagree, and the f32 run's gradients within
    1e-5 of the float64 ones: the bars of test_gpu_coarse_lite.py then measure this project, not the seed."""
    z = np.load(GOLDEN)
    assert int(z[case + '/relu_flips']) == 0
    assert float(z[case + '/f64_grad_err']) <= 1e-5
    nb, base, H, W, B, seed = [int(v) for v in z[case + '/meta']]
    assert (B, H, W) == {'sq': (2, 64, 64), 'rect': (2, 96, 64), 'b48': (2, 64, 64)}[case]
    assert (base, nb) == ((48, 16) if case == 'b48' else (64, 128))


def test_set_bin_centers_copies_in_place():
    m = CoarseDepthLite(2, 8, 8, 32)
    buf = m.bin_centers
    m.set_bin_centers(torch.arange(8.0))
    assert m.bin_centers is buf and torch.equal(buf, torch.arange(8.0))
    m.set_bin_centers(torch.arange(4.0))
    assert m.bin_centers.numel() == 4


def test_refusals():
    m = CoarseDepthLite(2, 8, 8, 64)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 2, 64, 64))                     # CPU tensor
    with pytest.raises(RuntimeError):
        m.eval()(torch.zeros(1, 2, 64, 64))
    eng = m.train().engine()                             # the engine's shape check runs before any device work
    assert isinstance(eng, CoarseLiteEngine)
    eng.check_input((3, 2, 64, 64))
    eng.check_input((3, 2, 96, 64))
    for shape in ((1, 2, 64, 32), (1, 2, 128, 128)):
        with pytest.raises(NotImplementedError, match='output_size'):
            eng.check_input(shape)
    with pytest.raises(RuntimeError, match='channels'):
        eng.check_input((1, 3, 64, 64))
    with pytest.raises(RuntimeError, match='divisible by 32'):
        eng.check_input((1, 2, 48, 64))
    for nb in (1, 513):
        with pytest.raises(NotImplementedError, match='n_bins'):
            CoarseDepthLite(2, nb, 8, 64).engine().check_input((1, 2, 64, 64))
    m.compute_dtype = torch.float8_e4m3fn
    with pytest.raises(NotImplementedError, match='mxfp8'):
        m.engine()


def test_factory_still_refuses_and_points_at_the_class():
    from audio_depth_estimation_amd.models import coarse_depth_model as M
    with pytest.raises(NotImplementedError, match='CoarseDepthLite directly'):
        M.define_coarse_depth_model('lite')


def test_train_coarse_depth_help_lists_reference_flags():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'audio_depth_estimation_amd.train_coarse_depth', '--help'],
                         capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    flags = set(re.findall(r'--[a-z_0-9]+', out.stdout))
    for f in ('--dataset', '--sparse_method', '--n_bins', '--bin_mode', '--sid_alpha', '--model_type', '--base_channels',
              '--batch_size', '--learning_rate', '--epochs', '--optimizer', '--ce_weight', '--regression_weight',
              '--use_focal', '--soft_ce_sigma', '--validation', '--validation_iter', '--experiment_name', '--checkpoints',
              '--use_wandb', '--wandb_project', '--wandb_entity', '--precision', '--graph', '--synthetic'):
        assert f in flags, f
    assert re.search(r'\{unet,lite,hybrid,dual_reg\}', out.stdout)


def test_train_coarse_depth_lite_without_synthetic_says_why():
    from audio_depth_estimation_amd import train_dc
    with pytest.raises(NotImplementedError, match='file decoding that is not available'):
        train_dc.main_coarse(['--model_type', 'lite'])


def test_abi_lists_the_thin_stats_kernel_and_rejects_its_bad_shapes():
    from audio_depth_estimation_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'adn.h')).read()
    for name in ('adn_l0_forward_stats', 'adn_l0_forward_stats_num_partials'):
        assert re.search(r'\b' + name + r'\(', text)
        assert name in _lib.symbol_names()
    assert re.search(r'adn_l0_forward_stats:.*?coarse_depth_model\.py:218-219', text, re.S)
    lib = _lib.load()
    assert lib.adn_version() == 3
    assert lib.adn_l0_forward_stats_num_partials(2, 3, 16) >= 1
    assert lib.adn_l0_forward_stats_num_partials(2, 3, 24) == -1 and lib.adn_l0_forward_stats_num_partials(0, 3, 16) == -1
    # one partial row per workgroup of at most 2048: the count the engine allocates never exceeds it
    assert lib.adn_l0_forward_stats_num_partials(16, 128, 128) <= 2048
    p = 16                                               # non-NULL placeholders: rejected before any launch
    for cin, cout, ws, what in ((2, 32, 16, b'2 -> 64'), (3, 64, 16, b'2 -> 64'), (2, 64, 24, b'Ws % 16'), (2, 64, 8, b'Ws % 16')):
        assert lib.adn_l0_forward_stats(p, p, None, 2, 3, ws, cin, cout, p, p, None) == -1
        assert b'adn_l0_forward_stats' in lib.adn_last_error() and what in lib.adn_last_error()
    assert lib.adn_l0_forward_stats(None, p, None, 2, 3, 16, 2, 64, p, p, None) == -1
    assert b'null' in lib.adn_last_error()


def _lite_layers(base):
    enc = [(2, base), (base, 2 * base), (2 * base, 4 * base), (4 * base, 8 * base), (8 * base, 8 * base)]
    dec = [(8 * base, 8 * base), (8 * base, 4 * base), (4 * base, 2 * base), (2 * base, base), (base, base)]
    return enc, dec


def test_base64_layers_do_not_fall_to_the_direct_form():
    """Every GEMM of the base-64 network at 256 x 256, B = 16, bf16 (forward, eval forward, input gradient) except the thin
    first layer's runs an MFMA form; the new planner shapes are T2 128 x 128 64 -> 64 and S2 128 x 128 from the padded input."""
    T, B = torch.bfloat16, 16
    enc, dec = _lite_layers(64)
    plans, h = {}, 256
    for i, (ci, co) in enumerate(enc):
        h //= 2
        for epi in (EPI_Z_STATS, EPI_ACT):
            plans[f'enc{i} fwd epi{epi}'] = K.igemm_describe(T, GEMM_S2, B, h, h, 8 if i == 0 else ci, 0, co, [co], epi=epi)
        if i:
            plans[f'enc{i} dgrad'] = K.igemm_describe(T, GEMM_T2, B, h, h, co, 0, ci, [ci], epi=EPI_BWD)
    for i, (ci, co) in enumerate(dec):
        for epi in (EPI_Z_STATS, EPI_ACT):
            plans[f'dec{i} fwd epi{epi}'] = K.igemm_describe(T, GEMM_T2, B, h, h, ci, 0, co, [co], epi=epi)
        plans[f'dec{i} dgrad'] = K.igemm_describe(T, GEMM_S2, B, h, h, co, 0, ci, [ci], epi=EPI_BWD)
        h *= 2
    assert h == 256
    plans['head fwd'] = K.igemm_describe(T, GEMM_S1, B, 256, 256, 64, 0, 128, [128], ks=3, epi=EPI_ACT)
    plans['head dgrad'] = K.igemm_describe(T, GEMM_S1, B, 256, 256, 128, 0, 64, [64], ks=3, epi=EPI_ADD)
    forms = {k: v.split()[0] for k, v in plans.items()}
    assert len(forms) == 5 * 2 + 4 + 5 * 3 + 2
    for k, f in forms.items():
        assert f in ('tile', 'patch', 'patch-tall', 'patch-pair', 'ring'), (k, plans[k])
    # base 48 (the class default) is the documented caveat: correct, on the generic form
    assert K.igemm_describe(T, GEMM_S2, 2, 16, 16, 48, 0, 96, [96], epi=EPI_Z_STATS).split()[0] == 'direct'


def test_thin_route_condition():
    """bf16, 2 -> 64 channels, small-grid width a multiple of 32 (adn_thin_wgrad's K-step); ADN_LITE_L0_IGEMM=1 selects the
    adn_igemm route."""
    from types import SimpleNamespace
    from audio_depth_estimation_amd.dc_engine import ConvK4BNAct
    m = CoarseDepthLite(2, 8, 64, 64)
    bf, f32 = SimpleNamespace(dtype=torch.bfloat16), SimpleNamespace(dtype=torch.float32)
    os.environ.pop('ADN_LITE_L0_IGEMM', None)
    assert ConvK4BNAct.thin_ok(bf, m.encoder[0], 64) and ConvK4BNAct.thin_ok(bf, m.encoder[0], 256)
    assert not ConvK4BNAct.thin_ok(bf, m.encoder[0], 32) and not ConvK4BNAct.thin_ok(bf, m.encoder[0], 96)
    assert not ConvK4BNAct.thin_ok(f32, m.encoder[0], 64)
    assert not ConvK4BNAct.thin_ok(bf, CoarseDepthLite(2, 8, 48, 64).encoder[0], 64)
    assert not ConvK4BNAct.thin_ok(bf, CoarseDepthLite(3, 8, 64, 64).encoder[0], 64)
    os.environ['ADN_LITE_L0_IGEMM'] = '1'
    try:
        assert not ConvK4BNAct.thin_ok(bf, m.encoder[0], 64)
    finally:
        del os.environ['ADN_LITE_L0_IGEMM']
