"""CPU-only: the host side of the coarse-depth family's evaluation (test_coarse_depth.py, adn_coarse_decode /
adn_coarse_eval_stats argument checks, the float64 restatement of adn_coarse_eval_finish that the GPU tests use as oracle).
"""
import ctypes
import math

import pytest
import torch

import coarse_decode_cases as cc


def test_parser_lists_the_flags():
    from audio_depth_estimation_amd import test_coarse_depth as T
    from audio_depth_estimation_amd.test import build_parser
    flags = {o for a in T.build_parser()._actions for o in a.option_strings}
    assert {o for a in build_parser()._actions for o in a.option_strings} <= flags          # test.py's
    assert {'--model_type', '--n_bins', '--bin_mode', '--sid_alpha', '--base_channels', '--sparse_method', '--decode'} <= flags
    a = T.build_parser().parse_args([])
    assert (a.model_type, a.n_bins, a.bin_mode, a.sid_alpha, a.base_channels, a.sparse_method, a.decode) == \
        ('unet', 128, 'linear', 0.6, 64, 'downup_015', 'soft')
    for flag, bad in (('--model_type', 'resnet'), ('--decode', 'median'), ('--bin_mode', 'sqrt')):
        with pytest.raises(SystemExit):
            T.build_parser().parse_args([flag, bad])
    assert T.build_parser().parse_args(['--model_type', 'dual_reg', '--decode', 'hard']).decode == 'hard'


@pytest.mark.parametrize('argv', [[], ['--model_type', 'hybrid']])
def test_real_dataset_is_refused_as_the_trainer_refuses_it(argv):
    from audio_depth_estimation_amd import test_coarse_depth as T
    with pytest.raises(NotImplementedError, match='file decoding that is not available'):
        T.main(argv)


def test_argument_validation_without_gpu():
    from audio_depth_estimation_amd import _lib
    lib = _lib.load()
    assert lib.adn_coarse_decode(None, None) == -1
    assert b'adn_coarse_decode' in lib.adn_last_error()
    assert lib.adn_coarse_eval_stats(None, None) == -1
    assert b'adn_coarse_eval_stats' in lib.adn_last_error()
    assert lib.adn_coarse_eval_stats_workspace_bytes(0) == -1
    assert lib.adn_coarse_eval_stats_workspace_bytes(1) == cc.N_SUMS * 8
    assert lib.adn_coarse_eval_finish(None, 0, None, None, None) == -1
    assert b'adn_coarse_eval_finish' in lib.adn_last_error()
    # a descriptor with operands (never dereferenced on the host) and one thing wrong at a time
    buf = (ctypes.c_float * 8)()
    addr = ctypes.addressof(buf)

    def desc(**kw):
        d = _lib.AdnCoarseDecode()
        d.logits, d.centers, d.mean, d.dtype, d.nb, d.ld, d.pixels = addr, addr, addr, _lib.ADN_F32, 8, 8, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for kw, word in ((dict(nb=1), b'n_bins'), (dict(nb=513, ld=520), b'n_bins'), (dict(ld=7), b'row stride'),
                     (dict(mean=None), b'every output is NULL'), (dict(dtype=7), b'dtype'), (dict(pixels=0), b'no pixels')):
        assert lib.adn_coarse_decode(ctypes.byref(desc(**kw)), None) == -1, kw
        err = lib.adn_last_error()
        assert b'adn_coarse_decode' in err and word in err, (kw, err)
    e = _lib.AdnCoarseEvalStats()
    assert lib.adn_coarse_eval_stats(ctypes.byref(e), None) == -1
    assert b'adn_coarse_eval_stats' in lib.adn_last_error()


def test_kernel_wrappers_refuse_host_tensors():
    from audio_depth_estimation_amd import kernels as K
    with pytest.raises(RuntimeError, match='device tensors'):
        K.coarse_decode(torch.zeros(4, 8), 8, torch.zeros(8), mean=torch.zeros(4))
    with pytest.raises(RuntimeError, match='device tensors'):
        K.coarse_eval_finish(None, 0, torch.zeros(K.EVAL_SUMS, dtype=torch.float64))
    assert (K.EVAL_SUMS, K.EVAL_OUT, K.EVAL_FIELDS) == (cc.N_SUMS, cc.N_OUT, cc.FIELDS)


def test_only_the_classifiers_have_a_distribution():
    from audio_depth_estimation_amd.models import coarse_depth_model as M
    assert not hasattr(M.DualRegressionModel, 'predict_distribution')
    for cls in (M.CoarseDepthUNet, M.CoarseDepthLite, M.CoarseWithOffsetModel):
        assert callable(cls.predict_distribution)
    from audio_depth_estimation_amd.coarse_engine import CoarseDistribution, HybridDistribution
    assert CoarseDistribution._fields == ('mean', 'hard', 'std', 'entropy', 'confidence', 'argmax')
    assert HybridDistribution._fields == CoarseDistribution._fields + ('offset', 'final')


def test_predict_distribution_refuses_what_forward_refuses():
    from audio_depth_estimation_amd.models.coarse_depth_model import CoarseDepthUNet
    m = CoarseDepthUNet(2, 8, 8, output_size=32).eval()
    x = torch.zeros(1, 2, 32, 32)
    errs = []
    for call in (m, m.predict_distribution):
        with pytest.raises(RuntimeError) as ei:
            call(x)
        errs.append(str(ei.value))
    assert errs[0] == errs[1] and 'no CPU path' in errs[0]


def test_finish_restatement_on_hand_made_sums():
    """Four valid pixels: std (1, 2, 3, 4) against error (2, 4, 6, 8) -> correlation 1; three of four bins right;
    reliability: two pixels at confidence 0.95 both right, two at 0.55 one right -> ECE = 0.5 * 0.05 + 0.5 * 0.05."""
    s = torch.zeros(cc.N_SUMS, dtype=torch.float64)
    s[:11] = torch.tensor([4, 3, 4, 1, 10, 2.0, 3.0, 20, 30, 120, 60], dtype=torch.float64)
    s[cc.TABLE + 15:cc.TABLE + 18] = torch.tensor([2, 1.1, 1], dtype=torch.float64)
    s[cc.TABLE + 27:cc.TABLE + 30] = torch.tensor([2, 1.9, 2], dtype=torch.float64)
    out = cc.finish_ref(s)
    want = dict(n_valid=4, top1=0.75, within1=1.0, mean_bin_error=0.25, mean_std=2.5, mean_entropy=0.5,
                mean_confidence=0.75, std_error_corr=1.0, ece=0.05)
    for k, name in enumerate(cc.FIELDS):
        assert abs(float(out[k]) - want[name]) <= 1e-12, (name, float(out[k]))
    assert torch.equal(out[9:], s[cc.TABLE:])
    # a constant std has no correlation; anti-correlated errors give -1
    s2 = s.clone()
    s2[8] = 25.0                                              # sum s^2 = (sum s)^2 / n
    assert math.isnan(float(cc.finish_ref(s2)[7])) and float(cc.finish_ref(s2)[8]) == float(out[8])
    s3 = s.clone()
    s3[10] = 40.0                                             # s (1, 2, 3, 4) against a (8, 6, 4, 2)
    assert abs(float(cc.finish_ref(s3)[7]) + 1.0) <= 1e-12
    # no valid pixel: counts 0, every ratio NaN
    z = cc.finish_ref(torch.zeros(cc.N_SUMS, dtype=torch.float64))
    assert float(z[0]) == 0.0 and bool(torch.isnan(z[1:9]).all()) and float(z[9:].abs().sum()) == 0.0


def test_eval_sums_restatement_bins_confidence_in_f32():
    conf = torch.tensor([0.05, 0.1, 0.7, 1.0, 0.3], dtype=torch.float32)       # f32(0.7) * 10 floors to 7, f32(0.3) * 10 to 3
    n = conf.numel()
    am, bn = torch.tensor([3, 4, 5, 6, 0]), torch.tensor([3, 5, 7, 6, 0])
    gt = torch.tensor([1.0, 2.0, 3.0, 4.0, 0.0])
    sums = cc.eval_sums_ref(am, bn, conf, torch.ones(n), torch.ones(n), gt + 0.5, gt)
    assert sums[:4].tolist() == [4.0, 2.0, 3.0, 3.0]
    assert sums[cc.TABLE::3].tolist() == [1, 1, 0, 0, 0, 0, 0, 1, 0, 1]
    assert sums[7].item() == 2.0 and sums[9].item() == 1.0
