"""GPU parity of the coarse-depth family's evaluation side (csrc/coarse_decode.hip, ClassLogits.decode,
predict_distribution, test_coarse_depth.py).

  * adn_coarse_decode against a float64 softmax of the same stored logits (bf16: the rounded values upcast), on every
    kernel form of test_gpu_coarse.py's loss test (f32 / bf16, each vector width, wave per pixel, padded rows) at 1, 63,
    257 and 2 046 pixels and, bf16, just past one pass of the 8- and 128-bin grids.  Rows: 3 randn, every third 40 randn
    (sharp), one all-zero tie, one -80 / +80 spike.  mean and argmax carry the bits of the forward-only adn_coarse_loss;
    hard == centers[argmax]; two runs into poisoned buffers are bit-identical; an output left out leaves the others as
    they were; std^2, entropy and confidence <= 2e-4 of their scales ((c_max - c_min)^2, ln nb, 1: the bar
    test_coarse_loss_vs_float64 grants the same fast exp / log on the soft depth; an f32 torch evaluation of the same
    formulas stays below 4e-7 of scale on these inputs, so the reference is far inside the bar);
  * adn_coarse_eval_stats / _finish against float64 torch on the same planes (coarse_decode_cases.py): counts exact, real
    sums <= 1e-10 relative (f64 summation of <= 6e5 f32 values in another order: N 2^-53), ECE and the correlation
    <= 1e-9; no valid pixel -> n = 0 and NaN ratios; the sums of two halves added up finish like the whole;
  * predict_distribution on the three classifiers: mean / hard / final bit-equal to forward / predict_depth, spread
    figures against a float64 softmax of the returned logits, no engine state leaking into the next training steps;
  * the command line on a checkpoint train_coarse_depth just wrote, for the four model types.
"""
import math

import pytest
import torch

import coarse_decode_cases as cc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 2e-4
PLANES = ('mean', 'hard', 'std', 'entropy', 'confidence', 'argmax')


def _bins_of(nb, mode='linear'):
    from audio_depth_estimation_amd.dataloader.utils_dataset import compute_bins
    return compute_bins(nb, mode, None, 30.0, 0.6)


def _logits(dtype, nb, ld, pixels, seed=0):
    g = torch.Generator().manual_seed(7000 + 13 * nb + pixels + seed)
    x = 3.0 * torch.randn(pixels, ld, generator=g)
    x[::3] = 40.0 * torch.randn(x[::3].shape, generator=g)                    # sharp rows
    if pixels > 5:
        x[5, :nb] = 0.0                                                       # a tie: bin 0 wins, 1 / nb, ln nb
    if pixels > 7:
        x[7, :nb] = -80.0                                                     # a spike: std and entropy collapse
        x[7, nb // 2] = 80.0
    return x.to(dtype)


def _poisoned(pixels):
    out = {k: torch.full((pixels,), float('nan'), device=DEV) for k in PLANES[:-1]}
    out['argmax'] = torch.full((pixels,), -7, dtype=torch.int32, device=DEV)
    return out


def _decode_case(dtype, nb, ld, pixels):
    from audio_depth_estimation_amd import kernels as K
    _, centers = _bins_of(nb)
    logits = _logits(dtype, nb, ld, pixels)
    lg, cen = logits.to(DEV), centers.to(DEV)
    runs = []
    for _ in range(2):
        out = _poisoned(pixels)
        K.coarse_decode(lg, nb, cen, **out)
        runs.append({k: v.cpu() for k, v in out.items()})
    for k in PLANES:
        assert torch.equal(runs[0][k].view(torch.uint8), runs[1][k].view(torch.uint8)), k
    got = runs[0]
    # the bits of the forward-only loss launch
    depth, am = torch.empty(pixels, device=DEV), torch.empty(pixels, dtype=torch.int32, device=DEV)
    K.coarse_loss(lg, nb, cen, depth, argmax=am)
    assert torch.equal(got['mean'].view(torch.int32), depth.cpu().view(torch.int32))
    assert torch.equal(got['argmax'], am.cpu())
    assert torch.equal(got['hard'], centers[got['argmax'].long()])
    # every output is optional: each alone, and all but each, give the same bits
    for k in PLANES:
        solo = _poisoned(pixels)
        K.coarse_decode(lg, nb, cen, **{k: solo[k]})
        assert torch.equal(solo[k].cpu().view(torch.uint8), got[k].view(torch.uint8)), k
        rest = {j: v for j, v in _poisoned(pixels).items() if j != k}
        K.coarse_decode(lg, nb, cen, **rest)
        for j, v in rest.items():
            assert torch.equal(v.cpu().view(torch.uint8), got[j].view(torch.uint8)), (k, j)
    ref = cc.decode_ref(logits[:, :nb].double(), centers.double())
    assert torch.equal(got['argmax'].long(), ref['argmax'])
    span2 = float(centers.max() - centers.min()) ** 2
    err = {'std^2': float((got['std'].double() ** 2 - ref['var']).abs().max()) / span2,
           'entropy': float((got['entropy'].double() - ref['entropy']).abs().max()) / math.log(nb),
           'confidence': float((got['confidence'].double() - ref['confidence']).abs().max()),
           'mean': float((got['mean'].double() - ref['mean']).abs().max()) / float(centers.max() - centers.min())}
    print(f'{dtype} nb {nb} ld {ld} pixels {pixels}: ' + ' '.join(f'{k} {v:.2e}' for k, v in err.items()))
    assert bool(torch.isfinite(got['std']).all()) and float(got['std'].min()) >= 0.0
    assert bool(torch.isfinite(got['entropy']).all()) and float(got['entropy'].min()) >= 0.0
    for k, v in err.items():
        assert v <= TOL, (k, v)
    if pixels > 7:
        assert int(got['argmax'][5]) == 0 and abs(float(got['confidence'][5]) - 1.0 / nb) <= TOL
        assert abs(float(got['entropy'][5]) - math.log(nb)) <= TOL * math.log(nb)
        assert int(got['argmax'][7]) == nb // 2 and float(got['std'][7]) == 0.0 and float(got['entropy'][7]) == 0.0
        assert float(got['confidence'][7]) == 1.0


@pytest.mark.parametrize('pixels', [2 * 33 * 31, 1, 63, 257])
@pytest.mark.parametrize('nb,ld', [(2, 8), (8, 64), (100, 128), (128, 128), (256, 256), (8, 8), (16, 16), (32, 32), (64, 64),
                                   (512, 512), (24, 24)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_coarse_decode_vs_float64(dtype, nb, ld, pixels):
    _decode_case(dtype, nb, ld, pixels)


@pytest.mark.parametrize('nb,pixels', [(8, 2048 * 4 * 64 + 1), (128, 2048 * 4 * 4 + 1)])
def test_coarse_decode_vs_float64_past_one_grid_pass(nb, pixels):
    """One pixel more than the 2048-block grid of that vector width serves in one pass (64 / (nb / 8) pixels per wave)."""
    _decode_case(torch.bfloat16, nb, nb, pixels)


def test_coarse_decode_rejects_bad_arguments():
    from audio_depth_estimation_amd import kernels as K
    lg = torch.zeros(4, 520, device=DEV)
    for nb in (1, 520):
        with pytest.raises(RuntimeError, match='adn_coarse_decode.*n_bins'):
            K.coarse_decode(lg, nb, torch.zeros(nb, device=DEV), mean=torch.empty(4, device=DEV))
    with pytest.raises(RuntimeError, match='adn_coarse_decode.*every output is NULL'):
        K.coarse_decode(lg, 8, torch.zeros(8, device=DEV))
    with pytest.raises(RuntimeError, match='coarse_decode: std has 3 elements'):
        K.coarse_decode(lg, 8, torch.zeros(8, device=DEV), std=torch.empty(3, device=DEV))


# ------------------------------------------------------------------------------------------------------- evaluation sums
def _planes_case(pixels, all_invalid=False):
    """Planes of adn_coarse_decode (8 bins, bf16) with gt as in test_gpu_coarse._loss_case: ~10 % zeros."""
    from audio_depth_estimation_amd import kernels as K
    nb = 8
    edges, centers = _bins_of(nb)
    out = _poisoned(pixels)
    K.coarse_decode(_logits(torch.bfloat16, nb, nb, pixels, seed=1).to(DEV), nb, centers.to(DEV), **out)
    g = torch.Generator().manual_seed(31 + pixels)
    gt = 31.0 * torch.rand(pixels, generator=g)
    gt[torch.rand(pixels, generator=g) < 0.1] = 0.0
    if all_invalid:
        gt.zero_()
    elif not bool((gt > 0).any()):
        gt[0] = 15.5
    bins = torch.clamp(torch.bucketize(gt, edges[1:-1].contiguous()), 0, nb - 1).int()
    return out, bins.to(DEV), gt.to(DEV)


def _eval(planes, bins, gt, sl=slice(None)):
    from audio_depth_estimation_amd import kernels as K
    n = gt[sl].numel()
    ws = torch.full((K.coarse_eval_stats_workspace_bytes(n) // 8 + 1,), float('nan'), dtype=torch.float64, device=DEV)
    sums = torch.full((K.EVAL_SUMS,), float('nan'), dtype=torch.float64, device=DEV)
    out = torch.full((K.EVAL_OUT,), -1.0, dtype=torch.float64, device=DEV)
    c = lambda t: t[sl].contiguous()
    K.coarse_eval_stats(c(planes['argmax']), c(bins), c(planes['confidence']), c(planes['std']), c(planes['entropy']),
                        c(planes['mean']), c(gt), ws)
    K.coarse_eval_finish(ws, n, sums, out)
    return sums, out


def _close(a, b, rel):
    return bool(((a - b).abs() <= rel * b.abs()).all())


@pytest.mark.parametrize('pixels', [1, 257, 2 * 33 * 31, 2048 * 256 + 1])
def test_eval_stats_vs_float64(pixels):
    from audio_depth_estimation_amd import kernels as K
    planes, bins, gt = _planes_case(pixels)
    sums, out = _eval(planes, bins, gt)
    sums2, out2 = _eval(planes, bins, gt)
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64)) and torch.equal(out.view(torch.int64), out2.view(torch.int64))
    cpu = {k: v.cpu() for k, v in planes.items()}
    want = cc.eval_sums_ref(cpu['argmax'], bins.cpu(), cpu['confidence'], cpu['std'], cpu['entropy'], cpu['mean'], gt.cpu())
    sums, out = sums.cpu(), out.cpu()
    counts = [0, 1, 2, 3] + list(range(cc.TABLE, cc.N_SUMS, 3)) + list(range(cc.TABLE + 2, cc.N_SUMS, 3))
    assert torch.equal(sums[counts], want[counts]), (sums[counts], want[counts])
    assert float(want[cc.TABLE::3].sum()) == float(want[0]) == float((gt > 0).sum())
    print(f'pixels {pixels}: sums rel err {float(((sums - want).abs() / want.abs().clamp(min=1e-300)).max()):.2e}')
    assert _close(sums, want, 1e-10)
    ref = cc.finish_ref(want)
    assert float(out[0]) == float(ref[0])
    assert _close(out[1:7], ref[1:7], 1e-10) and torch.equal(out[9:], sums[cc.TABLE:])
    assert abs(float(out[8]) - float(ref[8])) <= 1e-9 and 0.0 <= float(out[8]) <= 1.0
    if pixels == 1:
        assert math.isnan(float(out[7])) and math.isnan(float(ref[7]))        # one pixel has no variance
    else:
        assert abs(float(out[7]) - float(ref[7])) <= 1e-9 and -1.0 <= float(out[7]) <= 1.0
    # the sums of two halves, added up on the device, finish like the whole
    if pixels > 1:
        h = pixels // 2
        a, _ = _eval(planes, bins, gt, slice(0, h))
        b, _ = _eval(planes, bins, gt, slice(h, None))
        tot = a + b
        split = torch.full((K.EVAL_OUT,), -1.0, dtype=torch.float64, device=DEV)
        K.coarse_eval_finish(None, 0, tot, split)
        split = split.cpu()
        assert torch.equal(tot.cpu()[counts], want[counts])
        assert torch.equal(split[[0] + list(range(9, cc.N_OUT, 3))], out[[0] + list(range(9, cc.N_OUT, 3))])
        assert _close(split[1:7], out[1:7], 1e-10) and abs(float(split[8] - out[8])) <= 1e-9
        assert abs(float(split[7] - out[7])) <= 1e-9
        assert torch.equal(cc.finish_ref(tot.cpu())[[0, 1, 2, 3]], split[[0, 1, 2, 3]])


def test_eval_stats_without_a_valid_pixel():
    planes, bins, gt = _planes_case(2 * 33 * 31, all_invalid=True)
    sums, out = _eval(planes, bins, gt)
    assert float(sums.abs().sum()) == 0.0
    out = out.cpu()
    assert float(out[0]) == 0.0 and bool(torch.isnan(out[1:9]).all()) and float(out[9:].abs().sum()) == 0.0


def test_eval_stats_rejects_a_small_workspace():
    from audio_depth_estimation_amd import kernels as K
    planes, bins, gt = _planes_case(257)
    with pytest.raises(RuntimeError, match='adn_coarse_eval_stats.*workspace'):
        K.coarse_eval_stats(planes['argmax'], bins, planes['confidence'], planes['std'], planes['entropy'], planes['mean'], gt,
                            torch.empty(4, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------------------- models
def _unet(dtype, seed=0):
    from audio_depth_estimation_amd.models.coarse_depth_model import define_coarse_depth_model
    torch.manual_seed(seed)
    m = define_coarse_depth_model('unet', 2, 16, 16, 32)
    m.compute_dtype = dtype
    m = m.to(DEV)
    m.set_bin_centers(_bins_of(16)[1].to(DEV))
    return m


def _lite(dtype, seed=0):
    from audio_depth_estimation_amd.models.coarse_depth_model import CoarseDepthLite, init_net
    torch.manual_seed(seed)
    m = init_net(CoarseDepthLite(2, 16, 64, 64), 'kaiming')
    m.compute_dtype = dtype
    m = m.to(DEV)
    m.set_bin_centers(_bins_of(16)[1].to(DEV))
    return m


def _hybrid(dtype, seed=0):
    from audio_depth_estimation_amd.models.coarse_depth_model import CoarseWithOffsetModel
    torch.manual_seed(seed)
    m = CoarseWithOffsetModel(2, 16, 16, 32)
    m.compute_dtype = dtype
    m = m.to(DEV)
    m.set_bin_centers(_bins_of(16)[1].to(DEV))
    return m


def _check_spread(dist, logits_nchw, centers):
    nb = logits_nchw.shape[1]
    ref = cc.decode_ref(logits_nchw.permute(0, 2, 3, 1).reshape(-1, nb).double().cpu(), centers.double().cpu())
    flat = lambda t: t.reshape(-1).double().cpu()
    span2 = float(centers.max() - centers.min()) ** 2
    assert float((flat(dist.std) ** 2 - ref['var']).abs().max()) <= TOL * span2
    assert float((flat(dist.entropy) - ref['entropy']).abs().max()) <= TOL * math.log(nb)
    assert float((flat(dist.confidence) - ref['confidence']).abs().max()) <= TOL
    assert torch.equal(dist.argmax.reshape(-1).long().cpu(), ref['argmax'])
    assert torch.equal(dist.hard, centers[dist.argmax.long()])
    assert float(dist.std.min()) >= 0.0 and bool(torch.isfinite(dist.std).all())


@pytest.mark.parametrize('make,dtype,S', [(_unet, torch.float32, 32), (_unet, torch.bfloat16, 32), (_lite, torch.bfloat16, 64)])
def test_predict_distribution_matches_forward(make, dtype, S):
    m = make(dtype).eval()
    x = torch.rand(2, 2, S, S, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        logits, depth = m(x)
        dist = m.predict_distribution(x)
        again = m.predict_distribution(x)
        logits2, depth2 = m(x)
    assert dist._fields == PLANES and all(t.shape == (2, 1, S, S) for t in dist)
    assert dist.argmax.dtype == torch.int32 and all(t.dtype == torch.float32 for t in dist[:-1])
    assert torch.equal(dist.mean.view(torch.int32), depth.view(torch.int32))
    assert torch.equal(depth2, depth) and torch.equal(logits2, logits)
    for a, b in zip(dist, again):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()                # clones, not the engine's planes
    if hasattr(m, 'predict_depth'):
        assert torch.equal(dist.hard, m.predict_depth(x, mode='hard'))
    _check_spread(dist, logits, m.bin_centers)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_predict_distribution_hybrid(dtype):
    m = _hybrid(dtype).eval()
    x = torch.rand(2, 2, 32, 32, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        logits, coarse, offset, final = m(x)
        dist = m.predict_distribution(x)
        again = m.predict_distribution(x)
    assert dist._fields == PLANES + ('offset', 'final') and all(t.shape == (2, 1, 32, 32) for t in dist)
    assert torch.equal(dist.mean.view(torch.int32), coarse.view(torch.int32))
    assert torch.equal(dist.offset, offset) and torch.equal(dist.final.view(torch.int32), final.view(torch.int32))
    for a, b in zip(dist, again):
        assert torch.equal(a, b)
    _check_spread(dist, logits, m.bin_centers)


def test_predict_distribution_refuses_what_forward_refuses():
    m = _unet(torch.float32).eval()
    for x in (torch.rand(1, 3, 32, 32, device=DEV), torch.rand(1, 2, 32, 64, device=DEV), torch.rand(1, 2, 32, 32)):
        errs = []
        for call in (m, m.predict_distribution):
            with pytest.raises((RuntimeError, NotImplementedError)) as ei:
                call(x)
            errs.append((type(ei.value), str(ei.value)))
        assert errs[0] == errs[1]


def test_training_steps_do_not_see_a_decode_in_between():
    """Two fused steps with an eval-mode predict_distribution (at the training batch shape) between them leave the terms,
    the parameters and the buffers of two steps without it, bit for bit: the decode keeps no engine state."""
    from audio_depth_estimation_amd.coarse_engine import CoarseDepthTrainer
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 2, 32, 32, generator=g).to(DEV)
    gt = (30.0 * torch.rand(2, 1, 32, 32, generator=g)).to(DEV)
    edges = _bins_of(16)[0].to(DEV)
    results = []
    for peek in (False, True):
        m = _unet(torch.float32, seed=11).train()
        tr = CoarseDepthTrainer(m.engine(), 'soft', optimizer='AdamW', lr=1e-3, clip_norm=1.0)
        terms = []
        for i in range(2):
            terms.append(tr.step(x, None, gt, edges=edges)[1].clone())
            if peek and i == 0:
                m.eval()
                with torch.no_grad():
                    m.predict_distribution(x)
                m.train()
        results.append((torch.stack(terms).cpu(), [p.detach().cpu().clone() for p in m.parameters()],
                        [b.detach().cpu().clone() for b in m.buffers()]))
    (ta, pa, ba), (tb, pb, bb) = results
    assert torch.equal(ta.view(torch.int32), tb.view(torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(pa, pb)) and all(torch.equal(a, b) for a, b in zip(ba, bb))


# -------------------------------------------------------------------------------------------------------- command line
@pytest.mark.parametrize('model_type,S,extra', [('unet', 32, ['--base_channels', '16', '--n_bins', '16']),
                                                ('lite', 64, ['--n_bins', '16']),
                                                ('hybrid', 32, ['--base_channels', '16', '--n_bins', '16']),
                                                ('dual_reg', 32, ['--base_channels', '16'])])
def test_test_coarse_depth_on_a_fresh_checkpoint(model_type, S, extra, tmp_path, monkeypatch, capsys):
    from audio_depth_estimation_amd import test_coarse_depth as T
    from audio_depth_estimation_amd import train_dc

    def small(load):
        def patched(*a, **k):
            cfg = load(*a, **k)
            cfg.dataset.images_size, cfg.mode.saving_checkpoints = S, 1
            return cfg
        return patched
    monkeypatch.setattr(train_dc, 'load_config', small(train_dc.load_config))
    monkeypatch.setattr(T, 'load_config', small(T.load_config))
    monkeypatch.chdir(tmp_path)
    train_dc.main_coarse(['--model_type', model_type, '--synthetic', '8', '--epochs', '1', '--batch_size', '4',
                          '--precision', 'f32', '--validation', 'false'] + extra)
    nb = 16 if model_type != 'dual_reg' else 128
    folder = tmp_path / 'checkpoints' / f'coarse_downup_015_linear{nb}_{model_type}_exp1'
    assert (folder / 'checkpoint_1.pth').exists()
    capsys.readouterr()
    argv = ['--model_type', model_type, '--synthetic', '8', '--batch_size', '4', '--precision', 'f32'] + extra
    by_path = T.main(argv + ['--checkpoint_path', str(folder / 'checkpoint_1.pth')])
    text = capsys.readouterr().out
    again = T.main(argv + ['--checkpoints', '1'])                       # the trainer's folder, resolved from the flags
    hard = T.main(argv + ['--checkpoints', '1', '--decode', 'hard'])
    depth_keys = ['abs_rel', 'rmse', 'delta1', 'delta2', 'delta3', 'log10', 'mae']
    assert by_path == again or all(by_path[k] == again[k] or (math.isnan(by_path[k]) and math.isnan(again[k])) for k in by_path)
    assert set(by_path) == set(again) and all(math.isfinite(by_path[k]) for k in depth_keys)
    assert 'RMSE' in text and 'Eval Dataset of 8 instances' in text
    stats_file = (tmp_path / 'eval' / 'batvisionv2' / 'test' /
                  f'stats_on_batvisionv2_test_set_coarse_downup_015_linear{nb}_{model_type}_exp1_epoch_1.pt')
    assert stats_file.exists(), list((tmp_path).rglob('*.pt'))
    st = torch.load(stats_file, map_location='cpu', weights_only=False)
    for k in depth_keys + ['loss']:
        assert st[k].ndim == 1
    assert st['gt_images'].shape == st['pred_imgs'].shape == (8, S, S) and st['rmse'].shape == (8,)
    cls_keys = ['top1', 'within1', 'mean_bin_error', 'ece', 'std_error_corr']
    if model_type == 'dual_reg':
        assert 'no class head' in text and set(by_path) == set(depth_keys) and 'pred_std' not in st
        assert hard == by_path
        return
    assert 0.0 <= by_path['top1'] <= by_path['within1'] <= 1.0 and 0.0 <= by_path['ece'] <= 1.0
    assert by_path['mean_std'] > 0.0 and by_path['mean_entropy'] > 0.0 and 0.0 < by_path['mean_confidence'] <= 1.0
    assert by_path['n_valid'] == float((st['gt_images'] > 0).sum())
    assert 'Top-1 bin accuracy' in text and 'ECE' in text
    for k in ('pred_std', 'pred_entropy', 'pred_confidence'):
        assert st[k].shape == (8, S, S) and st[k].dtype == torch.float32
    assert st['reliability'].shape == (10, 3) and float(st['reliability'][:, 0].sum()) == by_path['n_valid']
    assert st['decode'] == 'hard' and all(isinstance(st[k], float) for k in cls_keys)
    assert [st[k] for k in cls_keys[:4]] == [hard[k] for k in cls_keys[:4]]
    # the decode changes the depth it scores, never the distribution
    changed = 'coarse_rmse' if model_type == 'hybrid' else 'rmse'
    assert hard[changed] != by_path[changed]
    for k in cc.FIELDS:
        assert hard[k] == by_path[k] or (math.isnan(hard[k]) and math.isnan(by_path[k])), k
    if model_type == 'hybrid':
        assert all(hard[k] == by_path[k] for k in depth_keys)               # final = soft coarse + offset either way
        assert all(math.isfinite(by_path['coarse_' + k]) for k in depth_keys)
