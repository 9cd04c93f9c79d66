"""GPU parity of the coarse-depth classification family (csrc/coarse.hip, coarse_engine, models.coarse_depth_model).

  * adn_coarse_targets against torch.bucketize / clamp / count: exact, including values that sit on an edge;
  * adn_coarse_loss against a float64 torch-CPU restatement with autograd (written here with log_softmax), on the same
    inputs (bf16 logits: the bf16-rounded values upcast to f64), on every kernel form (f32 / bf16, each vector width, wave
    per pixel, padded rows) at 1, 63, 257 and ~2 048 pixels and, bf16, just past one pass of the 8- and 128-bin grids.
    Bars: depth and the three terms <= 2e-4 relative;
    dlogits f32 <= 2e-4 of max|ref|; dlogits bf16 per element <= 2^-8 |ref| + 2e-4 max|ref| (one bf16 rounding of the output
    plus the f32 bar); padding columns exactly 0; two runs bit-identical; argmax == torch.argmax;
  * the model and the fused step against the golden vectors of the REFERENCE (tests/golden/coarse32_bc64.npz), f32 compute,
    soft / focal / ce: eval depth and sampled logits <= 2e-4, terms <= 2e-4, per-parameter gradient norm <= 5e-3, sampled
    entries <= 5e-3 of the tensor max (the bars of test_gpu_baseres.py); clipped norm <= 2e-3, sampled parameters after AdamW
    <= 0.05 lr where |g| > 1e-2 max|g| (Adam's sign-like step is ill-conditioned where g ~ 0), BatchNorm buffers <= 1e-4 of
    their max (the f32 bars of test_gpu_cvae.py's full-width case); bf16 compute: terms within 2e-2 (the bar of smoke());
  * trainer behaviour: reference-style autograd loop == fused step, device binning == supplied bins, graph replay with an
    eval at another batch size in between == eager, graph steps across a learning-rate change == eager, state_dict
    resume, the command line.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'coarse32_bc64.npz')
DEV = 'cuda'
MODES = {'soft': 0, 'focal': 1, 'ce': 2}


def synth_batch(B, C, S, seed, max_depth=30.0):
    """tests/golden/make_golden_coarse.py:synth_batch."""
    g = torch.Generator().manual_seed(seed)
    audio = torch.rand(B, C, S, S, generator=g)
    gt = max_depth * torch.rand(B, 1, S, S, generator=g)
    gt[gt < 0.1 * max_depth] = 0.0
    return audio, gt


def _hash_key(key):
    h = 0
    for ch in key:
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return h


def _sample_idx(numel, key, ns=512):
    g = torch.Generator().manual_seed(_hash_key(key))
    return torch.randint(0, numel, (min(ns, numel),), generator=g)


def _bins_of(nb, mode='linear'):
    from audio_depth_estimation_amd.dataloader.utils_dataset import compute_bins
    return compute_bins(nb, mode, None, 30.0, 0.6)


# ------------------------------------------------------------------------------------------------------------ targets
@pytest.mark.parametrize('mode', ['linear', 'log', 'sid'])
@pytest.mark.parametrize('nb', [8, 100, 128])
@pytest.mark.parametrize('shape', [(1, 5, 7), (2, 32, 32)])
def test_targets_equal_bucketize(shape, nb, mode):
    from audio_depth_estimation_amd import kernels as K
    edges, _ = _bins_of(nb, mode)
    inner = edges[1:-1].contiguous()
    g = torch.Generator().manual_seed(nb + shape[1])
    n = shape[0] * shape[1] * shape[2]
    depth = 36.0 * torch.rand(n, generator=g) - 1.0                     # some below 0, some above depth_max
    special = torch.cat([torch.tensor([0.0, 0.0, 0.05, 0.0999, 30.0, 31.0, 1e9, -2.0, edges[0], edges[-1], float('nan'), float('inf')]), inner])
    k = min(n // 2, special.numel())
    depth[:k] = special[:k]
    # every interior edge itself and its two f32 neighbours (a second, flat map: the small shape cannot hold them all)
    up = torch.nextafter(inner, torch.full_like(inner, 1e9))
    dn = torch.nextafter(inner, torch.full_like(inner, -1e9))
    for d in (depth.view(shape), torch.cat([inner, up, dn, torch.zeros(3)])):
        flat = d.reshape(-1).contiguous()
        want = torch.clamp(torch.bucketize(flat, inner), 0, nb - 1)
        bins = torch.full((flat.numel(),), -7, dtype=torch.int32, device=DEV)
        stats = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
        ws = torch.empty(K.coarse_targets_workspace_bytes(flat.numel()) // 8 + 1, dtype=torch.float64, device=DEV)
        K.coarse_targets(flat.to(DEV), inner.to(DEV), bins, stats, ws)
        assert torch.equal(bins.cpu().long(), want)
        assert float(stats[0]) == float((flat > 0).sum())
        stats.fill_(-1.0)
        K.coarse_targets(flat.to(DEV), None, None, stats, ws)             # the count alone
        assert float(stats[0]) == float((flat > 0).sum())


# ------------------------------------------------------------------------------------------------------------ loss kernel
def _restatement(x64, centers64, bins, gt64, mode, sigma, gamma, cew, regw):
    """CoarseDepthLoss on [pixels, nb] logits in float64: (depth, ce, regression, total)."""
    nb = x64.shape[1]
    lp = F.log_softmax(x64, dim=1)
    depth = (lp.exp() * centers64).sum(1)
    if mode == 0:
        k = torch.arange(nb, dtype=torch.float64)
        lab = torch.exp(-0.5 * ((k[None] - bins[:, None].double()) / sigma) ** 2)
        lab = lab / (lab.sum(1, keepdim=True) + 1e-8)
        ce = -(lab * lp).sum(1).mean()
    elif mode == 1:
        c = F.cross_entropy(x64, bins, reduction='none')
        ce = (((1 - torch.exp(-c)) ** gamma) * c).mean()
    else:
        ce = F.cross_entropy(x64, bins)
    valid = gt64 > 0
    reg = (depth[valid] - gt64[valid]).abs().mean()
    return depth, ce, reg, cew * ce + regw * reg


def _loss_case(mode, dtype, nb, ld, pixels, all_invalid=False):
    from audio_depth_estimation_amd import kernels as K
    sigma, gamma, cew, regw = 2.0, 2.0, 1.0, 0.5
    edges, centers = _bins_of(nb)
    g = torch.Generator().manual_seed(1000 * mode + nb + pixels)
    logits = (3.0 * torch.randn(pixels, ld, generator=g)).to(dtype)
    if pixels > 5:
        logits[5, :nb] = 0.0                                              # a tie: the first maximum wins
    gt = 31.0 * torch.rand(pixels, generator=g)
    gt[torch.rand(pixels, generator=g) < 0.1] = 0.0                       # ~10 % invalid
    if all_invalid:
        gt.zero_()
    elif not bool((gt > 0).any()):
        gt[0] = 15.5                                                      # a single pixel that drew "invalid"
    assert all_invalid or int((gt > 0).sum()) > 0                         # else the regression term is NaN by definition
    bins = torch.clamp(torch.bucketize(gt, edges[1:-1].contiguous()), 0, nb - 1)
    x64 = logits[:, :nb].double().requires_grad_(True)
    depth_r, ce_r, reg_r, tot_r = _restatement(x64, centers.double(), bins, gt.double(), mode, sigma, gamma, cew, regw)
    (tot_r if not all_invalid else cew * ce_r).backward()                # empty selection: autograd leaves the CE part alone
    gref = x64.grad
    d = lambda t: t.to(DEV)
    lg, cen, bn, gtd = d(logits), d(centers), d(bins.int()), d(gt)
    nv = torch.tensor([float((gt > 0).sum())], dtype=torch.float64, device=DEV)
    ws = torch.empty(K.coarse_loss_workspace_bytes(pixels) // 8 + 1, dtype=torch.float64, device=DEV)
    runs = []
    for _ in range(2):
        depth = torch.full((pixels,), -1.0, device=DEV)
        am = torch.full((pixels,), -1, dtype=torch.int32, device=DEV)
        dl = torch.full((pixels, ld), 7.0, dtype=dtype, device=DEV)
        sums = torch.zeros(2, dtype=torch.float64, device=DEV)
        terms = torch.zeros(3, device=DEV)
        K.coarse_loss(lg, nb, cen, depth, bins=bn, gt=gtd, n_valid=nv, ce_mode=mode, sigma=sigma, gamma=gamma,
                      ce_weight=cew, reg_weight=regw, argmax=am, dlogits=dl, workspace=ws)
        K.coarse_loss_finish(ws, pixels, sums, nv, pixels, cew, regw, terms)
        runs.append((depth.cpu(), am.cpu(), dl.cpu(), terms.cpu()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    depth, am, dl, terms = runs[0]
    print(f'mode {mode} {dtype} nb {nb} ld {ld} pixels {pixels}: depth {float(((depth.double() - depth_r).abs() / depth_r.abs()).max()):.2e} '
          f'terms {terms.tolist()} ref {[float(ce_r), float(reg_r), float(tot_r)]} '
          f'dlogits {float((dl[:, :nb].double() - gref).abs().max() / gref.abs().max()):.2e}')
    assert float(((depth.double() - depth_r.detach()).abs() / depth_r.detach().abs()).max()) <= 2e-4
    want = torch.stack([ce_r, reg_r, tot_r]).detach()
    assert torch.allclose(terms.double(), want, rtol=2e-4, atol=0.0, equal_nan=True), (terms, want)
    assert torch.isnan(want[1]).item() == all_invalid
    gmax = float(gref.abs().max())
    err = (dl[:, :nb].double() - gref).abs()
    if dtype == torch.float32:
        assert float(err.max()) <= 2e-4 * gmax
    else:
        assert bool((err <= 2.0 ** -8 * gref.abs() + 2e-4 * gmax).all()), float((err - 2.0 ** -8 * gref.abs()).max() / gmax)
    if ld > nb:
        assert float(dl[:, nb:].abs().max()) == 0.0
    assert torch.equal(am.long(), torch.argmax(logits[:, :nb].float(), dim=1))
    assert pixels <= 5 or int(am[5]) == 0
    # forward only (no bins, no gradient): the same depth bits
    depth2 = torch.empty(pixels, device=DEV)
    K.coarse_loss(lg, nb, cen, depth2)
    assert torch.equal(depth2.cpu(), depth)


# every width of the vector form (nb = ld = 8 .. 512), nb / 8 = 3 (no vector form), padded rows; 1, 63 and 257 pixels:
# less than one wave-iteration, dead lanes in the last one, more than one block
@pytest.mark.parametrize('pixels', [2 * 33 * 31, 2 * 32 * 32, 1, 63, 257])
@pytest.mark.parametrize('nb,ld', [(8, 64), (100, 128), (128, 128), (256, 256), (8, 8), (16, 16), (32, 32), (64, 64),
                                   (512, 512), (24, 24)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_coarse_loss_vs_float64(mode, dtype, nb, ld, pixels):
    _loss_case(mode, dtype, nb, ld, pixels)


@pytest.mark.parametrize('nb,pixels', [(8, 2048 * 4 * 64 + 1), (128, 2048 * 4 * 4 + 1)])
def test_coarse_loss_vs_float64_past_one_grid_pass(nb, pixels):
    """One pixel more than the 2048-block grid of that vector width serves in one pass (64 / (nb / 8) pixels per wave)."""
    _loss_case(0, torch.bfloat16, nb, nb, pixels)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_coarse_loss_all_invalid(dtype):
    _loss_case(0, dtype, 128, 128, 2 * 33 * 31, all_invalid=True)


def test_coarse_loss_rejects_unsupported_bins():
    from audio_depth_estimation_amd import kernels as K
    for nb in (1, 520):
        lg = torch.zeros(4, 520, device=DEV)
        with pytest.raises(RuntimeError, match='n_bins'):
            K.coarse_loss(lg, nb, torch.zeros(nb, device=DEV), torch.empty(4, device=DEV))


# ------------------------------------------------------------------------------------------------------------ golden parity
def _golden():
    z = np.load(GOLDEN)
    hyper = dict(zip(('lr', 'wd', 'cew', 'regw', 'sigma', 'gamma', 'dmin', 'dmax', 'alpha'), [float(v) for v in z['hyper']]))
    nb, base, S, B, seed = [int(v) for v in z['meta']]
    audio, gt = synth_batch(B, 2, S, seed, hyper['dmax'])
    bins = torch.from_numpy(z['bins'].astype(np.int64))
    return z, hyper, (nb, base, S, B), audio.to(DEV), gt.to(DEV), bins.to(DEV)


def _model(dtype, seed=0, nb=128, base=64, S=32):
    from audio_depth_estimation_amd.models.coarse_depth_model import define_coarse_depth_model
    torch.manual_seed(seed)
    m = define_coarse_depth_model('unet', 2, nb, base, S)
    m.compute_dtype = dtype
    m = m.to(DEV).train()
    m.set_bin_centers(_bins_of(nb)[1].to(DEV))
    return m


def _trainer(model, tag, h, **kw):
    from audio_depth_estimation_amd.coarse_engine import CoarseDepthTrainer
    return CoarseDepthTrainer(model.engine(), tag, h['cew'], h['regw'], h['sigma'], h['gamma'], optimizer='AdamW', lr=h['lr'],
                              weight_decay=h['wd'], clip_norm=1.0, **kw)


def rel_err(a, b):
    a, b = a.detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def test_eval_forward_golden_f32():
    z, h, (nb, base, S, B), audio, gt, bins = _golden()
    model = _model(torch.float32).eval()
    np.testing.assert_array_equal(model.bin_centers.cpu().numpy(), z['centers/linear'])
    logits, depth = model(audio)
    assert tuple(logits.shape) == (B, nb, S, S) and tuple(depth.shape) == (B, 1, S, S) and not depth.requires_grad
    assert rel_err(depth, z['eval/depth']) <= 2e-4
    li = _sample_idx(logits.numel(), 'eval/logits', 8192)
    assert rel_err(logits.cpu().reshape(-1)[li], z['eval/logits']) <= 2e-4
    assert torch.equal(model.predict_depth(audio), depth)
    hard = model.predict_depth(audio, mode='hard')
    assert torch.equal(hard, model.bin_centers[logits.argmax(dim=1, keepdim=True).squeeze(1)].unsqueeze(1))
    with pytest.raises(NotImplementedError, match='output_size'):
        model(torch.zeros(1, 2, 64, 64, device=DEV))
    with pytest.raises(RuntimeError):
        model(audio.cpu())


@pytest.mark.parametrize('tag', ['soft', 'focal', 'ce'])
def test_train_step_golden_f32(tag):
    z, h, (nb, base, S, B), audio, gt, bins = _golden()
    model = _model(torch.float32)
    sd0 = {k: v.detach().clone() for k, v in model.named_parameters()}
    tr = _trainer(model, tag, h)
    total, terms = tr.step(audio, bins, gt)
    eng = model.engine()
    got, want = terms.cpu().numpy().astype(np.float64), z[tag + '/terms']
    print(tag, 'terms', got, want, 'norm', float(tr.state[3]), float(z[tag + '/grad_norm']))
    np.testing.assert_allclose(got, want, rtol=2e-4)
    assert abs(float(total) - want[2]) <= 2e-4 * want[2]
    assert rel_err(eng.depth, z[tag + '/depth']) <= 2e-4
    for k, prm in model.named_parameters():
        g = eng.grad_view(prm).detach().float().cpu().reshape(-1)
        gn = float(z[f'{tag}/gnorm/{k}'])
        assert abs(float(g.double().norm()) - gn) <= 5e-3 * gn + 1e-7, (k, float(g.double().norm()), gn)
        si = _sample_idx(g.numel(), k)
        ref = z[f'{tag}/gsample/{k}']
        assert float(np.abs(g[si].numpy() - ref).max()) <= 1e-6 + 5e-3 * float(np.abs(ref).max()), k
    assert abs(float(tr.state[3]) - float(z[tag + '/grad_norm'])) <= 2e-3 * float(z[tag + '/grad_norm'])
    for k, prm in model.named_parameters():
        si = _sample_idx(prm.numel(), k)
        np.testing.assert_array_equal(sd0[k].cpu().reshape(-1)[si].numpy(), z[f'{tag}/p0sample/{k}'], err_msg=k)
        gs = torch.from_numpy(z[f'{tag}/gsample/{k}']).abs()
        msk = gs > 1e-2 * gs.max()
        dlt = (prm.detach().cpu().reshape(-1)[si] - torch.from_numpy(z[f'{tag}/p1sample/{k}'])).abs()[msk]
        assert float(dlt.max()) <= 0.05 * h['lr'], (k, float(dlt.max()) / h['lr'])
    sd = model.state_dict()
    for k in z.files:
        if k.startswith(tag + '/sd1/'):
            ref_v, gotv = torch.from_numpy(z[k]), sd[k[len(tag) + 5:]].cpu()
            if ref_v.dtype == torch.int64:
                assert int(gotv) == int(ref_v), k
            else:
                assert float((gotv - ref_v).abs().max()) <= 1e-4 * float(ref_v.abs().max()) + 1e-6, k


@pytest.mark.parametrize('tag', ['soft', 'focal', 'ce'])
def test_train_step_golden_bf16_terms(tag):
    z, h, _, audio, gt, bins = _golden()
    model = _model(torch.bfloat16)
    _, terms = _trainer(model, tag, h).step(audio, bins, gt)
    np.testing.assert_allclose(terms.cpu().numpy().astype(np.float64), z[tag + '/terms'], rtol=2e-2)


# ------------------------------------------------------------------------------------------------------------ trainer behaviour
@pytest.mark.parametrize('tag', ['soft', 'focal', 'ce'])
def test_reference_style_autograd_loop_matches_the_fused_trainer(tag):
    """train_coarse_depth.py's loop as written on the mirror modules: logits, depth = model(x); criterion(...)['total']
    .backward(); clip_grad_norm_; optimizer.step() -- against the fused trainer's step, to the golden bars."""
    from audio_depth_estimation_amd.coarse_engine import CoarseDepthTrainer
    from audio_depth_estimation_amd.models.coarse_depth_model import CoarseDepthLoss
    z, h, (nb, base, S, B), audio, gt, bins = _golden()
    ma, mb = _model(torch.float32), _model(torch.float32)
    crit = CoarseDepthLoss(nb, h['cew'], h['regw'], use_focal=tag == 'focal', focal_gamma=h['gamma'],
                           use_soft_ce=tag != 'ce', soft_ce_sigma=h['sigma'])
    opt = torch.optim.AdamW(ma.parameters(), lr=h['lr'], weight_decay=h['wd'])
    tr = CoarseDepthTrainer.from_criterion(mb.engine(), crit, lr=h['lr'], weight_decay=h['wd'], clip_norm=1.0)
    assert tr.ce_mode == MODES[tag]
    opt.zero_grad()
    logits, depth = ma(audio)
    assert logits.requires_grad and depth.requires_grad
    d = crit(logits, depth, bins, gt, valid_mask=gt > 0)
    d['total'].backward()
    total, terms = tr.step(audio, bins, gt)
    ref = np.array([float(d['ce']), float(d['regression']), float(d['total'])])
    np.testing.assert_allclose(terms.cpu().numpy().astype(np.float64), ref, rtol=2e-4)
    for (k, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        gb = mb.engine().grad_view(q)
        assert p.grad is not None, k
        gn = float(gb.double().norm())
        assert abs(float(p.grad.double().norm()) - gn) <= 5e-3 * gn + 1e-7, k
        assert float((p.grad - gb).abs().max()) <= 1e-6 + 5e-3 * float(gb.abs().max()), k
    tn = torch.nn.utils.clip_grad_norm_(ma.parameters(), 1.0)
    assert abs(float(tn) - float(tr.state[3])) <= 2e-3 * float(tr.state[3])
    opt.step()
    with torch.no_grad():
        assert not ma(audio)[1].requires_grad
    assert not ma.eval()(audio)[0].requires_grad


def test_device_binning_equals_supplied_bins():
    z, h, _, audio, gt, bins = _golden()
    edges = torch.from_numpy(z['edges/linear'])
    outs = []
    for given in (True, False):
        m = _model(torch.float32)
        tr = _trainer(m, 'soft', h)
        _, terms = tr.step(audio, bins, gt) if given else tr.step(audio, None, gt, edges=edges)
        outs.append((terms.cpu().clone(), m.engine().flat_p.detach().cpu().clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    with pytest.raises(ValueError):
        tr.step(audio, None, gt)


def test_graph_step_with_an_eval_in_between_equals_eager():
    z, h, _, audio, gt, bins = _golden()
    finals = []
    for mode in ('eager', 'graph'):
        m = _model(torch.bfloat16)
        tr = _trainer(m, 'soft', h)
        if mode == 'graph':
            tr.enable_graph(after_steps=1)
        losses = []
        for it in range(3):
            losses.append(float(tr.step(audio, bins, gt)[0]))
            if it == 1:
                m.eval()
                m(audio[:1])                                  # another batch size between the capture and its replay
                m.train()
        torch.cuda.synchronize()
        assert (tr._graph is not None) == (mode == 'graph')
        finals.append((losses, m.engine().flat_p.detach().clone()))
    assert finals[0][0] == finals[1][0]
    assert torch.isfinite(finals[1][1]).all() and torch.equal(finals[0][1], finals[1][1])


def test_graph_steps_follow_a_learning_rate_schedule():
    """The optimizer takes the learning rate by value, so a captured step would replay the rate it was captured with: steps
    in graph mode across per-epoch ``trainer.lr = ...`` assignments (train_coarse_depth --graph) equal the eager steps."""
    from audio_depth_estimation_amd.train_dc import warm_restart_lr
    z, h, _, audio, gt, bins = _golden()
    finals = []
    for mode in ('eager', 'graph'):
        m = _model(torch.float32)
        tr = _trainer(m, 'soft', h)
        if mode == 'graph':
            tr.enable_graph(after_steps=1)
        graphs = []
        for epoch in (0, 7, 19):
            tr.lr = warm_restart_lr(epoch, h['lr'])
            for _ in range(2):
                tr.step(audio, bins, gt)
            graphs.append(tr._graph)
        torch.cuda.synchronize()
        if mode == 'graph':
            assert all(g is not None for g in graphs) and len({id(g) for g in graphs}) == 3      # one capture per rate
        finals.append(m.engine().flat_p.detach().clone())
    assert torch.equal(finals[0], finals[1])
    # the three rates differ enough to show: the same six steps at the first rate end elsewhere
    m = _model(torch.float32)
    tr = _trainer(m, 'soft', h)
    for _ in range(6):
        tr.step(audio, bins, gt)
    assert not torch.equal(m.engine().flat_p, finals[0])


def test_trainer_resume_roundtrip():
    z, h, _, audio, gt, bins = _golden()
    ma = _model(torch.float32)
    ta = _trainer(ma, 'focal', h)
    for _ in range(2):
        ta.step(audio, bins, gt)
    sd_model = {k: v.detach().clone() for k, v in ma.state_dict().items()}
    sd_opt = ta.state_dict()
    assert float(sd_opt['state'][0]['step']) == 2 and 'param_groups' in sd_opt
    la = float(ta.step(audio, bins, gt)[0])
    mb = _model(torch.float32, seed=5)
    mb.load_state_dict(sd_model)
    tb = _trainer(mb, 'focal', h)
    tb.load_state_dict(sd_opt, DEV)
    assert float(tb.step(audio, bins, gt)[0]) == la
    for (k, a), (_, b) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert torch.equal(a, b), k


def test_train_coarse_depth_synthetic_run_writes_a_checkpoint(tmp_path, monkeypatch):
    from audio_depth_estimation_amd import train_dc
    load = train_dc.load_config

    def small(*a, **k):
        cfg = load(*a, **k)
        cfg.dataset.images_size, cfg.mode.saving_checkpoints = 32, 1
        return cfg
    monkeypatch.setattr(train_dc, 'load_config', small)
    monkeypatch.chdir(tmp_path)
    train_dc.main_coarse(['--synthetic', '8', '--epochs', '1', '--batch_size', '4', '--precision', 'f32'])
    path = tmp_path / 'checkpoints' / 'coarse_downup_015_linear128_unet_exp1' / 'checkpoint_1.pth'
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert ck['epoch'] == 1 and len(ck['state_dict']) == 111 and 'param_groups' in ck['optimizer']
    z = np.load(GOLDEN)
    np.testing.assert_array_equal(ck['bin_centers'].numpy(), z['centers/linear'])
    np.testing.assert_array_equal(ck['bin_edges'].numpy(), z['edges/linear'])
    np.testing.assert_array_equal(ck['state_dict']['bin_centers'].numpy(), z['centers/linear'])


def test_stale_backward_is_refused_across_shapes():
    """The pass counters belong to the engine, not to a shape's buffer set: a training forward at shape A, one at B and
    one at A again leave B's autograd context stale, and its backward is refused before any kernel runs.  (With the
    counters parked per shape, the third forward restored A's count 1 and raised it to 2 = the stamp of B's context.)"""
    m = _model(torch.bfloat16, nb=16, base=16, S=32)
    eng = m.engine()
    g = torch.Generator().manual_seed(4)
    xA = torch.rand(1, 2, 32, 32, generator=g).to(DEV)
    xB = torch.rand(1, 2, 64, 32, generator=g).to(DEV)        # only the width is tied to output_size
    serials = [eng.fwd_serial]
    m(xA)
    serials.append(eng.fwd_serial)
    _, dB = m(xB)
    serials.append(eng.fwd_serial)
    m(xA)
    serials.append(eng.fwd_serial)
    assert eng.autograd_pass == 3
    assert all(b > a for a, b in zip(serials, serials[1:])), serials
    with pytest.raises(RuntimeError, match='overwritten'):
        dB.sum().backward()
