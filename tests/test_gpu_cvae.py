"""GPU tests of the U-Net cVAE family (models.unet_cvae_model on libadn).

  * adn_vae_fwd / adn_vae_bwd against a float64 torch restatement (injected eps), bit-reproducibility, and the
    counter-based Gaussian generator;
  * parity with the reference's golden vectors (tests/golden/cvae*.npz, f32, injected eps) through both the autograd loop
    with torch.optim.AdamW and the fused CVAETrainer: prediction and loss 1e-4, gradients 2e-3 of the tensor max, the
    parameters after AdamW 0.02 * lr, BatchNorm running stats; the three unused BatchNorms stay bit-unchanged and
    have no optimizer state;
  * hipGraph and launch-plan replay against the eager step, the identity head (final_act 2), a 50-step descent at the
    benchmark shape and the train_cvae entry point.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
DEV = 'cuda'


def synth_batch(B, C, S, seed, max_depth=30.0, depth_norm=False):
    """Inputs of tests/golden/make_golden_cvae.py (same generator, same order of draws)."""
    g = torch.Generator().manual_seed(seed)
    audio = torch.rand(B, C, S, S, generator=g)
    gt = max_depth * torch.rand(B, 1, S, S, generator=g)
    gt[gt < 0.1 * max_depth] = 0.0
    if depth_norm:
        gt = gt / max_depth
    return audio, gt


def _cfg(depth_norm):
    return SimpleNamespace(dataset=SimpleNamespace(depth_norm=bool(depth_norm), max_depth=30.0))


def _build(netG, ngf, depth_norm, latent, dtype, out_bias=None, seed=0):
    from audio_depth_estimation_amd.models.unet_cvae_model import define_G_cvae
    torch.manual_seed(seed)
    model = define_G_cvae(_cfg(depth_norm), 2, 1, ngf, netG, latent_dim=latent)
    if out_bias is not None:
        with torch.no_grad():
            model.model.upconv.bias.fill_(out_bias)
    model.compute_dtype = dtype
    return model.to(DEV)


def rel_l1(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double()
    return float((a - b).abs().sum() / (b.abs().sum() + 1e-30))


def max_rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---------------------------------------------------------------------------------------------------------------- kernels
def _vae_ref(h, Wm, bm, Wl, bl, Wd, bd, eps, g_rec, g_kl):
    h, Wm, bm, Wl, bl, Wd, bd, eps, g_rec = [t.double().cpu() for t in (h, Wm, bm, Wl, bl, Wd, bd, eps, g_rec)]
    prm = [t.clone().requires_grad_(True) for t in (h, Wm, bm, Wl, bl, Wd, bd)]
    hh, wm, b1, wl, b2, wd, b3 = prm
    mu = hh @ wm.t() + b1
    lv = hh @ wl.t() + b2
    z = mu + eps * torch.exp(0.5 * lv)
    rec = z @ wd.t() + b3
    kl_img = -0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp(), dim=1)
    kl = kl_img.mean()
    out = torch.relu(rec)
    (torch.sum(out * g_rec) + g_kl * kl).backward()
    return dict(mu=mu, lv=lv, z=z, out=out, kl_img=kl_img, kl=kl, grads=[p.grad for p in prm])


def _vae_run(h, Wm, bm, Wl, bl, Wd, bd, eps, g_rec, g_kl, dtype=torch.float32):
    from audio_depth_estimation_amd import kernels as K
    B, C = h.shape
    L = Wm.shape[0]
    f = dict(dtype=torch.float32, device=DEV)
    o = dict(mu=torch.empty(B, L, **f), lv=torch.empty(B, L, **f), eps=torch.empty(B, L, **f), z=torch.empty(B, L, **f),
             kl_img=torch.empty(B, **f), kl=torch.empty(1, **f), out=torch.empty(B, C, dtype=dtype, device=DEV))
    K.vae_fwd(h, Wm, bm, Wl, bl, Wd, bd, 7, None, eps, o['mu'], o['lv'], o['eps'], o['z'], o['kl_img'], o['kl'], o['out'])
    gr = (g_rec * (o['out'].float() > 0)).to(dtype).contiguous()     # what the innermost upconv's dgrad hands over
    gk = torch.full((1,), g_kl, **f)
    gs = [torch.empty_like(t) for t in (Wm, bm, Wl, bl, Wd, bd)]
    ws = torch.empty(K.vae_bwd_workspace_bytes(B, L) // 4, **f)
    loss = torch.zeros(1, **f)
    K.vae_bwd(gr, h, o['mu'], o['lv'], o['eps'], o['z'], Wm, Wl, Wd, gk, *gs, gr, ws, kl=o['kl'], loss=loss)
    torch.cuda.synchronize()
    o['dh'], o['gparams'], o['loss'] = gr, gs, loss
    return o


@pytest.mark.parametrize('B', [1, 3, 32])
@pytest.mark.parametrize('L', [128, 100])
@pytest.mark.parametrize('C', [32, 512])
@pytest.mark.parametrize('g_kl', [0.0, 1e-4, 1.0])
def test_vae_kernels_against_float64(B, L, C, g_kl):
    g = torch.Generator().manual_seed(B * 1000 + L + C)
    r = lambda *s, sc=1.0: (sc * torch.randn(*s, generator=g)).float()
    h, eps, g_rec = r(B, C), r(B, L), r(B, C, sc=0.1)
    Wm, Wl, Wd = r(L, C, sc=C ** -0.5), r(L, C, sc=0.5 * C ** -0.5), r(C, L, sc=L ** -0.5)
    bm, bl, bd = r(L, sc=0.1), r(L, sc=0.1), r(C, sc=0.1)
    args = [t.to(DEV) for t in (h, Wm, bm, Wl, bl, Wd, bd, eps)]
    ref = _vae_ref(h, Wm, bm, Wl, bl, Wd, bd, eps, g_rec, g_kl)
    o = _vae_run(*args, g_rec.to(DEV), g_kl)
    for k in ('mu', 'lv', 'z', 'out', 'kl_img'):
        assert max_rel(o[k], ref[k]) <= 1e-5, k
    assert torch.equal(o['eps'], args[-1])
    assert abs(o['kl'].item() - ref['kl'].item()) <= 1e-5 * max(1.0, abs(ref['kl'].item()))
    assert abs(o['loss'].item() - g_kl * o['kl'].item()) <= 1e-6 * max(1.0, abs(o['kl'].item()))
    assert max_rel(o['dh'], ref['grads'][0]) <= 1e-5
    for got, want, name in zip(o['gparams'], ref['grads'][1:], ('W_mu', 'b_mu', 'W_lv', 'b_lv', 'W_dec', 'b_dec')):
        assert max_rel(got, want) <= 1e-5, name
    o2 = _vae_run(*args, g_rec.to(DEV), g_kl)                         # bit-reproducible run to run
    for k in ('mu', 'lv', 'z', 'out', 'kl_img', 'kl', 'dh', 'loss'):
        assert torch.equal(o[k], o2[k]), k
    for a, b in zip(o['gparams'], o2['gparams']):
        assert torch.equal(a, b)


def test_vae_bf16_output_and_argument_checks():
    from audio_depth_estimation_amd import kernels as K
    g = torch.Generator().manual_seed(3)
    B, C, L = 4, 64, 16
    r = lambda *s: (0.2 * torch.randn(*s, generator=g)).float().to(DEV)
    h, Wm, bm, Wl, bl, Wd, bd, eps = r(B, C), r(L, C), r(L), r(L, C), r(L), r(C, L), r(C), r(B, L)
    g_rec = r(B, C).to(torch.bfloat16).float()         # what a bf16 dgrad can hand over: exactly representable
    o32 = _vae_run(h, Wm, bm, Wl, bl, Wd, bd, eps, g_rec, 0.5)
    o16 = _vae_run(h, Wm, bm, Wl, bl, Wd, bd, eps, g_rec, 0.5, dtype=torch.bfloat16)
    assert o16['out'].dtype == torch.bfloat16 and max_rel(o16['out'], o32['out'].cpu()) <= 1e-2
    # bf16 backward: the bf16 g_rec load and the bf16 dh store against the float64 restatement.  g_rec is exact in bf16
    # and the ReLU mask keeps its sign under rounding, so the parameter gradients are f32-exact; dh carries one bf16
    # rounding (2^-9 relative)
    ref = _vae_ref(h, Wm, bm, Wl, bl, Wd, bd, eps, g_rec, 0.5)
    assert o16['dh'].dtype == torch.bfloat16 and max_rel(o16['dh'], ref['grads'][0]) <= 4e-3
    for got, want, name in zip(o16['gparams'], ref['grads'][1:], ('W_mu', 'b_mu', 'W_lv', 'b_lv', 'W_dec', 'b_dec')):
        assert max_rel(got, want) <= 1e-4, name
    assert abs(o16['loss'].item() - 0.5 * ref['kl'].item()) <= 1e-5 * max(1.0, abs(ref['kl'].item()))
    f = dict(dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match='adn_vae_fwd'):                    # L > 1024
        big = torch.empty(B, 1025, **f)
        K.vae_fwd(h, torch.empty(1025, C, **f), torch.empty(1025, **f), torch.empty(1025, C, **f), torch.empty(1025, **f),
                  torch.empty(C, 1025, **f), bd, 1, None, None, big, big.clone(), big.clone(), big.clone(),
                  torch.empty(B, **f), torch.empty(1, **f), torch.empty(B, C, **f))
    with pytest.raises(RuntimeError, match='vae_fwd: w_dec'):                # mismatched operand: refused on the host
        m = torch.empty(B, L, **f)
        K.vae_fwd(h, Wm, bm, Wl, bl, torch.empty(C, L + 1, **f), bd, 1, None, None, m, m.clone(), m.clone(), m.clone(),
                  torch.empty(B, **f), torch.empty(1, **f), torch.empty(B, C, **f))
    with pytest.raises(RuntimeError, match='vae_bwd: dh'):
        m = torch.empty(B, L, **f)
        K.vae_bwd(torch.empty(B, C, **f), h, m, m, m, m, Wm, Wl, Wd, torch.zeros(1, **f), torch.empty_like(Wm), torch.empty_like(bm),
                  torch.empty_like(Wl), torch.empty_like(bl), torch.empty_like(Wd), torch.empty_like(bd),
                  torch.empty(B, C // 2, **f), torch.empty(2 * B * L, **f))
    with pytest.raises(RuntimeError, match='adn_vae_fwd'):                    # C % 8 != 0
        hc = torch.empty(B, 12, **f)
        m = torch.empty(B, L, **f)
        K.vae_fwd(hc, torch.empty(L, 12, **f), bm, torch.empty(L, 12, **f), bl, torch.empty(12, L, **f),
                  torch.empty(12, **f), 1, None, None, m, m.clone(), m.clone(), m.clone(), torch.empty(B, **f),
                  torch.empty(1, **f), torch.empty(B, 12, **f))


def _draw(B, L, seed, counter):
    from audio_depth_estimation_amd import kernels as K
    f = dict(dtype=torch.float32, device=DEV)
    C = 8
    h = torch.zeros(B, C, **f)
    W, b = torch.zeros(L, C, **f), torch.zeros(L, **f)
    m = [torch.empty(B, L, **f) for _ in range(4)]
    K.vae_fwd(h, W, b, W, b, torch.zeros(C, L, **f), torch.zeros(C, **f), seed, counter, None, *m, torch.empty(B, **f),
              torch.empty(1, **f), torch.empty(B, C, **f))
    return m[2]


def test_gaussian_generator():
    eps = _draw(8192, 128, 11, None)                                  # 1 048 576 draws
    assert abs(eps.mean().item()) <= 5e-3
    assert abs(eps.var().item() - 1.0) <= 1e-2
    assert torch.isfinite(eps).all()
    c = torch.zeros(1, dtype=torch.float64, device=DEV)
    a = _draw(32, 128, 11, c)
    assert torch.equal(a, _draw(32, 128, 11, c))                      # same seed, same step: same eps
    c += 1
    assert not torch.equal(a, _draw(32, 128, 11, c))                  # next step: fresh eps
    assert not torch.equal(a, _draw(32, 128, 12, c - 1))              # another seed: fresh eps
    # a captured graph reads the counter on the device: every replay after an increment draws anew
    from audio_depth_estimation_amd import kernels as K
    f = dict(dtype=torch.float32, device=DEV)
    B, L, C = 32, 128, 8
    h, W, b = torch.zeros(B, C, **f), torch.zeros(L, C, **f), torch.zeros(L, **f)
    Wd, bd = torch.zeros(C, L, **f), torch.zeros(C, **f)
    m = [torch.empty(B, L, **f) for _ in range(4)]
    kli, kl, out = torch.empty(B, **f), torch.empty(1, **f), torch.empty(B, C, **f)
    K.vae_fwd(h, W, b, W, b, Wd, bd, 5, c, None, *m, kli, kl, out)   # warm-up outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.vae_fwd(h, W, b, W, b, Wd, bd, 5, c, None, *m, kli, kl, out)
    graph.replay()
    first = m[2].clone()
    c += 1
    graph.replay()
    assert not torch.equal(first, m[2])


# ------------------------------------------------------------------------------------------------------- identity head
def test_identity_head_kernels():
    from audio_depth_estimation_amd import kernels as K
    g = torch.Generator().manual_seed(5)
    n = 4096
    gout = torch.randn(n, generator=g).to(DEV)
    out = torch.randn(n, generator=g).to(DEV)
    dz = torch.empty(n, device=DEV)
    K.final_act_bwd(gout, out, 2, dz)
    assert torch.equal(dz, gout)                                      # identity: d pre-activation = d output
    K.final_act_bwd(gout, out, 0, dz)
    assert torch.equal(dz, gout * (out > 0))                          # code 0 unchanged
    # loss_finish_dz with the identity head == the plain loss gradient, bias gradient == its sum
    B, S = 2, 32
    pred = (2.0 + torch.randn(B, 1, S, S, generator=g)).to(DEV)
    gt = (30 * torch.rand(B, 1, S, S, generator=g)).to(DEV)
    gt[gt < 3] = 0
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    ws = torch.empty(4096 + 8, dtype=torch.float64, device=DEV)
    K.loss_stats(pred, gt, 1.0, 1, 1e-6, stats, ws)
    loss_a, loss_b = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    grad = torch.empty_like(pred)
    K.loss_finish(pred, gt, 1.0, 1, 1e-6, stats, 2, 0.3, 0.7, 0.5, loss_a, grad)
    dz2, bias = torch.empty_like(pred), torch.zeros(1, device=DEV)
    K.loss_finish_dz(pred, gt, 1.0, 1, 1e-6, stats, 2, 0.3, 0.7, 0.5, loss_b, dz2, 2, bias, ws)
    assert torch.equal(dz2, grad) and torch.equal(loss_a, loss_b)
    assert abs(bias.item() - grad.double().sum().item()) <= 1e-5 * grad.abs().sum().item()
    # convt_n1 (the 1-channel head) with code 2 returns the pre-activation: ReLU of it is the code-0 output
    Bc, Hs, C0 = 2, 16, 64
    x = torch.randn(Bc, Hs, Hs, C0, generator=g).to(DEV, torch.bfloat16)
    w = (0.1 * torch.randn(C0 * 16, generator=g)).to(DEV)
    bias_c = torch.full((1,), 0.05, device=DEV)
    wsb = torch.empty(K.convt_n1_workspace_bytes(Bc, Hs, Hs) // 4 + 4, device=DEV)
    o_id = torch.empty(Bc, 2 * Hs, 2 * Hs, 1, device=DEV)
    o_relu = torch.empty_like(o_id)
    K.convt_n1_forward(torch.bfloat16, Bc, Hs, Hs, x, None, w, bias_c, 2, o_id, wsb)
    K.convt_n1_forward(torch.bfloat16, Bc, Hs, Hs, x, None, w, bias_c, 0, o_relu, wsb)
    assert (o_id < 0).any() and torch.equal(torch.relu(o_id), o_relu)
    ref = torch.nn.functional.conv_transpose2d(x.float().permute(0, 3, 1, 2).cpu(), w.view(C0, 4, 4, 1).permute(0, 3, 1, 2)
                                               .cpu(), bias_c.cpu(), stride=2, padding=1)
    assert max_rel(o_id.permute(0, 3, 1, 2), ref) <= 1e-2


# ---------------------------------------------------------------------------------------------------- reference parity
CASES = (('cvae256_ngf4', 'unet_256'), ('cvae128_ngf4_dn', 'unet_128'))


def _load(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    ngf, S, dn, B, L, stride = [int(v) for v in z['meta']]
    lr, md, l1w, sw, lam, klw, ob = [float(v) for v in z['hyper']]
    return z, dict(ngf=ngf, S=S, dn=bool(dn), B=B, L=L, stride=stride, lr=lr, md=md, l1w=l1w, sw=sw, lam=lam, klw=klw, ob=ob)


def _unpack(z, tag, k):
    return torch.from_numpy(z[f'{tag}16/{k}'].astype(np.float64)) * float(z[f'{tag}max/{k}'])


def _check_after_step(model, z, sd0, m, unused_keys):
    lr = m['lr']
    sd1 = model.state_dict()
    for k, v in sd1.items():
        if k in unused_keys:
            assert torch.equal(v.cpu(), sd0[k].cpu()), k                     # never touched
        elif f'd16/{k}' in z.files:
            want = sd0[k].double().cpu() + _unpack(z, 'd', k)
            d = (v.double().cpu() - want).abs()
            # Adam's first step is lr * sign(g): where the reference gradient is ~0 (the gradients agree to 2e-3 of the
            # tensor max, not in sign there) the step may flip; compare where |g| > 1e-2 max, bound the rest by 2 lr
            g = _unpack(z, 'grad', k).abs()
            msk = g > 1e-2 * g.max()
            assert float(d[msk].max()) <= 0.02 * lr and float(d.max()) <= 2.0 * lr + 1e-7, k
        elif 'num_batches_tracked' in k:
            assert int(v) == int(z['buf1/' + k]), k
        else:
            assert max_rel(v, z['buf1/' + k]) <= 1e-3, k


def _unused_keys(model):
    ids = {id(p) for p in model._unused_params()}
    keys = {k for k, p in model.named_parameters() if id(p) in ids}
    for k in list(keys):
        base = k.rsplit('.', 1)[0]
        keys.update({base + '.running_mean', base + '.running_var', base + '.num_batches_tracked'})
    return keys


@pytest.mark.parametrize('name,netG', CASES)
def test_reference_parity_autograd_f32(name, netG):
    from audio_depth_estimation_amd.utils_loss import SIlogLoss
    z, m = _load(name)
    model = _build(netG, m['ngf'], m['dn'], m['L'], torch.float32, out_bias=m['ob'])
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    eng = model.engine()
    audio, gt = synth_batch(m['B'], 2, m['S'], 1234, m['md'], m['dn'])
    audio, gt = audio.to(DEV), gt.to(DEV)
    st = m['stride']
    eng.eps_in = torch.from_numpy(z['eps_eval']).to(DEV)
    model.eval()
    with torch.no_grad():
        pe, kle = model(audio)
    assert rel_l1(pe.reshape(-1)[::st], z['pred_eval']) <= 1e-4
    # at init the eval bottleneck sits at mu ~ logvar ~ 0 (KL ~ 1e-7, pure rounding): check its inputs instead
    assert max_rel(eng.vae_mu, z['mu_eval']) <= 1e-4 and max_rel(eng.vae_logvar, z['logvar_eval']) <= 1e-4
    assert abs(kle.item() - float(z['kl_eval'])) <= 1e-4 * abs(float(z['kl_eval'])) + 5e-6
    model.train()
    eng.eps_in = torch.from_numpy(z['eps_train']).to(DEV)
    opt = torch.optim.AdamW(model.parameters(), lr=m['lr'])
    opt.zero_grad()
    pred, kl = model(audio)
    valid = gt > 0
    scale = m['md'] if m['dn'] else 1.0
    p, g = pred[valid] * scale, gt[valid] * scale
    depth_loss = m['l1w'] * torch.nn.L1Loss()(p, g) + m['sw'] * SIlogLoss(lambda_scale=m['lam'])(p, g)
    loss = depth_loss + m['klw'] * kl
    loss.backward()
    assert abs(depth_loss.item() - float(z['depth_loss'])) <= 1e-4 * abs(float(z['depth_loss']))
    assert rel_l1(pred.reshape(-1)[::st], z['pred_train']) <= 1e-4
    assert max_rel(eng.vae_mu, z['mu']) <= 1e-4 and max_rel(eng.vae_logvar, z['logvar']) <= 1e-4
    assert abs(kl.item() - float(z['kl'])) <= 1e-4 * abs(float(z['kl'])) + 5e-6
    assert abs(loss.item() - float(z['loss'])) <= 1e-4 * abs(float(z['loss']))
    unused = {id(p) for p in model._unused_params()}
    for k, prm in model.named_parameters():
        if id(prm) in unused:
            assert prm.grad is None and f'grad16/{k}' not in z.files, k
        else:
            assert prm.grad is not None, k
            assert max_rel(prm.grad, _unpack(z, 'grad', k)) <= 2e-3, k
    tn = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    assert abs(tn.item() - float(z['grad_norm'])) <= 1e-3 * float(z['grad_norm'])
    opt.step()
    for p in model._unused_params():
        assert p not in opt.state
    _check_after_step(model, z, sd0, m, _unused_keys(model))


@pytest.mark.parametrize('name,netG', CASES)
def test_reference_parity_fused_trainer_f32(name, netG):
    from audio_depth_estimation_amd.cvae_engine import CVAETrainer
    z, m = _load(name)
    model = _build(netG, m['ngf'], m['dn'], m['L'], torch.float32, out_bias=m['ob']).train()
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    eng = model.engine()
    audio, gt = synth_batch(m['B'], 2, m['S'], 1234, m['md'], m['dn'])
    eng.eps_in = torch.from_numpy(z['eps_train']).to(DEV)
    tr = CVAETrainer(eng, 'Combined', m['l1w'], m['sw'], m['lam'], max_depth=m['md'], optimizer='AdamW', lr=m['lr'],
                     kl_weight=m['klw'], clip_norm=1.0)
    loss, pred = tr.step(audio.to(DEV), gt.to(DEV))
    torch.cuda.synchronize()
    assert rel_l1(pred.reshape(-1)[::m['stride']], z['pred_train']) <= 1e-4
    assert abs(loss.item() - float(z['loss'])) <= 1e-4 * abs(float(z['loss']))
    assert abs(tr.kl.item() - float(z['kl'])) <= 1e-4 * abs(float(z['kl'])) + 5e-6
    # the fused loss carries kl_weight * kl (the KL share is ~1 % of the loss, 100x the loss bound above)
    assert m['klw'] * float(z['kl']) > 50 * 1e-4 * abs(float(z['loss']))
    assert abs(loss.item() - float(z['depth_loss']) - m['klw'] * tr.kl.item()) <= 1e-4 * abs(float(z['loss']))
    assert abs(tr.state[3].item() - float(z['grad_norm'])) <= 1e-3 * float(z['grad_norm'])
    for prm, _, _ in eng.param_meta:
        k = next(n for n, q in model.named_parameters() if q is prm)
        assert max_rel(eng.grad_view(prm), _unpack(z, 'grad', k)) <= 2e-3, k
    _check_after_step(model, z, sd0, m, _unused_keys(model))
    sd = tr.state_dict()
    full = list(model.parameters())
    assert len(sd['param_groups'][0]['params']) == len(full)
    unused_idx = {i for i, p in enumerate(full) if any(p is q for q in model._unused_params())}
    assert len(unused_idx) == 6 and not (unused_idx & set(sd['state']))
    assert set(sd['state']) == set(range(len(full))) - unused_idx
    probe = torch.optim.AdamW([torch.nn.Parameter(torch.zeros_like(p, device='cpu')) for p in full], lr=m['lr'])
    probe.load_state_dict(sd)                                       # a real torch optimizer accepts it
    tr2 = CVAETrainer(eng, optimizer='AdamW', lr=m['lr'])
    tr2.load_state_dict(sd, torch.device(DEV))
    assert torch.equal(tr2.exp_avg, tr.exp_avg) and torch.equal(tr2.exp_avg_sq, tr.exp_avg_sq)


# ------------------------------------------------------------------------------------------ full width (ngf 64) parity
# Bounds of tests/test_gpu_unet.py::test_unet64_reference_fixture.  f32: prediction relative L1 1e-4, gradients (sampled
# relative L2 / norm) 2e-2 / 5e-3 -- the fp32 CPU reference's own noise floor at this depth --, parameters after AdamW
# 0.05 lr where the gradient is not negligible.  bf16: prediction 1e-2, loss 1e-3, gradients 0.5 of the tensor's RMS, and
# 0.08 for the outermost block's tensors, named below (parameters() runs innermost first here, so a positional
# names[-4:] would pick the unused BatchNorms).
BF16_PRED_REL_L1, BF16_LOSS_REL, BF16_GRAD_REL_L2, BF16_GRAD_REL_L2_OUTER = 1e-2, 1e-3, 0.5, 0.08
OUTER = ('model.upconv.weight', 'model.upconv.bias', 'model.submodule.upnorm.weight', 'model.submodule.upnorm.bias')


def _hash_key(key):
    h = 0
    for ch in key:
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return h


def _sample_idx(numel, key, ns=512):
    g = torch.Generator().manual_seed(_hash_key(key))
    return torch.randint(0, numel, (min(ns, numel),), generator=g)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_cvae64_reference_fixture(dtype):
    """unet_256 ngf 64 with the identity head (the bf16 path runs the thin edge kernels and the fused loss head with
    final_act 2) against tests/golden/cvae256_ngf64.npz: B = 32 eval samples + a B = 4 fused train step, injected eps."""
    from audio_depth_estimation_amd.cvae_engine import CVAETrainer
    z = np.load(os.path.join(GOLDEN, 'cvae256_ngf64.npz'))
    lr, md, l1w, sw, lam, klw, ob, L = [float(v) for v in z['hyper']]
    f32 = dtype == torch.float32
    model = _build('unet_256', 64, True, int(L), dtype, out_bias=ob)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k, v in sd0.items():                          # the regenerated weights ARE the reference's
        if v.dtype.is_floating_point:
            assert abs(float(v.double().sum()) - float(z['init_sum/' + k])) <= 1e-6 * max(1.0, float(z['init_abs/' + k])), k
    eng = model.engine()
    a32, _ = synth_batch(32, 2, 256, 4321, md, True)
    eng.eps_in = torch.from_numpy(z['eps_eval']).to(DEV)
    model.eval()
    with torch.no_grad():
        p32, _ = model(a32.to(DEV))
    rel = rel_l1(p32.reshape(-1).cpu()[torch.from_numpy(z['eval32_idx'])], z['eval32_val'])
    assert rel <= (1e-4 if f32 else BF16_PRED_REL_L1), rel
    assert max_rel(eng.vae_mu, z['mu_eval']) <= (1e-3 if f32 else 5e-2)
    audio, gt = synth_batch(4, 2, 256, 1234, md, True)
    model.train()
    eng.eps_in = torch.from_numpy(z['eps_train']).to(DEV)
    tr = CVAETrainer(eng, 'Combined', l1w, sw, lam, max_depth=md, optimizer='AdamW', lr=lr, kl_weight=klw, clip_norm=1.0)
    loss, pred = tr.step(audio.to(DEV), gt.to(DEV))
    torch.cuda.synchronize()
    relp = rel_l1(pred.reshape(-1).cpu()[torch.from_numpy(z['train_idx'])], z['pred_train'])
    assert relp <= (1e-4 if f32 else BF16_PRED_REL_L1), relp
    assert abs(loss.item() - float(z['loss'])) <= (1e-4 if f32 else BF16_LOSS_REL) * abs(float(z['loss']))
    assert abs(tr.kl.item() - float(z['kl'])) <= (1e-4 if f32 else 1e-2) * abs(float(z['kl']))
    names = [k for k, _ in model.named_parameters()]
    assert set(OUTER) <= set(names)
    unused = {id(p) for p in model._unused_params()}
    worst = {}
    for k, prm in model.named_parameters():
        if id(prm) in unused:
            assert 'gnorm/' + k not in z.files, k
            continue
        gflat = eng.grad_view(prm).detach().float().cpu().reshape(-1)
        si = _sample_idx(gflat.numel(), k)
        gn_ref = float(z['gnorm/' + k])
        if gn_ref < 1e-12:
            continue
        rms = gn_ref / (gflat.numel() ** 0.5)
        err = float((gflat[si] - torch.from_numpy(z['gsample/' + k])).norm() / (len(si) ** 0.5)) / rms
        nerr = abs(float(gflat.double().norm()) - gn_ref) / gn_ref
        worst[k] = (err, nerr)
        if f32:
            assert err <= 2e-2 and nerr <= 5e-3, (k, err, nerr)
    if not f32:
        for k, (err, _) in worst.items():
            assert err <= (BF16_GRAD_REL_L2_OUTER if k in OUTER else BF16_GRAD_REL_L2), (k, err)
    print(f'{dtype}: eval32 {rel:.3e} train {relp:.3e} worst grads', sorted(worst.items(), key=lambda kv: -kv[1][0])[:4])
    assert abs(tr.state[3].item() - float(z['grad_norm'])) <= (2e-3 if f32 else 5e-2) * float(z['grad_norm'])
    for k, prm in model.named_parameters():
        si = _sample_idx(prm.numel(), k)
        np.testing.assert_array_equal(sd0[k].cpu().reshape(-1)[si].numpy(), z['p0sample/' + k], err_msg=k)
        if id(prm) in unused:
            assert torch.equal(prm.detach().cpu(), sd0[k].cpu()), k          # never stepped
        elif f32:
            gs = torch.from_numpy(z['gsample/' + k]).abs()
            msk = gs > 1e-2 * gs.max()                 # Adam's sign-like step is ill-conditioned where g ~ 0
            d = (prm.detach().cpu().reshape(-1)[si] - torch.from_numpy(z['p1sample/' + k])).abs()[msk]
            assert float(d.max()) <= 0.05 * lr, (k, float(d.max()) / lr)
    sd = model.state_dict()
    for k in z.files:
        if k.startswith('sd1/'):
            ref_v, gotv = torch.from_numpy(z[k]), sd[k[4:]].cpu()
            if ref_v.dtype == torch.int64:
                assert int(gotv) == int(ref_v), k
            else:
                assert float((gotv - ref_v).abs().max()) <= (1e-4 if f32 else 2e-2) * float(ref_v.abs().max()) + 1e-6, k


# ------------------------------------------------------------------------------------------------- replay, descent, CLI
def _steps(mode, n=6, B=4):
    from audio_depth_estimation_amd.cvae_engine import CVAETrainer
    model = _build('unet_256', 64, True, 128, torch.bfloat16, out_bias=0.5).train()
    tr = CVAETrainer(model.engine(), 'Combined', 0.5, 0.5, 0.5, max_depth=30.0, lr=1e-3, kl_weight=1e-2)
    if mode == 'graph':
        tr.enable_graph(after_steps=3)
    elif mode == 'plan':
        tr.enable_launch_plan(after_steps=3)
    audio, gt = synth_batch(B, 2, 256, 99, 30.0, True)
    audio, gt = audio.to(DEV), gt.to(DEV)
    out = []
    for _ in range(n):
        loss, _ = tr.step(audio, gt)
        out.append((loss.item(), tr.kl.item()))
    return out, model.engine().vae_eps.clone()


def test_graph_and_plan_replay_match_eager():
    eager, e_eps = _steps('eager')
    assert all(np.isfinite(v) for pair in eager for v in pair)
    assert len({kl for _, kl in eager}) == len(eager)               # fresh noise every step
    for mode in ('graph', 'plan'):
        got, eps = _steps(mode)
        assert torch.equal(eps, e_eps), mode                         # the last (replayed) step drew the eager step's eps
        for (a, ka), (b, kb) in zip(eager, got):
            assert abs(a - b) <= 1e-6 * abs(a) and abs(ka - kb) <= 1e-6 * abs(ka), (mode, eager, got)


def test_descent_ngf64_b32_bf16():
    from audio_depth_estimation_amd.cvae_engine import CVAETrainer
    model = _build('unet_256', 64, False, 128, torch.bfloat16, out_bias=1.0).train()
    tr = CVAETrainer(model.engine(), 'Combined', 0.5, 0.5, 0.5, max_depth=30.0, lr=2e-3, kl_weight=1e-4)
    tr.enable_graph(after_steps=3)
    audio, gt = synth_batch(32, 2, 256, 7, 30.0, False)
    audio, gt = audio.to(DEV), gt.to(DEV)
    losses = [tr.step(audio, gt)[0].item() for _ in range(50)]
    assert all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10]), losses


def test_train_cvae_entrypoint_synthetic(tmp_path, monkeypatch):
    from audio_depth_estimation_amd import train_cvae
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    model = train_cvae.main(['--synthetic', '8', '--batch_size', '4', '--epochs', '10', '--validation', 'True',
                             '--validation_iter', '5', '--precision', 'bf16', '--graph'])
    exp = 'unet_256_batvisionv2_BS4_Lr0.002_AdamW_cvae_cvae_cvae'
    ck = torch.load(tmp_path / 'checkpoints' / exp / 'checkpoint_10.pth', map_location='cpu')
    assert set(ck) == {'epoch', 'state_dict', 'optimizer'} and ck['epoch'] == 10
    assert list(ck['state_dict']) == list(model.state_dict())
    full = list(model.parameters())
    opt_sd = ck['optimizer']
    assert len(opt_sd['param_groups'][0]['params']) == len(full) and len(opt_sd['state']) == len(full) - 6
    assert float(next(iter(opt_sd['state'].values()))['step']) == 20
    assert all(torch.isfinite(v).all() for v in ck['state_dict'].values() if v.is_floating_point())
