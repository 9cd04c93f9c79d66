"""Golden vectors of the U-Net cVAE family (cvae256_ngf4.npz, cvae128_ngf4_dn.npz, cvae256_ngf64.npz).

Run on a machine that has the reference checkout (it is imported, never copied): one eval forward and one training step
exactly as train_cvae.py:438-478 (mask gt > 0, depth loss + kl_weight * kl, clip_grad_norm_(1.0), AdamW), on CPU in f32.
The noise the reference draws (randn_like inside VAEBottleneck.reparameterize) is recorded by wrapping the INSTANCE's
reparameterize, so the port's tests can inject it.  Only numbers are saved.  The inputs are not stored: they are
regenerated from the seed by ``synth_batch`` (restated in tests/test_gpu_cvae.py); the 256x256 predictions are stored at
every 8th pixel, and to stay small the files hold
  * the initial state_dict as its key order plus one SHA-256 of the raw bytes per tensor (``sd_init_keys`` /
    ``sd_init_sha``: the port must reproduce the bits, so a digest is as strong as the tensor);
  * every gradient and every parameter change of the step (sd1 - sd0) as float16 of the tensor divided by its max-abs
    (``grad16/<key>`` + ``gradmax/<key>``, ``d16/<key>`` + ``dmax/<key>``: ~5e-4 of the max, well inside the tolerances);
  * BatchNorm buffers after the step in full (``buf1/<key>``).
cvae256_ngf64.npz is the full-width network (unet_256, ngf 64, identity head: the bf16 path runs the thin edge kernels
and the fused loss head with final_act 2), stored like unet256_ngf64.npz: per-tensor checksums of the initial weights,
8192 sampled points of a B = 32 eval prediction, and of a B = 4 training step the sampled prediction, the loss, per-tensor
gradient norms + 512-element samples, the clipped norm, parameter samples after AdamW and the BatchNorm running stats.
"""
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.environ.get('REFERENCE_ROOT', '/root/reference'))
from models.unet_cvae_model import define_G_cvae          # noqa: E402
from utils_loss import SIlogLoss                          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
L1_W, SILOG_W, SILOG_LAMBDA = 0.237, 0.637, 0.869         # conf/mode/train.yaml:12-14
KL_WEIGHT = 1.0          # far above the 1e-4 default: the KL term must show in the loss (~1 %) and in the gradients
NS = 512


def synth_batch(B, C, S, seed, max_depth=30.0, depth_norm=False):
    g = torch.Generator().manual_seed(seed)
    audio = torch.rand(B, C, S, S, generator=g)
    gt = max_depth * torch.rand(B, 1, S, S, generator=g)
    gt[gt < 0.1 * max_depth] = 0.0
    if depth_norm:
        gt = gt / max_depth
    return audio, gt


def pack(out, tag, key, t):
    m = float(t.abs().max())
    out[f'{tag}max/{key}'] = np.float64(m)
    out[f'{tag}16/{key}'] = (t / (m if m > 0 else 1.0)).numpy().astype(np.float16)


def innermost(model):
    blk = model.model
    while blk.submodule is not None:
        blk = blk.submodule
    return blk


def cvae_case(name, netG, S, depth_norm, latent, B=2, ngf=4, lr=0.002, max_depth=30.0, out_bias=1.0, stride=8):
    cfg = SimpleNamespace(dataset=SimpleNamespace(depth_norm=depth_norm, max_depth=max_depth))
    torch.manual_seed(0)
    model = define_G_cvae(cfg, 2, 1, ngf, netG, norm='batch', use_dropout=False, init_type='normal', init_gain=0.02,
                          gpu_ids=[], latent_dim=latent)
    out = {}
    sd_init = model.state_dict()
    out['sd_init_keys'] = np.array(list(sd_init))
    out['sd_init_sha'] = np.array([hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest()
                                   for v in sd_init.values()])
    with torch.no_grad():
        model.model.upconv.bias.fill_(out_bias)          # keep the head away from log(0) (see make_golden.py)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    pnames = {k for k, _ in model.named_parameters()}
    vae = innermost(model).vae
    rec = {}

    def reparameterize(mu, logvar):
        std = torch.exp(0.5 * logvar)
        eps = torch.randn_like(std)
        rec['eps'], rec['mu'], rec['logvar'] = eps.detach().clone(), mu.detach().clone(), logvar.detach().clone()
        return mu + eps * std
    vae.reparameterize = reparameterize
    audio, gt = synth_batch(B, 2, S, 1234, max_depth, depth_norm)
    sub = lambda t: t.detach().reshape(-1)[::stride].clone().numpy()

    model.eval()
    with torch.no_grad():
        pe, kle = model(audio)
    out['pred_eval'] = sub(pe)
    out['eps_eval'] = rec['eps'].numpy()
    out['mu_eval'], out['logvar_eval'] = rec['mu'].numpy(), rec['logvar'].numpy()
    out['kl_eval'] = np.float64(kle.item())

    model.train()
    optimizer = torch.optim.AdamW(model.parameters(), lr=lr)
    optimizer.zero_grad()
    pred, kl = model(audio)
    valid = gt > 0
    scale = max_depth if depth_norm else 1.0
    p, g = pred[valid] * scale, gt[valid] * scale
    depth_loss = L1_W * torch.nn.L1Loss()(p, g) + SILOG_W * SIlogLoss(lambda_scale=SILOG_LAMBDA)(p, g)
    loss = depth_loss + KL_WEIGHT * kl
    out['depth_loss'] = np.float64(depth_loss.item())
    loss.backward()
    out['eps_train'] = rec['eps'].numpy()
    out['mu'] = rec['mu'].numpy()
    out['logvar'] = rec['logvar'].numpy()
    out['kl'] = np.float64(kl.item())
    out['pred_train'] = sub(pred)
    out['loss'] = np.float64(loss.item())
    for k, prm in model.named_parameters():
        if prm.grad is not None:
            pack(out, 'grad', k, prm.grad.detach())
    out['grad_norm'] = np.float64(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0).item())
    optimizer.step()
    for k, v in model.state_dict().items():
        if k in pnames:
            pack(out, 'd', k, v.detach() - sd0[k])
        else:
            out['buf1/' + k] = v.detach().clone().numpy()
    out['meta'] = np.array([ngf, S, int(depth_norm), B, latent, stride], dtype=np.int64)
    out['hyper'] = np.array([lr, max_depth, L1_W, SILOG_W, SILOG_LAMBDA, KL_WEIGHT, out_bias], dtype=np.float64)
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print(name, 'loss', loss.item(), 'kl', kl.item(), 'grad_norm', float(out['grad_norm']), 'bytes', os.path.getsize(path))


def hash_key(key):
    h = 0
    for ch in key:
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return h


def sample_idx(numel, key, ns=NS):
    """Fixed sample positions of a tensor (same generator in the test)."""
    g = torch.Generator().manual_seed(hash_key(key))
    return torch.randint(0, numel, (min(ns, numel),), generator=g)


def cvae_ngf64(lr=0.002, max_depth=30.0, out_bias=1.0, latent=128, kl_weight=0.1):
    # out_bias 1.0: the identity head's pre-bias output spans about [-0.8, 1.0]; with the bias every prediction stays > 0.2
    # (6 m), away from SIlog's 1 / pred, where d loss / d pred would hinge on single pixels (make_golden_unet64.py)
    # full width: the bottleneck's KL is ~8 at init, so a smaller weight keeps the depth loss the larger term
    torch.set_num_threads(8)
    cfg = SimpleNamespace(dataset=SimpleNamespace(depth_norm=True, max_depth=max_depth))
    torch.manual_seed(0)
    model = define_G_cvae(cfg, 2, 1, 64, 'unet_256', norm='batch', use_dropout=False, init_type='normal', init_gain=0.02,
                          gpu_ids=[], latent_dim=latent)
    with torch.no_grad():
        model.model.upconv.bias.fill_(out_bias)
    out = {}
    for k, v in model.state_dict().items():
        if v.dtype.is_floating_point:
            out['init_sum/' + k] = np.float64(v.double().sum().item())
            out['init_abs/' + k] = np.float64(v.double().abs().sum().item())
    vae = innermost(model).vae
    rec = {}

    def reparameterize(mu, logvar):
        std = torch.exp(0.5 * logvar)
        eps = torch.randn_like(std)
        rec['eps'], rec['mu'], rec['logvar'] = eps.detach().clone(), mu.detach().clone(), logvar.detach().clone()
        return mu + eps * std
    vae.reparameterize = reparameterize
    a32, _ = synth_batch(32, 2, 256, 4321, max_depth, True)
    model.eval()
    with torch.no_grad():
        p32, kl32 = model(a32)
    g = torch.Generator().manual_seed(99)
    idx = torch.randint(0, p32.numel(), (8192,), generator=g)
    out['eval32_idx'], out['eval32_val'] = idx.numpy(), p32.reshape(-1)[idx].numpy()
    out['eps_eval'], out['mu_eval'], out['logvar_eval'] = rec['eps'].numpy(), rec['mu'].numpy(), rec['logvar'].numpy()
    out['kl_eval'] = np.float64(kl32.item())
    audio, gt = synth_batch(4, 2, 256, 1234, max_depth, True)
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=lr)
    opt.zero_grad()
    pred, kl = model(audio)
    valid = gt > 0
    p, t = pred[valid] * max_depth, gt[valid] * max_depth
    depth_loss = L1_W * torch.nn.L1Loss()(p, t) + SILOG_W * SIlogLoss(lambda_scale=SILOG_LAMBDA)(p, t)
    loss = depth_loss + kl_weight * kl
    loss.backward()
    idx = torch.randint(0, pred.numel(), (8192,), generator=g)
    out['train_idx'], out['pred_train'] = idx.numpy(), pred.detach().reshape(-1)[idx].numpy()
    out['eps_train'], out['mu'], out['logvar'] = rec['eps'].numpy(), rec['mu'].numpy(), rec['logvar'].numpy()
    out['kl'], out['loss'], out['depth_loss'] = np.float64(kl.item()), np.float64(loss.item()), np.float64(depth_loss.item())
    for k, prm in model.named_parameters():
        if prm.grad is None:
            continue
        gflat = prm.grad.detach().reshape(-1)
        out['gnorm/' + k] = np.float64(gflat.double().norm().item())
        out['gsample/' + k] = gflat[sample_idx(gflat.numel(), k)].numpy()
    out['grad_norm'] = np.float64(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0).item())
    before = {k: q.detach().clone() for k, q in model.named_parameters()}
    opt.step()
    for k, prm in model.named_parameters():
        si = sample_idx(prm.numel(), k)
        out['p0sample/' + k] = before[k].reshape(-1)[si].numpy()
        out['p1sample/' + k] = prm.detach().reshape(-1)[si].numpy()
    for k, v in model.state_dict().items():
        if 'running_' in k or 'num_batches' in k:
            out['sd1/' + k] = v.detach().clone().numpy()
    out['hyper'] = np.array([lr, max_depth, L1_W, SILOG_W, SILOG_LAMBDA, kl_weight, out_bias, latent], dtype=np.float64)
    path = os.path.join(HERE, 'cvae256_ngf64.npz')
    np.savez_compressed(path, **out)
    print('cvae256_ngf64 loss', loss.item(), 'kl', kl.item(), 'grad_norm', float(out['grad_norm']), 'bytes',
          os.path.getsize(path))


if __name__ == '__main__':
    cvae_case('cvae256_ngf4', 'unet_256', 256, False, 128)
    cvae_case('cvae128_ngf4_dn', 'unet_128', 128, True, 100, out_bias=0.5, stride=2)
    cvae_ngf64()
