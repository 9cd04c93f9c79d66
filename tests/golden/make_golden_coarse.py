"""Golden vectors of the coarse-depth classification family (coarse32_bc64.npz).

Run on a machine that has the reference checkout (it is imported, never copied), on the CPU in f32:
``define_coarse_depth_model('unet', 2, 128, 64, 32)`` after ``torch.manual_seed(0)``, B = 2 at 32 x 32, linear bins on
[0.1, 30] from the reference's own ``BinnedDepthDataset._compute_bins`` (called on a bare object; ``torchaudio`` /
``torchvision`` / ``pandas`` are only imported by that module's file readers, so empty stand-ins are registered when they
are missing).  Recorded:
  * the initial state_dict as key order + one SHA-256 per tensor (``sd_init_keys`` / ``sd_init_sha``);
  * bin edges / centres of all three bin modes at n_bins 128 (``edges/<mode>``, ``centers/<mode>``);
  * an eval forward: ``eval/depth`` in full, ``eval/logits`` at fixed sampled positions (``sample_idx``);
  * for each of soft / focal / ce one training step exactly as train_coarse_depth.py:446-463 (weights 1.0 / 0.5, mask
    gt > 0, clip_grad_norm_(1.0), AdamW lr 1e-3 wd 0.01): ce, regression, total; per-parameter gradient norms and
    512-entry samples; the clipped norm; sampled parameters before / after the step; the BatchNorm buffers after it.
The inputs are not stored: ``synth_batch`` (restated in tests/test_gpu_coarse.py) regenerates them from the seed.
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get('REFERENCE_ROOT', '/root/reference')
sys.path.insert(0, REF)
for name in ('torchaudio', 'torchaudio.transforms', 'torchvision', 'torchvision.transforms', 'pandas'):
    try:
        __import__(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
        if '.' in name:
            setattr(sys.modules[name.split('.')[0]], name.split('.')[1], sys.modules[name])
from dataloader.SparseDepth_Dataset import BinnedDepthDataset          # noqa: E402
from models.coarse_depth_model import CoarseDepthLoss, define_coarse_depth_model          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NS = 512
N_BINS, BASE, S, B = 128, 64, 32, 2
LR, WD, CE_W, REG_W, SIGMA, GAMMA = 1e-3, 0.01, 1.0, 0.5, 2.0, 2.0
DEPTH_MIN, DEPTH_MAX, SID_ALPHA = 0.1, 30.0, 0.6


def synth_batch(B, C, S, seed, max_depth=30.0):
    g = torch.Generator().manual_seed(seed)
    audio = torch.rand(B, C, S, S, generator=g)
    gt = max_depth * torch.rand(B, 1, S, S, generator=g)
    gt[gt < 0.1 * max_depth] = 0.0
    return audio, gt


def hash_key(key):
    h = 0
    for ch in key:
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return h


def sample_idx(numel, key, ns=NS):
    """Fixed sample positions of a tensor (same generator in the test)."""
    g = torch.Generator().manual_seed(hash_key(key))
    return torch.randint(0, numel, (min(ns, numel),), generator=g)


def reference_bins(n_bins, mode):
    ds = object.__new__(BinnedDepthDataset)
    ds.n_bins, ds.bin_mode, ds.sid_alpha, ds.depth_min, ds.depth_max = n_bins, mode, SID_ALPHA, DEPTH_MIN, DEPTH_MAX
    ds._compute_bins()
    return ds


def main():
    torch.set_num_threads(8)
    out = {}
    for mode in ('linear', 'log', 'sid'):
        ds = reference_bins(N_BINS, mode)
        out['edges/' + mode], out['centers/' + mode] = ds.bin_edges.numpy(), ds.bin_centers.numpy()
    ds = reference_bins(N_BINS, 'linear')
    audio, gt = synth_batch(B, 2, S, 1234, DEPTH_MAX)
    bins = torch.stack([ds.depth_to_bins(gt[b]) for b in range(B)])           # [B, H, W] int64, as the dataset yields them
    out['bins'] = bins.numpy().astype(np.int16)
    out['valid_fraction'] = np.float64((gt > 0).double().mean().item())

    def fresh():
        torch.manual_seed(0)
        m = define_coarse_depth_model('unet', 2, N_BINS, BASE, S)
        sd = m.state_dict()
        keys = np.array(list(sd))
        sha = np.array([hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest() for v in sd.values()])
        m.set_bin_centers(ds.bin_centers)
        return m, keys, sha

    model, out['sd_init_keys'], out['sd_init_sha'] = fresh()
    model.eval()
    with torch.no_grad():
        logits, depth = model(audio)
    out['eval/depth'] = depth.numpy()
    li = sample_idx(logits.numel(), 'eval/logits', 8192)
    out['eval/logits'] = logits.reshape(-1)[li].numpy()

    for tag, kw in (('soft', dict(use_focal=False, use_soft_ce=True)), ('focal', dict(use_focal=True, use_soft_ce=True)),
                    ('ce', dict(use_focal=False, use_soft_ce=False))):
        model, _, _ = fresh()
        model.train()
        crit = CoarseDepthLoss(n_bins=N_BINS, ce_weight=CE_W, regression_weight=REG_W, focal_gamma=GAMMA,
                               soft_ce_sigma=SIGMA, **kw)
        opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
        opt.zero_grad()
        logits, depth = model(audio)
        d = crit(logits, depth, bins, gt, valid_mask=gt > 0)
        d['total'].backward()
        out[tag + '/terms'] = np.array([d['ce'].item(), d['regression'].item(), d['total'].item()], dtype=np.float64)
        out[tag + '/depth'] = depth.detach().numpy()
        for k, prm in model.named_parameters():
            gflat = prm.grad.detach().reshape(-1)
            out[f'{tag}/gnorm/{k}'] = np.float64(gflat.double().norm().item())
            out[f'{tag}/gsample/{k}'] = gflat[sample_idx(gflat.numel(), k)].numpy()
        out[tag + '/grad_norm'] = np.float64(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0).item())
        before = {k: q.detach().clone() for k, q in model.named_parameters()}
        opt.step()
        for k, prm in model.named_parameters():
            si = sample_idx(prm.numel(), k)
            out[f'{tag}/p0sample/{k}'] = before[k].reshape(-1)[si].numpy()
            out[f'{tag}/p1sample/{k}'] = prm.detach().reshape(-1)[si].numpy()
        for k, v in model.state_dict().items():
            if 'running_' in k or 'num_batches' in k:
                out[f'{tag}/sd1/{k}'] = v.detach().clone().numpy()
        print(tag, out[tag + '/terms'], 'grad_norm', float(out[tag + '/grad_norm']))
    out['meta'] = np.array([N_BINS, BASE, S, B, 1234], dtype=np.int64)
    out['hyper'] = np.array([LR, WD, CE_W, REG_W, SIGMA, GAMMA, DEPTH_MIN, DEPTH_MAX, SID_ALPHA], dtype=np.float64)
    path = os.path.join(HERE, 'coarse32_bc64.npz')
    np.savez_compressed(path, **out)
    print('coarse32_bc64 valid fraction', float(out['valid_fraction']), 'bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
