"""Golden vectors of the dual-regression coarse-depth family (dualreg32_bc64.npz).

Run on a machine that has the reference checkout (it is imported, never copied), on the CPU in f32:
``torch.manual_seed(0); DualRegressionModel(2, 64, 32)``, B = 2 at 32 x 32.  Recorded:
  * the initial state_dict as key order + one SHA-256 per tensor (``sd_init_keys`` / ``sd_init_sha``) and the parameter
    count;
  * an eval forward: ``eval/coarse``, ``eval/offset``, ``eval/final`` in full;
  * one training step exactly as train_coarse_depth.py:422-463 (DualRegressionLoss 1.0 / 1.0 / 0.01, clip_grad_norm_(1.0),
    AdamW lr 1e-3 wd 0.01): coarse, final, offset_reg, total; the three training-mode maps; per-parameter gradient norms
    and 512-entry samples; the clipped norm; sampled parameters before / after the step; the BatchNorm buffers after it.
The inputs are not stored: ``synth_batch`` (restated in tests/test_gpu_dualreg.py) regenerates them from the seed.

L1 kinks: a pixel within rounding distance of a kink of |coarse - gt|, |final - gt| or |offset| can flip a gradient sign
between two correct implementations.  The maker counts the valid pixels with |coarse - gt| < 1e-2, those with
|final - gt| < 1e-2 and the pixels with 0 < |offset| < 1e-3 in the training forward, stores the counts (``kinks``) and
refuses to write the file unless all three are 0 (try another seed of SEEDS then).
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# the reference checkout: $REFERENCE_ROOT, or a directory ``reference`` next to this repository
REF = os.environ.get('REFERENCE_ROOT', os.path.join(HERE, '..', '..', '..', 'reference'))
sys.path.insert(0, os.path.abspath(REF))
from models.coarse_depth_model import DualRegressionLoss, DualRegressionModel          # noqa: E402

NS = 512
BASE, S, B = 64, 32, 2
LR, WD, COARSE_W, FINAL_W, OFFSET_W = 1e-3, 0.01, 1.0, 1.0, 0.01
DEPTH_MAX = 30.0
SEEDS = (1234, 1239, 1241, 1244)


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


def fresh():
    torch.manual_seed(0)
    m = DualRegressionModel(2, BASE, S)
    sd = m.state_dict()
    keys = np.array(list(sd))
    sha = np.array([hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest() for v in sd.values()])
    return m, keys, sha


def build(seed):
    out = {}
    audio, gt = synth_batch(B, 2, S, seed, DEPTH_MAX)
    out['valid_fraction'] = np.float64((gt > 0).double().mean().item())
    model, out['sd_init_keys'], out['sd_init_sha'] = fresh()
    out['num_params'] = np.int64(model.get_num_params())
    model.eval()
    with torch.no_grad():
        coarse, offset, final = model(audio)
    out['eval/coarse'], out['eval/offset'], out['eval/final'] = coarse.numpy(), offset.numpy(), final.numpy()

    model, _, _ = fresh()
    model.train()
    crit = DualRegressionLoss(coarse_weight=COARSE_W, final_weight=FINAL_W, offset_reg_weight=OFFSET_W)
    opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    opt.zero_grad()
    coarse, offset, final = model(audio)
    total, d = crit(coarse, offset, final, gt)
    total.backward()
    valid = gt > 0
    kinks = np.array([int(((coarse - gt).abs()[valid] < 1e-2).sum()), int(((final - gt).abs()[valid] < 1e-2).sum()),
                      int(((offset.abs() > 0) & (offset.abs() < 1e-3)).sum())], dtype=np.int64)
    out['kinks'] = kinks
    out['offset_zeros'] = np.int64(int((offset == 0).sum()))
    out['train/terms'] = np.array([d['coarse'].item(), d['final'].item(), d['offset_reg'].item(), d['total'].item()],
                                  dtype=np.float64)
    out['train/coarse'], out['train/offset'] = coarse.detach().numpy(), offset.detach().numpy()
    out['train/final'] = final.detach().numpy()
    for k, prm in model.named_parameters():
        gflat = prm.grad.detach().reshape(-1)
        out[f'train/gnorm/{k}'] = np.float64(gflat.double().norm().item())
        out[f'train/gsample/{k}'] = gflat[sample_idx(gflat.numel(), k)].numpy()
    out['train/grad_norm'] = np.float64(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0).item())
    before = {k: q.detach().clone() for k, q in model.named_parameters()}
    opt.step()
    for k, prm in model.named_parameters():
        si = sample_idx(prm.numel(), k)
        out[f'train/p0sample/{k}'] = before[k].reshape(-1)[si].numpy()
        out[f'train/p1sample/{k}'] = prm.detach().reshape(-1)[si].numpy()
    for k, v in model.state_dict().items():
        if 'running_' in k or 'num_batches' in k:
            out[f'train/sd1/{k}'] = v.detach().clone().numpy()
    out['meta'] = np.array([BASE, S, B, seed], dtype=np.int64)
    out['hyper'] = np.array([LR, WD, COARSE_W, FINAL_W, OFFSET_W, DEPTH_MAX], dtype=np.float64)
    return out


def main():
    torch.set_num_threads(8)
    for seed in SEEDS:
        out = build(seed)
        print('seed', seed, 'kinks', out['kinks'].tolist(), 'offset zeros', int(out['offset_zeros']), 'terms',
              out['train/terms'], 'grad_norm', float(out['train/grad_norm']))
        if not out['kinks'].any():
            break
    else:
        raise SystemExit('every seed leaves a pixel next to an L1 kink: nothing written')
    path = os.path.join(HERE, 'dualreg32_bc64.npz')
    np.savez_compressed(path, **out)
    print('dualreg32_bc64 valid fraction', float(out['valid_fraction']), 'bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
