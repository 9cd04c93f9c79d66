"""Golden vectors of the hybrid coarse-depth family (hybrid32_bc64.npz).

Run on a machine that has the reference checkout (it is imported, never copied), on the CPU in f32:
``torch.manual_seed(0); CoarseWithOffsetModel(2, 8, 64, 32)``, B = 2 at 32 x 32, linear bins on [0.1, 30] from the
reference's own ``BinnedDepthDataset._compute_bins`` (called on a bare object; ``torchaudio`` / ``torchvision`` /
``pandas`` are only imported by that module's file readers, so empty stand-ins are registered when they are missing);
target bins = clamp(bucketize(gt, edges[1:-1]), 0, n_bins - 1).  Recorded:
  * the initial state_dict as key order + one SHA-256 per tensor (``sd_init_keys`` / ``sd_init_sha``), the parameter count
    (``num_params``; ``nb128/num_params`` for 128 bins), the bin edges / centres and the target bins;
  * an eval forward: ``eval/logits`` in full (64 KB), ``eval/coarse``, ``eval/offset``, ``eval/final``;
  * one training step exactly as train_coarse_depth.py:433-463 (CoarseOffsetLoss 1.0 / 0.5 / 0.01, 'l1', label smoothing
    0.1, clip_grad_norm_(1.0), AdamW lr 1e-3 wd 0.01): ce, regression, offset_reg, coarse_l1, total; the three
    training-mode maps; per-parameter gradient norms and 512-entry samples; the clipped norm; sampled parameters before /
    after the step; the BatchNorm buffers after it;
  * ``nb128/``: the same step of a second model (2, 128, 64, 32): the five terms, the three maps, the gradient norms and the
    clipped norm (no logits).
The inputs are not stored: ``synth_batch`` (restated in tests/test_gpu_hybrid.py) regenerates them from the seed.

L1 kinks: the L1 of the final depth is UNMASKED, so every pixel counts.  A pixel within rounding distance of a kink of
|final - gt| or |offset| can flip a gradient sign between two correct implementations.  For both models the maker counts
the pixels with |final - gt| < 1e-2 and those with 0 < |offset| < 1e-3 in the training forward, walks SEEDS until all four
counts are 0, stores them (``kinks`` = 8-bin pair, 128-bin pair) and refuses to write the file otherwise.

ReLU kinks: a BatchNorm output within rounding distance of 0 switches its ReLU on in one correct implementation and off in
another; the whole gradient of that unit then appears or vanishes for every layer in front of it (measured on seed 1266,
where the f32 run and a float64 run of the reference disagree on ONE unit of the last fusion layer: the reference's own
f32 offset-decoder gradients then sit up to 2e-2 of the tensor max away from its float64 ones, its classification
branch 5e-6).  So the maker also runs each candidate in float64 and counts the BatchNorm outputs whose sign differs
between the two runs of the reference (``relu_flips``, both models); a seed is taken only when these are 0 as well.
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# the reference checkout: $REFERENCE_ROOT, or a directory ``reference`` next to this repository
REF = os.environ.get('REFERENCE_ROOT', os.path.join(HERE, '..', '..', '..', 'reference'))
sys.path.insert(0, os.path.abspath(REF))
for name in ('torchaudio', 'torchaudio.transforms', 'torchvision', 'torchvision.transforms', 'pandas'):
    try:
        __import__(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
        if '.' in name:
            setattr(sys.modules[name.split('.')[0]], name.split('.')[1], sys.modules[name])
from dataloader.SparseDepth_Dataset import BinnedDepthDataset          # noqa: E402
from models.coarse_depth_model import CoarseOffsetLoss, CoarseWithOffsetModel          # noqa: E402

NS = 512
BASE, S, B = 64, 32, 2
LR, WD, CE_W, REG_W, OFFSET_W, SMOOTH = 1e-3, 0.01, 1.0, 0.5, 0.01, 0.1
DEPTH_MIN, DEPTH_MAX = 0.1, 30.0
SEEDS = tuple(range(1234, 1234 + 512))
TERMS = ('ce', 'regression', 'offset_reg', 'coarse_l1', 'total')


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


def reference_bins(n_bins):
    ds = object.__new__(BinnedDepthDataset)
    ds.n_bins, ds.bin_mode, ds.sid_alpha, ds.depth_min, ds.depth_max = n_bins, 'linear', 0.6, DEPTH_MIN, DEPTH_MAX
    ds._compute_bins()
    return ds.bin_edges, ds.bin_centers


def fresh(nb):
    torch.manual_seed(0)
    m = CoarseWithOffsetModel(2, nb, BASE, S)
    sd = m.state_dict()
    keys = np.array(list(sd))
    sha = np.array([hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest() for v in sd.values()])
    return m, keys, sha


def train_step(nb, audio, gt, out, pre, full):
    edges, centers = reference_bins(nb)
    bins = torch.clamp(torch.bucketize(gt, edges[1:-1]), 0, nb - 1).squeeze(1)          # [B, H, W] int64
    model, _, _ = fresh(nb)
    out[pre + 'num_params'] = np.int64(model.get_num_params())
    model.set_bin_centers(centers)
    model.train()
    crit = CoarseOffsetLoss(ce_weight=CE_W, regression_weight=REG_W, offset_reg_weight=OFFSET_W, regression_loss='l1',
                            label_smoothing=SMOOTH)
    opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    opt.zero_grad()
    logits, coarse, offset, final = model(audio)
    total, d = crit(logits, coarse, offset, final, gt, bins)
    total.backward()
    kinks = [int(((final - gt).abs() < 1e-2).sum()), int(((offset.abs() > 0) & (offset.abs() < 1e-3)).sum())]
    out[pre + 'offset_zeros'] = np.int64(int((offset == 0).sum()))
    out[pre + 'train/terms'] = np.array([d[k].item() for k in TERMS], dtype=np.float64)
    out[pre + 'train/coarse'], out[pre + 'train/offset'] = coarse.detach().numpy(), offset.detach().numpy()
    out[pre + 'train/final'] = final.detach().numpy()
    for k, prm in model.named_parameters():
        gflat = prm.grad.detach().reshape(-1)
        out[f'{pre}train/gnorm/{k}'] = np.float64(gflat.double().norm().item())
        if full:
            out[f'{pre}train/gsample/{k}'] = gflat[sample_idx(gflat.numel(), k)].numpy()
    out[pre + 'train/grad_norm'] = np.float64(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0).item())
    if full:
        out['edges'], out['centers'], out['bins'] = edges.numpy(), centers.numpy(), bins.numpy().astype(np.int16)
        before = {k: q.detach().clone() for k, q in model.named_parameters()}
        opt.step()
        for k, prm in model.named_parameters():
            si = sample_idx(prm.numel(), k)
            out[f'train/p0sample/{k}'] = before[k].reshape(-1)[si].numpy()
            out[f'train/p1sample/{k}'] = prm.detach().reshape(-1)[si].numpy()
        for k, v in model.state_dict().items():
            if 'running_' in k or 'num_batches' in k:
                out[f'train/sd1/{k}'] = v.detach().clone().numpy()
    return kinks


def bn_outputs(nb, audio, dtype):
    """Training-mode forward of a fresh model in ``dtype``: (offset, final, every BatchNorm output before its ReLU)."""
    model, _, _ = fresh(nb)
    model.set_bin_centers(reference_bins(nb)[1])
    model = model.to(dtype).train()
    outs = []
    for mod in model.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone()))
    with torch.no_grad():
        _, _, offset, final = model(audio.to(dtype))
    return offset, final, outs


def screen(seed):
    """(L1 kink counts, ReLU flips) of both models from forward passes alone; the float64 runs only when they matter."""
    audio, gt = synth_batch(B, 2, S, seed, DEPTH_MAX)
    kinks, runs = [], []
    for nb in (8, 128):
        offset, final, outs = bn_outputs(nb, audio, torch.float32)
        kinks += [int(((final - gt).abs() < 1e-2).sum()), int(((offset.abs() > 0) & (offset.abs() < 1e-3)).sum())]
        runs.append(outs)
    if any(kinks):
        return kinks, None
    flips = []
    for nb, outs in zip((8, 128), runs):
        outs64 = bn_outputs(nb, audio, torch.float64)[2]
        flips.append(sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(outs, outs64)))
    return kinks, flips


def build(seed):
    out = {}
    audio, gt = synth_batch(B, 2, S, seed, DEPTH_MAX)
    kinks = train_step(8, audio, gt, out, '', True) + train_step(128, audio, gt, out, 'nb128/', False)
    out['kinks'] = np.array(kinks, dtype=np.int64)
    if any(kinks):
        return out
    model, out['sd_init_keys'], out['sd_init_sha'] = fresh(8)
    model.set_bin_centers(reference_bins(8)[1])
    model.eval()
    with torch.no_grad():
        logits, coarse, offset, final = model(audio)
    out['eval/logits'] = logits.numpy()
    out['eval/coarse'], out['eval/offset'], out['eval/final'] = coarse.numpy(), offset.numpy(), final.numpy()
    out['meta'] = np.array([BASE, S, B, seed], dtype=np.int64)
    out['hyper'] = np.array([LR, WD, CE_W, REG_W, OFFSET_W, SMOOTH, DEPTH_MAX], dtype=np.float64)
    return out


def main():
    torch.set_num_threads(8)
    assert len(SEEDS) >= 32
    for seed in SEEDS:
        kinks, flips = screen(seed)
        print('seed', seed, 'kinks', kinks, 'relu flips', flips, flush=True)
        if any(kinks) or any(flips):
            continue
        out = build(seed)
        out['relu_flips'] = np.array(flips, dtype=np.int64)
        print('seed', seed, 'kinks', out['kinks'].tolist(), 'offset zeros', int(out['offset_zeros']),
              int(out['nb128/offset_zeros']), 'terms', out['train/terms'], 'grad_norm', float(out['train/grad_norm']))
        if not out['kinks'].any():
            break
    else:
        raise SystemExit('every seed leaves a pixel or a unit next to a kink: nothing written')
    path = os.path.join(HERE, 'hybrid32_bc64.npz')
    np.savez_compressed(path, **out)
    print('hybrid32_bc64 bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
