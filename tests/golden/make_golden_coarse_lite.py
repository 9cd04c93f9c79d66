"""Golden vectors of CoarseDepthLite, the 'lite' model type of the coarse-depth family (coarse_lite64_bc64.npz).

Run on a machine that has the reference checkout (it is imported, never copied), on the CPU in f32:
``CoarseDepthLite(2, n_bins, base, 64)`` + ``init_weights(net, 'kaiming')`` after ``torch.manual_seed(seed)`` -- what the
reference's ``define_coarse_depth_model('lite', ...)`` does --, linear bins on [0.1, 30] from the reference's own
``BinnedDepthDataset._compute_bins``.  Three cases, each under its own key prefix:

  ``sq/``    B = 2, 64 x 64, base 64, 128 bins: the bottleneck is 2 x 2, i.e. 8 values per BatchNorm channel (32 x 32 would
             make the bottleneck BatchNorm a two-sample one)
  ``rect/``  B = 2, H = 96, W = 64 (bottleneck 3 x 2), base 64, 128 bins: catches H / W swaps in the k4 ops
  ``b48/``   B = 2, 64 x 64, base 48 (the class default, not a multiple of 64), 16 bins: eval forward + the soft step's terms

Recorded per case: the initial state_dict as key order + one SHA-256 per tensor, the parameter count, the bins, an eval
forward (``eval/depth`` in full, ``eval/logits`` at sampled positions) and, for each of soft / focal / ce (b48: soft), one
training step exactly as train_coarse_depth.py:446-463 (weights 1.0 / 0.5, mask gt > 0, clip_grad_norm_(1.0), AdamW lr
1e-3 wd 0.01): ce, regression, total; per-parameter gradient norms and 128-entry samples; the clipped norm; sampled
parameters after the step.  The training forward does not depend on the loss mode, so its depth (``train/depth``) and the
BatchNorm buffers after the step (``train/sd1/...``) are stored once per case (the maker asserts that the modes agree).
The inputs are not stored: ``synth_batch`` (restated in tests/test_gpu_coarse_lite.py) regenerates them from the case's
seed, which also seeds the weights.

Conditioning.  A BatchNorm output within rounding distance of 0 switches its ReLU / LeakyReLU side in one correct
implementation and not in another; the gradient of that unit then changes for every layer in front of it.  On the CPU the
reference's own f32-vs-float64 relative gradient error per parameter is bimodal: about 2e-6 when both runs agree on every
unit, 1e-3 .. 5e-3 when one unit flips.  So each candidate seed is also run in float64: ``<case>/relu_flips`` is the number
of BatchNorm outputs whose sign differs between the two runs and ``<case>/f64_grad_err`` the largest relative gradient
error over the parameters and loss modes (conv biases in front of BatchNorm left out: their true gradient is 0 and the
reference holds rounding noise there).  The maker walks the case's SEEDS, takes the first with 0 flips and an error
<= 1e-5, and writes nothing when there is none.
"""
import copy
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
from models.coarse_depth_model import CoarseDepthLite, CoarseDepthLoss, init_weights          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NS = 128
LR, WD, CE_W, REG_W, SIGMA, GAMMA = 1e-3, 0.01, 1.0, 0.5, 2.0, 2.0
DEPTH_MIN, DEPTH_MAX, SID_ALPHA = 0.1, 30.0, 0.6
MODES = (('soft', dict(use_focal=False, use_soft_ce=True)), ('focal', dict(use_focal=True, use_soft_ce=True)),
         ('ce', dict(use_focal=False, use_soft_ce=False)))
# (prefix, B, H, W, base, n_bins, loss modes, candidate seeds)
CASES = (('sq', 2, 64, 64, 64, 128, ('soft', 'focal', 'ce'), (7, 1, 2, 4, 5, 6, 8, 9)),
         ('rect', 2, 96, 64, 64, 128, ('soft', 'focal', 'ce'), (1, 2, 4, 5, 6, 7, 8, 9)),
         ('b48', 2, 64, 64, 48, 16, ('soft',), (7, 1, 2, 4, 5, 6, 8, 9)))
MAX_F64_ERR = 1e-5


def synth_batch(B, C, H, W, seed, max_depth=30.0):
    g = torch.Generator().manual_seed(seed)
    audio = torch.rand(B, C, H, W, generator=g)
    gt = max_depth * torch.rand(B, 1, H, W, generator=g)
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


def zero_grad_bias(name):
    """Conv / transposed-conv biases in front of BatchNorm: the true gradient is 0."""
    part = name.split('.')
    return part[0] in ('encoder', 'decoder') and int(part[1]) % 3 == 0 and part[2] == 'bias'


def bn_signs(model, audio):
    """Signs of every BatchNorm output of one training-mode forward."""
    outs, hooks = [], []
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            hooks.append(m.register_forward_hook(lambda _m, _i, o: outs.append(o.detach() > 0)))
    res = model(audio)
    for h in hooks:
        h.remove()
    return outs, res


def one_case(pre, B, H, W, base, n_bins, modes, seed):
    """-> (dict of arrays, relu flips, largest f32-vs-f64 relative gradient error)."""
    out = {}
    ds = reference_bins(n_bins, 'linear')
    audio, gt = synth_batch(B, 2, H, W, seed, DEPTH_MAX)
    bins = torch.stack([ds.depth_to_bins(gt[b]) for b in range(B)])           # [B, H, W] int64, as the dataset yields them
    out['bins'] = bins.numpy().astype(np.int16)
    out['edges'], out['centers'] = ds.bin_edges.numpy(), ds.bin_centers.numpy()

    def fresh():
        torch.manual_seed(seed)
        m = CoarseDepthLite(2, n_bins, base, W)
        init_weights(m, 'kaiming')
        sd = m.state_dict()
        keys = np.array(list(sd))
        sha = np.array([hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest() for v in sd.values()])
        m.set_bin_centers(ds.bin_centers)
        return m, keys, sha

    model, out['sd_init_keys'], out['sd_init_sha'] = fresh()
    out['num_params'] = np.int64(model.get_num_params())
    model.eval()
    with torch.no_grad():
        logits, depth = model(audio)
    out['eval/depth'] = depth.numpy()
    li = sample_idx(logits.numel(), 'eval/logits', 4096)
    out['eval/logits'] = logits.reshape(-1)[li].numpy()

    flips, err = 0, 0.0
    for tag, kw in MODES:
        if tag not in modes:
            continue
        model, _, _ = fresh()
        model.train()
        m64 = copy.deepcopy(model).double().train()
        crit = CoarseDepthLoss(n_bins=n_bins, ce_weight=CE_W, regression_weight=REG_W, focal_gamma=GAMMA,
                               soft_ce_sigma=SIGMA, **kw)
        opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
        opt.zero_grad()
        s32, (logits, depth) = bn_signs(model, audio)
        d = crit(logits, depth, bins, gt, valid_mask=gt > 0)
        d['total'].backward()
        # the same step of the reference in float64: unit flips and the reference's own rounding error
        s64, (l64, d64) = bn_signs(m64, audio.double())
        crit(l64, d64, bins, gt.double(), valid_mask=gt > 0)['total'].backward()
        flips = max(flips, sum(int((a != b).sum()) for a, b in zip(s32, s64)))
        for (k, p32), (_, p64) in zip(model.named_parameters(), m64.named_parameters()):
            if not zero_grad_bias(k):
                err = max(err, float((p32.grad.double() - p64.grad).norm() / p64.grad.norm()))
        out[tag + '/terms'] = np.array([d['ce'].item(), d['regression'].item(), d['total'].item()], dtype=np.float64)
        if 'train/depth' in out:         # the forward does not depend on the loss: one copy serves the three modes
            assert np.array_equal(out['train/depth'], depth.detach().numpy())
        out['train/depth'] = depth.detach().numpy()
        for k, prm in model.named_parameters():
            gflat = prm.grad.detach().reshape(-1)
            out[f'{tag}/gnorm/{k}'] = np.float64(gflat.double().norm().item())
            out[f'{tag}/gsample/{k}'] = gflat[sample_idx(gflat.numel(), k)].numpy()
        out[tag + '/grad_norm'] = np.float64(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0).item())
        opt.step()
        for k, prm in model.named_parameters():
            out[f'{tag}/p1sample/{k}'] = prm.detach().reshape(-1)[sample_idx(prm.numel(), k)].numpy()
        for k, v in model.state_dict().items():
            if 'running_' in k or 'num_batches' in k:
                assert f'train/sd1/{k}' not in out or np.array_equal(out[f'train/sd1/{k}'], v.numpy())
                out[f'train/sd1/{k}'] = v.detach().clone().numpy()
        print(pre, 'seed', seed, tag, out[tag + '/terms'], 'grad_norm', float(out[tag + '/grad_norm']), flush=True)
    out['meta'] = np.array([n_bins, base, H, W, B, seed], dtype=np.int64)
    out['relu_flips'] = np.int64(flips)
    out['f64_grad_err'] = np.float64(err)
    return {f'{pre}/{k}': v for k, v in out.items()}, flips, err


def main():
    torch.set_num_threads(8)
    out = {}
    for pre, B, H, W, base, n_bins, modes, seeds in CASES:
        for seed in seeds:
            arrays, flips, err = one_case(pre, B, H, W, base, n_bins, modes, seed)
            print(pre, 'seed', seed, 'relu flips', flips, 'f32-vs-f64 gradient error', err, flush=True)
            if flips == 0 and err <= MAX_F64_ERR:
                out.update(arrays)
                break
        else:
            raise SystemExit(f'{pre}: every seed leaves a unit next to its kink: nothing written')
    out['hyper'] = np.array([LR, WD, CE_W, REG_W, SIGMA, GAMMA, DEPTH_MIN, DEPTH_MAX, SID_ALPHA], dtype=np.float64)
    path = os.path.join(HERE, 'coarse_lite64_bc64.npz')
    np.savez_compressed(path, **out)
    print('coarse_lite64_bc64 bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
