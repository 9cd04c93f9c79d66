"""Coarse-depth family, evaluation side, at the reference defaults: 256x256, B = 16, bf16, 128 bins.

(a) adn_coarse_decode with all six outputs against the forward-only adn_coarse_loss launch (depth alone) on the same
    logits: by bytes per pixel (256 + 24) / (256 + 4) = 1.08.  Timed as tools/bench_coarse.py times its kernels: back to
    back in ONE process, alternating, ``--iters`` launches after ``--warmup``, ``--repeats`` times, a 512 MB buffer
    overwritten between timed loops (the 268 MB of logits do not fit the 256 MB last-level cache either).
(b) the wall time of ``test_coarse_depth --synthetic N --model_type unet --batch_size 16`` on a checkpoint of a freshly
    initialised CoarseDepthUNet (base_channels 64), in a temporary directory.
Prints one JSON line.

    python tools/bench_coarse_decode.py --iters 50 --warmup 10 --repeats 5 --synthetic 256
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_coarse import _loop  # noqa: E402


def bench_kernels(B, S, nb, iters, warmup, repeats):
    from audio_depth_estimation_amd import kernels as K
    from audio_depth_estimation_amd.dataloader.utils_dataset import compute_bins
    dev = 'cuda'
    pix = B * S * S
    g = torch.Generator().manual_seed(0)
    logits = (3 * torch.randn(B, S, S, nb, generator=g)).to(torch.bfloat16).to(dev)
    centers = compute_bins(nb, 'linear', None, 30.0)[1].to(dev)
    depth = torch.empty(pix, device=dev)
    planes = {k: torch.empty(pix, device=dev) for k in ('mean', 'hard', 'std', 'entropy', 'confidence')}
    planes['argmax'] = torch.empty(pix, dtype=torch.int32, device=dev)
    flush = torch.empty(128 << 20, device=dev)
    fns = {'decode': lambda: K.coarse_decode(logits, nb, centers, **planes),
           'forward_only': lambda: K.coarse_loss(logits, nb, centers, depth)}
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(_loop(fn, iters, warmup, flush))
    assert torch.equal(planes['mean'], depth)
    res = {'logits_MB': round(logits.numel() * 2 / 1e6, 1)}
    for k, out_bytes in (('decode', 24), ('forward_only', 4)):
        med = sorted(ms[k])[len(ms[k]) // 2]
        res[f'{k}_ms_median'] = round(med, 4)
        res[f'{k}_ms_all'] = [round(v, 4) for v in ms[k]]
        res[f'{k}_spread_pct'] = round(100 * (max(ms[k]) - min(ms[k])) / med, 2)
        res[f'{k}_TBps'] = round(pix * (nb * 2 + out_bytes) / (med * 1e-3) / 1e12, 3)
    res['decode_over_forward_only'] = round(res['decode_ms_median'] / res['forward_only_ms_median'], 4)
    res['bytes_ratio'] = round((nb * 2 + 24) / (nb * 2 + 4), 4)
    return res


def bench_script(n, B, nb):
    from audio_depth_estimation_amd import test_coarse_depth
    from audio_depth_estimation_amd.config_loader import load_config
    from audio_depth_estimation_amd.dataloader.utils_dataset import compute_bins
    from audio_depth_estimation_amd.models.coarse_depth_model import define_coarse_depth_model
    cfg = load_config(dataset_name='batvisionv2', mode='test', experiment_name='default')
    torch.manual_seed(0)
    model = define_coarse_depth_model('unet', 2, nb, 64, cfg.dataset.images_size)
    edges, centers = compute_bins(nb, 'linear', None, cfg.dataset.max_depth, 0.6)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'exp'))
        path = os.path.join(tmp, 'exp', 'checkpoint_1.pth')
        torch.save({'epoch': 1, 'state_dict': model.state_dict(), 'bin_centers': centers, 'bin_edges': edges}, path)
        os.chdir(tmp)
        try:
            argv = ['--synthetic', str(n), '--batch_size', str(B), '--n_bins', str(nb), '--checkpoint_path', path]
            walls = []
            for _ in range(2):          # the first run also builds the engine's buffers and loads the kernels
                t0 = time.time()
                res = test_coarse_depth.main(argv)
                torch.cuda.synchronize()
                walls.append(round(time.time() - t0, 3))
        finally:
            os.chdir(cwd)
    return {'script_items': n, 'script_batch': B, 'script_image': cfg.dataset.images_size, 'script_wall_s': walls,
            'script_rmse': round(res['rmse'], 4), 'script_top1': round(res['top1'], 4), 'script_ece': round(res['ece'], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--n_bins', type=int, default=128)
    ap.add_argument('--synthetic', type=int, default=256, help='items of the timed test_coarse_depth run (0: skip it)')
    a = ap.parse_args()
    res = {'workload': f'coarse decode {a.size}x{a.size} B{a.batch} bf16 {a.n_bins} bins', 'device': torch.cuda.get_device_name(0),
           'iters': a.iters, 'warmup': a.warmup, 'repeats': a.repeats}
    res.update(bench_kernels(a.batch, a.size, a.n_bins, a.iters, a.warmup, a.repeats))
    if a.synthetic:
        res.update(bench_script(a.synthetic, a.batch, a.n_bins))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
