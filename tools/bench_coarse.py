"""Coarse-depth family at the reference defaults: 256x256, B = 16, bf16, 128 bins.

(a) the fused loss head (adn_coarse_loss with gradients: one read of the logits, one write of the gradient) against the
    existing pair adn_bins_fwd + adn_bins_bwd on the same logits (two reads, one write, no classification term);
(b) the full graphed training step of CoarseDepthUNet (base_channels 64).
Kernels are timed back to back in ONE process, alternating, over ``--iters`` launches after ``--warmup``, ``--repeats``
times; between timed loops a 512 MB buffer is overwritten so that no run starts with the 268 MB of logits in the 256 MB
last-level cache of the previous one.  Prints one JSON line with medians, spread and achieved GB/s (algorithmic bytes:
fused = logits read once + gradient written once; pair = logits read twice + gradient written once).

    python tools/bench_coarse.py --iters 50 --warmup 10 --repeats 5
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _loop(fn, iters, warmup, flush):
    for _ in range(warmup):
        fn()
    flush.fill_(1.0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_head(B, S, nb, iters, warmup, repeats):
    from audio_depth_estimation_amd import kernels as K
    from audio_depth_estimation_amd.dataloader.utils_dataset import compute_bins
    dev = 'cuda'
    pix = B * S * S
    g = torch.Generator().manual_seed(0)
    logits = (3 * torch.randn(B, S, S, nb, generator=g)).to(torch.bfloat16).to(dev)
    edges, centers = compute_bins(nb, 'linear', None, 30.0)
    gt = 30 * torch.rand(pix, generator=g)
    gt[gt < 3] = 0
    bins = torch.clamp(torch.bucketize(gt, edges[1:-1].contiguous()), 0, nb - 1).int().to(dev)
    gt, centers = gt.to(dev), centers.to(dev)
    nv = torch.tensor([float((gt > 0).sum())], dtype=torch.float64, device=dev)
    depth, dl = torch.empty(pix, device=dev), torch.empty_like(logits)
    ws = torch.empty(max(K.coarse_loss_workspace_bytes(pix), K.bins_bwd_workspace_bytes(B, S * S, nb)) // 4 + 4, device=dev)
    cb = centers.view(1, nb).expand(B, nb).contiguous()
    dbase, dcent = torch.randn(pix, device=dev), torch.empty(B, nb, device=dev)
    flush = torch.empty(128 << 20, device=dev)

    def fused():
        K.coarse_loss(logits, nb, centers, depth, bins=bins, gt=gt, n_valid=nv, ce_mode=0, dlogits=dl, workspace=ws)

    def pair():
        K.bins_fwd(logits, cb, depth)
        K.bins_bwd(logits, cb, depth, dbase, None, dl, dcent, ws)

    ms = {'fused': [], 'pair': []}
    for _ in range(repeats):
        for k, fn in (('fused', fused), ('pair', pair)):
            ms[k].append(_loop(fn, iters, warmup, flush))
    nbytes = logits.numel() * 2
    res = {}
    for k, reads in (('fused', 1), ('pair', 2)):
        med = sorted(ms[k])[len(ms[k]) // 2]
        res[f'{k}_ms_median'] = round(med, 4)
        res[f'{k}_ms_all'] = [round(v, 4) for v in ms[k]]
        res[f'{k}_spread_pct'] = round(100 * (max(ms[k]) - min(ms[k])) / med, 2)
        res[f'{k}_GBps'] = round((reads + 1) * nbytes / (med * 1e-3) / 1e9, 1)
    res['fused_over_pair'] = round(res['fused_ms_median'] / res['pair_ms_median'], 4)
    # the criterion: the fused kernel does more arithmetic in fewer bytes, so its median must not exceed the pair's by more
    # than the run-to-run spread seen in this very run (the larger of the two kernels' max - min)
    spread_ms = max(max(ms[k]) - min(ms[k]) for k in ms)
    res['spread_ms'] = round(spread_ms, 4)
    res['fused_not_slower_within_spread'] = bool(res['fused_ms_median'] <= res['pair_ms_median'] + spread_ms)
    res['logits_MB'] = round(nbytes / 1e6, 1)
    return res


def bench_step(B, S, nb, steps, warmup, repeats):
    from audio_depth_estimation_amd.coarse_engine import CoarseDepthTrainer
    from audio_depth_estimation_amd.dataloader.utils_dataset import compute_bins
    from audio_depth_estimation_amd.models.coarse_depth_model import define_coarse_depth_model
    torch.manual_seed(0)
    model = define_coarse_depth_model('unet', 2, nb, 64, S)
    model.compute_dtype = torch.bfloat16
    model = model.cuda().train()
    edges, centers = compute_bins(nb, 'linear', None, 30.0)
    model.set_bin_centers(centers.cuda())
    tr = CoarseDepthTrainer(model.engine(), 'soft', lr=1e-3, weight_decay=0.01, clip_norm=1.0)
    tr.enable_graph(after_steps=3)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 2, S, S, generator=g).cuda()
    gt = 30 * torch.rand(B, 1, S, S, generator=g)
    gt[gt < 3] = 0
    gt, edges = gt.cuda(), edges.cuda()
    ms = []
    for _ in range(repeats):
        for _ in range(warmup):
            tr.step(x, None, gt, edges=edges)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            loss, _ = tr.step(x, None, gt, edges=edges)
        e1.record()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item()
        ms.append(e0.elapsed_time(e1) / steps)
    med = sorted(ms)[len(ms) // 2]
    return {'step_ms_median': round(med, 4), 'step_ms_all': [round(v, 4) for v in ms],
            'step_spread_pct': round(100 * (max(ms) - min(ms)) / med, 2), 'maps_per_s': round(B / (med * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--n_bins', type=int, default=128)
    ap.add_argument('--only', choices=['head', 'step'], default=None)
    a = ap.parse_args()
    res = {'workload': f'coarse depth {a.size}x{a.size} B{a.batch} bf16 {a.n_bins} bins', 'device': torch.cuda.get_device_name(0),
           'iters': a.iters, 'steps': a.steps, 'warmup': a.warmup, 'repeats': a.repeats}
    if a.only != 'step':
        res.update(bench_head(a.batch, a.size, a.n_bins, a.iters, a.warmup, a.repeats))
    if a.only != 'head':
        res.update(bench_step(a.batch, a.size, a.n_bins, a.steps, a.warmup, a.repeats))
    print(json.dumps(res))
    if not res.get('fused_not_slower_within_spread', True):
        sys.exit('adn_coarse_loss is slower than adn_bins_fwd + adn_bins_bwd beyond the run-to-run spread')


if __name__ == '__main__':
    main()
