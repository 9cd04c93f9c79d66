"""Hybrid coarse-depth family at the reference defaults: 256x256, B = 16, bf16, base_channels 64.

(a) the full graphed training step of CoarseWithOffsetModel at n_bins 128 (what train_coarse_depth passes) and 8 (the class
    default; its class head runs on the generic GEMM kernels).  Both trainers are built in ONE process and timed
    alternating: ``--warmup`` steps, then ``--steps`` timed steps, ``--repeats`` times each;
(b) adn_hybrid_loss (always with gradients) at the two logits shapes, alternating in the same process with the yardstick
    adn_coarse_loss with gradients (ce_mode 2) at the same shape: time over ``--iters`` launches, hot (the buffers of one
    batch stay in the last-level cache where they fit, as inside a training step) and with a 512 MB buffer overwritten
    before every timed launch.  Algorithmic bytes per pixel, bf16: both read and write nb logits (4 nb bytes); the coarse
    pass adds bins, gt (read) and depth (written) = 12 bytes, the hybrid pass coarse, offset, bins, gt (read) and final,
    doffset (written) = 24 bytes.  ``hybrid_over_coarse_<shape>_<hot|cold>`` is the ratio of the median times,
    ``byte_ratio_<shape>`` the ratio of those bytes.
Prints one JSON line (medians, spread) and, with ``--out``, writes it to that file.

    python tools/bench_hybrid.py --steps 30 --warmup 10 --repeats 5 --out profiles/hybrid_bench.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(ms, prefix):
    med = sorted(ms)[len(ms) // 2]
    return {f'{prefix}_ms_median': round(med, 4), f'{prefix}_ms_all': [round(v, 4) for v in ms],
            f'{prefix}_spread_pct': round(100 * (max(ms) - min(ms)) / med, 2)}


def bench_loss(B, S, nb, iters, warmup, repeats, flush):
    from audio_depth_estimation_amd import kernels as K
    from audio_depth_estimation_amd.dataloader.utils_dataset import compute_bins
    dev = 'cuda'
    pix = B * S * S
    g = torch.Generator().manual_seed(nb)
    edges, centers = compute_bins(nb, 'linear', None, 30.0)
    logits = (3.0 * torch.randn(pix, nb, generator=g)).to(torch.bfloat16).to(dev)
    offset = torch.randn(pix, generator=g).to(dev)
    gt = 30 * torch.rand(pix, generator=g)
    gt[gt < 3] = 0
    bins = torch.clamp(torch.bucketize(gt, edges[1:-1].contiguous()), 0, nb - 1).int().to(dev)
    gt, centers = gt.to(dev), centers.to(dev)
    nv = torch.tensor([float((gt > 0).sum())], dtype=torch.float64, device=dev)
    coarse, depth, final, doff = (torch.empty(pix, device=dev) for _ in range(4))
    dl = torch.empty_like(logits)
    ws = torch.empty(max(K.hybrid_loss_workspace_bytes(pix), K.coarse_loss_workspace_bytes(pix)) // 4 + 4, device=dev)
    K.coarse_loss(logits, nb, centers, coarse)

    def hybrid():
        K.hybrid_loss(logits, nb, centers, coarse, offset, bins, gt, final, dl, doff, ws, ce_weight=1.0, reg_weight=0.5,
                      offset_reg_weight=0.01, label_smoothing=0.1, reg_mode=0)

    def coarse_pass():
        K.coarse_loss(logits, nb, centers, depth, bins=bins, gt=gt, n_valid=nv, ce_mode=2, ce_weight=1.0, reg_weight=0.5,
                      dlogits=dl, workspace=ws)

    def timed(fn, n, cold):
        e = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n if cold else 1)]
        if cold:                         # one event pair per launch, the cache flushed in between
            for e0, e1 in e:
                flush.fill_(1.0)
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            return sum(e0.elapsed_time(e1) for e0, e1 in e) / n
        e0, e1 = e[0]
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    fns = {'hybrid': hybrid, 'coarse': coarse_pass}
    ms = {f'{k}_{t}': [] for k in fns for t in ('hot', 'cold')}
    for _ in range(repeats):
        for k, fn in fns.items():        # alternating: coarse and hybrid share every repeat's conditions
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            ms[f'{k}_hot'].append(timed(fn, iters, False))
            ms[f'{k}_cold'].append(timed(fn, iters, True))
    tag = f'nb{nb}'
    nbytes = {'hybrid': pix * (4 * nb + 24), 'coarse': pix * (4 * nb + 12)}
    res = {f'loss_{tag}_{k}_algorithmic_MB': round(v / 1e6, 2) for k, v in nbytes.items()}
    res[f'byte_ratio_{tag}'] = round(nbytes['hybrid'] / nbytes['coarse'], 4)
    for k in ms:
        res.update(_stats(ms[k], f'loss_{tag}_{k}'))
        res[f'loss_{tag}_{k}_GBps'] = round(nbytes[k.split('_')[0]] / (res[f'loss_{tag}_{k}_ms_median'] * 1e-3) / 1e9, 1)
    for t in ('hot', 'cold'):
        r = res[f'loss_{tag}_hybrid_{t}_ms_median'] / res[f'loss_{tag}_coarse_{t}_ms_median']
        res[f'hybrid_over_coarse_{tag}_{t}'] = round(r, 4)
        res[f'hybrid_over_coarse_{tag}_{t}_vs_byte_ratio'] = round(r / res[f'byte_ratio_{tag}'], 4)
    return res


def bench_step(B, S, steps, warmup, repeats):
    from audio_depth_estimation_amd.dataloader.utils_dataset import compute_bins
    from audio_depth_estimation_amd.hybrid_engine import HybridTrainer
    from audio_depth_estimation_amd.models.coarse_depth_model import CoarseWithOffsetModel
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 2, S, S, generator=g).cuda()
    gt = 30 * torch.rand(B, 1, S, S, generator=g)
    gt[gt < 3] = 0
    gt = gt.cuda()
    trainers, edges = {}, {}
    for nb in (128, 8):
        tag = f'nb{nb}'
        torch.manual_seed(0)
        model = CoarseWithOffsetModel(2, nb, 64, S)
        model.compute_dtype = torch.bfloat16
        e, c = compute_bins(nb, 'linear', None, 30.0)
        model.set_bin_centers(c)
        model = model.cuda().train()
        tr = HybridTrainer(model.engine(), 1.0, 0.5, 0.01, 'l1', 0.1, lr=1e-3, weight_decay=0.01, clip_norm=1.0)
        tr.enable_graph(after_steps=3)
        trainers[tag], edges[tag] = tr, e.cuda()
    ms = {tag: [] for tag in trainers}
    first = {}
    for _ in range(repeats):
        for tag, tr in trainers.items():
            for _ in range(warmup):
                loss, terms = tr.step(x, None, gt, edges=edges[tag])
                first.setdefault(tag, [round(float(v), 5) for v in terms])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                loss, _ = tr.step(x, None, gt, edges=edges[tag])
            e1.record()
            torch.cuda.synchronize()
            assert torch.isfinite(loss).item() and tr._graph is not None
            ms[tag].append(e0.elapsed_time(e1) / steps)
    res = {}
    for tag in ms:
        res.update(_stats(ms[tag], 'step_' + tag))
        res[f'step_{tag}_maps_per_s'] = round(B / (res[f'step_{tag}_ms_median'] * 1e-3), 1)
        res[f'step_{tag}_plane_channels'] = trainers[tag].engine.plane_channels
        res[f'step_{tag}_first_terms'] = first[tag]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--only', choices=['loss', 'step'], default=None)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_hybrid needs a HIP device: nothing can be timed without one')
    res = {'workload': f'hybrid {a.size}x{a.size} B{a.batch} bf16 base 64', 'device': torch.cuda.get_device_name(0),
           'iters': a.iters, 'steps': a.steps, 'warmup': a.warmup, 'repeats': a.repeats}
    if a.only != 'step':
        flush = torch.empty(128 << 20, device='cuda')
        for nb in (128, 8):
            res.update(bench_loss(a.batch, a.size, nb, a.iters, a.warmup, a.repeats, flush))
        del flush
    if a.only != 'loss':
        res.update(bench_step(a.batch, a.size, a.steps, a.warmup, a.repeats))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
