"""cVAE vs baseline U-Net: fused, graphed training step of unet_256 ngf 64 at 256x256, B = 32, bf16.

The two models alternate in ONE process (same clocks, same allocator state), each timed over ``--steps`` graph replays
after ``--warmup`` steps, ``--repeats`` times; prints one JSON line with the medians, the spread and the ratio.

    python tools/bench_cvae.py --steps 50 --warmup 10 --repeats 3
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(kind, B, S):
    from types import SimpleNamespace

    from audio_depth_estimation_amd.cvae_engine import CVAETrainer
    from audio_depth_estimation_amd.engine import FusedTrainer
    from audio_depth_estimation_amd.models.unet_cvae_model import define_G_cvae
    from audio_depth_estimation_amd.models.unetbaseline_model import define_G
    cfg = SimpleNamespace(dataset=SimpleNamespace(depth_norm=False, max_depth=30.0))
    torch.manual_seed(0)
    if kind == 'cvae':
        model = define_G_cvae(cfg, 2, 1, 64, 'unet_256', latent_dim=128)
    else:
        model = define_G(cfg, 2, 1, 64, 'unet_256')
    model.compute_dtype = torch.bfloat16
    model = model.cuda().train()
    hyper = ('Combined', 0.237, 0.637, 0.869)
    if kind == 'cvae':
        tr = CVAETrainer(model.engine(), *hyper, max_depth=30.0, lr=0.002, kl_weight=1e-4, clip_norm=1.0)
    else:
        tr = FusedTrainer(model.engine(), *hyper, max_depth=30.0, lr=0.002, clip_norm=1.0, mask_mode='gt0')
    tr.enable_graph(after_steps=3)
    g = torch.Generator().manual_seed(1)
    audio = torch.rand(B, 2, S, S, generator=g).cuda()
    gt = 30 * torch.rand(B, 1, S, S, generator=g)
    gt[gt < 3] = 0
    return tr, audio, gt.cuda()


def timed(tr, audio, gt, steps, warmup):
    for _ in range(warmup):
        tr.step(audio, gt)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss, _ = tr.step(audio, gt)
    e1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--only', choices=['cvae', 'baseline'], default=None, help='time one model (profiler runs)')
    a = ap.parse_args()
    kinds = [a.only] if a.only else ['cvae', 'baseline']
    runs = {k: make(k, a.batch, 256) for k in kinds}
    ms = {k: [] for k in kinds}
    for _ in range(a.repeats):
        for k in kinds:
            ms[k].append(timed(*runs[k], a.steps, a.warmup))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    res = {'workload': 'unet_256 ngf64 256x256 bf16 fused graphed step', 'batch': a.batch, 'steps': a.steps,
           'warmup': a.warmup, 'repeats': a.repeats, 'device': torch.cuda.get_device_name(0)}
    for k in kinds:
        res[f'{k}_step_ms_median'] = round(med[k], 4)
        res[f'{k}_step_ms_all'] = [round(v, 4) for v in ms[k]]
        res[f'{k}_spread_pct'] = round(100 * (max(ms[k]) - min(ms[k])) / med[k], 2)
    if len(kinds) == 2:
        res['cvae_over_baseline'] = round(med['cvae'] / med['baseline'], 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
