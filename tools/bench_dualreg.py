"""Dual-regression coarse-depth family at the reference defaults: 256x256, B = 16, bf16, base_channels 64.

(a) the full graphed training step of DualRegressionModel with the coarse-depth plane padded to one 16-byte chunk
    ('epc': the fusion conv, its input gradient and its weight gradient leave the MFMA kernels for the generic ones) and
    padded to 64 channels (MFMA kernels, K of that one layer doubled).  Both engines are built in ONE process and timed
    alternating: ``--warmup`` steps, then ``--steps`` timed steps, ``--repeats`` times each;
(b) adn_dualreg_loss with gradients (three f32 planes read, three written) and its finish launch: time over ``--iters``
    launches and achieved bytes/s against those algorithmic bytes.  The six planes of one batch (25 MB) stay in the last-level
    cache between launches, as they do inside a training step, where the two heads have just written the inputs; a
    second figure is taken with a 512 MB buffer overwritten before every timed launch (planes come from HBM).
Prints one JSON line (medians, spread) and, with ``--out``, writes it to that file.

    python tools/bench_dualreg.py --steps 30 --warmup 10 --repeats 5 --out profiles/dualreg_bench.json
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


def bench_loss(B, S, iters, warmup, repeats):
    from audio_depth_estimation_amd import kernels as K
    dev = 'cuda'
    pix = B * S * S
    g = torch.Generator().manual_seed(0)
    coarse = (30 * torch.rand(pix, generator=g)).to(dev)
    offset = torch.randn(pix, generator=g).to(dev)
    gt = 30 * torch.rand(pix, generator=g)
    gt[gt < 3] = 0
    gt = gt.to(dev)
    nv = torch.tensor([float((gt > 0).sum())], dtype=torch.float64, device=dev)
    final, dc, do = torch.empty(pix, device=dev), torch.empty(pix, device=dev), torch.empty(pix, device=dev)
    ws = torch.empty(K.dualreg_loss_workspace_bytes(pix) // 4 + 4, device=dev)
    sums, terms = torch.zeros(3, dtype=torch.float64, device=dev), torch.zeros(4, device=dev)
    flush = torch.empty(128 << 20, device=dev)

    def loss():
        K.dualreg_loss(coarse, offset, final, gt=gt, n_valid=nv, dcoarse=dc, doffset=do, workspace=ws)

    def finish():
        K.dualreg_loss_finish(ws, pix, sums, nv, pix, 1.0, 1.0, 0.01, terms)

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

    ms = {'loss_hot': [], 'loss_cold': [], 'finish': []}
    for _ in range(repeats):
        for _ in range(warmup):
            loss()
            finish()
        torch.cuda.synchronize()
        ms['loss_hot'].append(timed(loss, iters, False))
        ms['loss_cold'].append(timed(loss, iters, True))
        ms['finish'].append(timed(finish, iters, False))
    nbytes = 6 * pix * 4
    res = {'loss_algorithmic_MB': round(nbytes / 1e6, 2)}
    for k in ms:
        res.update(_stats(ms[k], k))
    for k in ('loss_hot', 'loss_cold'):
        res[f'{k}_GBps'] = round(nbytes / (res[f'{k}_ms_median'] * 1e-3) / 1e9, 1)
    return res


def bench_step(B, S, steps, warmup, repeats):
    from audio_depth_estimation_amd.dualreg_engine import DualRegressionTrainer
    from audio_depth_estimation_amd.models.coarse_depth_model import DualRegressionModel
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 2, S, S, generator=g).cuda()
    gt = 30 * torch.rand(B, 1, S, S, generator=g)
    gt[gt < 3] = 0
    gt = gt.cuda()
    trainers = {}
    for tag, plane in (('plane64', 64), ('plane_epc', 'epc')):
        torch.manual_seed(0)
        model = DualRegressionModel(2, 64, S)
        model.compute_dtype, model.plane_channels = torch.bfloat16, plane
        model = model.cuda().train()
        tr = DualRegressionTrainer(model.engine(), lr=1e-3, weight_decay=0.01, clip_norm=1.0)
        tr.enable_graph(after_steps=3)
        trainers[tag] = tr
    ms = {tag: [] for tag in trainers}
    first = {}
    for _ in range(repeats):
        for tag, tr in trainers.items():
            for _ in range(warmup):
                loss, terms = tr.step(x, gt)
                first.setdefault(tag, [round(float(v), 5) for v in terms])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                loss, _ = tr.step(x, gt)
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
    res['plane64_over_epc'] = round(res['step_plane64_ms_median'] / res['step_plane_epc_ms_median'], 4)
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
        sys.exit('bench_dualreg needs a HIP device: nothing can be timed without one')
    res = {'workload': f'dual regression {a.size}x{a.size} B{a.batch} bf16 base 64', 'device': torch.cuda.get_device_name(0),
           'iters': a.iters, 'steps': a.steps, 'warmup': a.warmup, 'repeats': a.repeats}
    if a.only != 'step':
        res.update(bench_loss(a.batch, a.size, a.iters, a.warmup, a.repeats))
    if a.only != 'loss':
        res.update(bench_step(a.batch, a.size, a.steps, a.warmup, a.repeats))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
