"""cVAE multi-hypothesis inference: K forwards + torch statistics against one ``sample(audio, K)`` call.

unet_256 ngf 64, latent 128, 256x256, B = 32, bf16, eval mode.  For every K in ``--ks``:
  (a) ``forward``: K successive ``model(audio)`` calls, ``torch.stack`` of the K maps, ``.mean(0)`` and ``.std(0)``
      (what a user had to write before ``sample`` existed; the forward path is the one ``sample`` leaves untouched);
  (b) ``sample``: ``model.sample(audio, K)`` on an engine that only samples (its sampling buffer set stays current);
  (c) ``sample_shared``: the same call on the engine that also runs (a): every call enters the sampling set, re-packs the
      weight operands there and hands the engine back (what a validation pass inside a training script pays).
The variants alternate in ONE process, each timed with device events over ``--iters`` calls after ``--warmup`` calls,
``--repeats`` times; medians and spread are reported.  The stats kernel is also timed alone at [K, B * 256 * 256] against a
device-to-device copy of the same number of bytes moved (the HBM copy rate of this run), both as achieved bytes/s from
the bytes the algorithm needs: (K + 2) * N * 4 for the kernel, 2 * bytes for the copy.  Prints one JSON line.

    python tools/bench_cvae_sample.py --ks 4 16 --iters 10 --warmup 3 --repeats 3
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make():
    from audio_depth_estimation_amd.models.unet_cvae_model import define_G_cvae
    cfg = SimpleNamespace(dataset=SimpleNamespace(depth_norm=False, max_depth=30.0))
    torch.manual_seed(0)
    model = define_G_cvae(cfg, 2, 1, 64, 'unet_256', latent_dim=128)
    with torch.no_grad():
        model.model.upconv.bias.fill_(1.0)
    model.compute_dtype = torch.bfloat16
    return model.cuda().eval()


def k_forwards(model, audio, Kn):
    with torch.no_grad():
        maps = torch.stack([model(audio)[0] for _ in range(Kn)])
        return maps, maps.mean(0), maps.std(0) if Kn > 1 else torch.zeros_like(maps[0])


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ks', type=int, nargs='+', default=[4, 16])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_cvae_sample.py measures on a HIP device: none is visible')
    from audio_depth_estimation_amd import kernels as K
    shared, alone = make(), make()
    audio = torch.rand(a.batch, 2, 256, 256, generator=torch.Generator().manual_seed(1)).cuda()
    res = {'workload': 'unet_256 ngf64 L128 256x256 bf16 eval: K forwards + torch mean/std vs sample(K)', 'batch': a.batch,
           'iters': a.iters, 'warmup': a.warmup, 'repeats': a.repeats, 'device': torch.cuda.get_device_name(0)}
    for Kn in a.ks:
        variants = {'forward': lambda: k_forwards(shared, audio, Kn), 'sample': lambda: alone.sample(audio, Kn),
                    'sample_shared': lambda: shared.sample(audio, Kn)}
        ms = {k: [] for k in variants}
        for _ in range(a.repeats):
            for name, fn in variants.items():
                t, out = timed(fn, a.iters, a.warmup)
                assert torch.isfinite(out[1]).all()
                ms[name].append(t)
        for name in variants:
            res[f'k{Kn}_{name}_ms_median'] = round(median(ms[name]), 3)
            res[f'k{Kn}_{name}_ms_all'] = [round(v, 3) for v in ms[name]]
        res[f'k{Kn}_sample_over_forward'] = round(median(ms['sample']) / median(ms['forward']), 4)
        res[f'k{Kn}_sample_shared_over_forward'] = round(median(ms['sample_shared']) / median(ms['forward']), 4)
        res[f'k{Kn}_flops_expectation'] = round((Kn + 1) / (2 * Kn), 4)
        # the stats kernel alone, against a copy that moves the same number of bytes
        N = a.batch * 256 * 256
        x = 30 * torch.rand(Kn, N, device='cuda')
        mean, std = torch.empty(N, device='cuda'), torch.empty(N, device='cuda')
        nbytes = (Kn + 2) * N * 4
        src = torch.empty(nbytes // 8, device='cuda')
        dst = torch.empty_like(src)
        ts, tc = [], []
        for _ in range(a.repeats):
            ts.append(timed(lambda: K.sample_stats(x, mean, std), 50, 5)[0])
            tc.append(timed(lambda: dst.copy_(src), 50, 5)[0])
        res[f'k{Kn}_stats_us_median'] = round(1e3 * median(ts), 2)
        res[f'k{Kn}_stats_gbps'] = round(nbytes / median(ts) / 1e6, 1)
        res[f'k{Kn}_copy_gbps'] = round(nbytes / median(tc) / 1e6, 1)
        res[f'k{Kn}_stats_over_copy_rate'] = round(median(tc) / median(ts), 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
