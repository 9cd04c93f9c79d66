"""CoarseDepthLite at the reference's training shape: 256x256, B = 16, bf16, base_channels 64, 128 bins.

(a) the full graphed training step (CoarseDepthTrainer, soft CE) with the thin first layer and with the first layer on
    adn_igemm (ADN_LITE_L0_IGEMM=1).  Both trainers are built in ONE process and timed alternating: ``--warmup`` steps, then
    ``--steps`` timed steps, ``--repeats`` times each;
(b) the first layer's forward up to (z, BatchNorm partial rows), alternating in the same process:
      thin   adn_l0_forward_stats on the f32 NCHW input                                      (1 launch)
      igemm  adn_nchw_slice_to_nhwc into the zero-padded bf16 record + adn_igemm S2 Z_STATS  (2 launches; the yardstick:
             code that exists without the thin kernel); ``l0_igemm_gemm`` is its GEMM launch alone
    time over ``--iters`` launches, hot (the 42 MB of one batch stay in the last-level cache where they fit, as inside a
    training step) and with a 512 MB buffer overwritten before every timed launch.  Algorithmic bytes of the layer: x f32
    read once (B * 2 * 256 * 256 * 4) + z bf16 written once (B * 128 * 128 * 64 * 2); the GB/s figures divide these bytes
    by the median time, whatever a route moves in fact.
    ``thin_stays_default_<hot|cold>``: the rule of DESIGN.md 9.3 -- the thin route's median is not above the igemm route's by
    more than the spread of the repeats (the larger of the two routes' max - min).
Prints one JSON line (medians, spread) and, with ``--out``, writes it to that file.

    python tools/bench_coarse_lite.py --steps 30 --warmup 10 --repeats 5 --out profiles/coarse_lite_bench.json
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


def bench_l0(B, S, iters, warmup, repeats, flush):
    from audio_depth_estimation_amd import kernels as K
    from audio_depth_estimation_amd._lib import EPI_Z_STATS, GEMM_S2
    dev, T = 'cuda', torch.bfloat16
    hs = ws_ = S // 2
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 2, S, S, generator=g).to(dev)
    wm = (0.25 * torch.randn(64, 16, 2, generator=g)).to(dev)
    bias = torch.randn(64, generator=g).to(dev)
    z = torch.empty(B, hs, ws_, 64, dtype=T, device=dev)
    p_thin = torch.empty(K.l0_forward_stats_num_partials(B, hs, ws_) * 128, device=dev)
    x8 = torch.empty(B, S, S, 8, dtype=T, device=dev)
    w_s2 = torch.zeros(64, 16, 8, dtype=T, device=dev)
    K.pack_weights(wm.view(-1), 64, 2, T, w_s2, None, y_pad=8)
    P, wsb = K.igemm_query(T, GEMM_S2, B, hs, ws_, 8, 0, 64, [64], epi=EPI_Z_STATS)
    p_ig = torch.empty(P * 128, device=dev)
    work = torch.empty(wsb // 4 + 4, device=dev)
    seg = [K.Seg(64, out0=z, partials=p_ig, bias=bias)]

    def thin():
        K.l0_forward_stats(x, wm, bias, B, hs, ws_, z, p_thin)

    def gemm():
        K.igemm(T, GEMM_S2, B, hs, ws_, x8, None, w_s2, 64, EPI_Z_STATS, seg, work)

    def igemm():
        K.nchw_slice_to_nhwc(x, 0, 2, x8)
        gemm()

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

    fns = {'thin': thin, 'igemm': igemm, 'igemm_gemm': gemm}
    ms = {f'{k}_{t}': [] for k in fns for t in ('hot', 'cold')}
    for _ in range(repeats):
        for k, fn in fns.items():        # alternating: the routes share every repeat's conditions
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            ms[f'{k}_hot'].append(timed(fn, iters, False))
            ms[f'{k}_cold'].append(timed(fn, iters, True))
    nbytes = B * 2 * S * S * 4 + B * hs * ws_ * 64 * 2
    res = {'l0_algorithmic_MB': round(nbytes / 1e6, 2), 'l0_thin_partial_rows': p_thin.numel() // 128, 'l0_igemm_partial_rows': P}
    for k in ms:
        res.update(_stats(ms[k], 'l0_' + k))
        res[f'l0_{k}_GBps'] = round(nbytes / (res[f'l0_{k}_ms_median'] * 1e-3) / 1e9, 1)
    for t in ('hot', 'cold'):
        a, b = ms[f'thin_{t}'], ms[f'igemm_{t}']
        spread = max(max(a) - min(a), max(b) - min(b))
        res[f'l0_thin_over_igemm_{t}'] = round(res[f'l0_thin_{t}_ms_median'] / res[f'l0_igemm_{t}_ms_median'], 4)
        res[f'l0_repeat_spread_ms_{t}'] = round(spread, 4)
        res[f'thin_stays_default_{t}'] = bool(res[f'l0_thin_{t}_ms_median'] <= res[f'l0_igemm_{t}_ms_median'] + spread)
    return res


def bench_step(B, S, steps, warmup, repeats):
    from audio_depth_estimation_amd.coarse_engine import CoarseDepthTrainer
    from audio_depth_estimation_amd.dataloader.utils_dataset import compute_bins
    from audio_depth_estimation_amd.models.coarse_depth_model import CoarseDepthLite, init_net
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 2, S, S, generator=g).cuda()
    gt = 30 * torch.rand(B, 1, S, S, generator=g)
    gt[gt < 3] = 0
    gt = gt.cuda()
    e, c = compute_bins(128, 'linear', None, 30.0)
    edges = e.cuda()
    trainers = {}
    for tag in ('thin', 'igemm'):
        if tag == 'igemm':
            os.environ['ADN_LITE_L0_IGEMM'] = '1'
        else:
            os.environ.pop('ADN_LITE_L0_IGEMM', None)
        torch.manual_seed(0)
        model = init_net(CoarseDepthLite(2, 128, 64, S), 'kaiming')
        model.compute_dtype = torch.bfloat16
        model.set_bin_centers(c)
        model = model.cuda().train()
        tr = CoarseDepthTrainer(model.engine(), 'soft', 1.0, 0.5, 2.0, 2.0, lr=1e-3, weight_decay=0.01, clip_norm=1.0)
        tr.enable_graph(after_steps=3)
        tr.step(x, None, gt, edges=edges)               # the route is chosen when the shape is prepared
        assert model.engine().thin_l0 == (tag == 'thin')
        trainers[tag] = tr
    os.environ.pop('ADN_LITE_L0_IGEMM', None)
    ms = {tag: [] for tag in trainers}
    first = {}
    for _ in range(repeats):
        for tag, tr in trainers.items():
            for _ in range(warmup):
                loss, terms = tr.step(x, None, gt, edges=edges)
                first.setdefault(tag, [round(float(v), 5) for v in terms])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                loss, _ = tr.step(x, None, gt, edges=edges)
            e1.record()
            torch.cuda.synchronize()
            assert torch.isfinite(loss).item() and tr._graph is not None
            ms[tag].append(e0.elapsed_time(e1) / steps)
    res = {}
    for tag in ms:
        res.update(_stats(ms[tag], 'step_' + tag))
        res[f'step_{tag}_maps_per_s'] = round(B / (res[f'step_{tag}_ms_median'] * 1e-3), 1)
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
    ap.add_argument('--only', choices=['l0', 'step'], default=None)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_coarse_lite needs a HIP device: nothing can be timed without one')
    res = {'workload': f'coarse lite {a.size}x{a.size} B{a.batch} bf16 base 64 nb128', 'device': torch.cuda.get_device_name(0),
           'iters': a.iters, 'steps': a.steps, 'warmup': a.warmup, 'repeats': a.repeats}
    if a.only != 'step':
        flush = torch.empty(128 << 20, device='cuda')
        res.update(bench_l0(a.batch, a.size, a.iters, a.warmup, a.repeats, flush))
        del flush
    if a.only != 'l0':
        res.update(bench_step(a.batch, a.size, a.steps, a.warmup, a.repeats))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
