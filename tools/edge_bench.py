"""Micro-benchmark of the thin-layer kernels (csrc/edge.hip) and their neighbours at the unet_256 B=32 shapes.

    python tools/edge_bench.py [--iters 20] [--only NAME]
Prints microseconds and algorithmic TB/s per kernel (HIP events around `iters` back-to-back launches).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from audio_depth_estimation_amd import kernels as K  # noqa: E402

DEV, BF = 'cuda', torch.bfloat16
B, Hs = 32, 128


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--only', default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    mk = lambda c: torch.randn(B, Hs, Hs, c, device=DEV).to(BF)
    x = torch.rand(B, 2, 2 * Hs, 2 * Hs, device=DEV)
    dz = torch.randn(B, 1, 2 * Hs, 2 * Hs, device=DEV)
    w0 = torch.randn(64 * 32, device=DEV) * 0.1
    wd = torch.randn(128 * 16, device=DEV) * 0.05
    ad, rd, ru, zu, Gd, Gu = mk(64), mk(64), mk(64), mk(64), mk(64), mk(64)
    mean, istd = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    P = K.d0_dgrad_num_partials(B, Hs, Hs)
    part = torch.empty(P, 2, 64, device=DEV)
    nbytes = max(K.thin_wgrad_workspace_bytes(B, Hs, Hs, 1, 64, 64), K.thin_wgrad_workspace_bytes(B, Hs, Hs, 2, 64, 0),
                 K.convt_n1_workspace_bytes(B, Hs, Hs))
    ws = torch.empty(nbytes // 4 + 4, device=DEV)
    dwd, dw0 = torch.empty(128 * 16, device=DEV), torch.empty(64 * 32, device=DEV)
    out = torch.empty(B, 2 * Hs, 2 * Hs, device=DEV)
    bias = torch.zeros(1, device=DEV)
    px = B * Hs * Hs
    def two_launch(fn):
        def run():
            os.environ['ADN_CONVT_N1_FUSED'] = '0'
            try:
                fn()
            finally:
                del os.environ['ADN_CONVT_N1_FUSED']
        return run

    n1 = lambda relu: K.convt_n1_forward(BF, B, Hs, Hs, ad if relu else rd, ru, wd, bias, 0, out, ws, relu_in0=relu)
    n1_bytes = px * 128 * 2 + out.numel() * 4
    cases = [
        # the step writes ONE copy of the outermost activation (the leaky one, l0_forward_1out); its readers clamp it
        ('l0_forward_1out', lambda: K.l0_forward(x, w0, B, Hs, Hs, 0.2, ad, None), px * 64 * 2 + x.numel() * 4),
        ('l0_forward_2out', lambda: K.l0_forward(x, w0, B, Hs, Hs, 0.2, ad, rd), px * 64 * 2 * 2 + x.numel() * 4),
        ('d0_dgrad', lambda: K.d0_dgrad(dz, wd, B, Hs, Hs, K.Seg(64, out0=Gd, ref=ad, slope=0.0),
                                        K.Seg(64, out0=Gu, ref=ru, slope=0.0, z=zu, mean=mean, istd=istd, partials=part)),
         px * 64 * 2 * 5 + dz.numel() * 4),
        ('d0_wgrad_clamp', lambda: K.thin_wgrad(dz, ad, ru, B, Hs, Hs, dwd, ws, relu_plain0=True), px * 128 * 2 + dz.numel() * 4),
        ('d0_wgrad', lambda: K.thin_wgrad(dz, rd, ru, B, Hs, Hs, dwd, ws), px * 128 * 2 + dz.numel() * 4),
        ('l0_wgrad', lambda: K.thin_wgrad(x, Gd, None, B, Hs, Hs, dw0, ws), px * 64 * 2 + x.numel() * 4),
        ('convt_n1_fwd_clamp', lambda: n1(True), n1_bytes),
        ('convt_n1_fwd', lambda: n1(False), n1_bytes),
        ('convt_n1_2launch', two_launch(lambda: n1(False)), n1_bytes + px * 64 * 2),
    ]
    for name, fn, byts in cases:
        if args.only and args.only not in name:
            continue
        t = timeit(fn, args.iters)
        print(f'{name:20s} {t * 1e6:8.1f} us  {byts / t / 1e12:6.2f} TB/s (algorithmic bytes)', flush=True)


if __name__ == '__main__':
    main()
