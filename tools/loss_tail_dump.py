"""Dumps every output of the loss-tail kernels (csrc/loss_tail.h and its users) for a byte-for-byte A/B of two libraries.

    ADN_LIB=/path/to/libadn.so python tools/loss_tail_dump.py --out A.npz      (one process per library, needs a GPU)
    python tools/loss_tail_dump.py --compare A.npz B.npz                       (host only; exit status 1 on a difference)

Covers adn_coarse_loss / _finish (every vector width, the wave-per-pixel forms, a misaligned view, past one grid pass; soft /
focal / plain; forward-only, without argmax, with argmax and gradient, no valid pixel, a two-rank global batch, both finish
phases), adn_hybrid_loss / _finish (CASES x VARIANTS of tests/test_gpu_hybrid.py), adn_dualreg_loss / _finish,
adn_coarse_targets, adn_baseres_stats, adn_distill_pix_stats and adn_l1tv_stats / _finish.  Inputs are seeded on the CPU;
every output buffer, the f64 workspace of per-block partial rows included (it pins the reduction order), is pre-filled with a
sentinel so that unwritten elements are compared too.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = 'cuda'
PIXELS = (1, 63, 257, 8193)
VEC = [(nb, nb) for nb in (8, 16, 32, 64, 128, 256, 512)]
COARSE_BF16 = VEC + [(24, 24), (12, 16), (100, 128), (8, 64)]
COARSE_F32 = [(8, 8), (5, 8), (512, 512)]
PAST_ONE_PASS = [(8, 8, 2048 * 4 * 64 + 1), (128, 128, 2048 * 4 * 4 + 1)]
N_CASES = [128, 2049, 70000, 2097152 + 3 * 2048 + 5]                    # tests/test_gpu_adabins_kernels.py
L1TV_SHAPES = [(2, 16, 16), (3, 7, 9), (4, 64, 64)]                     # tests/test_gpu_dcnet_kernels.py


def compare(a, b):
    za, zb = np.load(a), np.load(b)
    if sorted(za.files) != sorted(zb.files):
        print('different sets of arrays:', sorted(set(za.files) ^ set(zb.files))[:10])
        return 1
    nbytes, differing = 0, []
    for k in za.files:
        x, y = za[k], zb[k]
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            if not differing:
                same_form = x.shape == y.shape and x.dtype == y.dtype
                bad = int(np.flatnonzero(x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8))[0]) if same_form else -1
                print(f'first differing array: {k} ({x.dtype}{list(x.shape)} vs {y.dtype}{list(y.shape)}, first differing byte {bad})')
            differing.append(k)
        nbytes += x.nbytes
    if differing:
        print(f'{len(differing)} of {len(za.files)} arrays differ:', ' '.join(differing[:40]), '...' if len(differing) > 40 else '')
        return 1
    print(f'{len(za.files)} arrays, {nbytes} bytes: byte-identical')
    return 0


def dump(path):
    import torch

    from audio_depth_estimation_amd import _lib
    from audio_depth_estimation_amd import kernels as K
    out = {}

    def keep(tag, **arrays):
        torch.cuda.synchronize()
        for k, t in arrays.items():
            t = t.detach().cpu().contiguous()
            out[f'{tag}/{k}'] = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()

    dev = lambda t: t.to(DEV)
    f32 = lambda n, v=-7.0: torch.full((n,), v, device=DEV)
    f64 = lambda n, v=-7.0: torch.full((n,), v, dtype=torch.float64, device=DEV)

    def logits_of(dtype, nb, ld, pixels, g, misaligned=False):
        x = (3.0 * torch.randn(pixels, ld, generator=g)).to(dtype)
        x[min(5, pixels - 1), :nb] = 0.0                                # a tie: the first maximum wins
        if not misaligned:
            return dev(x)
        buf = torch.zeros(pixels * ld + 1, dtype=dtype, device=DEV)     # a view one element off the 16-byte boundary
        buf[1:] = dev(x).reshape(-1)
        return buf[1:].view(pixels, ld)

    def out_like(lg, v=7.0, misaligned=False):
        if not misaligned:
            return torch.full(lg.shape, v, dtype=lg.dtype, device=DEV)
        return torch.full((lg.numel() + 1,), v, dtype=lg.dtype, device=DEV)[1:].view(lg.shape)

    # ---- adn_coarse_loss / adn_coarse_loss_finish
    def coarse(dtype, nb, ld, pixels, modes, misaligned=False):
        name = ('bf16' if dtype == torch.bfloat16 else 'f32') + f'-nb{nb}-ld{ld}-px{pixels}' + ('-off1' if misaligned else '')
        g = torch.Generator().manual_seed(17 * nb + ld + pixels)
        lg = logits_of(dtype, nb, ld, pixels, g, misaligned)
        cen = dev(torch.linspace(0.5, 30.0, nb))
        gt = 31.0 * torch.rand(pixels, generator=g)
        gt[torch.rand(pixels, generator=g) < 0.1] = 0.0
        bins = dev(torch.randint(0, nb, (pixels,), generator=g).int())
        nws = K.coarse_loss_workspace_bytes(pixels) // 8
        depth = f32(pixels)
        K.coarse_loss(lg, nb, cen, depth)
        keep(f'coarse/{name}/fwd', depth=depth)
        for mode in modes:
            for var, gtv, scale, with_am, with_dl in (('noargmax', gt, 1, False, False), ('full', gt, 1, True, True),
                                                      ('novalid', torch.zeros(pixels), 1, True, True), ('x2', gt, 2, True, True)):
                nv = dev(torch.tensor([float((gtv > 0).sum()) * scale], dtype=torch.float64))
                depth, ws, sums, terms = f32(pixels), f64(nws + 1), f64(2), f32(3)
                am = torch.full((pixels,), -7, dtype=torch.int32, device=DEV) if with_am else None
                dl = out_like(lg, misaligned=misaligned) if with_dl else None
                K.coarse_loss(lg, nb, cen, depth, bins=bins, gt=dev(gtv), n_valid=nv, pixels_global=scale * pixels, ce_mode=mode,
                              sigma=2.0, gamma=2.0, ce_weight=1.0, reg_weight=0.5, argmax=am, dlogits=dl, workspace=ws)
                K.coarse_loss_finish(ws, pixels, sums, nv, scale * pixels, 1.0, 0.5, terms)
                terms2 = f32(3)                                          # second phase: the sums taken as given
                K.coarse_loss_finish(None, pixels, sums, nv, scale * pixels, 1.0, 0.5, terms2)
                sums3 = f64(2)                                           # first phase alone: no terms
                K.coarse_loss_finish(ws, pixels, sums3, None, scale * pixels, 1.0, 0.5, None)
                arrays = dict(depth=depth, ws=ws, sums=sums, terms=terms, terms2=terms2, sums3=sums3)
                if with_am:
                    arrays['argmax'] = am
                if with_dl:
                    arrays['dlogits'] = dl
                keep(f'coarse/{name}/mode{mode}/{var}', **arrays)

    for px in PIXELS:
        for nb, ld in COARSE_BF16:
            coarse(torch.bfloat16, nb, ld, px, (0, 1, 2))
        coarse(torch.bfloat16, 128, 128, px, (0, 1, 2), misaligned=True)
        for nb, ld in COARSE_F32:
            coarse(torch.float32, nb, ld, px, (0, 1, 2))
    for nb, ld, px in PAST_ONE_PASS:
        coarse(torch.bfloat16, nb, ld, px, (0, 1, 2))

    # ---- adn_hybrid_loss / adn_hybrid_loss_finish: CASES x VARIANTS of tests/test_gpu_hybrid.py
    forms = [(torch.float32, 8, 8), (torch.float32, 5, 8), (torch.float32, 512, 512), (torch.bfloat16, 8, 8),
             (torch.bfloat16, 128, 128), (torch.bfloat16, 512, 512), (torch.bfloat16, 12, 16)]
    cases = [(dt, nb, ld, px) for dt, nb, ld in forms for px in PIXELS]
    cases += [(torch.bfloat16, 8, 8, 2048 * 4 * 64 + 1), (torch.bfloat16, 128, 128, 2048 * 4 * 64 // 16 + 1)]
    for dtype, nb, ld, pixels in cases:
        name = ('bf16' if dtype == torch.bfloat16 else 'f32') + f'-nb{nb}-ld{ld}-px{pixels}'
        g = torch.Generator().manual_seed(11 * nb + pixels)
        lg = logits_of(dtype, nb, ld, pixels, g)
        cen = dev(torch.linspace(0.5, 30.0, nb))
        bins = dev(torch.randint(0, nb, (pixels,), generator=g).int())
        coarse_pl = dev(30.0 * torch.rand(pixels, generator=g))
        offset = 4.0 * torch.randn(pixels, generator=g)
        offset[::5] = 0.0
        gt = 31.0 * torch.rand(pixels, generator=g)
        gt[torch.rand(pixels, generator=g) < 0.1] = 0.0
        nws = K.hybrid_loss_workspace_bytes(pixels) // 8
        for reg_mode, scale in ((0, 1), (1, 2), (0, 2), (1, 1)):
            final, doff, dl, ws, sums, terms, terms2 = f32(pixels), f32(pixels), out_like(lg), f64(nws + 1), f64(4), f32(5), f32(5)
            K.hybrid_loss(lg, nb, cen, coarse_pl, dev(offset), bins, dev(gt), final, dl, doff, ws, pixels_global=scale * pixels,
                          ce_weight=1.0, reg_weight=0.5, offset_reg_weight=0.01, label_smoothing=0.1, reg_mode=reg_mode)
            K.hybrid_loss_finish(ws, pixels, sums, scale * pixels, 1.0, 0.5, 0.01, terms)
            K.hybrid_loss_finish(None, pixels, sums, scale * pixels, 1.0, 0.5, 0.01, terms2)
            keep(f'hybrid/{name}/reg{reg_mode}-x{scale}', final=final, doffset=doff, dlogits=dl, ws=ws, sums=sums, terms=terms,
                 terms2=terms2)

    # ---- adn_dualreg_loss / adn_dualreg_loss_finish
    for pixels in (1, 63, 257, 2048, 600001):
        g = torch.Generator().manual_seed(pixels)
        c, o = dev(30.0 * torch.rand(pixels, generator=g)), 4.0 * torch.randn(pixels, generator=g)
        o[::5] = 0.0
        o = dev(o)
        gt = 31.0 * torch.rand(pixels, generator=g)
        gt[torch.rand(pixels, generator=g) < 0.1] = 0.0
        nws = K.dualreg_loss_workspace_bytes(pixels) // 8
        final = f32(pixels)
        K.dualreg_loss(c, o, final)
        keep(f'dualreg/px{pixels}/fwd', final=final)
        for invalid in (False, True):
            for scale in (1, 2):
                gtv = torch.zeros(pixels) if invalid else gt
                nv = dev(torch.tensor([float((gtv > 0).sum()) * scale], dtype=torch.float64))
                final, dc, do, ws, sums, terms, terms2 = f32(pixels), f32(pixels), f32(pixels), f64(nws + 1), f64(3), f32(4), f32(4)
                K.dualreg_loss(c, o, final, gt=dev(gtv), n_valid=nv, pixels_global=scale * pixels, coarse_weight=1.0,
                               final_weight=0.7, offset_reg_weight=0.01, dcoarse=dc, doffset=do, workspace=ws)
                K.dualreg_loss_finish(ws, pixels, sums, nv, scale * pixels, 1.0, 0.7, 0.01, terms)
                K.dualreg_loss_finish(None, pixels, sums, nv, scale * pixels, 1.0, 0.7, 0.01, terms2)
                keep(f'dualreg/px{pixels}/invalid{int(invalid)}-x{scale}', final=final, dcoarse=dc, doffset=do, ws=ws, sums=sums,
                     terms=terms, terms2=terms2)

    # ---- adn_coarse_targets, adn_baseres_stats, adn_distill_pix_stats
    for n in N_CASES:
        g = torch.Generator().manual_seed(n)
        depth = 36.0 * torch.rand(n, generator=g) - 1.0
        depth[torch.rand(n, generator=g) < 0.1] = 0.0
        edges = dev(torch.linspace(0.0, 30.0, 129)[1:-1].contiguous())
        nws = K.coarse_targets_workspace_bytes(n) // 8
        bins, stats, ws = torch.full((n,), -7, dtype=torch.int32, device=DEV), f64(1), f64(nws + 1)
        K.coarse_targets(dev(depth), edges, bins, stats, ws)
        stats2, ws2 = f64(1), f64(nws + 1)
        K.coarse_targets(dev(depth), None, None, stats2, ws2)
        keep(f'targets/n{n}', bins=bins, stats=stats, ws=ws, stats_count=stats2, ws_count=ws2)
        base, resid, strct = (dev(10.0 * torch.randn(n, generator=g)) for _ in range(3))
        gt = dev(depth.clamp(min=0.0))
        recon = dev(torch.tensor([0.37]))
        stats, terms, ws = f64(3), f32(4), f64(1024 * 3 + 1)
        K.baseres_stats(base, resid, strct, gt, recon, 1.0, 0.5, 0.01, stats, terms, ws)
        keep(f'baseres/n{n}', stats=stats, terms=terms, ws=ws)
        for teacher in (None, dev(30.0 * torch.rand(n, generator=g))):
            fo, stats, ws = f32(n), f64(4), f64(1024 * 4 + 1)
            K.distill_pix_stats(base, resid, gt, teacher, 30.0, fo, stats, ws)
            keep(f'distill/n{n}/teacher{int(teacher is not None)}', final=fo, stats=stats, ws=ws)

    # ---- adn_l1tv_stats / adn_l1tv_finish
    for B, H, W in L1TV_SHAPES:
        g = torch.Generator().manual_seed(B * H * W)
        pred = dev((torch.rand(B, 1, H, W, generator=g) * 8).round().div(2))
        gt = dev((torch.rand(B, 1, H, W, generator=g) * 8).round().div(2))
        stats, ws = f64(4), f64(K.l1tv_workspace_bytes(B * H * W) // 8 + 1)
        K.l1tv_stats(pred, gt, stats, ws)
        lo, grad = f32(1), torch.full_like(pred, -7.0)
        K.l1tv_finish(pred, gt, stats, 1, 1.0, 0.1, lo, grad)
        keep(f'l1tv/{B}x{H}x{W}', stats=stats, ws=ws, loss=lo, grad=grad)

    np.savez(path, **out)
    print(f'{_lib.LIB_PATH}: {len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes -> {path}')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error('--out FILE.npz or --compare A B')
    dump(args.out)


if __name__ == '__main__':
    main()
