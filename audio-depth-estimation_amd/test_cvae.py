"""Evaluation entry point of the U-Net cVAE family on libadn: test.py for a ``define_G_cvae`` checkpoint, with K depth
hypotheses per input (the reference has no cVAE evaluation script; its cVAE draws once per forward).

Same flags, checkpoint resolution (--checkpoint_path | --experiment_name + --checkpoints under
./checkpoints/<exp>/checkpoint_<epoch>.pth, ``checkpoint["state_dict"]``) and stats file location as test.py, plus
--latent_dim (as train_cvae.py), --n_samples K and --decode sample|mean.  Each batch is one
``model.sample(audio, K)`` call: the encoder runs once, the decoder once per draw.  Reported, on metres (x max_depth
when depth_norm, negatives clipped to 0) with ``compute_errors`` per image:
  * the seven mean metrics of the mean-of-K prediction (and its L1 test loss on ``gt != 0``),
  * the same seven for the best-of-K prediction: per image the hypothesis with the lowest RMSE against gt, an oracle
    upper bound (it looks at gt),
  * the mean per-pixel std over the valid (gt != 0) pixels.
The stats dict is test.py's (for the mean-of-K prediction) plus ``pred_std`` [N, H, W], ``std_valid`` [N],
``sample_rmse`` [N, K], ``best_of_k_<metric>`` [N] and ``n_samples``.  ``--decode mean`` decodes z = mu: K = 1, std 0.
"""
import os

import torch
from torch.utils.data import DataLoader

from .config_loader import load_config
from .dataloader.utils_dataset import GpuAudioFrontend
from .models.unet_cvae_model import define_G_cvae
from .test import build_parser as _test_parser
from .test import resolve_checkpoint
from .utils_criterion import compute_errors_batch
from .utils_loss import MaskedDepthLoss

METRICS = ('abs_rel', 'rmse', 'delta1', 'delta2', 'delta3', 'log10', 'mae')


def build_parser():
    p = _test_parser()
    p.description = 'Test U-Net cVAE model on Batvision dataset (MI355X): K depth hypotheses per input'
    p.add_argument('--latent_dim', type=int, default=128, help='Latent dimension for VAE bottleneck')
    p.add_argument('--n_samples', type=int, default=8, help='depth hypotheses drawn per input')
    p.add_argument('--decode', type=str, default='sample', choices=['sample', 'mean'],
                   help='sample: K draws from the posterior; mean: the deterministic decode z = mu (K = 1)')
    p.add_argument('--seed', type=int, default=None, help='key of the noise (default: torch.initial_seed() stream)')
    return p


def _report(title, mean7):
    print('\n' + '=' * 50 + f'\n{title}:\n' + '=' * 50)
    for name, v in zip(('abs rel', 'RMSE', 'Delta1', 'Delta2', 'Delta3', 'Log10', 'MAE'), mean7):
        print('{}: {:.3f}'.format(name, v))


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.n_samples < 1:
        raise ValueError(f'--n_samples must be >= 1, got {args.n_samples}')
    if args.visualize:
        print('--visualize: PNG panels are not produced by this build (metrics and the stats file are); flag ignored')
    cfg = load_config(dataset_name=args.dataset, mode='test', experiment_name=args.experiment_name or 'default')
    if args.checkpoints is not None:
        cfg.mode.checkpoints = args.checkpoints
    cfg.mode.eval_on = args.eval_on
    if args.batch_size is not None:
        cfg.mode.batch_size = args.batch_size
    if cfg.mode.mode != 'test':
        raise Exception('This script is for test only. Please run train_cvae.py for training')
    if not torch.cuda.is_available():
        raise RuntimeError('test_cvae.py runs on libadn HIP kernels: no HIP device is visible (there is no CPU path)')
    device = torch.device('cuda', 0)
    S = cfg.dataset.images_size
    if args.synthetic:
        from .train import SyntheticBatvision
        eval_set, fe = SyntheticBatvision(args.synthetic, S, cfg.dataset.max_depth, cfg.dataset.depth_norm), None
    elif cfg.dataset.name == 'batvisionv1':
        from .dataloader.BatvisionV1_Dataset import BatvisionV1Dataset
        ann = cfg.dataset.annotation_file_val if args.eval_on == 'val' else cfg.dataset.annotation_file_test
        eval_set, fe = BatvisionV1Dataset(cfg, ann, frontend='raw'), GpuAudioFrontend('bv1', S)
    else:
        from .dataloader.BatvisionV2_Dataset import BatvisionV2Dataset
        ann = cfg.dataset.annotation_file_val if args.eval_on == 'val' else cfg.dataset.annotation_file_test
        eval_set = BatvisionV2Dataset(cfg, ann, frontend='raw')
        fe = GpuAudioFrontend(GpuAudioFrontend.bv2_mode(cfg.dataset.audio_format, cfg.dataset.max_depth), S)
    print(f'Eval Dataset of {len(eval_set)} instances')
    loader = DataLoader(eval_set, batch_size=cfg.mode.batch_size, shuffle=False, num_workers=cfg.mode.num_threads)

    model = define_G_cvae(cfg, input_nc=2, output_nc=1, ngf=64, netG=cfg.model.generator, norm='batch',
                          use_dropout=False, init_type='normal', init_gain=0.02, gpu_ids=[], latent_dim=args.latent_dim)
    model.compute_dtype = torch.bfloat16 if args.precision == 'bf16' else torch.float32
    path, exp, epoch = resolve_checkpoint(args, cfg)
    print(f'Loading checkpoint: {path}')
    ck = torch.load(path, map_location='cpu')
    model.load_state_dict({k[7:] if k.startswith('module.') else k: v for k, v in ck['state_dict'].items()})
    model = model.to(device).eval()
    l1 = MaskedDepthLoss('L1', mask_mode='ne0')
    sc = float(cfg.dataset.max_depth) if cfg.dataset.depth_norm else 1.0
    losses, rows, best_rows, sample_rmse, std_valid, gts, preds, stds = [], [], [], [], [], [], [], []
    n_drawn = 1
    for i, (audio, gt) in enumerate(loader):
        audio, gt = audio.to(device), gt.to(device)
        if fe is not None:
            audio = fe(audio)
        res = model.sample(audio, args.n_samples, mode=args.decode,
                           seed=None if args.seed is None else args.seed + i)
        n_drawn = res.samples.shape[0]
        gt_m = (gt * sc).clamp(min=0.0)
        losses.append(l1(res.mean, gt).detach().reshape(1))
        rows.append(compute_errors_batch(gt_m, (res.mean * sc).clamp(min=0.0)))
        per_k = torch.stack([compute_errors_batch(gt_m, (s * sc).clamp(min=0.0)) for s in res.samples])   # [K, B, 7]
        best = per_k[:, :, 1].argmin(0)                                                                   # [B]
        best_rows.append(per_k[best, torch.arange(best.numel(), device=device)])
        sample_rmse.append(per_k[:, :, 1].t())
        valid = (gt != 0).float()
        std_valid.append((res.std * sc * valid).flatten(1).sum(1) / valid.flatten(1).sum(1).clamp(min=1.0))
        gts.append(gt[:, 0].cpu())
        preds.append(res.mean[:, 0].cpu())
        stds.append(res.std[:, 0].cpu())
    m, mb = torch.cat(rows), torch.cat(best_rows)
    mean, best_mean = m.mean(0).tolist(), mb.mean(0).tolist()
    std_valid = torch.cat(std_valid)
    _report(f'Evaluation Results (mean of {n_drawn} hypotheses)', mean)
    _report(f'Best of {n_drawn} hypotheses per image (oracle: lowest RMSE against gt)', best_mean)
    print('\nMean per-pixel std over valid pixels: {:.4f} m'.format(std_valid.mean().item()))
    m, mb = m.cpu(), mb.cpu()
    stats = {'loss': torch.cat(losses).cpu(), 'gt_images': torch.cat(gts), 'pred_imgs': torch.cat(preds),
             'pred_std': torch.cat(stds), 'std_valid': std_valid.cpu(), 'sample_rmse': torch.cat(sample_rmse).cpu(),
             'n_samples': n_drawn}
    for j, name in enumerate(METRICS):
        stats[name] = m[:, j]
        stats['best_of_k_' + name] = mb[:, j]
    split = 'test' if cfg.mode.eval_on == 'test' else 'val'
    out_dir = os.path.join(cfg.mode.stat_dir, cfg.dataset.name, split)
    os.makedirs(out_dir, exist_ok=True)
    out_file = os.path.join(out_dir, f'stats_on_{cfg.dataset.name}_{split}_set_{exp}_epoch_{epoch}.pt')
    torch.save(stats, out_file)
    print(f'Evaluation results saved to: {out_file}')
    return mean, best_mean


if __name__ == '__main__':
    main()
