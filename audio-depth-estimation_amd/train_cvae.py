"""U-Net cVAE trainer on libadn (mirror of the reference's train_cvae.py entry point).

Same command line and defaults (/root/reference/train_cvae.py:27-143; --kl_weight 1e-4, --latent_dim 128), experiment
naming with the reference's doubled ``_cvae`` suffix (:154 and :222-237), model (:269-281: unet generator of the config,
ngf 64, norm batch, no dropout), loss (:451-473: mask gt > 0, depth loss + kl_weight * kl), clip_grad_norm_(1.0) and the
optimizer (:477-478), validation without the KL term (:512-575) and checkpoints {epoch, state_dict, optimizer}, resumed
from 'state_dict' only (:414-423, :633-648).  The step runs in cvae_engine.CVAETrainer; loaders and validation metrics are
train.py's.  Extra flags as in train.py: --precision {bf16,f32}, --graph, --synthetic N, --epochs.  Single GPU only:
the reference's DataParallel KL averaging is not ported, so a multi-process launch (WORLD_SIZE > 1) is refused.

    python -m audio_depth_estimation_amd.train_cvae --dataset batvisionv2 --batch_size 32 --graph
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import torch

from .config_loader import load_config
from .cvae_engine import CVAETrainer
from .models.unet_cvae_model import define_G_cvae
from .train import make_loaders, validate


def build_parser():
    p = argparse.ArgumentParser(description='Train U-Net+cVAE model on Batvision dataset (MI355X)')
    p.add_argument('--dataset', type=str, default='batvisionv2', choices=['batvisionv1', 'batvisionv2'])
    p.add_argument('--experiment_name', type=str, default='cvae')
    p.add_argument('--checkpoints', type=int, default=None)
    p.add_argument('--batch_size', type=int, default=None)
    p.add_argument('--learning_rate', type=float, default=None)
    p.add_argument('--use_wandb', action='store_true', default=False)
    p.add_argument('--wandb_project', type=str, default='batvision-depth-estimation')
    p.add_argument('--wandb_entity', type=str, default='branden')
    p.add_argument('--wandb_mode', type=str, default='online', choices=['online', 'offline', 'disabled'])
    p.add_argument('--criterion', type=str, default=None, choices=['L1', 'SIlog', 'Combined'])
    p.add_argument('--optimizer', type=str, default=None, choices=['Adam', 'AdamW', 'SGD'])
    p.add_argument('--silog_lambda', type=float, default=None)
    p.add_argument('--l1_weight', type=float, default=None)
    p.add_argument('--silog_weight', type=float, default=None)
    p.add_argument('--audio_format', type=str, default=None, choices=['spectrogram', 'mel_spectrogram', 'waveform'])
    p.add_argument('--validation', type=lambda x: (str(x).lower() == 'true'), default=None)
    p.add_argument('--validation_iter', type=int, default=None)
    p.add_argument('--kl_weight', type=float, default=1e-4, help='Weight for KL divergence term in total loss')
    p.add_argument('--latent_dim', type=int, default=128, help='Latent dimension for VAE bottleneck')
    g = p.add_argument_group('MI355X')
    g.add_argument('--precision', default='bf16', choices=['bf16', 'f32'])
    g.add_argument('--graph', action='store_true', help='replay the step as one hipGraph')
    g.add_argument('--synthetic', type=int, default=0, help='train on N synthetic items (no dataset on disk)')
    g.add_argument('--epochs', type=int, default=None)
    return p


def experiment_name(cfg):
    """cfg.mode.experiment_name already carries the first '_cvae' (:154); the name appends a second one (:222-237)."""
    return (f'{cfg.model.generator}_{cfg.dataset.name}_BS{cfg.mode.batch_size}_Lr{cfg.mode.learning_rate}_'
            f'{cfg.mode.optimizer}_{cfg.mode.experiment_name}_cvae')


def check_world():
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        sys.exit(f'train_cvae: WORLD_SIZE={world}: multi-GPU training of the cVAE family is not supported (the '
                 'DataParallel KL average of the reference is not ported); run it as a single process')


def resolve_loss(cfg, args):
    """Criterion / weights as train_cvae.py:289-339 (no auto-detection: the flags override the config)."""
    for name in ('criterion', 'optimizer', 'silog_lambda', 'l1_weight', 'silog_weight'):
        if getattr(args, name) is not None:
            setattr(cfg.mode, name, getattr(args, name))
    crit = cfg.mode.criterion
    if crit not in ('L1', 'SIlog', 'Combined'):
        raise ValueError(f'Unknown criterion: {crit}. Available: L1, SIlog, Combined')
    lam = getattr(cfg.mode, 'silog_lambda', 0.5)
    if crit == 'Combined':
        return crit, getattr(cfg.mode, 'l1_weight', 0.5), getattr(cfg.mode, 'silog_weight', 0.5), lam
    return crit, 1.0, 0.0, lam


class _DepthOnly(torch.nn.Module):
    """validate() of train.py wants depth = model(x): take it out of the (depth, kl) pair."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model(x)[0]


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_world()
    cfg = load_config(dataset_name=args.dataset, mode='train', experiment_name=args.experiment_name)
    cfg.mode.experiment_name = cfg.mode.experiment_name + '_cvae'
    if args.checkpoints is not None:
        cfg.mode.checkpoints = args.checkpoints
    if args.batch_size is not None:
        cfg.mode.batch_size = args.batch_size
    if args.learning_rate is not None:
        if args.learning_rate <= 0:
            raise ValueError(f'Learning rate must be positive, got {args.learning_rate}')
        if args.learning_rate > 0.1:
            raise ValueError(f'ERROR: Learning rate {args.learning_rate} exceeds safe maximum (0.1).')
        cfg.mode.learning_rate = args.learning_rate
    if args.audio_format is not None:
        if args.dataset == 'batvisionv1' and args.audio_format == 'mel_spectrogram':
            raise ValueError('mel_spectrogram is not supported for batvisionv1. Use \'spectrogram\' or \'waveform\'.')
        cfg.dataset.audio_format = args.audio_format
    if args.validation is not None:
        cfg.mode.validation = args.validation
    if args.validation_iter is not None:
        cfg.mode.validation_iter = args.validation_iter
    if args.epochs is not None:
        cfg.mode.epochs = args.epochs
    if cfg.mode.mode != 'train':
        raise Exception('This script is for training only. Please run test.py for evaluation')
    if cfg.model.name != 'unet_baseline':
        raise Exception('This script is for training on unet model only (cVAE variant)')
    if args.use_wandb:
        print('Warning: --use_wandb is accepted for command-line compatibility; W&B logging is not part of this build')
    if not torch.cuda.is_available():
        raise RuntimeError('train_cvae.py runs on libadn HIP kernels: no HIP device is visible (there is no CPU path)')
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    crit, l1w, sw, lam = resolve_loss(cfg, args)
    exp = experiment_name(cfg)
    train_loader, val_loader, fe, _ = make_loaders(cfg, SimpleNamespace(synthetic=args.synthetic, eval_img=False), 0, 1)

    model = define_G_cvae(cfg, input_nc=2, output_nc=1, ngf=64, netG=cfg.model.generator, norm='batch',
                          use_dropout=False, init_type='normal', init_gain=0.02, gpu_ids=[], latent_dim=args.latent_dim)
    model.compute_dtype = torch.bfloat16 if args.precision == 'bf16' else torch.float32
    model = model.to(device).train()
    start_epoch = 1
    ckpt_dir = os.path.join('./checkpoints', exp)
    if cfg.mode.checkpoints is not None:
        ck = torch.load(os.path.join(ckpt_dir, f'checkpoint_{cfg.mode.checkpoints}.pth'), map_location=device)
        model.load_state_dict({k[7:] if k.startswith('module.') else k: v for k, v in ck['state_dict'].items()})
        start_epoch = ck['epoch'] + 1
    max_depth = cfg.dataset.max_depth if cfg.dataset.max_depth else 30.0
    trainer = CVAETrainer(model.engine(), crit, l1w, sw, lam, max_depth=max_depth, optimizer=cfg.mode.optimizer,
                          lr=cfg.mode.learning_rate, kl_weight=args.kl_weight, clip_norm=1.0)
    if args.graph:
        trainer.enable_graph(after_steps=3)

    for epoch in range(start_epoch, cfg.mode.epochs + 1):
        t0 = time.time()
        losses = []
        for audio, gt in train_loader:
            audio, gt = audio.to(device, non_blocking=True), gt.to(device, non_blocking=True)
            if fe is not None:
                audio = fe(audio)
            loss, _ = trainer.step(audio, gt)
            losses.append(loss.detach().clone())
        if losses:
            print(f'Epoch {epoch}: Train Loss: {torch.stack(losses).mean().item():.6f}, Time: {time.time() - t0:.1f}s, '
                  f'KL weight: {args.kl_weight}')
        if cfg.mode.validation and epoch % cfg.mode.validation_iter == 0:
            (abs_rel, rmse, d1, d2, d3, log10, mae), val_loss = validate(_DepthOnly(model), val_loader, fe, cfg, device,
                                                                         (crit, l1w, sw, lam))
            model.train()
            print(f'Val - Loss: {val_loss:.6f}, RMSE: {rmse:.3f}, ABS_REL: {abs_rel:.3f}, Log10: {log10:.3f}, '
                  f'Delta1: {d1:.3f}, Delta2: {d2:.3f}, Delta3: {d3:.3f}')
        if epoch % cfg.mode.saving_checkpoints == 0:
            os.makedirs(ckpt_dir, exist_ok=True)
            torch.save({'epoch': epoch, 'state_dict': model.state_dict(), 'optimizer': trainer.state_dict()},
                       os.path.join(ckpt_dir, f'checkpoint_{epoch}.pth'))
    return model


if __name__ == '__main__':
    main()
