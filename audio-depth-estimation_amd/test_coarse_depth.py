"""Evaluation entry point of the coarse-depth family on libadn: test.py for a ``checkpoint_N.pth`` / ``best.pth`` written
by train_coarse_depth (the reference has no evaluation script for this family).

test.py's flags and stats file location, plus train_coarse_depth's --model_type unet|lite|hybrid|dual_reg, --n_bins,
--bin_mode, --sid_alpha, --base_channels and --sparse_method, which resolve
./checkpoints/coarse_<sparse>_<mode><n>_<type>_<exp>/checkpoint_<epoch>.pth when --checkpoint_path is not given
(--experiment_name defaults to the trainer's 'exp1'), and --decode soft|hard.  Bin centres and edges are the
checkpoint's ``bin_centers`` / ``bin_edges`` when present, else ``compute_bins``; divided by max_depth when depth_norm, as
the trainer does.  Like train_coarse_depth, only --synthetic N has a dataset in this build.

Each batch is one ``model.predict_distribution(audio)`` call (one adn_coarse_decode pass behind the class head), one
adn_coarse_targets and one adn_coarse_eval_stats; the 41 evaluation sums are added up on the device and finished once.
Reported, on metres (x max_depth when depth_norm, negatives clipped to 0) with ``compute_errors`` per image:
  * the seven mean metrics of the chosen decode ('soft': the softmax expectation, 'hard': the centre of the first-maximum
    bin); for 'hybrid' of the final depth, with the coarse branch's (the chosen decode) beside them,
  * over the pixels with gt > 0: top-1 and within-one-bin accuracy, mean |bin error|, mean predictive std (metres), mean
    entropy (nats), mean confidence, the Pearson correlation of the std with |mean - gt|, the expected calibration error
    and the 10-bin reliability table (count, mean confidence, accuracy).
'dual_reg' regresses depth directly: it has no class head, hence no distribution, and reports the depth metrics alone.
The stats dict is test.py's plus ``pred_std`` / ``pred_entropy`` / ``pred_confidence`` [N, H, W], ``top1``, ``within1``,
``mean_bin_error``, ``ece``, ``std_error_corr``, ``reliability`` [10, 3] = (count, sum confidence, sum correct) and
``decode``.  ``main()`` returns the dict of scalars.
"""
import os

import torch
from torch.utils.data import DataLoader

from . import kernels as K
from .config_loader import load_config
from .test import build_parser as _test_parser
from .test import resolve_checkpoint
from .utils_criterion import compute_errors_batch
from .utils_loss import MaskedDepthLoss

METRICS = ('abs_rel', 'rmse', 'delta1', 'delta2', 'delta3', 'log10', 'mae')


def build_parser():
    p = _test_parser()
    p.description = 'Test a coarse depth classification model (MI355X): depth metrics, bin accuracy and calibration'
    p.add_argument('--model_type', type=str, default='unet', choices=['unet', 'lite', 'hybrid', 'dual_reg'])
    p.add_argument('--n_bins', type=int, default=128)
    p.add_argument('--bin_mode', type=str, default='linear', choices=['linear', 'log', 'sid'])
    p.add_argument('--sid_alpha', type=float, default=0.6)
    p.add_argument('--base_channels', type=int, default=64)
    p.add_argument('--sparse_method', type=str, default='downup_015')
    p.add_argument('--decode', type=str, default='soft', choices=['soft', 'hard'],
                   help='soft: the softmax expectation; hard: the centre of the first-maximum bin')
    return p


def _report(title, mean7):
    print('\n' + '=' * 50 + f'\n{title}:\n' + '=' * 50)
    for name, v in zip(('abs rel', 'RMSE', 'Delta1', 'Delta2', 'Delta3', 'Log10', 'MAE'), mean7):
        print('{}: {:.3f}'.format(name, v))


def _build_model(args, S):
    from .models.coarse_depth_model import (CoarseDepthLite, CoarseWithOffsetModel, DualRegressionModel,
                                            define_coarse_depth_model)
    kw = dict(input_channels=2, base_channels=args.base_channels, output_size=S)
    if args.model_type == 'dual_reg':
        return DualRegressionModel(**kw)
    if args.model_type == 'hybrid':
        return CoarseWithOffsetModel(n_bins=args.n_bins, **kw)
    if args.model_type == 'lite':
        return CoarseDepthLite(n_bins=args.n_bins, **kw)
    return define_coarse_depth_model(model_type='unet', n_bins=args.n_bins, **kw)


def main(argv=None):
    from .dataloader.utils_dataset import compute_bins
    from .train_dc import SyntheticDepthItems
    args = build_parser().parse_args(argv)
    if args.visualize:
        print('--visualize: PNG panels are not produced by this build (metrics and the stats file are); flag ignored')
    cfg = load_config(dataset_name=args.dataset, mode='test', experiment_name=args.experiment_name or 'default')
    if args.checkpoints is not None:
        cfg.mode.checkpoints = args.checkpoints
    cfg.mode.eval_on = args.eval_on
    if args.batch_size is not None:
        cfg.mode.batch_size = args.batch_size
    if cfg.mode.mode != 'test':
        raise Exception('This script is for test only. Please run train_coarse_depth.py for training')
    if not args.synthetic:
        raise NotImplementedError('the sparse-depth dataset needs file decoding that is not available in this build '
                                  '(preprocessed .npy depth maps + audio files); use --synthetic N')
    if not torch.cuda.is_available():
        raise RuntimeError('test_coarse_depth.py runs on libadn HIP kernels: no HIP device is visible (there is no CPU path)')
    device = torch.device('cuda', 0)
    S, md = cfg.dataset.images_size, float(cfg.dataset.max_depth)
    norm = md if cfg.dataset.depth_norm else 1.0
    eval_set = SyntheticDepthItems(args.synthetic, S, md, 'audio')
    print(f'Eval Dataset of {len(eval_set)} instances')
    loader = DataLoader(eval_set, batch_size=cfg.mode.batch_size, shuffle=False, num_workers=0)

    dual, hybrid = args.model_type == 'dual_reg', args.model_type == 'hybrid'
    model = _build_model(args, S)
    model.compute_dtype = torch.bfloat16 if args.precision == 'bf16' else torch.float32
    if args.checkpoint_path is None:        # the trainer's folder name
        args.experiment_name = (f'coarse_{args.sparse_method}_{args.bin_mode}{args.n_bins}_{args.model_type}_'
                                f'{args.experiment_name or "exp1"}')
    path, exp, epoch = resolve_checkpoint(args, cfg)
    print(f'Loading checkpoint: {path}')
    ck = torch.load(path, map_location='cpu', weights_only=False)
    model.load_state_dict({k[7:] if k.startswith('module.') else k: v for k, v in ck['state_dict'].items()})
    model = model.to(device).eval()
    if ck.get('bin_centers') is not None and ck.get('bin_edges') is not None:
        edges, centers = ck['bin_edges'], ck['bin_centers']
    else:
        edges, centers = compute_bins(args.n_bins, args.bin_mode, None, md, args.sid_alpha)
    if not dual:
        model.set_bin_centers((centers.float() / norm).to(device))
        inner = (edges.float() / norm).reshape(-1)[1:-1].contiguous().to(device)
        f64 = dict(dtype=torch.float64, device=device)
        pix_max = cfg.mode.batch_size * S * S
        ws = torch.empty(max(K.coarse_eval_stats_workspace_bytes(pix_max), K.coarse_targets_workspace_bytes(pix_max)) // 8 + 1, **f64)
        total, part, n_valid = torch.zeros(K.EVAL_SUMS, **f64), torch.zeros(K.EVAL_SUMS, **f64), torch.zeros(1, **f64)
        bins = torch.empty(pix_max, dtype=torch.int32, device=device)

    l1 = MaskedDepthLoss('L1', mask_mode='ne0')
    metres = lambda t: (t * norm).clamp(min=0.0)
    losses, rows, coarse_rows, gts, preds, stds, ents, confs = [], [], [], [], [], [], [], []
    with torch.no_grad():
        for audio, gt in loader:
            audio, gt = audio.to(device), (gt.to(device) / norm).contiguous()
            if dual:
                pred = model(audio)[2]
            else:
                dist = model.predict_distribution(audio)
                decoded = dist.mean if args.decode == 'soft' else dist.hard
                pred = dist.final if hybrid else decoded
                pix = gt.numel()
                K.coarse_targets(gt.view(-1), inner, bins[:pix], n_valid, ws)
                K.coarse_eval_stats(dist.argmax.view(-1), bins[:pix], dist.confidence.view(-1), dist.std.view(-1),
                                    dist.entropy.view(-1), dist.mean.view(-1), gt.view(-1), ws)
                K.coarse_eval_finish(ws, pix, part)
                total += part
                if hybrid:
                    coarse_rows.append(compute_errors_batch(metres(gt), metres(decoded)))
                stds.append(dist.std[:, 0].cpu())
                ents.append(dist.entropy[:, 0].cpu())
                confs.append(dist.confidence[:, 0].cpu())
            losses.append(l1(pred, gt).detach().reshape(1))
            rows.append(compute_errors_batch(metres(gt), metres(pred)))
            gts.append(gt[:, 0].cpu())
            preds.append(pred[:, 0].cpu())
    m = torch.cat(rows)
    mean = m.mean(0).tolist()
    result = dict(zip(METRICS, mean))
    _report('Evaluation Results' + ('' if dual else f' ({args.decode} decode' + (', final depth)' if hybrid else ')')), mean)
    m = m.cpu()
    stats = {'loss': torch.cat(losses).cpu(), 'gt_images': torch.cat(gts), 'pred_imgs': torch.cat(preds)}
    for j, name in enumerate(METRICS):
        stats[name] = m[:, j]
    if hybrid:
        coarse_mean = torch.cat(coarse_rows).mean(0).tolist()
        _report(f'Coarse branch alone ({args.decode} decode)', coarse_mean)
        result.update({'coarse_' + k: v for k, v in zip(METRICS, coarse_mean)})
    if dual:
        print('\ndual_reg regresses depth directly: no class head, hence no per-pixel distribution; bin accuracy and '
              'calibration are not defined for it')
    else:
        out = torch.zeros(K.EVAL_OUT, **f64)
        K.coarse_eval_finish(None, 0, total, out)
        out = out.cpu()
        cls = dict(zip(K.EVAL_FIELDS, out[:len(K.EVAL_FIELDS)].tolist()))
        cls['mean_std'] *= norm
        table = out[len(K.EVAL_FIELDS):].view(10, 3)
        print('\n' + '=' * 50 + '\nPredictive distribution (pixels with gt > 0):\n' + '=' * 50)
        print('Top-1 bin accuracy: {top1:.4f}\nWithin one bin: {within1:.4f}\nMean |bin error|: {mean_bin_error:.3f}\n'
              'Mean std: {mean_std:.4f} m\nMean entropy: {mean_entropy:.4f} nats\nMean confidence: {mean_confidence:.4f}\n'
              'Corr(std, |mean - gt|): {std_error_corr:.4f}\nECE: {ece:.4f}'.format(**cls))
        print('Reliability (confidence bin: pixels, mean confidence, accuracy)')
        for b, (n, sc, sh) in enumerate(table.tolist()):
            if n > 0:
                print('  [{:.1f}, {:.1f}): {:10d}  {:.4f}  {:.4f}'.format(b / 10, (b + 1) / 10, int(n), sc / n, sh / n))
        result.update(cls)
        stats.update(pred_std=torch.cat(stds), pred_entropy=torch.cat(ents), pred_confidence=torch.cat(confs),
                     reliability=table.clone(), decode=args.decode,
                     **{k: cls[k] for k in ('top1', 'within1', 'mean_bin_error', 'ece', 'std_error_corr')})
    split = 'test' if cfg.mode.eval_on == 'test' else 'val'
    out_dir = os.path.join(cfg.mode.stat_dir, cfg.dataset.name, split)
    os.makedirs(out_dir, exist_ok=True)
    out_file = os.path.join(out_dir, f'stats_on_{cfg.dataset.name}_{split}_set_{exp}_epoch_{epoch}.pt')
    torch.save(stats, out_file)
    print(f'Evaluation results saved to: {out_file}')
    return result


if __name__ == '__main__':
    main()
