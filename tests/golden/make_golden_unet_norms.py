"""Golden vectors of the U-Net baseline with norm='instance' and norm='none', by IMPORTING THE REFERENCE on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_unet_norms.py

Same layout as make_golden.py's unet_case (sd0, inputs, eval / train predictions, the Combined loss, d loss / d pred, every
gradient, the clipped norm, sd1 after one AdamW step, the eval prediction at sd1); only numbers travel.  A fixture is
written as name.npz, name.p1.npz, ... so that no file reaches 1 MiB.  The last bias is shifted to 1.0 so that the
prediction is not all zeros (see make_golden.py).

Reference entry points exercised (file:line in the reference):
  models/unetbaseline_model.py:59   get_norm_layer ('instance': InstanceNorm2d(affine=False, track_running_stats=False);
                                    'none': Identity)
  models/unetbaseline_model.py:84   define_G
  train.py:646-691                  loss assembly, clip_grad_norm_(1.0), AdamW(lr) step
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, '/root/reference')
from models.unetbaseline_model import define_G          # noqa: E402
from utils_loss import SIlogLoss                         # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
L1_W, SILOG_W, SILOG_LAMBDA = 0.237, 0.637, 0.869       # conf/mode/train.yaml:12-14


def synth_batch(B, C, S, seed, max_depth, depth_norm):
    g = torch.Generator().manual_seed(seed)
    audio = torch.rand(B, C, S, S, generator=g)
    gt = max_depth * torch.rand(B, 1, S, S, generator=g)
    gt[gt < 0.1 * max_depth] = 0.0
    if depth_norm:
        gt = gt / max_depth
    return audio, gt


PART_BYTES = 900 * 1024      # every committed file stays below 1 MiB: a fixture is name.npz + name.p1.npz + ...


def save_parts(name, arrays):
    """Arrays in insertion order, packed greedily into parts of at most PART_BYTES raw bytes (tests/unet_norm_oracle.py:
    load_fixture puts them together again)."""
    for old in os.listdir(HERE):
        if old == name + '.npz' or (old.startswith(name + '.p') and old.endswith('.npz')):
            os.remove(os.path.join(HERE, old))
    parts, cur, used = [], {}, 0
    for k, v in arrays.items():
        n = np.asarray(v).nbytes + 256
        if cur and used + n > PART_BYTES:
            parts.append(cur)
            cur, used = {}, 0
        cur[k] = v
        used += n
    parts.append(cur)
    sizes = []
    for i, part in enumerate(parts):
        path = os.path.join(HERE, name + ('.npz' if i == 0 else f'.p{i}.npz'))
        np.savez_compressed(path, **part)
        sizes.append(os.path.getsize(path))
        assert sizes[-1] < 1 << 20, path
    return sizes


def unet_case(name, netG, norm, ngf, S, depth_norm, max_depth, B, lr=0.002, wscale=1.0):
    cfg = SimpleNamespace(dataset=SimpleNamespace(depth_norm=depth_norm, max_depth=max_depth))
    torch.manual_seed(0)
    model = define_G(cfg, input_nc=2, output_nc=1, ngf=ngf, netG=netG, norm=norm, use_dropout=False,
                     init_type='normal', init_gain=0.02, gpu_ids=[])
    with torch.no_grad():
        model.model.model[3].bias.fill_(1.0)
    out = {}
    for k, v in model.state_dict().items():
        out['sd0/' + k] = v.detach().clone().numpy()
    audio, gt = synth_batch(B, 2, S, 1234, max_depth, depth_norm)
    out['audio'], out['gt'] = audio.numpy(), gt.numpy()
    model.eval()
    with torch.no_grad():
        out['pred_eval'] = model(audio).numpy()
    model.train()
    optimizer = torch.optim.AdamW(model.parameters(), lr=lr)
    optimizer.zero_grad()
    pred = model(audio)
    valid = gt != 0.0
    scale = max_depth if depth_norm else 1.0
    p, g = pred[valid] * scale, gt[valid] * scale
    loss = wscale * L1_W * torch.nn.L1Loss()(p, g) + wscale * SILOG_W * SIlogLoss(lambda_scale=SILOG_LAMBDA)(p, g)
    pred.retain_grad()
    loss.backward()
    out['pred_grad'] = pred.grad.detach().clone().numpy()
    out['pred_train'] = pred.detach().numpy()
    out['loss'] = np.float64(loss.item())
    for k, prm in model.named_parameters():
        out['grad/' + k] = prm.grad.detach().clone().numpy()
    total_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    out['grad_norm'] = np.float64(total_norm.item())
    optimizer.step()
    for k, v in model.state_dict().items():
        out['sd1/' + k] = v.detach().clone().numpy()
    model.eval()
    with torch.no_grad():
        out['pred_eval_sd1'] = model(audio).numpy()
    out['meta'] = np.array([ngf, S, int(depth_norm), B], dtype=np.int64)
    out['hyper'] = np.array([lr, max_depth, wscale * L1_W, wscale * SILOG_W, SILOG_LAMBDA], dtype=np.float64)
    sizes = save_parts(name, out)
    print(name, 'keys', len(model.state_dict()), 'loss', loss.item(), 'grad_norm', total_norm.item(), 'bytes', sizes)


if __name__ == '__main__':
    torch.set_num_threads(8)
    unet_case('unet128_ngf4_instance', 'unet_128', 'instance', 4, 128, True, 12.0, B=2)
    unet_case('unet256_ngf4_instance_b1', 'unet_256', 'instance', 4, 256, False, 30.0, B=1, wscale=10.0)
    unet_case('unet128_ngf4_none', 'unet_128', 'none', 4, 128, False, 30.0, B=2, wscale=10.0)
