"""Float64 restatement of the U-Net baseline block for every norm setting and for dropout (TEST INFRASTRUCTURE ONLY).

Driven by a ``state_dict`` with the reference's key names (models/unetbaseline_model.py of the reference: the level
nesting :141-148, the per-level Sequential :199-229, the skip concat :235).  What it adds to oracle/unet_oracle.py, which
restates norm='batch' alone: InstanceNorm2d(affine=False) and Identity norms, the conv biases that come with
InstanceNorm2d, and nn.Dropout(0.5) on the ``num_downs - 5`` blocks above the innermost one, fed with given keep masks.
Used where no fixture of the reference can exist: ngf 64, bf16, dropout.

The in-place LeakyReLU of the reference aliases the skip tensor; every concat is consumed through a ReLU, so the effective
skip is ReLU(x) and the non-aliased form below has the same forward and backward (see oracle/unet_oracle.py).
"""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_fixture(name):
    """A fixture of tests/golden/make_golden_unet_norms.py: name.npz + name.p1.npz + ... as one dict of arrays."""
    out = {}
    paths = [os.path.join(GOLDEN, name + '.npz')] + sorted(glob.glob(os.path.join(GOLDEN, name + '.p*.npz')))
    for path in paths:
        with np.load(path) as z:
            for k in z.files:
                out[k] = z[k]
    return out


def level_keys(i, n):
    """Key prefixes of level i (0 = outermost) of an n-level generator: down conv, up conv, down norm, up norm."""
    p = 'model.model' + ('.1.model' if i >= 1 else '') + '.3.model' * max(0, i - 1)
    if i == 0:
        return dict(down=p + '.0', up=p + '.3', nd=None, nu=None)
    if i == n - 1:
        return dict(down=p + '.1', up=p + '.3', nd=None, nu=p + '.4')
    return dict(down=p + '.1', up=p + '.5', nd=p + '.2', nu=p + '.6')


def dropout_levels(n):
    """Levels whose block ends in nn.Dropout(0.5) under use_dropout=True, outermost first."""
    return list(range(max(1, n - 1 - (n - 5)), n - 1))


def normed_bias_keys(n, norm):
    """{bias key: weight key} of the convs whose output goes straight into an InstanceNorm2d: the norm removes a
    per-channel constant, so these gradients are mathematically zero."""
    if norm != 'instance':
        return {}
    out = {}
    for i in range(1, n):
        k = level_keys(i, n)
        if i < n - 1:
            out[k['down'] + '.bias'] = k['down'] + '.weight'
        out[k['up'] + '.bias'] = k['up'] + '.weight'
    return out


def param_keys(sd):
    return [k for k in sd if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]


def _norm(h, sd, key, norm):
    """-> (normalised h, amplification): how many times larger than its own spread the raw conv output is in the group a
    statistic runs over, rms(h) / std(h) >= 1.  A rounding error of h relative to rms(h) shows up that many times larger,
    relative to 1, in xhat = (h - mean) / std (four nearly equal values at the 2 x 2 level of an instance norm)."""
    if norm == 'none':
        return h, None
    dims = (2, 3) if norm == 'instance' else (0, 2, 3)          # per (sample, channel) / batch statistics (train mode)
    mean = h.mean(dims, keepdim=True)
    var = ((h - mean) ** 2).mean(dims, keepdim=True)
    amp = (torch.sqrt((h * h).mean(dims, keepdim=True)) / torch.sqrt(var + EPS)).detach().clamp_min(1.0)
    y = (h - mean) / torch.sqrt(var + EPS)
    if norm == 'batch':
        y = y * sd[key + '.weight'].view(1, -1, 1, 1) + sd[key + '.bias'].view(1, -1, 1, 1)
    return y, amp


def forward(sd, x, n, depth_norm, norm, masks=None, pre_acts=None):
    """Train-mode forward (instance / none: also the eval forward).  masks: keep masks [B, C, H, W] of the dropout
    levels, outermost first, or None for no dropout.  pre_acts: when a list, (tensor, amplification) of every tensor a
    ReLU / LeakyReLU decides on (each conv output after its norm, before the dropout mask: a dropped unit has no decision
    left; amplification: see _norm, None without a norm) is appended, detached."""
    skips, h = [], x
    for i in range(n):
        k = level_keys(i, n)
        skips.append(h)
        a = h if i == 0 else F.leaky_relu(h, 0.2)
        h = F.conv2d(a, sd[k['down'] + '.weight'], sd.get(k['down'] + '.bias'), stride=2, padding=1)
        amp = None
        if k['nd'] is not None:
            h, amp = _norm(h, sd, k['nd'], norm)
        if pre_acts is not None:
            pre_acts.append((h.detach(), amp))
    drops = dict(zip(dropout_levels(n), masks)) if masks is not None else {}
    u = None
    for i in reversed(range(n)):
        k = level_keys(i, n)
        inp = h if i == n - 1 else torch.cat([skips[i + 1], u], 1)
        u = F.conv_transpose2d(F.relu(inp), sd[k['up'] + '.weight'], sd.get(k['up'] + '.bias'), stride=2, padding=1)
        amp = None
        if k['nu'] is not None:
            u, amp = _norm(u, sd, k['nu'], norm)
        if pre_acts is not None and i > 0:
            pre_acts.append((u.detach(), amp))
        if i in drops:
            u = u * drops[i].to(u.dtype) * 2.0                  # nn.Dropout(0.5): keep / (1 - p)
    return torch.sigmoid(u) if depth_norm else F.relu(u)


def combined_loss(pred, gt, l1w, sw, lam, scale):
    """train.py:646-658 of the reference: mask gt != 0, l1w * L1 + sw * SIlog(lam)."""
    valid = gt != 0
    p, g = pred[valid] * scale, gt[valid] * scale
    d = torch.log(torch.clamp(p, min=1e-6)) - torch.log(torch.clamp(g, min=1e-6))
    return l1w * (p - g).abs().mean() + sw * torch.sqrt(torch.clamp((d * d).mean() - lam * d.mean() ** 2, min=0))


def kink_margin(pre_acts):
    """Distance of a forward pass from a kink of the piecewise-linear network: min over every element a ReLU / LeakyReLU
    decides on of |argument| / (RMS of its tensor * amplification of its norm group).  A reference gradient taken with an
    argument within f32 rounding of 0 says nothing about an f32 run (tests/test_gpu_unet.py, RECT_KINK_MARGIN; the
    amplification is what an instance norm over 4 nearly equal values adds to that)."""
    return min(float((a.abs() / (a.pow(2).mean().sqrt() * (1.0 if amp is None else amp))).min()) for a, amp in pre_acts)


def step(sd, audio, gt, n, depth_norm, norm, hyper, masks=None, pre_acts=None):
    """One forward + Combined loss + backward in float64 -> (pred, loss, {key: grad})."""
    l1w, sw, lam, max_depth = hyper
    sd = {k: v.detach().double().clone() for k, v in sd.items() if v.is_floating_point()}
    keys = param_keys(sd)
    for k in keys:
        sd[k].requires_grad_(True)
    pred = forward(sd, audio.double(), n, depth_norm, norm, masks, pre_acts)
    loss = combined_loss(pred, gt.double(), l1w, sw, lam, max_depth if depth_norm else 1.0)
    loss.backward()
    return pred.detach(), loss.item(), {k: sd[k].grad for k in keys}
