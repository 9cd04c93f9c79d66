"""Float64 torch restatements shared by test_coarse_decode_host.py and test_gpu_coarse_decode.py (no GPU needed here).

Layout of the 41 evaluation sums and of adn_coarse_eval_finish's 39 outputs: include/adn.h.
"""
import math

import torch

N_SUMS, N_OUT, TABLE = 41, 39, 11
FIELDS = ('n_valid', 'top1', 'within1', 'mean_bin_error', 'mean_std', 'mean_entropy', 'mean_confidence', 'std_error_corr',
          'ece')


def decode_ref(x64, centers64):
    """[pixels, nb] float64 logits -> dict of float64 mean, var (= std^2), entropy, confidence and the first-maximum bin."""
    p = torch.softmax(x64, dim=1)
    lp = torch.log_softmax(x64, dim=1)
    mean = (p * centers64).sum(1)
    var = (p * (centers64[None] - mean[:, None]) ** 2).sum(1)
    ent = -(torch.where(p > 0, p * lp, torch.zeros_like(p))).sum(1)
    return dict(mean=mean, var=var, entropy=ent, confidence=p.max(1).values, argmax=torch.argmax(x64, dim=1))


def eval_sums_ref(argmax, bins, confidence, std, entropy, mean, gt):
    """The 41 sums over gt > 0 in float64 from CPU planes (confidence / std / entropy / mean / gt f32, argmax / bins
    integer).  The reliability bin is taken in f32, as the kernel takes it, so bin edges agree."""
    v = gt > 0
    db = (argmax.long() - bins.long()).abs()[v].double()
    c32 = confidence[v]
    c, s, h = c32.double(), std[v].double(), entropy[v].double()
    a = (mean[v].double() - gt[v].double()).abs()
    hit = (db == 0).double()
    sums = torch.zeros(N_SUMS, dtype=torch.float64)
    sums[:TABLE] = torch.stack([torch.tensor(float(v.sum()), dtype=torch.float64), hit.sum(), (db <= 1).double().sum(),
                                db.sum(), s.sum(), h.sum(), c.sum(), a.sum(), (s * s).sum(), (a * a).sum(), (s * a).sum()])
    rb = (c32 * 10).floor().clamp(0, 9).long()
    for b in range(10):
        m = rb == b
        sums[TABLE + 3 * b:TABLE + 3 * b + 3] = torch.stack([m.double().sum(), c[m].sum(), hit[m].sum()])
    return sums


def finish_ref(sums):
    """adn_coarse_eval_finish in float64 torch: sums [41] -> out [39]."""
    s = sums.double()
    out = torch.full((N_OUT,), float('nan'), dtype=torch.float64)
    n = float(s[0])
    out[0] = n
    out[9:] = s[TABLE:]
    if n > 0:
        out[1:7] = s[1:7] / n
        vs, va = float(s[8] - s[4] * s[4] / n), float(s[9] - s[7] * s[7] / n)
        if vs > 0 and va > 0:
            out[7] = float(s[10] - s[4] * s[7] / n) / math.sqrt(vs * va)
        t = s[TABLE:].view(10, 3)
        k = t[:, 0] > 0
        out[8] = (t[k, 0] / n * (t[k, 2] / t[k, 0] - t[k, 1] / t[k, 0]).abs()).sum()
    return out
