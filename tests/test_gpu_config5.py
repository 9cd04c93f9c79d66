"""BASELINE.json configs[4]: RGBDepthNet (base 64, bilinear) at 512 x 512 (models/rgb_depth_model.py:148-218 of the
reference run with output_size 512).

  * f32 against the float64 CPU oracle at B = 1 (one image is 0.33 TFLOP forward; the oracle needs about a minute):
    prediction relative L1 <= 1e-5, every parameter gradient relative L2 <= 2e-2 and cosine >= 0.9999 (the gradient bound
    is the price of single ReLU flips at |pre-activation| ~ 1e-6, see test_gpu_dcnet.py), BatchNorm running statistics;
  * bf16 at B = 8 (the pixel count of configs[2]'s B = 32 at 256 x 256, every conv on the patch-staged MFMA kernel with
    its 512-wide tile grid): backward linearity, run-to-run determinism of two fused DepthLoss + AdamW steps, eval-mode
    batch independence;
  * the configuration's own precision, compute_dtype = torch.float8_e4m3fn (block-scaled MX e4m3 forward and
    input-gradient GEMMs of the 17 eligible 3 x 3 convs, csrc/mx8.hip; bf16 storage, BatchNorm and weight gradients):
    against the float64 oracle on the same weights (stated, measured tolerances below), against the bf16 engine, run-to-run
    determinism of fused steps at B = 8, and a short fused training run whose loss must fall like the bf16 run's.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
S = 512


def _rgb(dtype):
    from audio_depth_estimation_amd.models.rgb_depth_model import RGBDepthNet
    torch.manual_seed(0)
    m = RGBDepthNet(base_channels=64, bilinear=True, output_size=S, max_depth=30.0)
    m.compute_dtype = dtype
    return m.to(DEV)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-30))


def test_rgb512_f32_against_oracle():
    from oracle import dcnet_oracle
    model = _rgb(torch.float32)
    with torch.no_grad():
        model.outc.bias.fill_(2.0)
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone())
          for k, v in model.state_dict().items()}
    pkeys = [k for k, v in sd.items() if v.is_floating_point() and 'running_' not in k]
    for k in pkeys:
        sd[k].requires_grad_(True)
    g = torch.Generator().manual_seed(99)
    image = torch.rand(1, 3, S, S, generator=g)
    gt = 30 * torch.rand(1, 1, S, S, generator=g)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    pred_ref, stats_ref = dcnet_oracle.rgb_forward(sd, image.double(), 30.0, training=True)
    pred_ref.retain_grad()
    dcnet_oracle.depth_loss(pred_ref, gt.double()).backward()
    model.train()
    eng = model.engine()
    pred = eng.forward(image.to(DEV), True).clone()
    assert pred.shape == (1, 1, S, S)
    rl1 = float((pred.cpu().double() - pred_ref.detach()).abs().sum() / pred_ref.detach().abs().sum())
    assert rl1 <= 1e-5, rl1
    eng.backward(pred_ref.grad.float().to(DEV))
    for k, prm in model.named_parameters():
        got = eng.grad_view(prm).detach().double().cpu().reshape(-1)
        ref = sd[k].grad.reshape(-1)
        cos = float(torch.dot(got, ref) / (got.norm() * ref.norm() + 1e-30))
        rl2 = float((got - ref).norm() / (ref.norm() + 1e-30))
        assert rl2 <= 2e-2 and cos >= 0.9999, (k, rl2, cos)
    for k, v in stats_ref.items():
        got = model.state_dict()[k].cpu().double()
        assert float((got - v).abs().max()) <= 1e-5 * float(v.abs().max()) + 1e-6, k


def test_rgb512_bf16_properties_at_batch_8():
    from audio_depth_estimation_amd.engine import FusedTrainer
    B = 8
    g = torch.Generator().manual_seed(77)
    x = torch.rand(B, 3, S, S, generator=g).to(DEV)
    gt = (30 * torch.rand(B, 1, S, S, generator=g)).to(DEV)
    model = _rgb(torch.bfloat16).train()
    eng = model.engine()
    pred = eng.forward(x, True)
    assert pred.shape == (B, 1, S, S) and bool(torch.isfinite(pred).all())
    u = torch.randn(pred.shape, generator=g).to(DEV) / pred.numel()
    v = torch.randn(pred.shape, generator=g).to(DEV) / pred.numel()
    grads = []
    for up in (u, v, 1.3 * u + 0.6 * v):
        eng.backward(up)
        grads.append(eng.flat_g.clone())
    assert _rel(grads[2], 1.3 * grads[0] + 0.6 * grads[1]) <= 3e-2       # bf16 rounding of every stored dz
    del grads
    # eval mode: image 3 of the batch equals the same image run alone (different tile grids of the same layers)
    model.eval()
    with torch.no_grad():
        full = model(x).clone()
        one = model(x[3:4]).clone()
    assert float((full[3:4] - one).abs().max()) <= 2e-2 * 30.0
    del model, eng
    finals = []
    for _ in range(2):
        m = _rgb(torch.bfloat16).train()
        tr = FusedTrainer(m.engine(), 'DepthLoss', 1.0, 0.1, optimizer='AdamW', lr=1e-3, weight_decay=0.01, clip_norm=None)
        for _ in range(2):
            loss, _ = tr.step(x, gt)
        assert bool(torch.isfinite(loss))
        finals.append((float(loss), m.engine().flat_p.clone()))
        del m, tr
    assert finals[0][0] == finals[1][0] and torch.equal(finals[0][1], finals[1][1])


def test_rgb512_mxfp8_every_layer_in_situ_and_end_to_end():
    """Stated, measured tolerance of the fp8 path at config 5's shape (B = 1, 512 x 512, freshly initialised net).
    (1) Every one of the 17 fp8 convolutions INSIDE the running network: its stored output z against the float64
        convolution of the very bf16 activations it consumed (post-ReLU feature maps, the real data distribution) and the
        f32 master weights: relative L2 <= 5e-2 (measured 3.6e-2 .. 3.9e-2 on these one-sided post-ReLU inputs, 2.6e-2 .. 2.9e-2
        for Gaussian operands in test_gpu_mx8.py; e4m3 carries 3 mantissa bits on both operands).
        This also proves the wiring: every fp8 copy handed to a conv belongs to the right tensor of the right pass.
    (2) End to end against the float64 oracle: recorded, not a tight bound -- an untrained BatchNorm + ReLU stack amplifies
        any perturbation ~1.7x per conv stage (measured in test_gpu_dcnet.py), so 18 stages turn the 3e-2 per-layer noise
        into O(0.3) at the output (bf16's 4e-3 per layer becomes 5e-2).  What has to hold end to end is the training
        behaviour: test_rgb512_mxfp8_training_determinism_and_descent."""
    from oracle import dcnet_oracle
    model = _rgb(torch.float8_e4m3fn)
    with torch.no_grad():
        model.outc.bias.fill_(2.0)
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone())
          for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(99)
    image = torch.rand(1, 3, S, S, generator=g)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    model.train()
    eng = model.engine()
    assert eng.mx8 and eng.dtype == torch.bfloat16
    pred = eng.forward(image.to(DEV), True).clone()
    rows = []
    for op in eng.ops:
        if not getattr(op, 'mx8', False):
            continue
        x = torch.cat([s_.data for s_ in op.srcs], dim=-1).double().cpu().permute(0, 3, 1, 2)
        w = op.conv.weight.detach().double().cpu()
        ref = torch.nn.functional.conv2d(x, w, padding=1).permute(0, 2, 3, 1)
        got = op.out.z.double().cpu()
        rows.append((op.out.name, tuple(w.shape[:2]), float((got - ref).norm() / ref.norm())))
    print('fp8 conv layers in situ (rel L2 of z):', [(n, c, round(e, 4)) for n, c, e in rows])
    assert len(rows) == 17                               # every 3 x 3 conv but the thin first one
    assert max(e for _, _, e in rows) <= 5e-2, rows
    with torch.no_grad():
        pred_ref, _ = dcnet_oracle.rgb_forward(sd, image.double(), 30.0, training=True)
    rl1 = float((pred.cpu().double() - pred_ref).abs().sum() / pred_ref.abs().sum())
    print('fp8 end-to-end prediction rel-L1 vs the f64 oracle (fresh random net):', rl1)
    assert bool(torch.isfinite(pred).all()) and rl1 <= 0.5


def test_rgb512_mxfp8_training_determinism_and_descent():
    from audio_depth_estimation_amd.engine import FusedTrainer
    B = 8
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 3, S, S, generator=g).to(DEV)
    # a learnable target: a smooth function of the image
    gt = (30 * torch.nn.functional.avg_pool2d(x.mean(1, keepdim=True), 9, 1, 4)).contiguous()
    runs = {}
    for name, dt, reps in (('mxfp8', torch.float8_e4m3fn, 2), ('bf16', torch.bfloat16, 1)):
        for r in range(reps):
            m = _rgb(dt).train()
            tr = FusedTrainer(m.engine(), 'DepthLoss', 1.0, 0.1, optimizer='AdamW', lr=1e-3, weight_decay=0.01, clip_norm=None)
            losses = []
            for _ in range(12):
                loss, _ = tr.step(x, gt)
                losses.append(float(loss))
            runs[(name, r)] = (losses, m.engine().flat_p.clone())
            del m, tr
    a, b = runs[('mxfp8', 0)], runs[('mxfp8', 1)]
    assert a[0] == b[0] and torch.equal(a[1], b[1])                               # bit-identical fp8 runs
    l8, l16 = a[0], runs[('bf16', 0)][0]
    print('loss mxfp8', [round(v, 4) for v in l8], 'bf16', [round(v, 4) for v in l16])
    assert all(np.isfinite(l8)) and l8[-1] < 0.7 * l8[0]                          # it trains
    assert abs(l8[-1] - l16[-1]) <= 0.15 * l16[0]                                 # and tracks the bf16 run


@pytest.mark.parametrize('kind', ['binaural', 'adabins', 'baseres'])
def test_mxfp8_on_the_other_doubleconv_nets(kind):
    """compute_dtype = float8_e4m3fn on the sibling families (64 x 64, B = 2): the engine picks fp8 for the eligible 3 x 3
    convs (none of the stacked [left; right] encoder convs of the binaural net: their operands are halves of one buffer),
    three fused steps stay finite and the loss tracks the bf16 run of the same seed within 5 %."""
    from audio_depth_estimation_amd.engine import FusedTrainer
    g = torch.Generator().manual_seed(11)
    Sx, B = 64, 2
    audio, rgb = torch.rand(B, 2, Sx, Sx, generator=g).to(DEV), torch.rand(B, 3, Sx, Sx, generator=g).to(DEV)
    gt = (30 * torch.rand(B, 1, Sx, Sx, generator=g)).to(DEV)
    gt[gt < 3] = 0
    losses, n_mx = {}, 0
    for name, dt in (('bf16', torch.bfloat16), ('mxfp8', torch.float8_e4m3fn)):
        torch.manual_seed(0)
        if kind == 'binaural':
            from audio_depth_estimation_amd.models.binaural_attention_model import BinauralAttentionDepthNet
            m = BinauralAttentionDepthNet(64, True, Sx, 30.0)
            m.compute_dtype = dt
            m = m.to(DEV).train()
            tr = FusedTrainer(m.engine(), 'L1', optimizer='AdamW', lr=1e-4, weight_decay=0.01, clip_norm=None, mask_mode='gt0')
            step = lambda: tr.step(audio, gt)[0]
        elif kind == 'adabins':
            from audio_depth_estimation_amd.adabins_engine import AdaBinsTrainer
            from audio_depth_estimation_amd.models.adabins_distillation_model import AdaBinsDistillationModel
            m = AdaBinsDistillationModel(128, 64, Sx, 30.0)
            m.compute_dtype = dt
            m = m.to(DEV).train()
            tr = AdaBinsTrainer(m.engine(), lr=1e-4)
            step = lambda: tr.step(audio, rgb, gt)[0]
        else:
            from audio_depth_estimation_amd.base_residual_engine import BaseResidualTrainer
            from audio_depth_estimation_amd.models.base_residual_model import BaseResidualDepthNet
            m = BaseResidualDepthNet(2, 64, True, Sx, 30.0)
            m.compute_dtype = dt
            m = m.to(DEV).train()
            tr = BaseResidualTrainer(m.engine(), use_silog=True, lr=1e-4)
            step = lambda: tr.step(audio, gt)[0]
        ls = [float(step()) for _ in range(3)]
        assert all(np.isfinite(ls)), (name, ls)
        losses[name] = ls
        if name == 'mxfp8':
            eng = m.engine()
            assert eng.mx8 and eng.dtype == torch.bfloat16
            n_mx = sum(1 for op in eng.ops if getattr(op, 'mx8', False))
        del m, tr
    print(kind, 'fp8 convs:', n_mx, losses)
    assert n_mx >= 4
    assert abs(losses['mxfp8'][-1] - losses['bf16'][-1]) <= 0.05 * abs(losses['bf16'][-1])


def _sibling(kind, dtype, Sx):
    """(model, fused trainer step(audio, rgb, gt), eval forwards(audio, rgb) -> list of output maps) of a sibling family, built as
    in test_mxfp8_on_the_other_doubleconv_nets."""
    torch.manual_seed(0)
    if kind == 'adabins':
        from audio_depth_estimation_amd.adabins_engine import AdaBinsTrainer
        from audio_depth_estimation_amd.models.adabins_distillation_model import AdaBinsDistillationModel
        m = AdaBinsDistillationModel(128, 64, Sx, 30.0)
        m.compute_dtype = dtype
        m = m.to(DEV)
        step = lambda audio, rgb, gt: AdaBinsTrainer(m.engine(), lr=1e-4).step(audio, rgb, gt)
        keys = ('bin_centers', 'bin_widths', 'bin_logits', 'base_depth', 'residual', 'final_depth')

        def maps(audio, rgb):
            res = []
            for o in (m.forward_rgb(rgb), m.forward_audio(audio)):
                res += [o[k] for k in keys] + list(o['features'].values())
            return res
        return m, step, maps
    from audio_depth_estimation_amd.base_residual_engine import BaseResidualTrainer
    from audio_depth_estimation_amd.models.base_residual_model import BaseResidualDepthNet
    m = BaseResidualDepthNet(2, 64, True, Sx, 30.0)
    m.compute_dtype = dtype
    m = m.to(DEV)
    step = lambda audio, rgb, gt: BaseResidualTrainer(m.engine(), use_silog=True, lr=1e-4).step(audio, gt)
    return m, step, (lambda audio, rgb: list(m(audio)))


@pytest.mark.parametrize('first', ['eval', 'train_step'])
@pytest.mark.parametrize('kind', ['adabins', 'baseres'])
def test_mxfp8_eval_reads_the_current_batch(kind, first):
    """An eval forward under compute_dtype = float8_e4m3fn reads THIS batch: in eval mode no producer writes the fp8 operand
    copy of its output, so the consuming conv quantises it itself, once per forward pass (DCEngine.q8_of keyed by
    fwd_serial).  m1 sees batch a first (an eval forward, or one fused training step) and then evaluates batch b; m2, a fresh
    model with m1's state, evaluates b as its first forward.  Same kernels, same operands, same shape: every returned map is
    bit-equal.  The eval path's own run-to-run spread is measured first, on m2 (0 on every map, all four cases); a map with
    a non-zero spread would be held to twice that spread instead.  Before fwd_serial advanced in these two families'
    forwards, m1's fp8 convs kept reading batch a."""
    Sx, B = 64, 2
    g = torch.Generator().manual_seed(23)
    xa = [torch.rand(B, c, Sx, Sx, generator=g).to(DEV) for c in (2, 3)]
    xb = [torch.rand(B, c, Sx, Sx, generator=g).to(DEV) for c in (2, 3)]
    gt = (30 * torch.rand(B, 1, Sx, Sx, generator=g)).to(DEV)
    gt[gt < 3] = 0
    dt = torch.float8_e4m3fn
    m1, step1, maps1 = _sibling(kind, dt, Sx)
    if first == 'eval':
        m1.eval()
        with torch.no_grad():
            maps1(*xa)
    else:
        m1.train()
        assert bool(torch.isfinite(step1(*xa, gt)[0]))
        m1.eval()
    with torch.no_grad():
        got = [t.clone() for t in maps1(*xb)]
    assert sum(1 for op in m1.engine().ops if getattr(op, 'mx8', False)) >= 4
    m2, _, maps2 = _sibling(kind, dt, Sx)
    m2.load_state_dict(m1.state_dict())
    m2.eval()
    with torch.no_grad():
        want = [t.clone() for t in maps2(*xb)]
        again = [t.clone() for t in maps2(*xb)]
    dist = lambda p, q: float((p.float() - q.float()).abs().max())
    spread = [dist(w, r) for w, r in zip(want, again)]          # run-to-run spread of the eval forward itself: measured 0
    errs = [dist(p, w) for p, w in zip(got, want)]
    print(kind, first, 'run-to-run max |diff| per map:', spread)
    print(kind, first, 'max |m1(xb) - fresh model(xb)| per map:', [f'{e:.3e}' for e in errs])
    assert len(got) == len(want) == len(again)
    for p, w, s, e in zip(got, want, spread, errs):
        assert torch.equal(p, w) if s == 0.0 else e <= 2 * s, (errs, spread)
