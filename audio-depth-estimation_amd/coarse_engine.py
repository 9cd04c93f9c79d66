"""Coarse depth classification model on libadn: the DoubleConv U-Net tape, the 1x1 class head and the fused loss step.

Replaces /root/reference/models/coarse_depth_model.py:134-189 and the training step of
/root/reference/train_coarse_depth.py:446-463 with CoarseDepthLoss (:391-468).  The encoder / decoder are the ops of
dc_engine.py, the class head is adabins_engine.ConvLinear, and everything behind the logits is ONE pass of
adn_coarse_loss (csrc/coarse.hip): softmax expectation, classification loss (soft CE / focal / CE), masked L1 of the
expectation and the gradient of their weighted sum, written once in the logits' dtype.  The logits [B,H,W,n_bins] stay
NHWC in the compute dtype and are only expanded to f32 NCHW when a caller asks for them (forward()).
CoarseLiteEngine runs CoarseDepthLite (:199-287) through the same engine: only the tape in front of the logits differs
(the ``_tape`` hook).
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import kernels as K
from .adabins_engine import ConvLinear
from .dc_engine import Act, ConvK4BNAct, ConvS2BNLeaky, ConvT2BNReLU, DCEngine, decoder_ops, run_engine, unet_encoder_ops
from .trainer import OptimTail


class ClassLogits:
    """Engine mixin: a class head (ConvLinear ``class_op``) onto an NHWC ``logits`` record in the compute dtype whose
    softmax expectation over ``centers`` (the module's ``bin_centers``) is a depth map."""
    head_attr = 'outc'               # the model's attribute that holds the class-head conv
    fused_trainer = 'CoarseDepthTrainer'

    def check_bins(self):
        nb = self.module.n_bins
        if not 2 <= nb <= 512:
            raise NotImplementedError(f'{self.model_name}: n_bins={nb} is outside the range [2, 512] of adn_coarse_loss')

    def class_head(self, src):
        """-> the class-head op over ``src``; sets ``logits`` and ``class_op``."""
        self.logits = Act('logits', self.module.n_bins, src.H, src.W)
        self.class_op = ConvLinear(src, getattr(self.module, self.head_attr), self.logits)
        return self.class_op

    def logits_workspace_bytes(self, B, H, W):
        nb, pix = self.module.n_bins, B * H * W
        ws = max(1 << 16, K.coarse_loss_workspace_bytes(pix), K.coarse_targets_workspace_bytes(pix))
        return max(ws, K.bins_bwd_workspace_bytes(B, H * W, nb)) if nb <= 256 else ws

    def alloc_centers(self):
        self.centers = torch.empty(self.module.n_bins, dtype=torch.float32, device=self.dev)
        self._bridge = None
        self._planes = None

    def load_centers(self):
        self.centers.copy_(self.module.bin_centers.detach().to(torch.float32).reshape(-1))

    def bridge_scratch(self):
        """Per-shape buffers of the autograd bridge: centres per sample [B,nb] (what adn_bins_bwd takes), its unused
        d centres output, and the NHWC f32 copy of the upstream logits gradient."""
        if self._bridge is None:
            lg = self.logits
            f32 = dict(dtype=torch.float32, device=self.dev)
            self._bridge = (torch.empty(self.B, lg.C, **f32), torch.empty(self.B, lg.C, **f32),
                            torch.empty(self.B, lg.H, lg.W, lg.C, **f32))
        return self._bridge

    def decode_head(self, mean):
        """ONE adn_coarse_decode pass over ``logits``: the expectation into ``mean`` (the engine's depth plane, the bits
        the forward-only adn_coarse_loss writes there) and the rest of the distribution into the per-shape planes."""
        if self._planes is None:
            lg = self.logits
            plane = lambda dt: torch.empty(self.B, 1, lg.H, lg.W, dtype=dt, device=self.dev)
            self._planes = {k: plane(torch.float32) for k in ('hard', 'std', 'entropy', 'confidence')}
            self._planes['argmax'] = plane(torch.int32)
        pl = self._planes
        pl['mean'] = mean
        K.coarse_decode(self.logits.data, self.module.n_bins, self.centers,
                        **{k: pl[k].view(-1) for k in CoarseDistribution._fields})

    def decode(self, x, training=False):
        """The tape up to the logits, then the distribution read out instead of collapsed: -> dict of the engine's own
        planes [B,1,H,W] (mean, hard, std, entropy, confidence f32, argmax int32; the hybrid engine adds offset, final)."""
        self.forward_net(x, training, decode=True)
        return self._planes

    def logits_nchw(self):
        lg = self.logits
        out = torch.empty(self.B, lg.C, lg.H, lg.W, dtype=torch.float32, device=self.dev)
        K.nhwc_to_nchw(lg.data, out)
        return out

    def route_logits_grad(self, g_logits, g_depth, depth):
        """logits.grad of the autograd bridge = g_logits (NCHW -> NHWC) + the soft-bin backward of ``g_depth`` (f32, the
        upstream gradient of the expectation ``depth``); either may be None."""
        lg, nb = self.logits, self.module.n_bins
        if g_depth is not None:
            if nb > 256:
                raise NotImplementedError('autograd through the soft depth needs n_bins <= 256 (adn_bins_bwd); use '
                                          f'{self.fused_trainer}')
            centers_b, dcent, _ = self.bridge_scratch()
            centers_b.copy_(self.centers.view(1, nb).expand_as(centers_b))
            K.bins_bwd(lg.data, centers_b, depth.view(-1), g_depth.view(-1), None, lg.grad, dcent, self.workspace)
        if g_logits is not None:
            glog = self.bridge_scratch()[2]
            K.nchw_to_nhwc(g_logits.contiguous().float(), glog)
            K.bcast_add(lg.grad.view(-1, 1, 1, nb), glog.view(-1, nb), 1.0, accumulate=g_depth is not None)
        if g_depth is None and g_logits is None:
            lg.grad.zero_()

    def backward_class_head(self):
        """From ``logits.grad``: the class head's backward; its parameters' gradients are final."""
        conv = self.class_op.conv
        self.class_op.bwd(self)
        self._mark(conv.bias)
        self._ready(conv.weight)


class CoarseDepthEngine(ClassLogits, DCEngine):
    model_name = 'CoarseDepthUNet'

    def __init__(self, module, compute_dtype=torch.bfloat16):
        super().__init__(module, None, compute_dtype, self.model_name)

    def _tape(self, B, Cin, H, W):
        m = self.module
        inp = self.thin_input('x', Cin, H, W)
        self.inputs = [(inp, 0, Cin)]
        ops, feats = unet_encoder_ops(m, inp, H, W)
        o, d = decoder_ops((m.up1, m.up2, m.up3, m.up4), feats, '')
        return ops + o + [self.class_head(d)]

    def check_input(self, shape):
        """The shape refusals of forward, on the host (no device work)."""
        B, Cin, H, W = shape
        m = self.module
        if Cin != m.input_channels:
            raise RuntimeError(f'expected input[{B}, {Cin}, {H}, {W}] to have {m.input_channels} channels, but got {Cin} '
                               'channels instead')
        if W != m.output_size:
            raise NotImplementedError(f'{self.model_name}: input width {W} != output_size {m.output_size}: the bilinear '
                                      f'resize of the {m.n_bins}-channel logits (coarse_depth_model.py:159-161) is not '
                                      'implemented')
        self.check_bins()

    def _workspace_floor(self, B, Cin, H, W):
        return self.logits_workspace_bytes(B, H, W)

    def _alloc_outputs(self, B, Cin, H, W):
        self.depth = torch.empty(B, 1, H, W, dtype=torch.float32, device=self.dev)
        self.alloc_centers()

    def forward_net(self, x, training, argmax=None, head=True, decode=False):
        """-> (logits NHWC in the compute dtype, depth f32 [B,1,H,W]); both are the engine's own buffers.  ``head=False``
        (the fused trainer): the softmax expectation is left to the caller's own adn_coarse_loss pass, which writes
        ``depth`` together with the loss and the gradient, so the logits are read once per step.  ``decode=True``:
        ``depth`` comes from the adn_coarse_decode pass that also fills the distribution planes."""
        self._begin_forward(x)
        self._forward_ops(self.ops, training)
        self.load_centers()
        if decode:
            self.decode_head(self.depth)
        elif head:
            K.coarse_loss(self.logits.data, self.module.n_bins, self.centers, self.depth, argmax=argmax)
        return self.logits.data, self.depth

    def run(self, x, training):
        self.forward_net(x, training)
        return self.logits_nchw(), self.depth.clone()

    def route_grads(self, g_logits, g_depth):
        self.route_logits_grad(g_logits, None if g_depth is None else g_depth.contiguous().float(), self.depth)
        return ()

    def backward_net(self):
        """The tape in reverse, starting from ``logits.grad`` (written by adn_coarse_loss or by the autograd bridge)."""
        self._begin_backward(self.acts)
        self.backward_class_head()
        self._backward_ops(self.ops[:-1])


class CoarseLiteEngine(CoarseDepthEngine):
    """CoarseDepthLite (reference coarse_depth_model.py:199-287): five ConvS2BNLeaky, five ConvT2BNReLU, no skips, and the
    biased 3x3 class head (ConvLinear); everything behind the logits is CoarseDepthEngine's.  The first layer of the
    bf16 / base-64 network reads the f32 NCHW input itself (adn_l0_forward_stats / adn_thin_wgrad, ``thin_l0``)."""
    model_name = 'CoarseDepthLite'
    head_attr = 'head'

    def __init__(self, module, compute_dtype=torch.bfloat16):
        if compute_dtype == torch.float8_e4m3fn:
            raise NotImplementedError('CoarseDepthLite: the MX-fp8 path covers the 3x3 DoubleConv layers only (mxfp8 has no '
                                      'k4 stride-2 kernels)')
        super().__init__(module, compute_dtype)

    def check_input(self, shape):
        super().check_input(shape)
        H, W = shape[2], shape[3]
        if H % 32 or W % 32:
            raise RuntimeError(f'CoarseDepthLite: input {H}x{W} is not divisible by 32 (five stride-2 levels)')

    def _tape(self, B, Cin, H, W):
        m = self.module
        enc, dec = m.encoder, m.decoder
        self.thin_l0 = ConvK4BNAct.thin_ok(self, enc[0], W)
        inp = self.thin_input('x', Cin, H, W)
        if self.thin_l0:            # nothing reads the padded NHWC copy of the input: neither allocated nor written
            inp.data = torch.empty(0, dtype=self.dtype, device=self.dev)
        ops, src, h, w = [], inp, H, W
        for i in range(0, len(enc), 3):
            h, w = h // 2, w // 2
            out = Act(f'e{i // 3}', enc[i].out_channels, h, w)
            ops.append(ConvS2BNLeaky(src, enc[i], enc[i + 1], out, slope=enc[i + 2].negative_slope))
            src = out
        for i in range(0, len(dec), 3):
            h, w = h * 2, w * 2
            out = Act(f'd{i // 3}', dec[i].out_channels, h, w)
            ops.append(ConvT2BNReLU(src, dec[i], dec[i + 1], out))
            src = out
        self.inputs = [] if self.thin_l0 else [(inp, 0, Cin)]
        return ops + [self.class_head(src)]

    def load_input(self, x):
        self.x_in = x
        super().load_input(x)


# model(x) in training mode under autograd returns (logits NCHW f32, depth) hanging off one node, so the reference's loop
# ``criterion(logits, depth, bins, gt, valid_mask=gt > 0)['total'].backward(); clip_grad_norm_; optimizer.step()``
# (train_coarse_depth.py:446-463) runs unchanged
run_coarse = run_engine


def run_coarse_hard(engine, x, training):
    """predict_depth(mode='hard'): the centre of the first-maximum bin, [B,1,H,W]."""
    with torch.no_grad():
        idx = torch.empty(x.shape[0] * x.shape[2] * x.shape[3], dtype=torch.int32, device=x.device)
        engine.forward_net(x, training, argmax=idx)
        centers = engine.module.bin_centers
        return centers[idx.long()].view(x.shape[0], 1, x.shape[2], x.shape[3])


CoarseDistribution = namedtuple('CoarseDistribution', 'mean hard std entropy confidence argmax')
HybridDistribution = namedtuple('HybridDistribution', CoarseDistribution._fields + ('offset', 'final'))


def run_distribution(engine, x, training, result=CoarseDistribution):
    """predict_distribution(x): clones of the planes of ``engine.decode``, each [B,1,H,W]."""
    if not engine._bound():              # as run_engine: the refusals of forward come in forward's order
        engine.bind_parameters()
    with torch.no_grad():
        planes = engine.decode(x, training)
        return result(*(planes[k].clone() for k in result._fields))


class BinTargets:
    """Trainer mixin: the ``target_bins`` / ``edges`` arguments of ``step``."""
    edges = None

    def _bin_targets(self, x, target_bins, edges):
        """-> target_bins as the captured step takes them (f32), or None after refreshing ``self.edges`` (the inner bin
        edges on the device) from ``edges``."""
        if target_bins is not None:
            return target_bins.to(torch.float32)            # the capture's static inputs are f32; exact below 2^24
        if edges is None:
            raise ValueError(f'{type(self).__name__}.step: give target_bins or the bin edges')
        if edges.numel() != self.engine.module.n_bins + 1:
            raise ValueError(f'edges must hold n_bins + 1 = {self.engine.module.n_bins + 1} values, got {edges.numel()}')
        e = edges.detach().to(device=x.device, dtype=torch.float32).reshape(-1)[1:-1].contiguous()
        if self.edges is None or self.edges.shape != e.shape or self.edges.device != e.device:
            self.edges = e.clone()              # a captured step reads this buffer: refreshed in place
        else:
            self.edges.copy_(e)
        return None


class CoarseDepthTrainer(BinTargets, OptimTail):
    """One fused step of train_coarse_depth.py:446-463: forward, CoarseDepthLoss (valid = gt > 0), backward,
    clip_grad_norm_(1.0), optimizer.  ``ce_mode``: 'soft' (SoftCrossEntropyLoss(sigma)), 'focal' (FocalLoss(gamma)) or
    'ce' (nn.CrossEntropyLoss)."""

    def __init__(self, engine, ce_mode='soft', ce_weight=1.0, regression_weight=0.5, sigma=2.0, gamma=2.0,
                 optimizer='AdamW', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, clip_norm=1.0, ddp=None):
        self._init_optim(engine, optimizer, lr, betas, eps, weight_decay, clip_norm, ddp)
        self.ce_mode = K.CE_MODES[ce_mode]
        self.ce_weight, self.regression_weight = float(ce_weight), float(regression_weight)
        self.sigma, self.gamma = float(sigma), float(gamma)

    @classmethod
    def from_criterion(cls, engine, criterion, **kw):
        """Build from a models.coarse_depth_model.CoarseDepthLoss instance."""
        mode, sigma, gamma = criterion.fused_spec()
        return cls(engine, mode, criterion.ce_weight, criterion.regression_weight, sigma, gamma, **kw)

    def _new_scratch(self, pix, dev):
        f64 = dict(dtype=torch.float64, device=dev)
        return dict(stats=torch.zeros(1, **f64), sums=torch.zeros(2, **f64),
                    terms=torch.zeros(3, dtype=torch.float32, device=dev),
                    bins=torch.empty(pix, dtype=torch.int32, device=dev))

    def step(self, x, target_bins, target_depth, edges=None):
        """x [B,C,H,W]; target_bins [B,H,W] / [B,1,H,W] integer bins, or None with ``edges`` (the n_bins + 1 bin edges,
        BinnedDepthDataset.bin_edges) to bin target_depth on the device; target_depth [B,1,H,W].
        Returns (total loss 0-dim device tensor, terms f32[3] = ce, regression, total)."""
        return self._graphed(x, self._bin_targets(x, target_bins, edges), target_depth)

    def _step_impl(self, x, target_bins, gt):
        eng = self.engine
        logits, depth = eng.forward_net(x, True, head=False)
        self._ensure_setup(x.device)
        gt = gt.contiguous().float().view(-1)
        pix, nb = gt.numel(), eng.module.n_bins
        if pix != depth.numel():
            raise RuntimeError(f'CoarseDepthTrainer: target depth has {pix} pixels, the model output {depth.numel()}')
        s = self._shape_scratch((tuple(depth.shape), x.device), lambda: self._new_scratch(pix, x.device))
        stats, sums, terms, bins = s['stats'], s['sums'], s['terms'], s['bins']
        if target_bins is None:
            K.coarse_targets(gt, self.edges, bins, stats, eng.workspace)
        else:
            bins.copy_(target_bins.reshape(-1))
            K.coarse_targets(gt, None, None, stats, eng.workspace)
        pix_global = pix
        if self.ddp is not None:          # one global-batch loss, as under DataParallel: global valid count and pixel count
            self.ddp.all_reduce_loss_stats(stats)
            pix_global = pix * self.ddp.world_size
        K.coarse_loss(logits, nb, eng.centers, depth.view(-1), bins=bins, gt=gt, n_valid=stats, pixels_global=pix_global,
                      ce_mode=self.ce_mode, sigma=self.sigma, gamma=self.gamma, ce_weight=self.ce_weight,
                      reg_weight=self.regression_weight, dlogits=eng.logits.grad, workspace=eng.workspace)
        self._finish_loss(K.coarse_loss_finish, eng.workspace, pix, sums, (stats,), pix_global,
                          (self.ce_weight, self.regression_weight), terms)
        eng.backward_net()
        if self.ddp is not None:
            self.ddp.finish()
        self._apply()
        return terms[2], terms
