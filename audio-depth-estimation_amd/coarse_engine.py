"""Coarse depth classification model on libadn: the DoubleConv U-Net tape, the 1x1 class head and the fused loss step.

Replaces /root/reference/models/coarse_depth_model.py:134-189 and the training step of
/root/reference/train_coarse_depth.py:446-463 with CoarseDepthLoss (:391-468).  The encoder / decoder are the ops of
dc_engine.py, the class head is adabins_engine.ConvLinear, and everything behind the logits is ONE pass of
adn_coarse_loss (csrc/coarse.hip): softmax expectation, classification loss (soft CE / focal / CE), masked L1 of the
expectation and the gradient of their weighted sum, written once in the logits' dtype.  The logits [B,H,W,n_bins] stay
NHWC in the compute dtype and are only expanded to f32 NCHW when a caller asks for them (forward()).
CoarseLiteEngine runs CoarseDepthLite (:199-287) through the same engine: only the tape in front of the logits differs
(the ``_build_tape`` hook).
"""
from __future__ import annotations

import torch

from . import kernels as K
from .adabins_engine import ConvLinear
from .dc_engine import Act, ConvK4BNAct, ConvS2BNLeaky, ConvT2BNReLU, DCEngine, flag_solo, mark_tail_writers
from .trainer import OptimTail


class CoarseDepthEngine(DCEngine):
    name = 'CoarseDepthUNet'
    head_attr = 'outc'               # the model's attribute that holds the class-head conv

    def __init__(self, module, compute_dtype=torch.bfloat16):
        super().__init__(module, None, compute_dtype, self.name)
        self.autograd_pass = 0

    def _build_tape(self, Cin, H, W):
        """-> (inputs, ops, feature record in front of the class head): the tape hook of _prepare_net."""
        m = self.module
        inp = self.thin_input('x', Cin, H, W)
        ops, f = m.inc.adn_ops([inp], 'x1', H, W)
        feats = [f]
        for i, down in enumerate((m.down1, m.down2, m.down3, m.down4)):
            o, f = down.adn_ops(feats[-1], f'x{i + 2}')
            ops += o
            feats.append(f)
        d = feats[4]
        for i, up in enumerate((m.up1, m.up2, m.up3, m.up4)):
            o, d = up.adn_ops(d, feats[3 - i], f'd{4 - i}')
            ops += o
        return [(inp, 0, Cin)], ops, d

    def check_input(self, shape):
        """The shape refusals of forward, on the host (no device work)."""
        B, Cin, H, W = shape
        m = self.module
        if Cin != m.input_channels:
            raise RuntimeError(f'expected input[{B}, {Cin}, {H}, {W}] to have {m.input_channels} channels, but got {Cin} '
                               'channels instead')
        if W != m.output_size:
            raise NotImplementedError(f'{self.name}: input width {W} != output_size {m.output_size}: the bilinear resize '
                                      f'of the {m.n_bins}-channel logits (coarse_depth_model.py:159-161) is not implemented')
        if not 2 <= m.n_bins <= 512:
            raise NotImplementedError(f'{self.name}: n_bins={m.n_bins} is outside the range [2, 512] of adn_coarse_loss')

    def _prepare_net(self, x):
        if not self._bound():
            self.bind_parameters()
        B, Cin, H, W = x.shape
        key = (B, Cin, H, W, x.device)
        if self._shape_enter(key):
            return
        m = self.module
        self.check_input((B, Cin, H, W))
        self.B, self.dev = B, x.device
        self._scratch = {}
        self.epc = 8 if self.dtype == torch.bfloat16 else 4
        self.pairs = []
        self.inputs, ops, d = self._build_tape(Cin, H, W)
        self.logits = Act('logits', m.n_bins, H, W)
        self.class_op = ConvLinear(d, getattr(m, self.head_attr), self.logits)
        ops.append(self.class_op)
        self.ops = ops
        acts = {}
        for op in ops:
            for a in list(getattr(op, 'srcs', [])) + [getattr(op, 'src', None), getattr(op, 'out', None)]:
                if a is not None:
                    acts[id(a)] = a
        self.acts = list(acts.values())
        for a in self.acts:
            flag_solo(a)
            a.alloc(B, self.dtype, x.device)
        mark_tail_writers(ops)
        pix = B * H * W
        ws = max(1 << 16, K.coarse_loss_workspace_bytes(pix), K.coarse_targets_workspace_bytes(pix))
        if m.n_bins <= 256:
            ws = max(ws, K.bins_bwd_workspace_bytes(B, H * W, m.n_bins))
        for op in ops:
            op.prepare(self)
            ws = max(ws, op.workspace_bytes(self))
        f32 = dict(dtype=torch.float32, device=x.device)
        self.depth = torch.empty(B, 1, H, W, **f32)
        self.centers = torch.empty(m.n_bins, **f32)
        self._bridge = None
        self.workspace = torch.empty(ws // 4 + 4, **f32)
        self.weights_dirty = True
        self._shape_key = key

    def forward_net(self, x, training, argmax=None, head=True):
        """-> (logits NHWC in the compute dtype, depth f32 [B,1,H,W]); both are the engine's own buffers.  ``head=False``
        (the fused trainer): the softmax expectation is left to the caller's own adn_coarse_loss pass, which writes
        ``depth`` together with the loss and the gradient, so the logits are read once per step."""
        if not x.is_cuda:
            raise RuntimeError(f'{self.name} needs a HIP device tensor (libadn has no CPU path)')
        x = x.contiguous().float()
        self._prepare_net(x)
        if self.weights_dirty or self._packed_version != self._version_sum():
            self._pack_weights()
        self.fwd_serial += 1
        self.load_input(x)
        for op in self.ops:
            op.fwd(self, training)
        self.centers.copy_(self.module.bin_centers.detach().to(torch.float32).reshape(-1))
        if head:
            K.coarse_loss(self.logits.data, self.module.n_bins, self.centers, self.depth, argmax=argmax)
        return self.logits.data, self.depth

    def bridge_scratch(self):
        """Per-shape buffers of the autograd bridge: centres per sample [B,nb] (what adn_bins_bwd takes), its unused
        d centres output, and the NHWC f32 copy of the upstream logits gradient."""
        if self._bridge is None:
            lg = self.logits
            f32 = dict(dtype=torch.float32, device=self.dev)
            self._bridge = (torch.empty(self.B, lg.C, **f32), torch.empty(self.B, lg.C, **f32),
                            torch.empty(self.B, lg.H, lg.W, lg.C, **f32))
        return self._bridge

    def logits_nchw(self):
        lg = self.logits
        out = torch.empty(self.B, lg.C, lg.H, lg.W, dtype=torch.float32, device=self.dev)
        K.nhwc_to_nchw(lg.data, out)
        return out

    def run(self, x, training):
        self.forward_net(x, training)
        return self.logits_nchw(), self.depth.clone()

    def backward_net(self):
        """The tape in reverse, starting from ``logits.grad`` (written by adn_coarse_loss or by the autograd bridge)."""
        for a in self.acts:
            a.written = False
        self._final = set(id(p) for p, _, _ in self.param_meta if not p.requires_grad)
        self._wm = len(self.param_meta)
        outc = getattr(self.module, self.head_attr)
        for op in reversed(self.ops):
            if op.out.needs_grad:
                op.bwd(self)
                if op is self.class_op:
                    self._mark(outc.bias)
                    self._ready(outc.weight)


class CoarseLiteEngine(CoarseDepthEngine):
    """CoarseDepthLite (reference coarse_depth_model.py:199-287): five ConvS2BNLeaky, five ConvT2BNReLU, no skips, and the
    biased 3x3 class head (ConvLinear); everything behind the logits is CoarseDepthEngine's.  The first layer of the
    bf16 / base-64 network reads the f32 NCHW input itself (adn_l0_forward_stats / adn_thin_wgrad, ``thin_l0``)."""
    name = 'CoarseDepthLite'
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

    def _build_tape(self, Cin, H, W):
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
        return ([] if self.thin_l0 else [(inp, 0, Cin)]), ops, src

    def load_input(self, x):
        self.x_in = x
        super().load_input(x)


class _CoarseFunction(torch.autograd.Function):
    """torch.autograd bridge: parameters are inputs, the outputs are (logits NCHW f32, depth), so the reference's loop
    ``criterion(logits, depth, bins, gt, valid_mask=gt > 0)['total'].backward(); clip_grad_norm_; optimizer.step()``
    (train_coarse_depth.py:446-463) runs unchanged.  logits.grad = g_logits (NHWC) + the soft-bin backward of g_depth."""

    @staticmethod
    def forward(ctx, x, engine, *params):
        engine.forward_net(x, True)
        engine.autograd_pass += 1
        ctx.engine, ctx.stamp = engine, engine.autograd_pass
        ctx.set_materialize_grads(False)
        return engine.logits_nchw(), engine.depth.clone()

    @staticmethod
    def backward(ctx, g_logits, g_depth):
        eng = ctx.engine
        if ctx.stamp != eng.autograd_pass:
            raise RuntimeError(f'{eng.name}: backward through a forward whose activations were overwritten by a later '
                               'training forward of the same module')
        lg, nb = eng.logits, eng.module.n_bins
        if g_depth is not None:
            if nb > 256:
                raise NotImplementedError('autograd through the soft depth needs n_bins <= 256 (adn_bins_bwd); use '
                                          'CoarseDepthTrainer')
            centers_b, dcent, _ = eng.bridge_scratch()
            centers_b.copy_(eng.centers.view(1, nb).expand_as(centers_b))
            K.bins_bwd(lg.data, centers_b, eng.depth.view(-1), g_depth.contiguous().float().view(-1), None, lg.grad, dcent,
                       eng.workspace)
        if g_logits is not None:
            glog = eng.bridge_scratch()[2]
            K.nchw_to_nhwc(g_logits.contiguous().float(), glog)
            K.bcast_add(lg.grad.view(-1, 1, 1, nb), glog.view(-1, nb), 1.0, accumulate=g_depth is not None)
        if g_depth is None and g_logits is None:
            lg.grad.zero_()
        eng.backward_net()
        return (None, None) + tuple(eng.grad_view(p) if p.requires_grad else None for p, _, _ in eng.param_meta)


def run_coarse(engine, x, training):
    if not engine._bound():
        engine.bind_parameters()
    if training and torch.is_grad_enabled() and any(p.requires_grad for p, _, _ in engine.param_meta):
        return _CoarseFunction.apply(x, engine, *[p for p, _, _ in engine.param_meta])
    with torch.no_grad():
        return engine.run(x, training)


def run_coarse_hard(engine, x, training):
    """predict_depth(mode='hard'): the centre of the first-maximum bin, [B,1,H,W]."""
    with torch.no_grad():
        idx = torch.empty(x.shape[0] * x.shape[2] * x.shape[3], dtype=torch.int32, device=x.device)
        engine.forward_net(x, training, argmax=idx)
        centers = engine.module.bin_centers
        return centers[idx.long()].view(x.shape[0], 1, x.shape[2], x.shape[3])


class CoarseDepthTrainer(OptimTail):
    """One fused step of train_coarse_depth.py:446-463: forward, CoarseDepthLoss (valid = gt > 0), backward,
    clip_grad_norm_(1.0), optimizer.  ``ce_mode``: 'soft' (SoftCrossEntropyLoss(sigma)), 'focal' (FocalLoss(gamma)) or
    'ce' (nn.CrossEntropyLoss)."""

    def __init__(self, engine, ce_mode='soft', ce_weight=1.0, regression_weight=0.5, sigma=2.0, gamma=2.0,
                 optimizer='AdamW', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, clip_norm=1.0, ddp=None):
        self._init_optim(engine, optimizer, lr, betas, eps, weight_decay, clip_norm, ddp)
        self.ce_mode = K.CE_MODES[ce_mode]
        self.ce_weight, self.regression_weight = float(ce_weight), float(regression_weight)
        self.sigma, self.gamma = float(sigma), float(gamma)
        self.edges = None

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
        if target_bins is None:
            if edges is None:
                raise ValueError('CoarseDepthTrainer.step: give target_bins or the bin edges')
            if edges.numel() != self.engine.module.n_bins + 1:
                raise ValueError(f'edges must hold n_bins + 1 = {self.engine.module.n_bins + 1} values, got {edges.numel()}')
            e = edges.detach().to(device=x.device, dtype=torch.float32).reshape(-1)[1:-1].contiguous()
            if self.edges is None or self.edges.shape != e.shape or self.edges.device != e.device:
                self.edges = e.clone()              # a captured step reads this buffer: refreshed in place
            else:
                self.edges.copy_(e)
        else:
            target_bins = target_bins.to(torch.float32)         # the capture's static inputs are f32; exact below 2^24
        return self._graphed(x, target_bins, target_depth)

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
        if self.ddp is not None:
            K.coarse_loss_finish(eng.workspace, pix, sums, None, pix_global, 0.0, 0.0, None)
            self.ddp.all_reduce_loss_stats(sums)
            K.coarse_loss_finish(None, pix, sums, stats, pix_global, self.ce_weight, self.regression_weight, terms)
            self.ddp.begin_backward()
        else:
            K.coarse_loss_finish(eng.workspace, pix, sums, stats, pix_global, self.ce_weight, self.regression_weight, terms)
        eng.backward_net()
        if self.ddp is not None:
            self.ddp.finish()
        self._apply()
        return terms[2], terms
