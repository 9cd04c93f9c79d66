"""Hybrid coarse-depth model on libadn: one op tape (shared encoder, classification decoder + class head, offset branch)
and the fused step.

Replaces the reference's models/coarse_depth_model.py:677-740 and the hybrid training step of the reference's
train_coarse_depth.py:433-463 with CoarseOffsetLoss (:773-850).  The encoder / decoders are the ops of dc_engine.py, the
class head is adabins_engine.ConvLinear onto an NHWC ``logits`` record in the compute dtype (as in coarse_engine.py), and
the offset branch is dualreg_engine.offset_branch_ops.  The coarse depth is the softmax expectation of a forward-only
adn_coarse_loss pass; it enters the fusion conv through the plane record (detached, as in the reference) and, unchanged,
the loss tail.  Everything behind the two heads is ONE pass of adn_hybrid_loss (csrc/hybrid.hip): final = coarse + offset,
label-smoothed cross-entropy, L1 / L2 of final, mean |offset|, and the gradients towards the logits (which also carry the
regression gradient through the coarse depth) and the offset plane.
"""
from __future__ import annotations

import torch

from . import kernels as K
from .adabins_engine import ConvLinear
from .dc_engine import Act, DCEngine, flag_solo, mark_tail_writers
from .dualreg_engine import offset_branch_ops
from .trainer import OptimTail


class HybridEngine(DCEngine):
    def __init__(self, module, compute_dtype=torch.bfloat16, plane_channels=None):
        super().__init__(module, None, compute_dtype, 'CoarseWithOffsetModel')
        if self.mx8:
            raise NotImplementedError('CoarseWithOffsetModel: the mxfp8 path is not wired for this family')
        self.requested_plane = plane_channels
        self.autograd_pass = 0

    def _plane_width(self):
        epc = 8 if self.dtype == torch.bfloat16 else 4
        p = self.requested_plane
        if p is None:
            p = 64 if self.module.base_channels % 64 == 0 else epc
        elif p == 'epc':
            p = epc
        if p < 1 or p % epc != 0:
            raise ValueError(f'HybridEngine: plane_channels must be a positive multiple of {epc} (one 16-byte chunk), got {p}')
        return p

    def check_input(self, shape):
        """Host-only: the input shapes this family runs."""
        B, Cin, H, W = shape
        m = self.module
        if Cin != m.input_channels:
            raise RuntimeError(f'expected input[{B}, {Cin}, {H}, {W}] to have {m.input_channels} channels, but got {Cin} '
                               'channels instead')
        if H != m.output_size or W != m.output_size:
            raise NotImplementedError(f'CoarseWithOffsetModel: input {H} x {W} != output_size {m.output_size}: the bilinear '
                                      f'resize of the {m.n_bins}-channel logits and the {m.base_channels}-channel offset '
                                      'features (coarse_depth_model.py:706-727) is not implemented')
        if not 2 <= m.n_bins <= 512:
            raise NotImplementedError(f'CoarseWithOffsetModel: n_bins={m.n_bins} is outside the range [2, 512] of '
                                      'adn_coarse_loss / adn_hybrid_loss')

    def _prepare_net(self, x):
        self.check_input(x.shape)
        if not self._bound():
            self.bind_parameters()
        B, Cin, H, W = x.shape
        key = (B, Cin, H, W, x.device)
        if self._shape_enter(key):
            return
        m = self.module
        self.B, self.dev = B, x.device
        self._scratch = {}
        self.epc = 8 if self.dtype == torch.bfloat16 else 4
        self.plane_channels = self._plane_width()
        self.pairs = []
        inp = self.thin_input('x', Cin, H, W)
        ops, f = m.inc.adn_ops([inp], 'x1', H, W)
        feats = [f]
        for i, down in enumerate((m.down1, m.down2, m.down3, m.down4)):
            o, f = down.adn_ops(feats[-1], f'x{i + 2}')
            ops += o
            feats.append(f)
        d = feats[4]
        for i, up in enumerate((m.coarse_up1, m.coarse_up2, m.coarse_up3, m.coarse_up4)):
            o, d = up.adn_ops(d, feats[3 - i], f'coarse.d{4 - i}')
            ops += o
        self.logits = Act('logits', m.n_bins, H, W)
        self.class_op = ConvLinear(d, m.coarse_head, self.logits)
        self.ops_coarse = ops                                                 # encoder + classification decoder
        self.ops_offset, self.plane, self.head_offset = offset_branch_ops(
            self, feats, (m.offset_up1, m.offset_up2, m.offset_up3, m.offset_up4), m.offset_fusion, m.offset_head)
        self.inputs, self.ops = [(inp, 0, Cin)], self.ops_coarse + [self.class_op] + self.ops_offset
        tape = self.ops + [self.head_offset]
        acts = {}
        for op in self.ops:
            for a in list(getattr(op, 'srcs', [])) + [getattr(op, 'src', None), getattr(op, 'out', None)]:
                if a is not None:
                    acts[id(a)] = a
        self.acts = list(acts.values())
        for a in self.acts:
            flag_solo(a)
            a.alloc(B, self.dtype, x.device)
        mark_tail_writers(tape)
        pix = B * H * W
        ws = max(1 << 16, K.hybrid_loss_workspace_bytes(pix), K.coarse_loss_workspace_bytes(pix),
                 K.dualreg_loss_workspace_bytes(pix), K.coarse_targets_workspace_bytes(pix))
        if m.n_bins <= 256:
            ws = max(ws, K.bins_bwd_workspace_bytes(B, H * W, m.n_bins))
        for op in tape:
            op.prepare(self)
            ws = max(ws, op.workspace_bytes(self))
        f32 = dict(dtype=torch.float32, device=x.device)
        self.coarse = torch.empty(B, 1, H, W, **f32)
        self.final = torch.empty(B, 1, H, W, **f32)
        self.centers = torch.empty(m.n_bins, **f32)
        self._bridge = None
        self.workspace = torch.empty(ws // 4 + 4, **f32)
        self.weights_dirty = True
        self._shape_key = key

    def forward_net(self, x, training, head=True):
        """-> (logits NHWC in the compute dtype, coarse, offset, final), the maps f32 [B,1,H,W]; all four are the engine's
        own buffers.  ``head=False`` (the fused trainer): final is left to the caller's own adn_hybrid_loss pass, which
        writes it together with the loss and the gradients."""
        if not x.is_cuda:
            raise RuntimeError('CoarseWithOffsetModel needs a HIP device tensor (libadn has no CPU path)')
        x = x.contiguous().float()
        self._prepare_net(x)
        if self.weights_dirty or self._packed_version != self._version_sum():
            self._pack_weights()
        self.fwd_serial += 1
        self.load_input(x)
        for op in self.ops_coarse:
            op.fwd(self, training)
        self.class_op.fwd(self, training)
        self.centers.copy_(self.module.bin_centers.detach().to(torch.float32).reshape(-1))
        K.coarse_loss(self.logits.data, self.module.n_bins, self.centers, self.coarse)        # forward only
        K.nchw_to_nhwc(self.coarse, self.plane.data)                          # channel 0 = coarse depth, the rest zero
        for op in self.ops_offset:
            op.fwd(self, training)
        self.head_offset.fwd(self, training)
        offset = self.head_offset.result
        if head:
            K.dualreg_loss(self.coarse.view(-1), offset.view(-1), self.final.view(-1))
        return self.logits.data, self.coarse, offset, self.final

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
        _, c, o, f = self.forward_net(x, training)
        return self.logits_nchw(), c.clone(), o.clone(), f.clone()

    def backward_net(self, doffset):
        """The tape in reverse: offset head, fusion convs and offset decoder, then from ``logits.grad`` (written by
        adn_hybrid_loss or by the autograd bridge) the class head, the classification decoder and the encoder."""
        for a in self.acts:
            a.written = False
        self._final = set(id(p) for p, _, _ in self.param_meta if not p.requires_grad)
        self._wm = len(self.param_meta)
        self.head_offset.bwd_head(self, doffset)
        for op in reversed(self.ops_offset):
            if op.out.needs_grad:
                op.bwd(self)
        head = self.module.coarse_head
        self.class_op.bwd(self)
        self._mark(head.bias)
        self._ready(head.weight)
        for op in reversed(self.ops_coarse):
            if op.out.needs_grad:
                op.bwd(self)


class _HybridFunction(torch.autograd.Function):
    """torch.autograd bridge: parameters are inputs, the outputs are (logits NCHW f32, coarse, offset, final), so the
    reference's loop ``criterion(*model(x), gt, bins)[0].backward(); clip_grad_norm_; optimizer.step()``
    (train_coarse_depth.py:433-463) runs unchanged.  logits.grad = g_logits (NHWC) + the soft-bin backward of
    g_coarse + g_final; doffset = g_offset + g_final; missing gradients count as zero."""

    @staticmethod
    def forward(ctx, x, engine, *params):
        _, c, o, f = engine.forward_net(x, True)
        engine.autograd_pass += 1
        ctx.engine, ctx.stamp = engine, engine.autograd_pass
        ctx.set_materialize_grads(False)
        return engine.logits_nchw(), c.clone(), o.clone(), f.clone()

    @staticmethod
    def backward(ctx, g_logits, g_coarse, g_offset, g_final):
        eng = ctx.engine
        if ctx.stamp != eng.autograd_pass:
            raise RuntimeError('CoarseWithOffsetModel: backward through a forward whose activations were overwritten by a '
                               'later training forward of the same module')
        lg, nb = eng.logits, eng.module.n_bins
        add_ = lambda dst, src: K.bcast_add(dst.view(-1, 1, 1, 1), src.contiguous().float().view(-1, 1), 1.0, accumulate=True)
        doffset = torch.zeros_like(eng.final)
        for g in (g_offset, g_final):
            if g is not None:
                add_(doffset, g)
        have_depth = g_coarse is not None or g_final is not None
        if have_depth:
            if nb > 256:
                raise NotImplementedError('autograd through the coarse depth needs n_bins <= 256 (adn_bins_bwd); use '
                                          'HybridTrainer')
            gdepth = torch.zeros_like(eng.final)
            for g in (g_coarse, g_final):
                if g is not None:
                    add_(gdepth, g)
            centers_b, dcent, _ = eng.bridge_scratch()
            centers_b.copy_(eng.centers.view(1, nb).expand_as(centers_b))
            K.bins_bwd(lg.data, centers_b, eng.coarse.view(-1), gdepth.view(-1), None, lg.grad, dcent, eng.workspace)
        if g_logits is not None:
            glog = eng.bridge_scratch()[2]
            K.nchw_to_nhwc(g_logits.contiguous().float(), glog)
            K.bcast_add(lg.grad.view(-1, 1, 1, nb), glog.view(-1, nb), 1.0, accumulate=have_depth)
        if not have_depth and g_logits is None:
            lg.grad.zero_()
        eng.backward_net(doffset)
        return (None, None) + tuple(eng.grad_view(p) if p.requires_grad else None for p, _, _ in eng.param_meta)


def run_hybrid(engine, x, training):
    if not engine._bound():
        engine.bind_parameters()
    if training and torch.is_grad_enabled() and any(p.requires_grad for p, _, _ in engine.param_meta):
        return _HybridFunction.apply(x, engine, *[p for p, _, _ in engine.param_meta])
    with torch.no_grad():
        return engine.run(x, training)


class HybridTrainer(OptimTail):
    """One fused step of train_coarse_depth.py:433-463 for model_type 'hybrid': forward, CoarseOffsetLoss (every pixel
    counts, no valid mask), backward, clip_grad_norm_(1.0), optimizer.  ``regression_loss``: 'l1' or 'l2'."""

    def __init__(self, engine, ce_weight=1.0, regression_weight=1.0, offset_reg_weight=0.1, regression_loss='l1',
                 label_smoothing=0.0, optimizer='AdamW', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None,
                 clip_norm=1.0, ddp=None):
        self._init_optim(engine, optimizer, lr, betas, eps, weight_decay, clip_norm, ddp)
        self.ce_weight, self.regression_weight = float(ce_weight), float(regression_weight)
        self.offset_reg_weight, self.label_smoothing = float(offset_reg_weight), float(label_smoothing)
        self.reg_mode = K.REG_MODES[regression_loss]
        self.edges = None

    @classmethod
    def from_criterion(cls, engine, criterion, **kw):
        """Build from a models.coarse_depth_model.CoarseOffsetLoss instance."""
        return cls(engine, *criterion.fused_spec(), **kw)

    def _new_scratch(self, final):
        dev = final.device
        return dict(sums=torch.zeros(4, dtype=torch.float64, device=dev), stats=torch.zeros(1, dtype=torch.float64, device=dev),
                    terms=torch.zeros(5, dtype=torch.float32, device=dev),
                    bins=torch.empty(final.numel(), dtype=torch.int32, device=dev), doffset=torch.empty_like(final))

    def step(self, x, target_bins, target_depth, edges=None):
        """x [B,C,S,S]; target_bins [B,S,S] / [B,1,S,S] integer bins, or None with ``edges`` (the n_bins + 1 bin edges,
        BinnedDepthDataset.bin_edges) to bin target_depth on the device; target_depth [B,1,S,S].
        Returns (total loss 0-dim device tensor, terms f32[5] = ce, regression, offset_reg, coarse_l1, total)."""
        if target_bins is None:
            if edges is None:
                raise ValueError('HybridTrainer.step: give target_bins or the bin edges')
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
        logits, coarse, offset, final = eng.forward_net(x, True, head=False)
        self._ensure_setup(x.device)
        gt = gt.contiguous().float().view(-1)
        pix, nb = gt.numel(), eng.module.n_bins
        if pix != final.numel():
            raise RuntimeError(f'HybridTrainer: target depth has {pix} pixels, the model output {final.numel()}')
        s = self._shape_scratch((tuple(final.shape), x.device), lambda: self._new_scratch(final))
        sums, stats, terms, bins, doffset = s['sums'], s['stats'], s['terms'], s['bins'], s['doffset']
        if target_bins is None:
            K.coarse_targets(gt, self.edges, bins, stats, eng.workspace)
        else:
            bins.copy_(target_bins.reshape(-1))
        pix_global = pix
        if self.ddp is not None:          # one global-batch loss, as under DataParallel: the global pixel count
            pix_global = pix * self.ddp.world_size
        w = (self.ce_weight, self.regression_weight, self.offset_reg_weight)
        K.hybrid_loss(logits, nb, eng.centers, coarse.view(-1), offset.view(-1), bins, gt, final.view(-1), eng.logits.grad,
                      doffset.view(-1), eng.workspace, pixels_global=pix_global, ce_weight=w[0], reg_weight=w[1],
                      offset_reg_weight=w[2], label_smoothing=self.label_smoothing, reg_mode=self.reg_mode)
        if self.ddp is not None:
            K.hybrid_loss_finish(eng.workspace, pix, sums, pix_global, 0.0, 0.0, 0.0, None)
            self.ddp.all_reduce_loss_stats(sums)
            K.hybrid_loss_finish(None, pix, sums, pix_global, *w, terms)
            self.ddp.begin_backward()
        else:
            K.hybrid_loss_finish(eng.workspace, pix, sums, pix_global, *w, terms)
        eng.backward_net(doffset)
        if self.ddp is not None:
            self.ddp.finish()
        self._apply()
        return terms[4], terms
