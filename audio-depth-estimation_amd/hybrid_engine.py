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
from .adabins_engine import _f32_add_
from .coarse_engine import BinTargets, ClassLogits
from .dc_engine import DCEngine, decoder_ops, run_engine, unet_encoder_ops
from .dualreg_engine import OffsetBranch
from .trainer import OptimTail


class HybridEngine(ClassLogits, OffsetBranch, DCEngine):
    head_attr = 'coarse_head'
    fused_trainer = 'HybridTrainer'

    def __init__(self, module, compute_dtype=torch.bfloat16, plane_channels=None):
        super().__init__(module, None, compute_dtype, 'CoarseWithOffsetModel')
        self._init_plane(plane_channels)

    def check_input(self, shape):
        m = self.module
        self.check_square(shape, f'the {m.n_bins}-channel logits and the {m.base_channels}-channel offset features '
                                 '(coarse_depth_model.py:706-727)')
        self.check_bins()

    def _tape(self, B, Cin, H, W):
        m = self.module
        inp = self.thin_input('x', Cin, H, W)
        self.inputs = [(inp, 0, Cin)]
        ops, feats = unet_encoder_ops(m, inp, H, W)
        o, d = decoder_ops((m.coarse_up1, m.coarse_up2, m.coarse_up3, m.coarse_up4), feats, 'coarse')
        self.ops_coarse = ops + o                                             # encoder + classification decoder
        return self.ops_coarse + [self.class_head(d)] + self.offset_branch(feats)

    def _workspace_floor(self, B, Cin, H, W):
        pix = B * H * W
        return max(self.logits_workspace_bytes(B, H, W), K.hybrid_loss_workspace_bytes(pix),
                   K.dualreg_loss_workspace_bytes(pix))

    def _alloc_outputs(self, B, Cin, H, W):
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.coarse = torch.empty(B, 1, H, W, **f32)
        self.final = torch.empty(B, 1, H, W, **f32)
        self.alloc_centers()

    def forward_net(self, x, training, head=True, decode=False):
        """-> (logits NHWC in the compute dtype, coarse, offset, final), the maps f32 [B,1,H,W]; all four are the engine's
        own buffers.  ``head=False`` (the fused trainer): final is left to the caller's own adn_hybrid_loss pass, which
        writes it together with the loss and the gradients.  ``decode=True``: the adn_coarse_decode pass stands in for
        the forward-only adn_coarse_loss; its mean plane is the coarse depth the offset branch reads."""
        self._begin_forward(x)
        self._forward_ops(self.ops_coarse, training)
        self.class_op.fwd(self, training)
        self.load_centers()
        if decode:
            self.decode_head(self.coarse)
        else:
            K.coarse_loss(self.logits.data, self.module.n_bins, self.centers, self.coarse)        # forward only
        offset = self.forward_offset(self.coarse, training)
        if head:
            K.dualreg_loss(self.coarse.view(-1), offset.view(-1), self.final.view(-1))
        if decode:
            self._planes.update(offset=offset, final=self.final)
        return self.logits.data, self.coarse, offset, self.final

    def run(self, x, training):
        _, c, o, f = self.forward_net(x, training)
        return self.logits_nchw(), c.clone(), o.clone(), f.clone()

    def route_grads(self, g_logits, g_coarse, g_offset, g_final):
        """(doffset,) of the autograd bridge, and logits.grad = g_logits (NHWC) + the soft-bin backward of g_coarse +
        g_final; doffset = g_offset + g_final."""
        doffset = torch.zeros_like(self.final)
        for g in (g_offset, g_final):
            if g is not None:
                _f32_add_(doffset, g)
        gdepth = None
        if g_coarse is not None or g_final is not None:
            gdepth = torch.zeros_like(self.final)
            for g in (g_coarse, g_final):
                if g is not None:
                    _f32_add_(gdepth, g)
        self.route_logits_grad(g_logits, gdepth, self.coarse)
        return (doffset,)

    def backward_net(self, doffset):
        """The tape in reverse: offset head, fusion convs and offset decoder, then from ``logits.grad`` (written by
        adn_hybrid_loss or by the autograd bridge) the class head, the classification decoder and the encoder."""
        self._begin_backward(self.acts)
        self.backward_offset(doffset)
        self.backward_class_head()
        self._backward_ops(self.ops_coarse)


# model(x) in training mode under autograd returns (logits NCHW f32, coarse, offset, final) hanging off one node, so the
# reference's loop ``criterion(*model(x), gt, bins)[0].backward(); clip_grad_norm_; optimizer.step()``
# (train_coarse_depth.py:433-463) runs unchanged
run_hybrid = run_engine


class HybridTrainer(BinTargets, OptimTail):
    """One fused step of train_coarse_depth.py:433-463 for model_type 'hybrid': forward, CoarseOffsetLoss (every pixel
    counts, no valid mask), backward, clip_grad_norm_(1.0), optimizer.  ``regression_loss``: 'l1' or 'l2'."""

    def __init__(self, engine, ce_weight=1.0, regression_weight=1.0, offset_reg_weight=0.1, regression_loss='l1',
                 label_smoothing=0.0, optimizer='AdamW', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None,
                 clip_norm=1.0, ddp=None):
        self._init_optim(engine, optimizer, lr, betas, eps, weight_decay, clip_norm, ddp)
        self.ce_weight, self.regression_weight = float(ce_weight), float(regression_weight)
        self.offset_reg_weight, self.label_smoothing = float(offset_reg_weight), float(label_smoothing)
        self.reg_mode = K.REG_MODES[regression_loss]

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
        return self._graphed(x, self._bin_targets(x, target_bins, edges), target_depth)

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
        self._finish_loss(K.hybrid_loss_finish, eng.workspace, pix, sums, (), pix_global, w, terms)
        eng.backward_net(doffset)
        if self.ddp is not None:
            self.ddp.finish()
        self._apply()
        return terms[4], terms
