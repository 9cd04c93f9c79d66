"""Dual-regression coarse-depth model on libadn: one op tape (shared encoder, coarse decoder + head, offset branch) and the
fused step.

Replaces the reference's models/coarse_depth_model.py:930-986 and the dual_reg training step of
the reference's train_coarse_depth.py:422-463 with DualRegressionLoss (:997-1056).  The encoder / decoders are the ops of
dc_engine.py; the offset branch (``offset_branch_ops``: second decoder, the biased 3x3 fusion conv over [decoder features,
detached coarse depth], the 32-channel layer and the 1x1 head) is a helper of its own so that the hybrid model can reuse
it.  Everything behind the two heads is ONE pass of adn_dualreg_loss (csrc/dualreg.hip): final = coarse + offset, the
three L1 terms and both head gradients.

The coarse depth enters the fusion conv as the LAST source of a virtual concat: an NHWC record in the compute dtype whose
channel 0 is the head's f32 result and whose other ``plane_channels - 1`` channels are zero (adn_nchw_to_nhwc zero-fills
them on every call).  It needs no gradient -- that is the reference's ``.detach()`` -- so its share of the input-gradient
GEMM lands in a throw-away buffer.  Width 64 keeps the conv on the MFMA kernels at the price of a doubled K for this one
layer; one 16-byte chunk (8 bf16 / 4 f32 channels) sends the conv, its input gradient and its weight gradient to the
generic kernels.  The default is 64 when ``base_channels % 64 == 0`` (profiles/dualreg_bench.json has both).
"""
from __future__ import annotations

import torch

from . import kernels as K
from .adabins_engine import _f32_add_
from .dc_engine import Act, ConvBNReLU, DCEngine, Head1x1, decoder_ops, run_engine, unet_encoder_ops
from .trainer import OptimTail


def offset_branch_ops(eng, feats, ups, fusion, head_conv, tag='offset'):
    """The offset branch shared by the dual-regression and the hybrid model: decoder ``ups`` over the encoder records
    ``feats`` (x1..x5), the plane record of ``eng.plane_channels`` channels that the caller fills with the detached
    coarse depth before these ops run, ``fusion`` = Sequential(conv3x3 + bias, BN, ReLU, conv3x3 + bias, BN, ReLU) and the
    1x1 ``head_conv`` with identity activation.  -> (ops in forward order, plane record, Head1x1)."""
    ops, d = decoder_ops(ups, feats, tag)
    plane = Act(f'{tag}.coarse_plane', eng.plane_channels, d.H, d.W, needs_grad=False)
    plane.C_real = 1
    mid = Act(f'{tag}.fuse0', fusion[0].out_channels, d.H, d.W)
    fused = Act(f'{tag}.fuse1', fusion[3].out_channels, d.H, d.W)
    ops.append(ConvBNReLU([d, plane], fusion[0], fusion[1], mid))           # torch.cat([o, coarse.detach()], dim=1)
    ops.append(ConvBNReLU([mid], fusion[3], fusion[4], fused))
    return ops, plane, Head1x1(fused, head_conv, 3, 0.0)


class OffsetBranch:
    """Engine mixin of the two families with an offset branch: the width of the plane record (``requested_plane``: None,
    'epc' or a channel count), the square-input refusal, and the branch's forward / backward walks."""

    def _init_plane(self, plane_channels):
        if self.mx8:
            raise NotImplementedError(f'{self.model_name}: the mxfp8 path is not wired for this family')
        self.requested_plane = plane_channels

    def _plane_width(self):
        epc = 8 if self.dtype == torch.bfloat16 else 4
        p = self.requested_plane
        if p is None:
            p = 64 if self.module.base_channels % 64 == 0 else epc
        elif p == 'epc':
            p = epc
        if p < 1 or p % epc != 0:
            raise ValueError(f'{type(self).__name__}: plane_channels must be a positive multiple of {epc} (one 16-byte chunk), '
                             f'got {p}')
        return p

    def check_square(self, shape, what):
        """Host-only: the channel count, and H == W == output_size (``what`` names the resize that is not implemented)."""
        B, Cin, H, W = shape
        m = self.module
        if Cin != m.input_channels:
            raise RuntimeError(f'expected input[{B}, {Cin}, {H}, {W}] to have {m.input_channels} channels, but got {Cin} '
                               'channels instead')
        if H != m.output_size or W != m.output_size:
            raise NotImplementedError(f'{self.model_name}: input {H} x {W} != output_size {m.output_size}: the bilinear '
                                      f'resize of {what} is not implemented')

    def offset_branch(self, feats):
        """-> the offset branch's tape (head last); sets ``plane_channels``, ``ops_offset``, ``plane``, ``head_offset``."""
        m = self.module
        self.plane_channels = self._plane_width()
        self.ops_offset, self.plane, self.head_offset = offset_branch_ops(
            self, feats, (m.offset_up1, m.offset_up2, m.offset_up3, m.offset_up4), m.offset_fusion, m.offset_head)
        return self.ops_offset + [self.head_offset]

    def forward_offset(self, coarse, training):
        """The offset branch over the detached ``coarse`` depth (f32 [B,1,H,W]) -> offset, the head's own buffer."""
        K.nchw_to_nhwc(coarse, self.plane.data)                               # channel 0 = coarse depth, the rest zero
        self._forward_ops(self.ops_offset, training)
        self.head_offset.fwd(self, training)
        return self.head_offset.result

    def backward_offset(self, doffset):
        self.head_offset.bwd_head(self, doffset)
        self._backward_ops(self.ops_offset)


class DualRegEngine(OffsetBranch, DCEngine):
    def __init__(self, module, compute_dtype=torch.bfloat16, plane_channels=None):
        super().__init__(module, None, compute_dtype, 'DualRegressionModel')
        self._init_plane(plane_channels)

    def check_input(self, shape):
        self.check_square(shape, f'the {self.module.base_channels}-channel offset features (coarse_depth_model.py:972-974)')

    def _tape(self, B, Cin, H, W):
        m = self.module
        inp = self.thin_input('x', Cin, H, W)
        self.inputs = [(inp, 0, Cin)]
        ops, feats = unet_encoder_ops(m, inp, H, W)
        o, d = decoder_ops((m.coarse_up1, m.coarse_up2, m.coarse_up3, m.coarse_up4), feats, 'coarse')
        self.ops_coarse = ops + o                                             # encoder + coarse decoder
        self.head_coarse = Head1x1(d, m.coarse_head, 3, 0.0)
        return self.ops_coarse + [self.head_coarse] + self.offset_branch(feats)

    def _workspace_floor(self, B, Cin, H, W):
        pix = B * H * W
        return max(1 << 16, K.dualreg_loss_workspace_bytes(pix), K.coarse_targets_workspace_bytes(pix))

    def _alloc_outputs(self, B, Cin, H, W):
        self.final = torch.empty(B, 1, H, W, dtype=torch.float32, device=self.dev)

    def forward_net(self, x, training, head=True):
        """-> (coarse, offset, final), f32 [B,1,H,W], the engine's own buffers.  ``head=False`` (the fused trainer): final
        is left to the caller's own adn_dualreg_loss pass, which writes it together with the loss and the gradients."""
        self._begin_forward(x)
        self._forward_ops(self.ops_coarse, training)
        self.head_coarse.fwd(self, training)
        coarse = self.head_coarse.result
        offset = self.forward_offset(coarse, training)
        if head:
            K.dualreg_loss(coarse.view(-1), offset.view(-1), self.final.view(-1))
        return coarse, offset, self.final

    def run(self, x, training):
        c, o, f = self.forward_net(x, training)
        return c.clone(), o.clone(), f.clone()

    def route_grads(self, g_coarse, g_offset, g_final):
        """(dcoarse, doffset) of the autograd bridge: final = coarse + offset routes its gradient into both heads."""
        dcoarse, doffset = torch.zeros_like(self.final), torch.zeros_like(self.final)
        for g, dsts in ((g_coarse, (dcoarse,)), (g_offset, (doffset,)), (g_final, (dcoarse, doffset))):
            if g is not None:
                for dst in dsts:
                    _f32_add_(dst, g)
        return dcoarse, doffset

    def backward_net(self, dcoarse, doffset):
        """The tape in reverse: offset head, fusion convs and offset decoder, coarse head, coarse decoder, encoder."""
        self._begin_backward(self.acts)
        self.backward_offset(doffset)
        self.head_coarse.bwd_head(self, dcoarse)
        self._backward_ops(self.ops_coarse)


# model(x) in training mode under autograd returns (coarse, offset, final) hanging off one node, so the reference's loop
# ``criterion(*model(x), gt)[0].backward(); clip_grad_norm_; optimizer.step()`` (train_coarse_depth.py:422-463) runs unchanged
run_dualreg = run_engine


class DualRegressionTrainer(OptimTail):
    """One fused step of train_coarse_depth.py:422-463 for model_type 'dual_reg': forward, DualRegressionLoss (valid =
    gt > 0, every pixel when the global batch has none), backward, clip_grad_norm_(1.0), optimizer."""

    def __init__(self, engine, coarse_weight=1.0, final_weight=1.0, offset_reg_weight=0.01, optimizer='AdamW', lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, weight_decay=None, clip_norm=1.0, ddp=None):
        self._init_optim(engine, optimizer, lr, betas, eps, weight_decay, clip_norm, ddp)
        self.coarse_weight, self.final_weight = float(coarse_weight), float(final_weight)
        self.offset_reg_weight = float(offset_reg_weight)

    @classmethod
    def from_criterion(cls, engine, criterion, **kw):
        """Build from a models.coarse_depth_model.DualRegressionLoss instance."""
        return cls(engine, criterion.coarse_weight, criterion.final_weight, criterion.offset_reg_weight, **kw)

    def _new_scratch(self, final):
        f64 = dict(dtype=torch.float64, device=final.device)
        return dict(stats=torch.zeros(1, **f64), sums=torch.zeros(3, **f64),
                    terms=torch.zeros(4, dtype=torch.float32, device=final.device),
                    dcoarse=torch.empty_like(final), doffset=torch.empty_like(final))

    def step(self, x, gt):
        """x [B,C,S,S]; gt [B,1,S,S].  Returns (total loss 0-dim device tensor, terms f32[4] = coarse, final, offset_reg,
        total)."""
        return self._graphed(x, gt)

    def _step_impl(self, x, gt):
        eng = self.engine
        coarse, offset, final = eng.forward_net(x, True, head=False)
        self._ensure_setup(x.device)
        gt = gt.contiguous().float().view(-1)
        pix = gt.numel()
        if pix != final.numel():
            raise RuntimeError(f'DualRegressionTrainer: target depth has {pix} pixels, the model output {final.numel()}')
        s = self._shape_scratch((tuple(final.shape), x.device), lambda: self._new_scratch(final))
        stats, sums, terms, dcoarse, doffset = s['stats'], s['sums'], s['terms'], s['dcoarse'], s['doffset']
        K.coarse_targets(gt, None, None, stats, eng.workspace)
        pix_global = pix
        if self.ddp is not None:          # one global-batch loss, as under DataParallel: global valid count and pixel count
            self.ddp.all_reduce_loss_stats(stats)
            pix_global = pix * self.ddp.world_size
        w = (self.coarse_weight, self.final_weight, self.offset_reg_weight)
        K.dualreg_loss(coarse.view(-1), offset.view(-1), final.view(-1), gt=gt, n_valid=stats, pixels_global=pix_global,
                       coarse_weight=w[0], final_weight=w[1], offset_reg_weight=w[2], dcoarse=dcoarse.view(-1),
                       doffset=doffset.view(-1), workspace=eng.workspace)
        self._finish_loss(K.dualreg_loss_finish, eng.workspace, pix, sums, (stats,), pix_global, w, terms)
        eng.backward_net(dcoarse, doffset)
        if self.ddp is not None:
            self.ddp.finish()
        self._apply()
        return terms[3], terms
