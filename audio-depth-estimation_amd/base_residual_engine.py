"""Base + Residual model on libadn: one op tape (shared encoder, two decoders, two 1x1 heads) and the fused step.

Replaces /root/reference/models/base_residual_model.py:151-202 and the training step of
/root/reference/train_base_residual.py:375-388 with utils_base_residual_loss.BaseResidualLoss (:72-160): the
reconstruction term (masked L1 or SIlog of the final depth) reuses the masked-loss kernels of the U-Net path
(adn_loss_stats / adn_loss_finish), the structural target is adn_lowpass(gt), the rest is csrc/baseres.hip.
The encoder activations x1..x4 receive gradients from both decoders (accumulated in their gradient buffers).
"""
from __future__ import annotations

import torch

from . import kernels as K
from .adabins_engine import _f32_add_
from .dc_engine import DCEngine, Head1x1, decoder_ops, run_engine, unet_encoder_ops
from .trainer import OptimTail


class BaseResidualEngine(DCEngine):
    def __init__(self, module, compute_dtype=torch.bfloat16):
        super().__init__(module, None, compute_dtype, 'BaseResidualDepthNet')

    def check_input(self, shape):
        B, Cin, H, W = shape
        if Cin != self.module.input_channels:
            raise RuntimeError(f'expected input[{B}, {Cin}, {H}, {W}] to have {self.module.input_channels} channels, but got '
                               f'{Cin} channels instead')

    def _out_size(self, H, W):
        """input size != output_size: both heads resize their ACTIVATED map (bilinear, align_corners=False) before the sum
        and the clamp (base_residual_model.py:185-211)"""
        S = self.module.output_size
        return S if (H != S or W != S) else None

    def _tape(self, B, Cin, H, W):
        m = self.module
        osz = self._out_size(H, W)
        inp = self.thin_input('x', Cin, H, W)
        self.inputs = [(inp, 0, Cin)]
        ops, feats = unet_encoder_ops(m, inp, H, W)
        o, d = decoder_ops((m.base_up1, m.base_up2, m.base_up3, m.base_up4), feats, 'base')
        ops += o
        self.head_base = Head1x1(d, m.base_head, 1, m.max_depth, osz, clamp_after_resize=False)   # sigmoid * max_depth
        o, d = decoder_ops((m.res_up1, m.res_up2, m.res_up3, m.res_up4), feats, 'res')
        ops += o
        self.head_res = Head1x1(d, m.res_head, 2, 0.3 * m.max_depth, osz, clamp_after_resize=False)  # tanh * 0.3 max_depth
        return ops + [self.head_base, self.head_res]

    def _workspace_floor(self, B, Cin, H, W):
        return max(1 << 16, K.lowpass_workspace_bytes(B, H, W, 64))

    def _alloc_outputs(self, B, Cin, H, W):
        S = self._out_size(H, W)
        self.final = torch.empty(B, 1, S or H, S or W, dtype=torch.float32, device=self.dev)

    def forward_net(self, x, training):
        self._begin_forward(x)
        self._forward_ops(self.ops, training)
        self.head_base.fwd(self, training)
        self.head_res.fwd(self, training)
        K.clamp_add(self.head_base.result, self.head_res.result, self.module.max_depth, self.final)
        return self.head_base.result, self.head_res.result, self.final

    def run(self, x, training):
        b, r, f = self.forward_net(x, training)
        return b.clone(), r.clone(), f.clone()

    def route_grads(self, g_base, g_res, g_final):
        """(dbase, dres) of the autograd bridge: final = clamp(base + residual, 0, max_depth)
        (base_residual_model.py:150-152) routes its gradient into both heads."""
        base, resid = self.head_base.result, self.head_res.result
        dbase, dres = torch.zeros_like(base), torch.zeros_like(resid)
        if g_final is not None:
            s = base.clone()
            _f32_add_(s, resid)
            masked = torch.empty_like(s)
            K.clamp_range(s, self.module.max_depth, masked, g=g_final.contiguous().float())
            _f32_add_(dbase, masked)
            _f32_add_(dres, masked)
        if g_base is not None:
            _f32_add_(dbase, g_base)
        if g_res is not None:
            _f32_add_(dres, g_res)
        return dbase, dres

    def backward_net(self, dbase, dres):
        self._begin_backward(self.acts)
        self.head_res.bwd_head(self, dres)
        self.head_base.bwd_head(self, dbase)
        self._backward_ops(self.ops)


# model(x) in training mode under autograd returns (base_depth, residual, final_depth) hanging off one node, so that
# ``criterion(base, res, final, gt, mask)[0].backward()`` of train_base_residual.py reaches the parameters
run_base_residual = run_engine


class BaseResidualTrainer(OptimTail):
    """One fused step of train_base_residual.py:375-388: forward, BaseResidualLoss (valid = gt > 0), backward,
    clip_grad_norm_(1.0), optimizer."""

    def __init__(self, engine, lambda_recon=1.0, lambda_base=1.2, lambda_sparse=0.05, lowpass_kernel=16, use_l1=True,
                 use_silog=False, silog_lambda=0.5, optimizer='AdamW', lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=None, clip_norm=1.0, ddp=None):
        self._init_optim(engine, optimizer, lr, betas, eps, weight_decay, clip_norm, ddp)
        self.use_l1 = use_l1
        self.lambda_recon, self.lambda_base, self.lambda_sparse = lambda_recon, lambda_base, lambda_sparse
        self.k, self.use_silog, self.silog_lambda = lowpass_kernel, use_silog, silog_lambda

    @classmethod
    def from_criterion(cls, engine, criterion, **kw):
        """Build from a utils_base_residual_loss.BaseResidualLoss / AdaptiveBaseResidualLoss instance."""
        c = getattr(criterion, 'base_loss', criterion)
        return cls(engine, c.lambda_recon, c.lambda_base, c.lambda_sparse, c.lowpass_kernel, c.use_l1, c.use_silog,
                   c.silog_lambda, **kw)

    def set_criterion(self, criterion):
        c = getattr(criterion, 'base_loss', criterion)
        self.set_weights(c.lambda_recon, c.lambda_base)

    def set_weights(self, lambda_recon, lambda_base):
        """AdaptiveBaseResidualLoss.set_epoch (utils_base_residual_loss.py:210-229) result."""
        self.lambda_recon, self.lambda_base = lambda_recon, lambda_base

    def _new_scratch(self, pred):
        """Loss / gradient scratch of one batch shape (lstats, bstats, loss_ws, recon, terms, struct, gfinal, dbase, dres)."""
        f64, f32 = dict(dtype=torch.float64, device=pred.device), dict(dtype=torch.float32, device=pred.device)
        return dict(lstats=torch.zeros(4, **f64), bstats=torch.zeros(4, **f64), loss_ws=torch.empty(4096 + 8, **f64),
                    recon=torch.zeros(1, **f32), terms=torch.zeros(4, **f32), struct=torch.empty_like(pred),
                    gfinal=torch.empty_like(pred), dbase=torch.empty_like(pred), dres=torch.empty_like(pred))

    def step(self, x, gt):
        """Returns (total loss 0-dim device tensor, terms f32[4] = weighted recon, mean|base-struct|, mean|res|, total)."""
        return self._graphed(x, gt)

    def _step_impl(self, x, gt):
        eng = self.engine
        base, resid, final = eng.forward_net(x, True)
        gt = gt.contiguous().float()
        self._ensure_setup(final.device)
        vars(self).update(self._shape_scratch(tuple(final.shape), lambda: self._new_scratch(final)))
        K.lowpass(gt, self.k, self.struct, eng.workspace)
        from .utils_base_residual_loss import recon_criterion
        crit, mm = recon_criterion(self.use_l1, self.use_silog)   # weighted SIlog / L1 (Combined, one weight) or masked MSE
        l1w, sw = (0.0, self.lambda_recon) if self.use_silog else (self.lambda_recon, 0.0)
        K.loss_stats(final, gt, 1.0, mm, 1e-6, self.lstats, self.loss_ws)
        if self.ddp is not None:          # one global-batch loss, as under DataParallel (base_residual_model.py:266-269)
            self.ddp.all_reduce_loss_stats(self.lstats)
        K.loss_finish(final, gt, 1.0, mm, 1e-6, self.lstats, crit, l1w, sw, self.silog_lambda, self.recon, self.gfinal)
        K.baseres_stats(base, resid, self.struct, gt, self.recon, self.lambda_recon, self.lambda_base, self.lambda_sparse,
                        self.bstats, self.terms, eng.workspace)
        if self.ddp is not None:
            self.ddp.all_reduce_loss_stats(self.bstats)
            n = self.bstats[0].clamp_min(1.0)
            self.terms[1], self.terms[2] = self.bstats[1] / n, self.bstats[2] / n
            self.terms[3] = self.terms[0] + self.lambda_base * self.terms[1] + self.lambda_sparse * self.terms[2]
            self.ddp.begin_backward()
        K.baseres_grad(base, resid, self.struct, gt, self.gfinal, eng.module.max_depth, self.bstats, self.lambda_base,
                       self.lambda_sparse, self.dbase, self.dres)
        eng.backward_net(self.dbase, self.dres)
        if self.ddp is not None:
            self.ddp.finish()
        self._apply()
        return self.terms[3], self.terms
