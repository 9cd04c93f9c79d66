"""Fused U-Net cVAE pipeline: the U-Net engine with a VAE bottleneck at the 1x1 innermost level.

Replaces what PyTorch dispatches for /root/reference/models/unet_cvae_model.py (UnetGeneratorVAE) and the training step of
/root/reference/train_cvae.py:438-478.  Topology differences from the plain U-Net (engine.UNetEngine hooks):
  * innermost level: down conv with the RAW epilogue (f32 h [B, C], no norm), then adn_vae_fwd writes ReLU(fc_dec(z))
    straight into that level's ``rd`` buffer, the operand of the unchanged innermost transposed conv;
  * level n-2: no skip; its transposed conv reads ``ru[n-1]`` alone and the dgrad of L(n-1) is the only writer of Gd[n-2];
  * head: identity (depth_norm) or ReLU, no Sigmoid.
The three BatchNorms the reference builds but never calls (outermost downnorm / upnorm, innermost downnorm) are kept out of
the flat buffers: no kernel, no gradient (their .grad stays None), no optimizer step, no optimizer state.
Inference with K hypotheses per input (``CVAEEngine.sample``): the down path once, adn_vae_sample for K draws, the up path
per draw with shared skips, adn_sample_stats for the per-pixel mean / std; on a buffer set of its own.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import kernels as K
from .engine import FusedTrainer, UNetEngine


class CVAEEngine(UNetEngine):
    """Runs UnetGeneratorVAE.forward/backward through libadn.  The KL scalar of the last forward is ``vae_kl`` (f32 [1])."""

    def __init__(self, module, num_downs, depth_norm, compute_dtype=torch.bfloat16):
        super().__init__(module, num_downs, depth_norm, compute_dtype)
        self.model_name = 'UnetGeneratorVAE'
        self.final_act = 2 if self.depth_norm else 0
        self.vae = module._vae_module()
        self.unused_params = frozenset(id(p) for p in module._unused_params())
        # noise stream: keyed by (seed, device step counter, element) in training under a fused trainer (replay-safe);
        # by (seed, host draw count, element) otherwise.  The seed is the default CPU generator's, read without
        # consuming a draw, so torch.manual_seed makes a run reproducible and the data order stays the reference's.
        self.vae_seed = (torch.initial_seed() * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
        self.vae_draws = 0
        self._sample_k = 0           # > 0 while sample() runs: _prepare builds / enters that (shape, K) sampling set
        self.step_counter = None
        self.eps_in = None           # f32 [B, L] device tensor: replaces the draw (tests inject the reference's eps)
        self.g_kl = None             # device f32 [1]: d loss / d kl for the backward
        self.loss_acc = None         # device f32 [1] or None: backward adds g_kl * kl to it

    def _flat_params(self):
        return [p for p in self.module.parameters() if id(p) not in self.unused_params]

    def _prepare(self, x):
        B, Cin, H, W = x.shape
        if H != 1 << self.n or W != 1 << self.n:
            raise RuntimeError(f'UnetGeneratorVAE with {self.n} downsamplings needs a {1 << self.n}x{1 << self.n} input '
                               f'(the VAE bottleneck reads a 1x1 innermost map), got {H}x{W}')
        super()._prepare(x)

    def _prepare_vae(self, B, dev):
        C, L = self.levels[-1]['cd_out'], self.vae.latent_dim
        f32 = dict(dtype=torch.float32, device=dev)
        self.vae_h = torch.empty(B, C, **f32)
        self.vae_mu = torch.empty(B, L, **f32)
        self.vae_logvar = torch.empty(B, L, **f32)
        self.vae_eps = torch.empty(B, L, **f32)
        self.vae_z = torch.empty(B, L, **f32)
        self.vae_kl_img = torch.empty(B, **f32)
        self.vae_kl = torch.zeros(1, **f32)
        self.vae_ws = torch.empty(max(K.vae_bwd_workspace_bytes(B, L), 16) // 4, **f32)
        if self._sample_k:
            self._prepare_sample(B, self._sample_k, dev)

    def _vae_params(self):
        v = self.vae
        return (v.fc_mu.weight, v.fc_mu.bias, v.fc_logvar.weight, v.fc_logvar.bias, v.fc_dec.weight, v.fc_dec.bias)

    def _vae_forward(self, training):
        fp = [self._flat_slice(self.flat_p, p) for p in self._vae_params()]
        if training and self.step_counter is not None:
            seed, counter = self.vae_seed, self.step_counter
        else:
            self.vae_draws += 1
            seed, counter = self.vae_seed ^ ((self.vae_draws * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF), None
        eps_in = self.eps_in
        if eps_in is not None and tuple(eps_in.shape) != tuple(self.vae_mu.shape):
            raise RuntimeError(f'eps_in has shape {tuple(eps_in.shape)}, the bottleneck draws {tuple(self.vae_mu.shape)}')
        K.vae_fwd(self.vae_h, *fp, seed, counter, eps_in, self.vae_mu, self.vae_logvar, self.vae_eps, self.vae_z,
                  self.vae_kl_img, self.vae_kl, self.levels[-1]['rd'])

    def _vae_backward(self):
        if self.g_kl is None:
            raise RuntimeError('CVAEEngine.backward needs g_kl (d loss / d kl as a device f32[1])')
        wm, _, wl, _, wd, _ = [self._flat_slice(self.flat_p, p) for p in self._vae_params()]
        g = [self._flat_slice(self.flat_g, p) for p in self._vae_params()]
        gd = self.levels[-1]['Gd']
        K.vae_bwd(gd, self.vae_h, self.vae_mu, self.vae_logvar, self.vae_eps, self.vae_z, wm, wl, wd, self.g_kl, *g, gd,
                  self.vae_ws, kl=self.vae_kl, loss=self.loss_acc)

    # ------------------------------------------------------------------ multi-hypothesis inference
    def _buffer_key(self, x):
        key = super()._buffer_key(x)
        return key + ('sample', self._sample_k) if self._sample_k else key

    def _prepare_sample(self, B, Kn, dev):
        """What a (B, K) sampling set holds beyond an ordinary set: the K draws and the K * B rows of the innermost
        ``rd`` operand.  The up path then runs sample by sample on the set's own batch-B buffers."""
        C, L = self.levels[-1]['cd_out'], self.vae.latent_dim
        self.s_eps = torch.empty(Kn, B, L, dtype=torch.float32, device=dev)
        self.s_z = torch.empty(Kn, B, L, dtype=torch.float32, device=dev)
        self.s_rd = torch.empty(Kn * B, 1, 1, C, dtype=self.dtype, device=dev)

    def sample(self, x, n_samples, mode='sample', eps=None, seed=None):
        """K depth hypotheses for one input: the down path once, K draws from the bottleneck in one adn_vae_sample
        call, the up path once per draw with the encoder's skips shared, mean / std by adn_sample_stats.

        Eval mode only (BatchNorm from running statistics; nothing is written back).  ``mode='mean'`` decodes z = mu
        (K = 1).  Noise: ``eps`` [K, B, L] is used as given; ``seed`` keys a reproducible draw; otherwise the draw
        continues the engine's host counter (``vae_draws`` advances by K).  Runs on a buffer set of its own per
        (input shape, K): the activations, tape and captured steps of a trainer on this engine are left alone."""
        if self.module.training:
            raise RuntimeError('UnetGeneratorVAE.sample runs in eval mode only (BatchNorm from running statistics): '
                               'call model.eval() first')
        if mode not in ('sample', 'mean'):
            raise ValueError(f"sample mode must be 'sample' or 'mean', got {mode!r}")
        if not x.is_cuda:
            raise RuntimeError('UnetGeneratorVAE.sample needs a HIP device tensor (libadn has no CPU path)')
        Kn = 1 if mode == 'mean' else int(n_samples)
        if Kn < 1:
            raise ValueError(f'n_samples must be >= 1, got {n_samples}')
        if eps is not None and mode == 'sample':
            want = (Kn, x.shape[0], self.vae.latent_dim)
            if tuple(eps.shape) != want:
                raise RuntimeError(f'eps has shape {tuple(eps.shape)}, {Kn} draws of this bottleneck are {want}')
            eps = eps.to(device=x.device, dtype=torch.float32).contiguous()
        else:
            eps = None
        x = x.contiguous().float()
        if not self._bound():
            self.bind_parameters()
        prev_key = self._shape_key
        flags = (self.weights_dirty, self.s2_fresh, self._packed_version)
        self._sample_k = Kn
        try:
            with torch.no_grad():
                return self._sample(x, Kn, mode, eps, seed)
        finally:
            self._sample_k = 0
            # back to the set the caller was on (a trainer reads its KL and replays its captured step there), with its
            # packed operands as valid as they were: sampling packed its own and changed no parameter
            if prev_key is not None and prev_key != self._shape_key and self._shape_enter(prev_key):
                self.weights_dirty, self.s2_fresh, self._packed_version = flags

    def _sample(self, x, Kn, mode, eps, seed):
        self._begin(x)
        if seed is not None:
            call_seed = (int(seed) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
        else:
            call_seed = self.vae_seed ^ (((self.vae_draws + 1) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF)
            if eps is None and mode == 'sample':
                self.vae_draws += Kn
        B, n, L = self.B, self.n, self.levels
        # ---- down path, once, BatchNorm in eval form
        for i in range(n):
            self._down_conv(i, x, False)
        # ---- bottleneck: mu / logvar once, K draws, the innermost rd operand for all K * B rows
        fp = [self._flat_slice(self.flat_p, p) for p in self._vae_params()]
        K.vae_sample(self.vae_h, *fp, call_seed, eps, self.vae_mu, self.vae_logvar, self.s_eps, self.s_z, self.vae_kl_img,
                     self.vae_kl, self.s_rd, mode=K.VAE_MEAN if mode == 'mean' else K.VAE_DRAW)
        # ---- up path: forward()'s walk per draw, at batch B, skips shared; the eval affines once for all draws
        for lv in L[1:]:
            self._eval_affine(lv['u'])
        l0 = L[0]
        out = torch.empty(Kn * B, 2 * l0['hs'], 2 * l0['ws'], l0['cu_out'], dtype=torch.float32, device=x.device)
        for k in range(Kn):
            rows = slice(k * B, (k + 1) * B)
            for i in reversed(range(n)):
                in0, in1 = (self.s_rd[rows], None) if i == n - 1 else self._up_inputs(i)
                self._up_conv(i, in0, in1, out[rows], False, affine=False)
        samples = self._nchw(out)
        samples = samples.view(Kn, B, *samples.shape[1:])
        mean, std = torch.empty_like(samples[0]), torch.empty_like(samples[0])
        K.sample_stats(samples, mean, std)
        return SampleResult(samples, mean, std, self.vae_mu.clone(), self.vae_logvar.clone(), self.vae_kl[0].clone(),
                            self.s_eps.clone())


class SampleResult(NamedTuple):
    """What ``sample`` returns: f32 device tensors the caller owns."""
    samples: torch.Tensor        # [K, B, C, H, W] depth hypotheses
    mean: torch.Tensor           # [B, C, H, W] per-pixel mean over the K hypotheses
    std: torch.Tensor            # [B, C, H, W] per-pixel unbiased std (0 for K = 1)
    mu: torch.Tensor             # [B, L]
    logvar: torch.Tensor         # [B, L]
    kl: torch.Tensor             # 0-dim, the batch-mean KL
    eps: torch.Tensor            # [K, B, L] the noise that was used (zeros for mode='mean')


class _CVAEFunction(torch.autograd.Function):
    """torch.autograd bridge: ``depth, kl = model(x); (crit(depth, gt) + w * kl).backward()`` reaches every used
    parameter; the unused BatchNorms are not inputs, so their gradients stay None as in the reference."""

    @staticmethod
    def forward(ctx, x, engine, training, *params):
        ctx.engine = engine
        out = engine.forward(x, training)
        return out.clone(), engine.vae_kl[0].clone()

    @staticmethod
    def backward(ctx, gout, gkl):
        eng = ctx.engine
        g_kl = gkl.reshape(1).float().contiguous() if gkl is not None else torch.zeros(1, device=gout.device)
        eng.g_kl, eng.loss_acc = g_kl, None
        try:
            eng.backward(gout)
        finally:
            eng.g_kl = None
        grads = tuple(eng.grad_view(p) for p, _, _ in eng.param_meta)
        return (None, None, None) + grads


def run_cvae(engine, x, training):
    """(depth [B, 1, H, W] f32, kl 0-dim f32): differentiable in training mode under grad, plain values otherwise."""
    if not engine._bound():
        engine.bind_parameters()
    needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p, _, _ in engine.param_meta)
    if needs_grad and training:
        return _CVAEFunction.apply(x, engine, training, *[p for p, _, _ in engine.param_meta])
    with torch.no_grad():
        out = engine.forward(x, training).clone()
        return out, engine.vae_kl[0].clone()


class CVAETrainer(FusedTrainer):
    """Fused train_cvae.py step (:438-478): forward, masked depth loss (gt > 0), + kl_weight * kl, backward,
    clip_grad_norm_(1.0), optimizer.  ``step`` returns (total loss 0-dim device tensor, prediction); ``kl`` holds the
    step's KL.  The noise of a step is keyed by the device-side step count, so eager, hipGraph and launch-plan steps
    draw the same eps for the same seed."""

    def __init__(self, engine, criterion='Combined', l1_weight=0.5, silog_weight=0.5, silog_lambda=0.5, max_depth=30.0,
                 optimizer='AdamW', lr=0.002, kl_weight=1e-4, mask_mode='gt0', **kw):
        if kw.get('ddp') is not None:
            raise NotImplementedError('the cVAE trainer is single-GPU (the DataParallel KL average is not wired)')
        super().__init__(engine, criterion, l1_weight, silog_weight, silog_lambda, max_depth=max_depth,
                         optimizer=optimizer, lr=lr, mask_mode=mask_mode, **kw)
        self.kl_weight = float(kl_weight)

    @property
    def kl(self):
        return self.engine.vae_kl[0]

    def _setup(self, dev):
        super()._setup(dev)
        self.kl_w = torch.full((1,), self.kl_weight, dtype=torch.float32, device=dev)

    def _step_impl(self, audio, gt):
        eng = self.engine
        self._ensure_setup(audio.device)
        eng.step_counter, eng.g_kl, eng.loss_acc = self.state, self.kl_w, self.loss
        try:
            return super()._step_impl(audio, gt)
        finally:
            eng.step_counter, eng.g_kl, eng.loss_acc = None, None, None

    def _full_params(self):
        return list(self.engine.module.parameters())

    def state_dict(self):
        """torch.optim format over ALL of model.parameters() (what the reference's optimizer holds): the unused
        BatchNorms are listed in param_groups and carry no state."""
        from . import optim_state
        sd = super().state_dict()
        full = self._full_params()
        pos = {id(p): i for i, p in enumerate(full)}
        out = optim_state._torch_optimizer(self.opt_kind, full, self.lr, self.betas, self.eps,
                                           self.weight_decay).state_dict()
        out['state'] = {pos[id(p)]: sd['state'][i] for i, (p, _, _) in enumerate(self.engine.param_meta)
                        if i in sd['state']}
        return out

    def load_state_dict(self, sd, device):
        from . import optim_state
        eng = self.engine
        if not eng._bound():
            eng.bind_parameters()
        if optim_state.is_torch_format(sd) and len(sd['param_groups']) == 1:
            ids = list(sd['param_groups'][0]['params'])
            full = self._full_params()
            if len(ids) == len(full):
                pos = {id(p): i for i, p in enumerate(full)}
                keep = [ids[pos[id(p)]] for p, _, _ in eng.param_meta]
                sd = {'state': {k: sd['state'][k] for k in keep if k in sd['state']},
                      'param_groups': [dict(sd['param_groups'][0], params=keep)]}
        super().load_state_dict(sd, device)
