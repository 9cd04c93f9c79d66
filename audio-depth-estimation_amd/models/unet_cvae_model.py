"""U-Net cVAE generator on libadn (drop-in for the reference's models/unet_cvae_model.py).

Same public surface: VAEBottleneck (:8-46), UnetSkipConnectionBlockVAE (:49-206), UnetGeneratorVAE (:209-305) and
define_G_cvae (:308-353).  The blocks keep the reference's named attributes and creation order (submodule first, then
downconv, downrelu, downnorm, uprelu, upnorm, upconv, vae / final_relu / dropout), so parameters() runs innermost block
first and every state_dict key, the ``module.`` prefix of the key-compatible DataParallel stand-in and the same-seed
initial weights are identical.  ``forward(x)`` returns ``(depth, kl)``; the arithmetic runs in the fused HIP pipeline of
cvae_engine.py, never layer by layer (there is no CPU path).

Supported as in the baseline: norm='batch', use_dropout=False (every reference caller); anything else is refused.
"""
import functools

import torch
import torch.nn as nn

from ..cvae_engine import CVAEEngine, run_cvae
from .unetbaseline_model import default_compute_dtype, get_norm_layer, init_net


class VAEBottleneck(nn.Module):
    """fc_mu / fc_logvar = Linear(C, L), fc_dec = Linear(L, C) on the [B, C, 1, 1] innermost map; KL averaged over B."""

    def __init__(self, in_channels: int, latent_dim: int = 128):
        super().__init__()
        self.in_channels = in_channels
        self.latent_dim = latent_dim
        self.fc_mu = nn.Linear(in_channels, latent_dim)
        self.fc_logvar = nn.Linear(in_channels, latent_dim)
        self.fc_dec = nn.Linear(latent_dim, in_channels)

    def forward(self, h):
        raise RuntimeError('VAEBottleneck is executed by the fused libadn pipeline (adn_vae_fwd) of its UnetGeneratorVAE; '
                           'call the generator')


class UnetSkipConnectionBlockVAE(nn.Module):
    """One level of the cVAE U-Net.  Holds the parameters; executed by the enclosing generator's engine."""

    def __init__(self, cfg, outer_nc, inner_nc, input_nc=None, submodule=None, outermost=False, innermost=False,
                 norm_layer=nn.BatchNorm2d, use_dropout=False, latent_dim: int = 128):
        super().__init__()
        self.outermost = outermost
        self.innermost = innermost
        self.submodule = submodule
        norm_cls = norm_layer.func if isinstance(norm_layer, functools.partial) else norm_layer
        use_bias = norm_cls == nn.InstanceNorm2d
        if input_nc is None:
            input_nc = outer_nc
        # creation order = parameter order = RNG consumption order of the reference
        self.downconv = nn.Conv2d(input_nc, inner_nc, kernel_size=4, stride=2, padding=1, bias=use_bias)
        self.downrelu = nn.LeakyReLU(0.2, True)
        self.downnorm = norm_layer(inner_nc)
        self.uprelu = nn.ReLU(True)
        self.upnorm = norm_layer(outer_nc)
        if outermost:
            self.upconv = nn.ConvTranspose2d(inner_nc * 2, outer_nc, kernel_size=4, stride=2, padding=1)
            self.use_final_relu = not cfg.dataset.depth_norm        # depth_norm: identity head (no Sigmoid)
            if self.use_final_relu:
                self.final_relu = nn.ReLU()
        elif innermost:
            self.upconv = nn.ConvTranspose2d(inner_nc, outer_nc, kernel_size=4, stride=2, padding=1, bias=use_bias)
            self.vae = VAEBottleneck(inner_nc, latent_dim=latent_dim)
        else:
            # the level right above the bottleneck gets inner_nc channels (no skip concat below it), the others 2x
            below_innermost = isinstance(submodule, UnetSkipConnectionBlockVAE) and submodule.innermost
            up_in = inner_nc if below_innermost else inner_nc * 2
            self.upconv = nn.ConvTranspose2d(up_in, outer_nc, kernel_size=4, stride=2, padding=1, bias=use_bias)
            self.use_dropout = use_dropout
            self.dropout = nn.Dropout(0.5) if use_dropout else None
        self.cfg = cfg

    def forward(self, x):
        raise RuntimeError('UnetSkipConnectionBlockVAE is executed by the fused libadn pipeline of its UnetGeneratorVAE; '
                           'call the generator, not an inner block')


class UnetGeneratorVAE(nn.Module):
    """U-Net with a VAE bottleneck at the innermost level; ``depth, kl = model(audio)``."""

    def __init__(self, cfg, input_nc, output_nc, num_downs, ngf=64, norm_layer=nn.BatchNorm2d, use_dropout=False,
                 latent_dim: int = 128):
        super().__init__()
        norm_cls = norm_layer.func if isinstance(norm_layer, functools.partial) else norm_layer
        if norm_cls is not nn.BatchNorm2d:
            raise NotImplementedError('the fused libadn cVAE pipeline implements norm="batch" (what train_cvae.py uses)')
        if use_dropout:
            raise NotImplementedError('use_dropout=True is not on the cVAE hot path (train_cvae.py passes False)')
        mk = functools.partial(UnetSkipConnectionBlockVAE, cfg, norm_layer=norm_layer, latent_dim=latent_dim)
        block = mk(ngf * 8, ngf * 8, input_nc=None, submodule=None, innermost=True)
        for _ in range(num_downs - 5):
            block = mk(ngf * 8, ngf * 8, input_nc=None, submodule=block, use_dropout=use_dropout)
        for mult in (4, 2, 1):
            block = mk(ngf * mult, ngf * mult * 2, input_nc=None, submodule=block)
        self.model = mk(output_nc, ngf, input_nc=input_nc, submodule=block, outermost=True)
        self._num_downs = num_downs
        self._depth_norm = bool(cfg.dataset.depth_norm)
        self._engine = None
        self.compute_dtype = default_compute_dtype()

    def _blocks(self):
        out, blk = [], self.model
        while blk is not None:
            out.append(blk)
            blk = blk.submodule
        return out                                   # outermost first

    def _adn_levels(self):
        levels = []
        for blk in self._blocks():
            inner = not blk.outermost and not blk.innermost
            levels.append({'down': blk.downconv, 'up': blk.upconv, 'bn_d': blk.downnorm if inner else None,
                           'bn_u': None if blk.outermost else blk.upnorm})
        return levels

    def _vae_module(self):
        return self._blocks()[-1].vae

    def unused_norms(self):
        """The BatchNorms the forward never calls: outermost downnorm and upnorm, innermost downnorm."""
        blocks = self._blocks()
        return [blocks[0].downnorm, blocks[0].upnorm, blocks[-1].downnorm]

    def _unused_params(self):
        return [p for m in self.unused_norms() for p in m.parameters()]

    def engine(self):
        if self._engine is None or self._engine.dtype != self.compute_dtype:
            object.__setattr__(self, '_engine', CVAEEngine(self, self._num_downs, self._depth_norm, self.compute_dtype))
        return self._engine

    def forward(self, input):
        """[B, input_nc, 2^n, 2^n] f32 -> (depth [B, output_nc, 2^n, 2^n] f32, kl 0-dim f32)."""
        side = 1 << self._num_downs
        if input.dim() != 4 or input.shape[2] != side or input.shape[3] != side:
            raise RuntimeError(f'UnetGeneratorVAE with {self._num_downs} downsamplings needs a {side}x{side} input: the '
                               f'VAE bottleneck reads a 1x1 innermost map (got {tuple(input.shape)})')
        return run_cvae(self.engine(), input, self.training)

    def sample(self, input, n_samples=8, mode='sample', eps=None, seed=None):
        """``n_samples`` depth hypotheses for one input in one call (eval mode): the encoder runs once, the decoder once
        per draw.  Returns a cvae_engine.SampleResult: samples [K, B, 1, H, W], their per-pixel mean / std
        [B, 1, H, W], mu / logvar [B, L], kl.  ``mode='mean'`` decodes z = mu (K = 1, std = 0); ``eps`` [K, B, L]
        replaces the draw; ``seed`` makes the draw reproducible, without it successive calls differ."""
        if not isinstance(input, torch.Tensor) or not input.is_cuda:
            raise RuntimeError('UnetGeneratorVAE.sample needs a HIP device tensor (libadn has no CPU path)')
        side = 1 << self._num_downs
        if input.dim() != 4 or input.shape[2] != side or input.shape[3] != side:
            raise RuntimeError(f'UnetGeneratorVAE with {self._num_downs} downsamplings needs a {side}x{side} input: the '
                               f'VAE bottleneck reads a 1x1 innermost map (got {tuple(input.shape)})')
        with torch.no_grad():
            return self.engine().sample(input, n_samples, mode=mode, eps=eps, seed=seed)


def define_G_cvae(cfg, input_nc, output_nc, ngf, netG, norm='batch', use_dropout=False, init_type='normal',
                  init_gain=0.02, gpu_ids=None, latent_dim: int = 128):
    """'unet_128' (7 downs) or 'unet_256' (8 downs) with the VAE bottleneck, initialised as the reference (:308-353)."""
    if gpu_ids is None:
        gpu_ids = []
    norm_layer = get_norm_layer(norm_type=norm)
    if netG == 'unet_128':
        num_downs = 7
    elif netG == 'unet_256':
        num_downs = 8
    else:
        raise NotImplementedError(f'Generator model name [{netG}] is not recognized for cVAE U-Net')
    net = UnetGeneratorVAE(cfg, input_nc, output_nc, num_downs, ngf=ngf, norm_layer=norm_layer, use_dropout=use_dropout,
                           latent_dim=latent_dim)
    return init_net(net, init_type, init_gain, gpu_ids)
