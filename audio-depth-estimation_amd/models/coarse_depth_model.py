"""Coarse depth classification model, MI355X-native mirror of /root/reference/models/coarse_depth_model.py.

Same public surface for ``model_type='unet'`` (the reference script's default): ``CoarseDepthUNet`` with its own
``DoubleConv`` / ``Down`` / ``Up`` (the reference's attribute names here are ``conv`` / ``pool_conv`` / ``up``, not
rgb_depth_model's, so the state_dict keys differ and the classes cannot be shared), the ``bin_centers`` buffer,
``set_bin_centers`` / ``predict_depth`` / ``get_num_params``, ``init_weights`` / ``init_net`` /
``define_coarse_depth_model`` (same-seed-same-weights) and the loss modules ``CoarseDepthLoss`` /
``SoftCrossEntropyLoss`` / ``FocalLoss`` / ``OrdinalRegressionLoss`` with the reference's constructor signatures.
``forward(x) -> (logits [B, n_bins, H, W], depth [B, 1, H, W])`` runs as an op tape on libadn (coarse_engine.py); the
fused coarse_engine.CoarseDepthTrainer is the fast path, the loss modules below serve the reference-style autograd loop
and ``CoarseDepthTrainer.from_criterion``.  ``DualRegressionModel`` / ``DualRegressionLoss`` (reference :857-1056, model_type
'dual_reg' of the script) are constructed directly, as the reference does; they run on dualreg_engine.py.
``CoarseWithOffsetModel`` / ``CoarseOffsetLoss`` (reference :591-850, model_type 'hybrid') are constructed directly too and
run on hybrid_engine.py.  ``CoarseDepthLite`` (reference :199-287, model_type 'lite') is constructed directly as well and
runs on coarse_engine.CoarseLiteEngine.  Functional gaps raise NotImplementedError: model_type 'lite' / 'hybrid' /
'dual_reg' through the factory, ``bilinear=False``, and an input size different from ``output_size`` (the bilinear resize of the logits / offset features; train_coarse_depth.py
always feeds images_size inputs).  ``2 <= n_bins <= 512``; back-propagating through the returned ``depth`` in the autograd
loop additionally needs ``n_bins <= 256`` (adn_bins_bwd), the fused trainer does not.
"""
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn import init

from ..dc_engine import Act, ConvBNReLU, MaxPool2, Upsample2x
from .unetbaseline_model import DataParallel, default_compute_dtype


def _inner(name):
    raise RuntimeError(f'{name} is executed by the fused libadn pipeline of its network; call the network, '
                       'not an inner block')


class DoubleConv(nn.Module):
    """Double convolution block (reference :28-44)."""

    def __init__(self, in_ch, out_ch, mid_ch=None):
        super().__init__()
        mid_ch = mid_ch or out_ch
        self.conv = nn.Sequential(
            nn.Conv2d(in_ch, mid_ch, 3, padding=1, bias=False),
            nn.BatchNorm2d(mid_ch),
            nn.ReLU(inplace=True),
            nn.Conv2d(mid_ch, out_ch, 3, padding=1, bias=False),
            nn.BatchNorm2d(out_ch),
            nn.ReLU(inplace=True),
        )

    def forward(self, x):
        _inner('DoubleConv')

    def adn_ops(self, srcs, out_name, H, W):
        dc = self.conv
        mid = Act(out_name + '.mid', dc[0].out_channels, H, W)
        out = Act(out_name, dc[3].out_channels, H, W)
        return [ConvBNReLU(srcs, dc[0], dc[1], mid), ConvBNReLU([mid], dc[3], dc[4], out)], out


class Down(nn.Module):
    """Downscaling with maxpool then double conv (reference :47-58)."""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.pool_conv = nn.Sequential(nn.MaxPool2d(2), DoubleConv(in_ch, out_ch))

    def forward(self, x):
        _inner('Down')

    def adn_ops(self, src, out_name):
        H, W = src.H // 2, src.W // 2
        if H < 1 or W < 1:
            raise RuntimeError(f'Given input size: ({src.C}x{src.H}x{src.W}). Calculated output size: '
                               f'({src.C}x{H}x{W}). Output size is too small')
        pooled = Act(out_name + '.pool', src.C, H, W)
        ops, out = self.pool_conv[1].adn_ops([pooled], out_name, H, W)
        return [MaxPool2(src, pooled)] + ops, out


class Up(nn.Module):
    """Upscaling then double conv (reference :61-83)."""

    def __init__(self, in_ch, out_ch, bilinear=True):
        super().__init__()
        if bilinear:
            self.up = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True)
            self.conv = DoubleConv(in_ch, out_ch, in_ch // 2)
        else:
            self.up = nn.ConvTranspose2d(in_ch, in_ch // 2, kernel_size=2, stride=2)
            self.conv = DoubleConv(in_ch, out_ch)

    def forward(self, x1, x2):
        _inner('Up')

    def adn_ops(self, x1, x2, out_name):
        if not isinstance(self.up, nn.Upsample):
            raise NotImplementedError('CoarseDepthUNet(bilinear=False) is not implemented (no reference caller builds it)')
        if x2.H < 2 * x1.H or x2.W < 2 * x1.W:
            raise NotImplementedError('negative padding (skip smaller than the upsampled tensor) cannot occur with '
                                      'MaxPool2d(2) encoders and is not implemented')
        up = Act(out_name + '.up', x1.C, x2.H, x2.W)
        ops, out = self.conv.adn_ops([x2, up], out_name, x2.H, x2.W)       # torch.cat([x2, x1], dim=1)
        return [Upsample2x(x1, up)] + ops, out


class CoarseDepthUNet(nn.Module):
    """UNet-based model for coarse depth classification (reference :86-192)."""

    def __init__(self, input_channels: int = 2, n_bins: int = 128, base_channels: int = 64, bilinear: bool = True,
                 output_size: int = 256):
        super().__init__()
        self.n_bins = n_bins
        self.output_size = output_size
        self.input_channels = input_channels
        factor = 2 if bilinear else 1
        self.inc = DoubleConv(input_channels, base_channels)
        self.down1 = Down(base_channels, base_channels * 2)
        self.down2 = Down(base_channels * 2, base_channels * 4)
        self.down3 = Down(base_channels * 4, base_channels * 8)
        self.down4 = Down(base_channels * 8, base_channels * 16 // factor)
        self.up1 = Up(base_channels * 16, base_channels * 8 // factor, bilinear)
        self.up2 = Up(base_channels * 8, base_channels * 4 // factor, bilinear)
        self.up3 = Up(base_channels * 4, base_channels * 2 // factor, bilinear)
        self.up4 = Up(base_channels * 2, base_channels, bilinear)
        self.outc = nn.Conv2d(base_channels, n_bins, kernel_size=1)
        self.register_buffer('bin_centers', torch.linspace(0, 1, n_bins))
        self._engine = None
        self.compute_dtype = default_compute_dtype()

    def set_bin_centers(self, bin_centers: torch.Tensor):
        """Set bin centers for depth reconstruction (in place when the shape allows: a captured step reads the buffer)."""
        if bin_centers.shape == self.bin_centers.shape:
            self.bin_centers.copy_(bin_centers.detach())
        else:
            self.bin_centers = bin_centers.to(self.bin_centers.device)

    def engine(self):
        from ..coarse_engine import CoarseDepthEngine
        if self._engine is None or self._engine.requested_dtype != self.compute_dtype:
            object.__setattr__(self, '_engine', CoarseDepthEngine(self, self.compute_dtype))
        return self._engine

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x [B, C, H, W] -> (logits [B, n_bins, H, W] f32, depth [B, 1, H, W] f32 = sum_k softmax_k * bin_centers[k]).
        In training mode under autograd both hang off one autograd node, so the reference's
        ``criterion(logits, depth, ...)['total'].backward()`` loop works."""
        from ..coarse_engine import run_coarse
        return run_coarse(self.engine(), x, self.training)

    def predict_depth(self, x: torch.Tensor, mode: str = 'soft') -> torch.Tensor:
        """'soft': expected value; anything else: centre of the argmax bin (reference :170-189).  [B, 1, H, W]."""
        if mode == 'soft':
            return self.forward(x)[1]
        from ..coarse_engine import run_coarse_hard
        return run_coarse_hard(self.engine(), x, self.training)

    def predict_distribution(self, x: torch.Tensor):
        """The per-pixel predictive distribution of the class head in one adn_coarse_decode pass (call under
        ``torch.no_grad()``): named tuple ``(mean, hard, std, entropy, confidence, argmax)``, each [B, 1, H, W] -- the
        softmax expectation (= ``forward(x)``'s depth), the centre of the first-maximum bin, the distribution's standard
        deviation over the bin centres, its entropy in nats, max_k p_k, and the first-maximum bin (int32)."""
        from ..coarse_engine import run_distribution
        return run_distribution(self.engine(), x, self.training)

    def get_num_params(self) -> int:
        return sum(p.numel() for p in self.parameters() if p.requires_grad)


class CoarseDepthLite(nn.Module):
    """Lightweight encoder-decoder for coarse depth classification (reference :199-287): five Conv2d(k4, s2, p1, bias) ->
    BatchNorm2d -> LeakyReLU(0.2), five ConvTranspose2d(k4, s2, p1, bias) -> BatchNorm2d -> ReLU without skips, a biased 3x3
    class head.  ``forward(x) -> (logits [B, n_bins, H, W], depth [B, 1, H, W])`` runs on coarse_engine.CoarseLiteEngine:
    the k4 geometries of adn_igemm with post-activation BatchNorm (dc_engine.ConvS2BNLeaky / ConvT2BNReLU), and the same
    fused loss tail as CoarseDepthUNet.  Constructed directly (``init_net(CoarseDepthLite(...), 'kaiming')`` is what the
    reference's factory does); ``torch.manual_seed(s)`` before the constructor + ``init_weights(net, 'kaiming')`` give the
    reference's weights.  The inner Sequentials only hold the parameters.  No ``predict_depth`` (the reference has none).
    Channel widths that are multiples of 64 run on the MFMA kernels; others (the default 48) are correct but take the
    generic ``direct`` form of adn_igemm."""

    def __init__(self, input_channels: int = 2, n_bins: int = 128, base_channels: int = 48, output_size: int = 256):
        super().__init__()
        self.n_bins = n_bins
        self.output_size = output_size
        self.input_channels = input_channels
        b = base_channels
        enc, c = [], input_channels
        for w in (b, b * 2, b * 4, b * 8, b * 8):
            enc += [nn.Conv2d(c, w, 4, 2, 1), nn.BatchNorm2d(w), nn.LeakyReLU(0.2, inplace=True)]
            c = w
        self.encoder = nn.Sequential(*enc)
        dec = []
        for w in (b * 8, b * 4, b * 2, b, b):
            dec += [nn.ConvTranspose2d(c, w, 4, 2, 1), nn.BatchNorm2d(w), nn.ReLU(inplace=True)]
            c = w
        self.decoder = nn.Sequential(*dec)
        self.head = nn.Conv2d(b, n_bins, 3, 1, 1)
        self.register_buffer('bin_centers', torch.linspace(0, 1, n_bins))
        self._engine = None
        self.compute_dtype = default_compute_dtype()

    def set_bin_centers(self, bin_centers: torch.Tensor):
        """Set bin centers for depth reconstruction (in place when the shape allows: a captured step reads the buffer)."""
        if bin_centers.shape == self.bin_centers.shape:
            self.bin_centers.copy_(bin_centers.detach())
        else:
            self.bin_centers = bin_centers.to(self.bin_centers.device)

    def engine(self):
        from ..coarse_engine import CoarseLiteEngine
        if self._engine is None or self._engine.requested_dtype != self.compute_dtype:
            object.__setattr__(self, '_engine', CoarseLiteEngine(self, self.compute_dtype))
        return self._engine

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x [B, C, H, W] -> (logits [B, n_bins, H, W] f32, depth [B, 1, H, W] f32).  In training mode under autograd both
        hang off one autograd node, so the reference's ``criterion(logits, depth, ...)['total'].backward()`` loop works."""
        from ..coarse_engine import run_coarse
        return run_coarse(self.engine(), x, self.training)

    def predict_distribution(self, x: torch.Tensor):
        """The per-pixel predictive distribution of the class head in one adn_coarse_decode pass (call under
        ``torch.no_grad()``): named tuple ``(mean, hard, std, entropy, confidence, argmax)``, each [B, 1, H, W] -- the
        softmax expectation (= ``forward(x)``'s depth), the centre of the first-maximum bin, the distribution's standard
        deviation over the bin centres, its entropy in nats, max_k p_k, and the first-maximum bin (int32)."""
        from ..coarse_engine import run_distribution
        return run_distribution(self.engine(), x, self.training)

    def get_num_params(self) -> int:
        return sum(p.numel() for p in self.parameters() if p.requires_grad)


class DualRegressionModel(nn.Module):
    """Pure regression model (reference :857-994): a shared encoder, a coarse regression decoder + 1x1 head, and an offset
    decoder whose features are fused with the DETACHED coarse depth ([64 + 1] -> 64 -> 32 channels, biased 3x3 convs in
    front of BatchNorm) before the 1x1 offset head.  ``forward(x) -> (coarse_depth, offset, final_depth)``, each f32
    [B, 1, H, W], final = coarse + offset.  Constructed directly (the reference's factory does not know it either,
    train_coarse_depth.py:282-288); ``torch.manual_seed(s)`` before the constructor gives the reference's weights.
    ``plane_channels``: width of the NHWC record that carries the coarse depth into the fusion conv (None: the engine's
    default, see dualreg_engine.DualRegEngine)."""

    def __init__(self, input_channels: int = 2, base_channels: int = 64, output_size: int = 256, bilinear: bool = True):
        super().__init__()
        if not bilinear:
            raise NotImplementedError('DualRegressionModel(bilinear=False) is not implemented (no reference caller builds it)')
        self.output_size = output_size
        self.input_channels = input_channels
        self.base_channels = base_channels
        factor = 2 if bilinear else 1
        self.inc = DoubleConv(input_channels, base_channels)
        self.down1 = Down(base_channels, base_channels * 2)
        self.down2 = Down(base_channels * 2, base_channels * 4)
        self.down3 = Down(base_channels * 4, base_channels * 8)
        self.down4 = Down(base_channels * 8, base_channels * 16 // factor)
        self.coarse_up1 = Up(base_channels * 16, base_channels * 8 // factor, bilinear)
        self.coarse_up2 = Up(base_channels * 8, base_channels * 4 // factor, bilinear)
        self.coarse_up3 = Up(base_channels * 4, base_channels * 2 // factor, bilinear)
        self.coarse_up4 = Up(base_channels * 2, base_channels, bilinear)
        self.coarse_head = nn.Conv2d(base_channels, 1, kernel_size=1)
        self.offset_up1 = Up(base_channels * 16, base_channels * 8 // factor, bilinear)
        self.offset_up2 = Up(base_channels * 8, base_channels * 4 // factor, bilinear)
        self.offset_up3 = Up(base_channels * 4, base_channels * 2 // factor, bilinear)
        self.offset_up4 = Up(base_channels * 2, base_channels, bilinear)
        self.offset_fusion = nn.Sequential(
            nn.Conv2d(base_channels + 1, base_channels, 3, padding=1),
            nn.BatchNorm2d(base_channels),
            nn.ReLU(inplace=True),
            nn.Conv2d(base_channels, base_channels // 2, 3, padding=1),
            nn.BatchNorm2d(base_channels // 2),
            nn.ReLU(inplace=True),
        )
        self.offset_head = nn.Conv2d(base_channels // 2, 1, kernel_size=1)
        self._init_weights()
        self._engine = None
        self.compute_dtype = default_compute_dtype()
        self.plane_channels = None

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def engine(self):
        from ..dualreg_engine import DualRegEngine
        e = self._engine
        if e is None or e.requested_dtype != self.compute_dtype or e.requested_plane != self.plane_channels:
            object.__setattr__(self, '_engine', DualRegEngine(self, self.compute_dtype, self.plane_channels))
        return self._engine

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """x [B, C, S, S] -> (coarse_depth, offset, final_depth).  In training mode under autograd all three hang off one
        autograd node, so the reference's ``criterion(*model(x), gt)[0].backward()`` loop works."""
        from ..dualreg_engine import run_dualreg
        return run_dualreg(self.engine(), x, self.training)

    def predict_depth(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward(x)[2]

    def get_num_params(self) -> int:
        return sum(p.numel() for p in self.parameters() if p.requires_grad)


class DualRegressionLoss(nn.Module):
    """L1 of the coarse depth + L1 of the final depth on gt > 0 (every pixel when none is valid) + mean |offset|
    (reference :997-1056).  Plain torch; dualreg_engine.DualRegressionTrainer.from_criterion reads the weights."""

    def __init__(self, coarse_weight: float = 1.0, final_weight: float = 1.0, offset_reg_weight: float = 0.01):
        super().__init__()
        self.coarse_weight = coarse_weight
        self.final_weight = final_weight
        self.offset_reg_weight = offset_reg_weight

    def forward(self, coarse_depth: torch.Tensor, offset: torch.Tensor, final_depth: torch.Tensor,
                target_depth: torch.Tensor) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        valid_mask = target_depth > 0
        if valid_mask.any():
            coarse_loss = F.l1_loss(coarse_depth[valid_mask], target_depth[valid_mask])
            final_loss = F.l1_loss(final_depth[valid_mask], target_depth[valid_mask])
        else:
            coarse_loss = F.l1_loss(coarse_depth, target_depth)
            final_loss = F.l1_loss(final_depth, target_depth)
        offset_reg = offset.abs().mean()
        total_loss = (self.coarse_weight * coarse_loss + self.final_weight * final_loss +
                      self.offset_reg_weight * offset_reg)
        return total_loss, {'total': total_loss, 'coarse': coarse_loss, 'final': final_loss, 'offset_reg': offset_reg}


class CoarseWithOffsetModel(nn.Module):
    """Hybrid model (reference :591-770): a shared encoder, a classification decoder + 1x1 class head whose softmax
    expectation over ``bin_centers`` is the coarse depth, and an offset decoder whose features are fused with the DETACHED
    coarse depth ([64 + 1] -> 64 -> 32 channels, biased 3x3 convs in front of BatchNorm) before the 1x1 offset head.
    ``forward(x) -> (logits [B, n_bins, H, W], coarse_depth, offset, final_depth)``, f32, final = coarse + offset.
    Constructed directly (the reference's factory does not build it, train_coarse_depth.py:290-296);
    ``torch.manual_seed(s)`` before the constructor gives the reference's weights.  ``plane_channels``: width of the NHWC
    record that carries the coarse depth into the fusion conv (None: the engine's default, see
    dualreg_engine.DualRegEngine).  ``2 <= n_bins <= 512``; back-propagating through the returned depths in the autograd
    loop additionally needs ``n_bins <= 256`` (adn_bins_bwd), the fused trainer does not."""

    def __init__(self, input_channels: int = 2, n_bins: int = 8, base_channels: int = 64, output_size: int = 256,
                 bilinear: bool = True):
        super().__init__()
        if not bilinear:
            raise NotImplementedError('CoarseWithOffsetModel(bilinear=False) is not implemented (no reference caller builds it)')
        self.n_bins = n_bins
        self.output_size = output_size
        self.input_channels = input_channels
        self.base_channels = base_channels
        factor = 2 if bilinear else 1
        self.inc = DoubleConv(input_channels, base_channels)
        self.down1 = Down(base_channels, base_channels * 2)
        self.down2 = Down(base_channels * 2, base_channels * 4)
        self.down3 = Down(base_channels * 4, base_channels * 8)
        self.down4 = Down(base_channels * 8, base_channels * 16 // factor)
        self.coarse_up1 = Up(base_channels * 16, base_channels * 8 // factor, bilinear)
        self.coarse_up2 = Up(base_channels * 8, base_channels * 4 // factor, bilinear)
        self.coarse_up3 = Up(base_channels * 4, base_channels * 2 // factor, bilinear)
        self.coarse_up4 = Up(base_channels * 2, base_channels, bilinear)
        self.coarse_head = nn.Conv2d(base_channels, n_bins, kernel_size=1)
        self.offset_up1 = Up(base_channels * 16, base_channels * 8 // factor, bilinear)
        self.offset_up2 = Up(base_channels * 8, base_channels * 4 // factor, bilinear)
        self.offset_up3 = Up(base_channels * 4, base_channels * 2 // factor, bilinear)
        self.offset_up4 = Up(base_channels * 2, base_channels, bilinear)
        self.offset_fusion = nn.Sequential(
            nn.Conv2d(base_channels + 1, base_channels, 3, padding=1),
            nn.BatchNorm2d(base_channels),
            nn.ReLU(inplace=True),
            nn.Conv2d(base_channels, base_channels // 2, 3, padding=1),
            nn.BatchNorm2d(base_channels // 2),
            nn.ReLU(inplace=True),
        )
        self.offset_head = nn.Conv2d(base_channels // 2, 1, kernel_size=1)
        self.register_buffer('bin_centers', torch.linspace(0, 1, n_bins))
        self._init_weights()
        self._engine = None
        self.compute_dtype = default_compute_dtype()
        self.plane_channels = None

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def set_bin_centers(self, bin_centers: torch.Tensor):
        """Set bin centers for depth reconstruction (in place when the shape allows: a captured step reads the buffer)."""
        if bin_centers.shape == self.bin_centers.shape:
            self.bin_centers.copy_(bin_centers.detach())
        else:
            self.bin_centers = bin_centers.to(self.bin_centers.device)

    def engine(self):
        from ..hybrid_engine import HybridEngine
        e = self._engine
        if e is None or e.requested_dtype != self.compute_dtype or e.requested_plane != self.plane_channels:
            object.__setattr__(self, '_engine', HybridEngine(self, self.compute_dtype, self.plane_channels))
        return self._engine

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """x [B, C, S, S] -> (logits, coarse_depth, offset, final_depth).  In training mode under autograd all four hang
        off one autograd node, so the reference's ``criterion(*model(x), gt, bins)[0].backward()`` loop works."""
        from ..hybrid_engine import run_hybrid
        return run_hybrid(self.engine(), x, self.training)

    def predict_depth(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward(x)[3]

    def predict_distribution(self, x: torch.Tensor):
        """The per-pixel predictive distribution of the class head in one adn_coarse_decode pass (call under
        ``torch.no_grad()``): named tuple ``(mean, hard, std, entropy, confidence, argmax, offset, final)``, each
        [B, 1, H, W]; ``mean`` is the coarse depth the offset branch read, ``final = mean + offset``."""
        from ..coarse_engine import HybridDistribution, run_distribution
        return run_distribution(self.engine(), x, self.training, HybridDistribution)

    def get_num_params(self) -> int:
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    def get_component_params(self) -> Dict:
        """Parameter count of each component (reference :750-770)."""
        count = lambda mods: sum(p.numel() for m in mods for p in m.parameters() if p.requires_grad)
        return {
            'encoder': count([self.inc, self.down1, self.down2, self.down3, self.down4]),
            'coarse_decoder': count([self.coarse_up1, self.coarse_up2, self.coarse_up3, self.coarse_up4, self.coarse_head]),
            'offset_decoder': count([self.offset_up1, self.offset_up2, self.offset_up3, self.offset_up4,
                                     self.offset_fusion, self.offset_head]),
            'total': self.get_num_params(),
        }


class CoarseOffsetLoss(nn.Module):
    """Label-smoothed cross-entropy of the class logits + L1 / L2 of the final depth + mean |offset|, all over every
    pixel (no valid mask), and |coarse - gt| for monitoring (reference :773-850).  Plain torch;
    hybrid_engine.HybridTrainer.from_criterion reads ``fused_spec()``."""

    def __init__(self, ce_weight: float = 1.0, regression_weight: float = 1.0, offset_reg_weight: float = 0.1,
                 regression_loss: str = 'l1', label_smoothing: float = 0.0):
        super().__init__()
        self.ce_weight = ce_weight
        self.regression_weight = regression_weight
        self.offset_reg_weight = offset_reg_weight
        self.ce_loss = nn.CrossEntropyLoss(label_smoothing=label_smoothing)
        self.regression_loss_type = regression_loss

    def fused_spec(self):
        """(ce_weight, regression_weight, offset_reg_weight, reg_mode, label_smoothing) as adn_hybrid_loss takes them;
        every regression_loss other than 'l1' is the reference's mse branch."""
        return (float(self.ce_weight), float(self.regression_weight), float(self.offset_reg_weight),
                'l1' if self.regression_loss_type == 'l1' else 'l2', float(self.ce_loss.label_smoothing))

    def forward(self, logits: torch.Tensor, coarse_depth: torch.Tensor, offset: torch.Tensor, final_depth: torch.Tensor,
                target_depth: torch.Tensor, target_bins: torch.Tensor) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        ce_loss = self.ce_loss(logits, target_bins)
        if self.regression_loss_type == 'l1':
            reg_loss = F.l1_loss(final_depth, target_depth)
        else:
            reg_loss = F.mse_loss(final_depth, target_depth)
        offset_reg = offset.abs().mean()
        total_loss = self.ce_weight * ce_loss + self.regression_weight * reg_loss + self.offset_reg_weight * offset_reg
        return total_loss, {'total': total_loss, 'ce': ce_loss, 'regression': reg_loss, 'offset_reg': offset_reg,
                            'coarse_l1': F.l1_loss(coarse_depth, target_depth)}


# ---- loss modules (reference :294-468); plain torch on whatever device their inputs live on ---------------------------
class OrdinalRegressionLoss(nn.Module):
    """Ordinal regression loss (reference :294-321; no caller uses it)."""

    def __init__(self, n_bins: int, weight: float = 1.0):
        super().__init__()
        self.n_bins = n_bins
        self.weight = weight

    def forward(self, logits: torch.Tensor, target_bins: torch.Tensor) -> torch.Tensor:
        N = logits.shape[1]
        idx = torch.arange(N, device=logits.device).view(1, N, 1, 1)
        labels = (idx <= target_bins.unsqueeze(1)).float()
        return self.weight * F.binary_cross_entropy_with_logits(logits, labels)


class SoftCrossEntropyLoss(nn.Module):
    """Soft cross entropy with a Gaussian label around the target bin (reference :324-355)."""

    def __init__(self, n_bins: int, sigma: float = 2.0, weight: float = 1.0):
        super().__init__()
        self.n_bins = n_bins
        self.sigma = sigma
        self.weight = weight

    def forward(self, logits: torch.Tensor, target_bins: torch.Tensor) -> torch.Tensor:
        N = logits.shape[1]
        t = target_bins.unsqueeze(1).float()
        idx = torch.arange(N, device=logits.device, dtype=torch.float32).view(1, N, 1, 1)
        soft = torch.exp(-0.5 * ((idx - t) / self.sigma) ** 2)
        soft = soft / (soft.sum(dim=1, keepdim=True) + 1e-8)
        return self.weight * -(soft * F.log_softmax(logits, dim=1)).sum(dim=1).mean()


class FocalLoss(nn.Module):
    """Focal loss (reference :358-384)."""

    def __init__(self, gamma: float = 2.0, weight: float = 1.0):
        super().__init__()
        self.gamma = gamma
        self.weight = weight

    def forward(self, logits: torch.Tensor, target_bins: torch.Tensor) -> torch.Tensor:
        N = logits.shape[1]
        ce = F.cross_entropy(logits.permute(0, 2, 3, 1).reshape(-1, N), target_bins.reshape(-1), reduction='none')
        pt = torch.exp(-ce)
        return self.weight * (((1 - pt) ** self.gamma) * ce).mean()


class CoarseDepthLoss(nn.Module):
    """Classification loss (soft CE / focal / CE) + L1 of the soft depth on the valid pixels (reference :391-468)."""

    def __init__(self, n_bins: int = 128, ce_weight: float = 1.0, regression_weight: float = 0.5, use_focal: bool = False,
                 focal_gamma: float = 2.0, use_soft_ce: bool = True, soft_ce_sigma: float = 2.0):
        super().__init__()
        self.ce_weight = ce_weight
        self.regression_weight = regression_weight
        if use_focal:
            self.ce_loss = FocalLoss(gamma=focal_gamma)
        elif use_soft_ce:
            self.ce_loss = SoftCrossEntropyLoss(n_bins, sigma=soft_ce_sigma)
        else:
            self.ce_loss = nn.CrossEntropyLoss()
        self.regression_loss = nn.L1Loss()
        self.use_soft_ce = use_soft_ce

    def fused_spec(self):
        """(ce_mode, sigma, gamma) of the classification term as adn_coarse_loss takes them."""
        if isinstance(self.ce_loss, FocalLoss):
            if self.ce_loss.weight != 1.0:
                raise NotImplementedError('FocalLoss(weight != 1) inside CoarseDepthLoss (the reference never builds it)')
            return 'focal', 2.0, float(self.ce_loss.gamma)
        if isinstance(self.ce_loss, SoftCrossEntropyLoss):
            if self.ce_loss.weight != 1.0:
                raise NotImplementedError('SoftCrossEntropyLoss(weight != 1) inside CoarseDepthLoss')
            return 'soft', float(self.ce_loss.sigma), 2.0
        return 'ce', 2.0, 2.0

    def forward(self, logits: torch.Tensor, pred_depth: torch.Tensor, target_bins: torch.Tensor,
                target_depth: torch.Tensor, valid_mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        if target_bins.dim() == 4:
            target_bins = target_bins.squeeze(1)
        if self.use_soft_ce and not isinstance(self.ce_loss, FocalLoss):
            ce_loss = self.ce_loss(logits, target_bins)
        else:
            ce_loss = self.ce_loss(logits, target_bins.long())
        if valid_mask is not None:
            reg_loss = self.regression_loss(pred_depth[valid_mask], target_depth[valid_mask])
        else:
            reg_loss = self.regression_loss(pred_depth, target_depth)
        total_loss = self.ce_weight * ce_loss + self.regression_weight * reg_loss
        return {'total': total_loss, 'ce': ce_loss, 'regression': reg_loss}


# ---- factory (reference :475-538) -------------------------------------------------------------------------------------
def init_weights(net, init_type='kaiming', init_gain=0.02):
    def init_func(m):
        classname = m.__class__.__name__
        if hasattr(m, 'weight') and (classname.find('Conv') != -1 or classname.find('Linear') != -1):
            if init_type == 'kaiming':
                init.kaiming_normal_(m.weight.data, a=0.2, mode='fan_in', nonlinearity='leaky_relu')
            elif init_type == 'xavier':
                init.xavier_normal_(m.weight.data, gain=init_gain)
            if hasattr(m, 'bias') and m.bias is not None:
                init.constant_(m.bias.data, 0.0)
        elif classname.find('BatchNorm2d') != -1:
            init.normal_(m.weight.data, 1.0, 0.02)
            init.constant_(m.bias.data, 0.0)
    net.apply(init_func)


def init_net(net, init_type='kaiming', init_gain=0.02, gpu_ids=[]):
    """Device placement, key-compatible DataParallel wrap (``module.`` prefix) and weight init (reference :491-497)."""
    if len(gpu_ids) > 0:
        assert torch.cuda.is_available()
        net.to(gpu_ids[0])
        net = DataParallel(net, gpu_ids)
    init_weights(net, init_type, init_gain)
    return net


_UNBUILT = {
    'lite': "model_type 'lite' is not built by this factory yet: construct CoarseDepthLite directly and call "
            "init_net(net, 'kaiming'), as train_coarse_depth does",
    'hybrid': "model_type 'hybrid' is not built by this factory (nor by the reference's): construct "
              "CoarseWithOffsetModel directly, as train_coarse_depth does",
    'dual_reg': "model_type 'dual_reg' is not built by this factory (nor by the reference's): construct "
                "DualRegressionModel directly, as train_coarse_depth does",
}


def define_coarse_depth_model(model_type: str = 'unet', input_channels: int = 2, n_bins: int = 128,
                              base_channels: int = 64, output_size: int = 256, init_type: str = 'kaiming',
                              gpu_ids: List[int] = []) -> nn.Module:
    """Factory with the reference's signature (:500-538)."""
    if model_type == 'unet':
        net = CoarseDepthUNet(input_channels=input_channels, n_bins=n_bins, base_channels=base_channels,
                              output_size=output_size)
    elif model_type in _UNBUILT:
        raise NotImplementedError(_UNBUILT[model_type])
    else:
        raise ValueError(f"Unknown model_type: {model_type}")
    return init_net(net, init_type, gpu_ids=gpu_ids)
