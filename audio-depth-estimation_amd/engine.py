"""Fused U-Net pipeline on libadn kernels: forward and backward (loss, clip and optimizer: trainer.FusedTrainer).

This is the MI355X-side replacement of what PyTorch dispatches for the reference's
``model(audio)`` / ``loss.backward()`` / ``clip_grad_norm_`` / ``optimizer.step()``
(/root/reference/train.py:642-691) for ``models.unetbaseline_model.UnetGenerator``.

Data layout in HBM
  * activations: NHWC, dtype f32 (exact path) or bf16 (throughput path); per down level i the raw conv
    output ``zd[i]`` (BatchNorm / InstanceNorm levels only) plus the two materialised consumer views ``ad[i]`` =
    LeakyReLU(BN(z)) (operand of the next down conv) and ``rd[i]`` = ReLU(BN(z)) (skip operand of the
    same level's transposed conv); per up level ``zu[i]`` and ``ru[i]`` = ReLU(BN(zu)).  The skip
    concat (unetbaseline_model.py:235) is virtual: the consumer GEMM reads two base pointers.
  * parameters / gradients / Adam moments: one flat f32 buffer each, parameters() order, conv weights
    in torch channels_last memory order ([X][4][4][Y]) which IS the S2 GEMM operand layout; the module's
    nn.Parameters are views into the flat buffer so state_dict()/load_state_dict()/torch.optim keep working.
  * per step the f32 master weights are cast/packed to the two GEMM operand forms (adn_pack_weights).
Gradients become final from the END of the flat buffer towards its start (outermost up layer first,
outermost down layer last), which is the bucket order of the data-parallel all-reduce (ddp.py).
"""
from __future__ import annotations

import os

import torch

from . import _lib
from . import kernels as K
from .flat import FlatParamEngine
from ._lib import EPI_ACT, EPI_BWD, EPI_FINAL, EPI_RAW, EPI_Z_STATS, GEMM_S2, GEMM_T2

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
LEAKY = 0.2

THIN, GROUP, MULTI, OWN = 'thin', 'group', 'multi', 'own'      # routes of a weight gradient (UNetEngine._emit_wgrad)


class Side:
    """One conv layer of a U-Net level as the walks see it: 'd' the strided conv, 'u' the transposed conv.
    Built per input shape by UNetEngine._prepare; the level dict holds them as lv['d'] and lv['u']."""
    __slots__ = ('tag', 'conv', 'X', 'Y', 'ypad', 'C', 'hs', 'ws', 'px',        # layer: weight [X, Y, 4, 4], Y padded to ypad
                 'norm', 'bn', 'eps', 'drop',                                   # 'batch' | 'instance' | 'none' behind it
                 'z', 'mean', 'istd', 'scale', 'shift', 'coef', 'part', 'bpart',
                 'P', 'Pg', 'Pb', 's2', 't2', 't2_off',                         # partial rows: forward, own dgrad, of bpart
                 'wshape', 'c_valid', 'route', 'trigger', 'patch_ok', 'wclass', 'wq', 'sq')

    def __init__(self, tag, conv, hs, ws, ypad, bn, inorm, eps, drop=False):
        for k in self.__slots__:
            setattr(self, k, None)
        self.tag, self.conv, self.hs, self.ws, self.bn, self.eps, self.drop = tag, conv, hs, ws, bn, eps, drop
        self.X, self.Y = conv.weight.shape[0], conv.weight.shape[1]
        self.ypad = self.Y if ypad is None else ypad              # gathered channels as the kernels see them
        self.C = self.X if tag == 'd' else self.Y                 # output channels and pixels per image
        self.px = hs * ws if tag == 'd' else 4 * hs * ws
        self.norm = 'batch' if bn is not None else 'instance' if inorm else 'none'
        self.c_valid = self.Y if self.ypad != self.Y else 0
        self.P = self.Pg = self.Pb = self.wclass = self.wq = 0
        self.route, self.trigger, self.patch_ok = OWN, False, False


class UNetEngine(FlatParamEngine):
    """Runs UnetGenerator.forward/backward through libadn.  One engine per module instance."""

    def __init__(self, module, num_downs, depth_norm, compute_dtype=torch.bfloat16):
        self.module = module
        self.n = num_downs
        self.depth_norm = bool(depth_norm)
        self.dtype = compute_dtype
        self.levels = module._adn_levels()          # list of dicts with layer objects, outermost first
        assert len(self.levels) == num_downs
        self.model_name = 'UnetGenerator'
        self.final_act = 1 if self.depth_norm else 0      # head: 0 ReLU, 1 Sigmoid, 2 identity (cVAE)
        self.vae = None                                    # cVAE bottleneck (CVAEEngine); None: the plain U-Net
        for lv in self.levels:                             # (the cVAE's level dicts carry the BatchNorm keys only)
            for k, v in (('in_d', False), ('in_u', False), ('drop', False), ('eps_d', None), ('eps_u', None)):
                lv.setdefault(k, v)
        self.uses_dropout = any(lv['drop'] for lv in self.levels)
        # norm='batch' without dropout: the configuration the thin edge kernels and the data-parallel reducer are wired for
        self.batch_only = all(lv['bn_u'] is not None for lv in self.levels[1:]) and not self.uses_dropout
        # dropout masks: keyed by (seed, level, device step counter) under a fused trainer (a hipGraph replay draws fresh
        # ones); by (seed, level, host draw count) otherwise.  The seed is the default CPU generator's, read without
        # consuming a draw.
        self.dropout_seed = torch.initial_seed()
        self.step_counter = None
        self.drop_draws = 0
        self._drop_active = False
        self._init_flat()
        self._saved = None

    DROP_P = 0.5                                           # nn.Dropout(0.5), unetbaseline_model.py:227

    def set_dropout_seed(self, seed):
        """Restart the dropout mask stream from ``seed`` (default: torch.initial_seed() at construction)."""
        self.dropout_seed = int(seed)
        self.drop_draws = 0

    def dropout_masks(self):
        """Keep masks of the last training forward as bool [B, C, H, W] tensors, outermost dropout level first."""
        return [lv['keep_u'].permute(0, 3, 1, 2).bool() for lv in self.levels if lv['drop'] and lv.get('keep_u') is not None]

    def _draw_masks(self):
        """One fresh keep mask per dropout level (adn_dropout_mask; Bernoulli(1 - p) per element)."""
        for i, lv in enumerate(self.levels):
            if lv['drop']:
                seed = self.dropout_seed * 1000003 + i * 7919
                if self.step_counter is None:
                    seed += self.drop_draws * 0x9E3779B97F4A7C15
                K.dropout_mask(lv['keep_u'], self.DROP_P, seed, self.step_counter)
        self.drop_draws += 1

    def _pack_weights(self):
        """Cast/pack the f32 master weights into the GEMM operand forms.

        S2 operands: views of the bf16 mirror (written by the fused optimizer; re-cast here only when the
        parameters were changed from outside) or the f32 master itself; padded edge layers get their own
        small pack.  T2 operands: every layer in ONE launch (adn_pack_t2_multi).
        """
        T = self.dtype
        fresh = self._mirror_fresh()
        if T == torch.bfloat16 and not fresh:
            # the whole mirror, not only the conv ranges the S2 operands view: afterwards flat_w16 == bf16(flat_p)
            # everywhere, whoever changed the parameters (a torch copy: part of a launch plan as a Python action)
            _lib.record_py(lambda: self.flat_w16.copy_(self.flat_p))
        for s in self._sides():
            if s.ypad != s.Y:
                K.pack_weights(self._flat_slice(self.flat_p, s.conv.weight), s.X, s.Y, T, s.s2, None, y_pad=s.ypad)
        # source of the T2 pack: the bf16 mirror when the fused optimizer has just written ALL of it (half the read
        # traffic, identical values); the f32 masters otherwise
        src = self.flat_w16 if (T == torch.bfloat16 and fresh) else self.flat_p
        K.pack_t2_multi(src, self.t2_table, self.t2_layers, self.t2_blocks, T, self.t2_all)
        self.weights_dirty = False
        self.s2_fresh = False
        self._packed_version = self._version_sum()

    # ------------------------------------------------------------------ buffers
    def _sides(self):
        """Every conv layer's Side, in parameter order of the level list: down then up, outermost level first."""
        return [lv[tag] for lv in self.levels for tag in ('d', 'u')]

    def _prepare(self, x):
        if not self._bound():
            self.bind_parameters()
        self._check_input(x)
        key = self._buffer_key(x)
        if self._shape_enter(key):
            return
        B, Cin, H, W = x.shape
        dev = x.device
        self._decide_edge_paths(Cin, W)
        self._build_sides(H, W)
        ws_bytes = self._query_plans(B)
        self._alloc_activations(B, H, W, dev)
        self._build_t2(dev)
        ws_bytes = max(ws_bytes, self._group_patch_launches(B))
        self._prepare_fused_norm(B, dev)
        for lv in self.levels:        # the names tests and tools read a layer's operands by; the engine reads the Side
            d, u = lv['d'], lv['u']
            lv.update(down_ypad=d.ypad, up_ypad=u.ypad, down_s2=d.s2, up_s2=u.s2, down_t2=d.t2, up_t2=u.t2,
                      down_sq=d.sq, up_sq=u.sq)
        if self.vae is not None:
            self._prepare_vae(B, dev)
        self.workspace = torch.empty(ws_bytes // 4 + 4, dtype=torch.float32, device=dev)
        self.red_ws = torch.empty(4096, dtype=torch.float64, device=dev)
        self.weights_dirty = True
        self._shape_key = key
        self.B = B

    def _check_input(self, x):
        B, _, H, W = x.shape
        n = self.n
        # (torch raises this from the first InstanceNorm2d that sees a 1 x 1 image, before the conv below it fails)
        for i, lv in enumerate(self.levels):
            if lv['in_d'] and (H >> (i + 1)) * (W >> (i + 1)) < 2:
                raise ValueError(f'Expected more than 1 spatial element when training, got input size '
                                 f'[{B}, {lv["down"].weight.shape[0]}, {H >> (i + 1)}, {W >> (i + 1)}] (InstanceNorm2d of '
                                 f'level {i}: a {H}x{W} input is too small for {n} downsamplings)')
        if H % (1 << n) or W % (1 << n):
            raise RuntimeError(f'input {H}x{W} is not divisible by 2^{n}: Kernel size can\'t be greater than '
                               f'actual input size')

    def _decide_edge_paths(self, Cin, W):
        """How the two thin outermost layers run: cin_pad / cout_pad, n1_path, edge_path, skip0_leaky, ru1_virtual_ok."""
        T, l0 = self.dtype, self.levels[0]
        epc = 8 if T == torch.bfloat16 else 4          # elements per 16-byte chunk
        # Edge layers: the first conv (Cin = 2) and the last transposed conv (Cout = 1) run on the MFMA
        # kernels with their thin channel dimension zero-padded to one 16-byte chunk.
        self.cin_pad = Cin
        if l0['down'].weight.shape[0] % 64 == 0 and Cin % epc:
            self.cin_pad = (Cin + epc - 1) // epc * epc
        cu_in0, cout0 = l0['up'].weight.shape[0], l0['up'].weight.shape[1]
        ks = 4 * epc
        self.n1_path = (cout0 == 1 and cu_in0 % 64 == 0 and (cu_in0 // 2) % ks == 0)
        self.cout_pad = epc if self.n1_path else cout0
        # Dedicated HBM-bound kernels for the thin outermost layers (csrc/edge.hip; bf16 path, the unet_256 / ngf 64
        # geometry): first conv 2 -> 64 forward + weight gradient, last transposed conv 128 -> 1 input / weight gradient.
        # They read the thin operand (network input, output gradient) as planar f32: no channel padding at all.
        self.edge_path = (T == torch.bfloat16 and self.n1_path and self.n >= 2 and Cin == 2
                          and l0['down'].weight.shape[0] == 64 and cu_in0 == 128 and l0['bn_d'] is None
                          and self.batch_only and l0['down'].bias is None
                          and (W // 2) % 32 == 0 and not os.environ.get('ADN_NO_EDGE'))
        if self.edge_path:
            self.cin_pad, self.cout_pad = Cin, cout0
        # One copy of the outermost activation: every reader of level 0's skip operand is then an edge kernel that takes
        # the LeakyReLU copy ad[0] and applies the ReLU itself (relu(leaky(v)) == relu(v) bit for bit for a positive
        # slope), so rd[0] is neither allocated nor written.  ADN_L0_TWO_COPIES=1 keeps the separate ReLU copy (A/B).
        self.skip0_leaky = (self.edge_path and self.n1_path and not self._no_skip(0)
                            and not os.environ.get('ADN_L0_TWO_COPIES'))
        # Level 1's decoder output ru[1] = ReLU(BN(zu[1])) is the widest activation of the net and all of its readers are
        # edge kernels that transform their operand in registers.  With a train-mode BatchNorm and no dropout behind D1 a
        # training forward runs only bn_fwd_finalize for D1, and every reader (last transposed conv, its weight gradient,
        # the mask of its input gradient) takes zu[1] with the BatchNorm's scale / shift and computes the value bn_act
        # would have stored: ru[1] is neither written nor read (an eval forward still writes it).
        # ADN_D1_MATERIALISED=1 keeps bn_act + the materialised ru[1] (A/B).
        l1 = self.levels[1] if self.n > 1 else None
        self.ru1_virtual_ok = bool(self.edge_path and not self._no_skip(0) and l1['bn_u'] is not None and not l1['in_u']
                                   and not l1['drop'] and not os.environ.get('ADN_D1_MATERIALISED'))
        self._ru1_virtual = False         # what the last D1 forward on this buffer set did (_up_conv); backward follows it

    def _build_sides(self, H, W):
        """The two Side records of every level: layer geometry, norm kind, weight-gradient problem."""
        for i, lv in enumerate(self.levels):
            hs, wsz = H >> (i + 1), W >> (i + 1)
            d = Side('d', lv['down'], hs, wsz, self.cin_pad if i == 0 else None, lv['bn_d'], lv['in_d'], lv['eps_d'])
            u = Side('u', lv['up'], hs, wsz, self.cout_pad if i == 0 else None, lv['bn_u'], lv['in_u'], lv['eps_u'],
                     drop=bool(lv['drop']))
            d.wshape = (hs, wsz, d.X, 0, d.ypad, 0)
            u.wshape = (hs, wsz, d.X, u.X - d.X, u.ypad, 0)        # plain operands: the skip and the level below
            if i == 0 and self.edge_path:
                d.route = u.route = THIN
            lv.update(d=d, u=u, hs=hs, ws=wsz, cd_in=d.Y, cd_out=d.X, cu_in=u.X, cu_out=u.Y)

    def _query_plans(self, B):
        """Partial-row counts of every GEMM, the class of every weight gradient, and the workspace all of them need."""
        T, n = self.dtype, self.n
        ws_bytes = 16
        batching = T == torch.bfloat16 and not os.environ.get('ADN_NO_WGRAD_BATCH')
        batching_patch = batching and not os.environ.get('ADN_NO_PATCH_BATCH')
        for i, lv in enumerate(self.levels):
            d, u = lv['d'], lv['u']
            hs, wsz = d.hs, d.ws
            c_up = [d.X, u.X - d.X] if u.X - d.X else [d.X]
            if d.route == THIN:
                u.Pg = K.d0_dgrad_num_partials(B, hs, wsz)
                need = [K.thin_wgrad_workspace_bytes(B, hs, wsz, 2, 64, 0), K.thin_wgrad_workspace_bytes(B, hs, wsz, 1, 64, 64)]
            else:
                epi_d = EPI_RAW if self._vae_level(i) else (EPI_Z_STATS if d.norm == 'batch' else EPI_ACT)
                d.P, w1 = K.igemm_query(T, GEMM_S2, B, hs, wsz, d.ypad, 0, d.X, [d.X], epi=epi_d)               # Li fwd
                u.Pg, w3 = K.igemm_query(T, GEMM_S2, B, hs, wsz, u.ypad, 0, u.X, c_up, epi=EPI_BWD)            # Di dgrad
                need = [w1, w3] + [K.wgrad_workspace_bytes(T, B, *s.wshape, s.c_valid) for s in (d, u)]
            if i == 0 and self.n1_path:
                need.append(K.convt_n1_workspace_bytes(B, hs, wsz))                                           # D0 fwd
            else:
                epi_u = EPI_Z_STATS if u.norm == 'batch' else (EPI_FINAL if i == 0 else EPI_ACT)
                u.P, w2 = K.igemm_query(T, GEMM_T2, B, hs, wsz, d.X, u.X - d.X, u.Y, [u.Y], epi=epi_u)         # Di fwd
                need.append(w2)
            if i > 0:
                d.Pg, w4 = K.igemm_query(T, GEMM_T2, B, hs, wsz, d.X, 0, d.Y, [d.Y], epi=EPI_BWD)              # Li dgrad
                need.append(w4)
            for s in (d, u):
                # instance-norm statistics and the bias gradients (channel sums of dz) share the workspace
                if s.norm == 'instance':
                    need.append(K.inorm_workspace_bytes(B, s.px, s.C))
                if s.conv.bias is not None and not (s.tag == 'u' and i == 0):
                    need.append(K.channel_sum_workspace_bytes(B * s.px, s.C))
                if s.route == THIN or s.ypad != s.Y:
                    continue
                # patch-staged levels: candidates for the shared-split launch (_group_patch_launches); small-image
                # levels: class of the problem in the multi-problem launch (0 = own launch) and its norm partials
                s.patch_ok = batching_patch and K.wgrad_patch_batch_workspace_bytes(T, B, [s.wshape]) >= 0
                if batching:
                    s.wclass, s.wq = K.wgrad_batchable(T, B, *s.wshape)
                    if s.wclass:
                        s.route = MULTI
            ws_bytes = max(ws_bytes, *need)
        return ws_bytes

    def _alloc_activations(self, B, H, W, dev):
        """Level by level: activations, packed S2 operands, norm statistics (the order the buffers have always had)."""
        T, n = self.dtype, self.n
        self.x_nhwc = None if self.edge_path else torch.empty(B, H, W, self.cin_pad, dtype=T, device=dev)
        for i, lv in enumerate(self.levels):
            d, u = lv['d'], lv['u']
            act = lambda c, k=1: torch.empty(B, k * d.hs, k * d.ws, c, dtype=T, device=dev)
            lv['ad'] = act(d.C) if i < n - 1 else None
            lv['rd'] = None if self._no_skip(i) or (i == 0 and self.skip0_leaky) else act(d.C)
            # the skip operand as its readers get it (level 0 with skip0_leaky: before the ReLU, see _skip_relu)
            lv['skip'] = lv['ad'] if i == 0 and self.skip0_leaky else lv['rd']
            lv['Gd'] = act(d.C)
            lv['zd'] = d.z = act(d.C) if d.norm != 'none' else None
            if i > 0:
                lv['zu'] = u.z = act(u.C, 2) if u.norm != 'none' else None
                lv['ru'] = act(u.C, 2)
                lv['keep_u'] = torch.ones(B, 2 * d.hs, 2 * d.ws, u.C, dtype=torch.uint8, device=dev) if u.drop else None
                lv['Gu'] = act(u.C, 2)
            else:
                lv['out'] = torch.empty(B, 2 * d.hs, 2 * d.ws, u.C, dtype=torch.float32, device=dev)
                lv['dz0'] = torch.empty(B, 1, 2 * d.hs, 2 * d.ws, dtype=torch.float32, device=dev) if self.edge_path \
                    else act(u.ypad, 2)
            # packed weights: S2 = view of the bf16 parameter mirror (unpadded bf16 layers), own buffer when
            # padded, the f32 master itself on the exact path; T2 = slices of one flat buffer (_build_t2)
            for s in (d, u):
                if s.ypad != s.Y:
                    s.s2 = torch.empty(s.X, 16, s.ypad, dtype=T, device=dev)
                else:                                              # (f32: channels_last memory == S2 operand)
                    s.s2 = self._flat_slice(self.flat_p if T == torch.float32 else self.flat_w16, s.conv.weight).view(s.X, 16, s.Y)
            self._alloc_stats(lv, B, dev)
        self._alloc_bparts(dev)

    def _alloc_stats(self, lv, B, dev):
        """Norm statistics of one level's two sides (the backward partials: _alloc_bparts)."""
        f32 = dict(dtype=torch.float32, device=dev)
        for s in (lv['d'], lv['u']):
            if s.norm == 'instance':
                s.mean, s.istd = torch.empty(B * s.C, **f32), torch.empty(B * s.C, **f32)
            elif s.norm == 'batch':
                s.mean, s.istd, s.scale, s.shift = (torch.empty(s.C, **f32) for _ in range(4))
                s.coef = torch.empty(2 * s.C, **f32)
                s.part = torch.empty(s.P * 2 * s.C, **f32)

    def _alloc_bparts(self, dev):
        """The backward partials of the tensor normed at (level i, side) come with its final gradient: 'u' (zu[i], i >= 1)
        from the dgrad of D(i-1), 'd' (zd[i], 1 <= i <= n-2) from the dgrad of L(i+1)."""
        L = self.levels
        for i, lv in enumerate(L):
            for s in (lv['u'], lv['d']):
                if s.norm == 'batch':
                    s.Pb = L[i + 1]['d'].Pg if s.tag == 'd' else L[i - 1]['u'].Pg
                    s.bpart = torch.empty(s.Pb * 2 * s.C, dtype=torch.float32, device=dev)

    def _build_t2(self, dev):
        """One flat T2 buffer + the layer table of adn_pack_t2_multi."""
        rows, t2_off, blk = [], 0, 0
        for s in self._sides():
            rows.append([self.offset[id(s.conv.weight)], s.X, s.Y, t2_off, blk])
            s.t2_off = t2_off
            t2_off += 16 * s.X * s.Y
            blk += ((s.X + 63) // 64) * ((s.Y + 63) // 64) * 16
        self.t2_all = torch.empty(t2_off, dtype=self.dtype, device=dev)
        for s in self._sides():
            s.t2 = self.t2_all[s.t2_off:s.t2_off + 16 * s.X * s.Y]
        self.t2_table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.t2_layers, self.t2_blocks = len(rows), blk

    def _group_patch_launches(self, B):
        """The patch-staged weight gradients of consecutive wide levels share ONE launch with 1/n of the pixel splits each
        (adn_wgrad_patch_batch: n layers then write and re-read 1/n of the f32 slabs each): the down group L3, L2, L1 goes
        out when L1's output gradient is final, the up group D1, D2, D3 when D3's is.  Returns the slab scratch bytes."""
        ws_bytes = 0
        for tag in ('d', 'u'):
            idx = [i for i, lv in enumerate(self.levels) if lv[tag].patch_ok][:4]
            if len(idx) < 2 or idx != list(range(idx[0], idx[0] + len(idx))):
                continue
            group = [self.levels[i][tag] for i in idx]
            for s in group:
                s.route = GROUP
            group[0 if tag == 'd' else -1].trigger = True          # the member the backward walk reaches last
            ws_bytes = max(ws_bytes, K.wgrad_patch_batch_workspace_bytes(self.dtype, B, [s.wshape for s in group]))
        return ws_bytes

    # ------------------------------------------------------------------ topology hooks (cVAE: CVAEEngine)
    def _buffer_key(self, x):
        """Key of the per-shape buffer set an input runs on (CVAEEngine.sample: a set of its own per (shape, K))."""
        return (*x.shape, x.device)

    def _vae_level(self, i):
        """Level whose down conv feeds the VAE bottleneck (raw f32 output, no activation)."""
        return self.vae is not None and i == self.n - 1

    def _no_skip(self, i):
        """Level without a skip operand: the one directly above the cVAE bottleneck."""
        return self.vae is not None and i == self.n - 2

    def _up_inputs(self, i):
        """Operands of level i's transposed conv: the skip operand of level i and the level below's ru[i+1] (a virtual
        concat).  The forward and the weight gradient of the layer both take them from here, with _skip_relu(i)."""
        L = self.levels
        if self._no_skip(i):
            return L[i + 1]['ru'], None
        if i == 0 and self._ru1_virtual:                  # zu[1], to be read with _up_bn1(0)
            return L[0]['skip'], L[1]['zu']
        return L[i]['skip'], (L[i + 1]['ru'] if i < self.n - 1 else None)

    def _up_bn1(self, i):
        """(scale, shift) when the second operand of _up_inputs(i) is the raw output of a BatchNorm + ReLU layer whose
        readers apply both on load (level 0 after a training forward with ru1_virtual_ok), else None."""
        if i == 0 and self._ru1_virtual:
            u1 = self.levels[1]['u']
            return u1.scale, u1.shift
        return None

    def _skip_relu(self, i):
        """True when the first operand of _up_inputs(i) still needs its ReLU (the reader clamps it on load)."""
        return i == 0 and self.skip0_leaky

    # ------------------------------------------------------------------ fused gradient norm
    supports_fused_norm = True
    NORM_ROW = 8192          # elements per row of adn_grad_norm_ranges

    def _prepare_fused_norm(self, B, dev):
        """clip_grad_norm_ (train.py:689) without a pass over the 54 M-element gradient: the kernel that writes a
        conv layer's final dW leaves partial sums of dW^2 in ``sq_all`` (AdnWgradDesc.sq_partials); the parameters
        without such a kernel (BatchNorm affine, bias, the thin edge layers) are covered by ``norm_ranges``."""
        self.sq_all = self.norm_ranges = None
        if os.environ.get('ADN_NO_FUSED_NORM'):
            return
        # (a problem of the multi-problem launch runs unsplit: its own partial count)
        counts = [0 if s.route == THIN else s.wq if s.wclass else K.wgrad_sq_count(self.dtype, B, *s.wshape, s.c_valid)
                  for s in self._sides()]
        covered = {id(s.conv.weight) for s, cnt in zip(self._sides(), counts) if cnt}
        rows = []
        for p, off, numel in self.param_meta:
            if id(p) in covered:
                continue
            for o in range(0, numel, self.NORM_ROW):
                rows.append([off + o, (min(self.NORM_ROW, numel - o) + 3) // 4 * 4])   # the tail reads zero padding
        if not covered or len(rows) > 1024:
            return
        self.sq_all = torch.zeros(sum(counts), dtype=torch.float64, device=dev)
        o = 0
        for s, cnt in zip(self._sides(), counts):
            s.sq = self.sq_all[o:o + cnt] if cnt else None
            o += cnt
        self.norm_ranges = torch.tensor(rows, dtype=torch.int64, device=dev).view(-1, 2) if rows else None

    # ------------------------------------------------------------------ forward
    def _begin(self, x):
        """Buffers, packed weights and the input operand of a forward walk over ``x`` (contiguous f32 NCHW)."""
        self._prepare(x)
        if self.weights_dirty or self._packed_version != self._version_sum():
            self._pack_weights()
        if self.edge_path:
            self._x_in, self._x_ver = x, x._version          # the first conv and its weight gradient read x itself
        else:
            K.nchw_to_nhwc(x, self.x_nhwc)

    def forward(self, x, training):
        if not x.is_cuda:
            raise RuntimeError('UnetGenerator.forward needs a HIP device tensor (libadn has no CPU path)')
        x = x.contiguous().float()
        self._begin(x)
        self._drop_active = bool(training) and self.uses_dropout
        if self._drop_active:
            self._draw_masks()
        for i in range(self.n):
            self._down_conv(i, x, training)
        if self.vae is not None:
            self._vae_forward(training)
        out = self.levels[0]['out']                         # [B, H, W, Cout] f32
        for i in reversed(range(self.n)):
            self._up_conv(i, *self._up_inputs(i), out, training)
        return self._nchw(out)

    def _nchw(self, out):
        """f32 [N, H, W, C] -> [N, C, H, W]: a view for one channel."""
        N, H, W, Cout = out.shape
        if Cout == 1:
            return out.view(N, 1, H, W)
        res = torch.empty(N, Cout, H, W, dtype=torch.float32, device=out.device)
        K.nhwc_to_nchw(out, res)
        return res

    def _eval_affine(self, s):
        """Eval-mode BatchNorm of a side as the scale / shift its GEMM epilogue applies."""
        bn = s.bn
        K.bn_eval_affine(bn.weight, bn.bias, bn.running_mean, bn.running_var, BN_EPS, s.scale, s.shift)

    def _down_conv(self, i, x, training):
        """Strided conv of level i with its norm: writes ad[i] (LeakyReLU, the next level's operand) and rd[i] (ReLU, the
        skip operand).  The VAE level writes the raw f32 ``vae_h`` only: the bottleneck is the caller's next call."""
        T, B, ws, lv = self.dtype, self.B, self.workspace, self.levels[i]
        s, C, ad, rd = lv['d'], lv['d'].C, lv['ad'], lv['rd']

        def gemm(epi, **seg):
            K.igemm(T, GEMM_S2, B, s.hs, s.ws, self.x_nhwc if i == 0 else self.levels[i - 1]['ad'], None, s.s2, C, epi,
                    [K.Seg(C, **seg)], ws, algo_c=s.Y)
        if self._vae_level(i):
            gemm(EPI_RAW, out0=self.vae_h)
        elif s.route == THIN:
            K.l0_forward(x, self._flat_slice(self.flat_p, s.conv.weight), B, s.hs, s.ws, LEAKY, ad, rd)
        elif s.norm == 'instance':        # raw z (+ bias) through the identity form of the ACT epilogue, then the norm
            gemm(EPI_ACT, out0=s.z, bias=s.conv.bias, slope=1.0)
            K.inorm_fwd(s.z, B, s.px, C, s.eps, LEAKY, s.mean, s.istd, ad, rd, ws)
        elif s.norm == 'none':
            gemm(EPI_ACT, out0=ad, out1=rd, bias=s.conv.bias, slope=LEAKY)
        elif training:
            gemm(EPI_Z_STATS, out0=s.z, partials=s.part)
            self._bn_forward(s, LEAKY, ad, rd)
        else:
            self._eval_affine(s)
            gemm(EPI_ACT, out0=ad, out1=rd, scale=s.scale, shift=s.shift, slope=LEAKY)

    def _up_conv(self, i, in0, in1, out, training, affine=True):
        """Transposed conv of level i over the virtual concat (in0, in1) with its norm, ReLU and dropout: writes ru[i], or
        for level 0 the head into ``out`` (f32 [B, H, W, Cout]).  ``affine=False``: the caller has issued _eval_affine."""
        T, B, ws, lv = self.dtype, self.B, self.workspace, self.levels[i]
        s, C, ru = lv['u'], lv['u'].C, lv.get('ru')
        keep = lv.get('keep_u') if s.drop and training else None
        keep_scale = 1.0 / (1.0 - self.DROP_P)

        def gemm(epi, **seg):
            K.igemm(T, GEMM_T2, B, s.hs, s.ws, in0, in1, s.t2, C, epi, [K.Seg(C, **seg)], ws)
        if i == 0 and self.n1_path:
            K.convt_n1_forward(T, B, s.hs, s.ws, in0, in1, self._flat_slice(self.flat_p, s.conv.weight), s.conv.bias,
                               self.final_act, out, ws, relu_in0=self._skip_relu(i), bn1=self._up_bn1(i))
        elif i == 0:
            gemm(EPI_FINAL, out0=out, bias=s.conv.bias, final_act=self.final_act)
        elif s.norm == 'instance':
            gemm(EPI_ACT, out0=s.z, bias=s.conv.bias, slope=1.0)
            K.inorm_fwd(s.z, B, s.px, C, s.eps, 0.0, s.mean, s.istd, None, ru, ws, keep=keep, keep_scale=keep_scale)
        elif s.norm == 'none':
            gemm(EPI_ACT, out1=ru)
        elif training:
            gemm(EPI_Z_STATS, out0=s.z, partials=s.part)
            virtual = i == 1 and self.ru1_virtual_ok      # the readers of ru[1] apply the BatchNorm + ReLU themselves
            self._bn_forward(s, 0.0, None, ru, apply=not virtual)
        else:
            if affine:
                self._eval_affine(s)
            gemm(EPI_ACT, out1=ru, scale=s.scale, shift=s.shift)
        if i == 1:
            self._ru1_virtual = bool(training) and s.norm == 'batch' and self.ru1_virtual_ok
        if keep is not None and s.norm != 'instance':     # (dropout levels are <= 8 x 8 images: an unfused pass over ru)
            K.dropout_apply(ru, keep, keep_scale)

    # tensors up to this many elements take the one-launch finalize + apply kernels (innermost levels: the two
    # separate launches cost 6-9 us each there, launch-latency bound)
    BN_FUSED_MAX = int(os.environ.get('ADN_BN_FUSED_MAX', 1 << 20))

    def _bn_one_launch(self, s):
        return self.B * s.px * s.C <= self.BN_FUSED_MAX and s.C % 32 == 0

    def _bn_forward(self, s, slope, out_leaky, out_relu, apply=True):
        """Train-mode BatchNorm + activation of a side's raw conv output: statistics finalize (+ running stats), apply.
        ``apply=False``: the finalize alone (scale / shift for readers that apply them on load)."""
        bn, count = s.bn, self.B * s.px
        track = bn.track_running_stats and bn.running_mean is not None
        args = (s.part, s.P, s.C, count, bn.weight, bn.bias, BN_EPS,
                BN_MOMENTUM if bn.momentum is None else bn.momentum,
                bn.running_mean if track else None, bn.running_var if track else None,
                bn.num_batches_tracked if track else None, s.mean, s.istd, s.scale, s.shift)
        if not apply:
            K.bn_fwd_finalize(*args)
        elif self._bn_one_launch(s):
            K.bn_fwd_fused(*args, s.z, count, slope, out_leaky, out_relu)
        else:
            K.bn_fwd_finalize(*args)
            K.bn_act(s.z, count, s.C, s.scale, s.shift, slope, out_leaky, out_relu)

    # ------------------------------------------------------------------ backward
    def _norm_backward(self, s, g):
        """d loss / d (activation input) ``g`` of a side -> d loss / d (conv output), in place: the norm's backward (BatchNorm:
        + dgamma / dbeta), the dropout factor 1 / (1 - p) of a dropout level, and the conv's bias gradient.  Returns g."""
        B, ws = self.B, self.workspace
        gscale = 1.0 / (1.0 - self.DROP_P) if s.drop and self._drop_active else 1.0
        scaled = [g]
        if s.norm == 'instance':
            K.inorm_bwd(g, s.z, s.mean, s.istd, B, s.px, s.C, gscale, ws)
            scaled = []
        elif s.norm == 'batch':
            count = B * s.px
            dg, db = self._flat_slice(self.flat_g, s.bn.weight), self._flat_slice(self.flat_g, s.bn.bias)
            if self._bn_one_launch(s):
                K.bn_bwd_fused(s.bpart, s.Pb, s.C, count, dg, db, g, s.z, count, s.scale, s.mean, s.istd)
            else:
                K.bn_bwd_finalize(s.bpart, s.Pb, s.C, count, dg, db, s.coef)
                K.bn_bwd_apply(g, s.z, count, s.C, s.scale, s.mean, s.istd, s.coef)
            scaled = [g, dg, db]                          # BatchNorm backward is linear in g: the factor rides behind it
        if gscale != 1.0:                                 # (no norm: the masked gradient is dz)
            for t in scaled:
                K.dropout_apply(t, None, gscale)
        if s.conv.bias is not None:                       # (instance: every conv has a bias)
            K.channel_sum(g, B * s.px, s.C, s.C, self._flat_slice(self.flat_g, s.conv.bias), ws)
        return g

    def _grad_seg(self, s, g, ref, slope, accumulate=False):
        """The segment by which a dgrad GEMM writes ``g``, the gradient of the activation behind side ``s`` (mask from
        ``ref``), and, in front of a BatchNorm, the partial sums of its backward statistics."""
        kw = {}
        if s.norm == 'batch':
            kw = dict(z=s.z, mean=s.mean, istd=s.istd, partials=s.bpart)
            if not s.drop:    # (a dropped unit is a zero of ru: on a dropout level the mask must come from ref, never from z)
                kw.update(scale=s.scale, shift=s.shift)
        return K.Seg(s.C, out0=g, ref=ref, slope=slope, accumulate=accumulate, **kw)

    def _ready(self, param):
        if self.on_grad_ready is not None:
            off = self.offset[id(param)]
            _lib.record_py(lambda: self.on_grad_ready(off))

    def _flush_wgrad(self, pend):
        if pend[MULTI]:
            K.wgrad_multi(self.dtype, self.B, pend[MULTI])
            del pend[MULTI][:]

    def _emit_wgrad(self, pend, s, plain0, plain1, gath, fused_norm, relu_plain0=False, bn1=None):
        """Weight gradient of side ``s`` by the route _prepare chose.  Nothing inside backward reads a dW and the operands
        stay untouched until the end of the pass, so the small-image problems are collected in ``pend[MULTI]`` (one
        adn_wgrad_multi launch per 8) and the members of a patch-staged group in ``pend[tag]`` until its trigger.  Under
        the reducer's gradient-ready hook every dW goes out as early as possible: the collected problems then leave as
        one-problem launches of the same entry point -- same kernel form, unsplit --, so both modes produce identical
        bits."""
        T, B, ws = self.dtype, self.B, self.workspace
        dw = self._flat_slice(self.flat_g, s.conv.weight)
        prob = (s.hs, s.ws, plain0, plain1, gath, None, dw, s.sq if fused_norm else None)
        ready = True
        if s.route == THIN:
            K.thin_wgrad(gath, plain0, plain1, B, s.hs, s.ws, dw, ws, relu_plain0=relu_plain0, bn1=bn1)
        elif s.route == MULTI:
            if len(pend[MULTI]) == 8:
                self._flush_wgrad(pend)
            pend[MULTI].append(prob)
            if self.on_grad_ready is not None:
                self._flush_wgrad(pend)
        else:
            if s.tag == 'd':                              # back at the wide levels: the collected small ones go first
                self._flush_wgrad(pend)
            if s.route == GROUP:
                pend[s.tag].append(prob)
                if s.trigger:                             # all of the group in one launch
                    K.wgrad_patch_batch(T, B, pend[s.tag], ws)
                ready = s.trigger
            else:
                K.wgrad(T, B, *prob[:6], dw, ws, c_valid=s.c_valid, sq=prob[7])
        if ready:
            self._ready(s.conv.weight)

    def dz_target(self):
        """Where a loss kernel may write d loss / d pre-activation of the output directly (adn_loss_finish_dz), together
        with the bias-gradient slot of the last layer: (dz [B, 1, H, W] f32, bias_grad or None, final_act), or None when
        this engine's last layer wants the padded bf16 form (then ``backward`` converts ``gout`` itself)."""
        l0 = self.levels[0]
        if not getattr(self, 'edge_path', False) or l0.get('cu_out') != 1 or os.environ.get('ADN_NO_FUSED_DZ'):
            return None
        bias = l0['up'].bias
        return l0['dz0'], (None if bias is None else self._flat_slice(self.flat_g, bias)), self.final_act

    def backward(self, gout, fused_norm=False, dz_ready=False):
        """gout: d loss / d output, f32 [B, Cout, H, W].  Fills flat_g (all parameters); with ``fused_norm`` also
        ``sq_all`` (see _prepare_fused_norm).  ``dz_ready``: the caller's loss kernel already wrote ``dz_target()``
        (gout is ignored)."""
        T, B, n, L, ws = self.dtype, self.B, self.n, self.levels, self.workspace
        fused_norm = fused_norm and self.sq_all is not None
        l0 = L[0]
        if l0['cu_out'] != 1:
            raise NotImplementedError('backward is implemented for output_nc == 1 (the depth map)')
        up0 = l0['up']
        if not dz_ready:
            gout = gout.contiguous().float()
            K.final_act_bwd(gout, l0['out'], self.final_act, l0['dz0'])
            if up0.bias is not None:
                K.sum_to_scalar(l0['dz0'], self._flat_slice(self.flat_g, up0.bias), self.red_ws)
        pend = {MULTI: [], 'd': [], 'u': []}              # weight gradients waiting for their launch (_emit_wgrad)
        # ---- up layers, outermost first
        for i in range(n):
            lv, s = L[i], L[i]['u']
            dz = lv['dz0'] if i == 0 else self._norm_backward(s, lv['Gu'])
            in0, in1 = self._up_inputs(i)
            # (ref is only compared with 0: the LeakyReLU copy of level 0 gives the same mask as the ReLU copy)
            segs = [] if self._no_skip(i) else [K.Seg(lv['cd_out'], out0=lv['Gd'], ref=lv['skip'], slope=0.0)]
            if i < n - 1:
                nx = L[i + 1]
                # (level 0 behind a forward that did not write ru[1]: no ref, d0_dgrad masks by z, scale and shift)
                segs.append(self._grad_seg(nx['u'], nx['Gu'], None if i == 0 and self._ru1_virtual else nx['ru'], 0.0))
            self._emit_wgrad(pend, s, in0, in1, dz, fused_norm, relu_plain0=self._skip_relu(i), bn1=self._up_bn1(i))
            if s.route == THIN:
                K.d0_dgrad(dz, self._flat_slice(self.flat_p, s.conv.weight), B, s.hs, s.ws, segs[0], segs[1])
            else:
                K.igemm(T, GEMM_S2, B, s.hs, s.ws, dz, None, s.s2, s.X, EPI_BWD, segs, ws, algo_c=s.Y)
        if self.vae is not None:
            self._vae_backward()                          # Gd[n-1]: d h_recon -> d h
        # ---- down layers, innermost first
        for i in reversed(range(n)):
            lv, s = L[i], L[i]['d']
            g = self._norm_backward(s, lv['Gd'])
            src = self.x_nhwc if i == 0 else L[i - 1]['ad']
            if s.route == THIN:
                if self._x_in._version != self._x_ver:
                    raise RuntimeError('the network input was modified in place between forward and backward')
                src = self._x_in
            self._emit_wgrad(pend, s, g, None, src, fused_norm)
            if i > 0:
                pv = L[i - 1]                             # (no skip above the cVAE bottleneck: the only writer of Gd)
                seg = self._grad_seg(pv['d'], pv['Gd'], pv['ad'], LEAKY, accumulate=not self._no_skip(i - 1))
                K.igemm(T, GEMM_T2, B, s.hs, s.ws, g, None, s.t2, s.Y, EPI_BWD, [seg], ws)
        self._flush_wgrad(pend)
        if self.on_grad_ready is not None:
            _lib.record_py(lambda: self.on_grad_ready(0))


class _UNetFunction(torch.autograd.Function):
    """torch.autograd bridge: parameters are inputs so that loss.backward() reaches them."""

    @staticmethod
    def forward(ctx, x, engine, training, *params):
        ctx.engine = engine
        out = engine.forward(x, training)
        return out.clone()          # engine buffers are reused by the next step

    @staticmethod
    def backward(ctx, gout):
        eng = ctx.engine
        eng.backward(gout)
        grads = tuple(eng.grad_view(p) for p, _, _ in eng.param_meta)
        return (None, None, None) + grads


def run_unet(engine, x, training):
    if not engine._bound():
        engine.bind_parameters()
    needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p, _, _ in engine.param_meta)
    if needs_grad and training:
        return _UNetFunction.apply(x, engine, training, *[p for p, _, _ in engine.param_meta])
    with torch.no_grad():
        return engine.forward(x, training).clone()


from .trainer import FusedTrainer, GraphedStep  # noqa: E402,F401  (the trainer classes live in trainer.py)
