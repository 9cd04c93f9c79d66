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
        for lv in self.levels:
            for key in ('down', 'up'):
                w = lv[key].weight
                X, Y = w.shape[0], w.shape[1]
                master = self._flat_slice(self.flat_p, w)
                ypad = lv[key + '_ypad']
                if ypad != Y:
                    K.pack_weights(master, X, Y, T, lv[key + '_s2'], None, y_pad=ypad)
                elif T == torch.float32:
                    lv[key + '_s2'] = master                       # channels_last memory == S2 operand
        # source of the T2 pack: the bf16 mirror when the fused optimizer has just written ALL of it (half the read
        # traffic, identical values); the f32 masters otherwise
        src = self.flat_w16 if (T == torch.bfloat16 and fresh) else self.flat_p
        K.pack_t2_multi(src, self.t2_table, self.t2_layers, self.t2_blocks, T, self.t2_all)
        self.weights_dirty = False
        self.s2_fresh = False
        self._packed_version = self._version_sum()

    # ------------------------------------------------------------------ buffers
    def _prepare(self, x):
        if not self._bound():
            self.bind_parameters()
        B, Cin, H, W = x.shape
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
        key = self._buffer_key(x)
        if self._shape_enter(key):
            return
        dev, T = x.device, self.dtype
        f32 = dict(dtype=torch.float32, device=dev)
        ws_bytes = 16
        epc = 8 if T == torch.bfloat16 else 4          # elements per 16-byte chunk
        l0 = self.levels[0]
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
        self.edge_path = (T == torch.bfloat16 and self.n1_path and n >= 2 and Cin == 2
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
        self.x_nhwc = None if self.edge_path else torch.empty(B, H, W, self.cin_pad, dtype=T, device=dev)
        batching_patch = (T == torch.bfloat16 and not os.environ.get('ADN_NO_WGRAD_BATCH')
                          and not os.environ.get('ADN_NO_PATCH_BATCH'))
        pshape_d, pshape_u = {}, {}
        for i, lv in enumerate(self.levels):
            dw, uw = lv['down'].weight, lv['up'].weight
            cd_in, cd_out = dw.shape[1], dw.shape[0]
            cu_in, cu_out = uw.shape[0], uw.shape[1]
            hs, wsz = H >> (i + 1), W >> (i + 1)
            lv.update(hs=hs, ws=wsz, cd_in=cd_in, cd_out=cd_out, cu_in=cu_in, cu_out=cu_out)
            cd_in_p = self.cin_pad if i == 0 else cd_in          # gathered channels as the kernels see them
            cu_out_p = self.cout_pad if i == 0 else cu_out
            lv.update(down_ypad=cd_in_p, up_ypad=cu_out_p)
            act = lambda c, h=hs, w_=wsz: torch.empty(B, h, w_, c, dtype=T, device=dev)
            lv['ad'] = act(cd_out) if i < n - 1 else None
            lv['rd'] = None if self._no_skip(i) or (i == 0 and self.skip0_leaky) else act(cd_out)
            # the skip operand as its readers get it (level 0 with skip0_leaky: before the ReLU, see _skip_relu)
            lv['skip'] = lv['ad'] if i == 0 and self.skip0_leaky else lv['rd']
            lv['Gd'] = act(cd_out)
            lv['zd'] = act(cd_out) if lv['bn_d'] is not None or lv['in_d'] else None
            big = lambda c, h=hs, w_=wsz: torch.empty(B, 2 * h, 2 * w_, c, dtype=T, device=dev)
            if i > 0:
                lv['zu'] = big(cu_out) if lv['bn_u'] is not None or lv['in_u'] else None
                lv['ru'] = big(cu_out)
                lv['keep_u'] = torch.ones(B, 2 * hs, 2 * wsz, cu_out, dtype=torch.uint8, device=dev) if lv['drop'] else None
                lv['Gu'] = big(cu_out)
            else:
                lv['out'] = torch.empty(B, 2 * hs, 2 * wsz, cu_out, **f32)
                lv['dz0'] = torch.empty(B, 1, 2 * hs, 2 * wsz, **f32) if self.edge_path else big(cu_out_p)
            # packed weights: S2 = view of the bf16 parameter mirror (unpadded bf16 layers), own buffer when
            # padded, the f32 master itself on the exact path; T2 = slices of one flat buffer (below)
            for wk, X, Y, Yp in (('down', cd_out, cd_in, cd_in_p), ('up', cu_in, cu_out, cu_out_p)):
                if Yp != Y:
                    lv[wk + '_s2'] = torch.empty(X, 16, Yp, dtype=T, device=dev)
                elif T != torch.float32:
                    lv[wk + '_s2'] = self._flat_slice(self.flat_w16, lv[wk].weight).view(X, 16, Y)
            # GEMM plans: partial rows + workspace
            c_up0 = cd_out
            c_up1 = cu_in - cd_out
            edge0 = i == 0 and self.edge_path
            epi_d = EPI_RAW if self._vae_level(i) else (EPI_Z_STATS if lv['bn_d'] is not None else EPI_ACT)
            pd, w1 = (0, 0) if edge0 else K.igemm_query(T, GEMM_S2, B, hs, wsz, cd_in_p, 0, cd_out, [cd_out],   # Li fwd
                                                       epi=epi_d)
            if i == 0 and self.n1_path:
                pu, w2 = 0, K.convt_n1_workspace_bytes(B, hs, wsz)                                  # D0 fwd
            else:
                pu, w2 = K.igemm_query(T, GEMM_T2, B, hs, wsz, c_up0, c_up1, cu_out, [cu_out],     # Di fwd
                                        epi=EPI_Z_STATS if lv['bn_u'] is not None else (EPI_FINAL if i == 0 else EPI_ACT))
            pgu, w3 = (0, 0) if edge0 else K.igemm_query(T, GEMM_S2, B, hs, wsz, cu_out_p, 0, cu_in,   # Di dgrad
                                                         [c_up0, c_up1] if c_up1 else [c_up0], epi=EPI_BWD)
            pgd, w4 = (0, 0) if i == 0 else K.igemm_query(T, GEMM_T2, B, hs, wsz, cd_out, 0, cd_in, [cd_in], epi=EPI_BWD)  # Li dgrad
            w5 = 0 if edge0 else K.wgrad_workspace_bytes(T, B, hs, wsz, cd_out, 0, cd_in_p, 0,
                                                         cd_in if cd_in_p != cd_in else 0)
            w6 = 0 if edge0 else K.wgrad_workspace_bytes(T, B, hs, wsz, c_up0, c_up1, cu_out_p, 0,
                                                         cu_out if cu_out_p != cu_out else 0)
            if i == 0 and self.edge_path:
                pgu = K.d0_dgrad_num_partials(B, hs, wsz)
                w3 = 0
                w5 = K.thin_wgrad_workspace_bytes(B, hs, wsz, 2, 64, 0)
                w6 = K.thin_wgrad_workspace_bytes(B, hs, wsz, 1, 64, 64)
            ws_bytes = max(ws_bytes, w1, w2, w3, w4, w5, w6)
            # instance-norm statistics and the bias gradients (channel sums of dz) share the workspace
            for tag, C, px in (('d', cd_out, hs * wsz), ('u', cu_out, 4 * hs * wsz)):
                if lv['in_' + tag]:
                    ws_bytes = max(ws_bytes, K.inorm_workspace_bytes(B, px, C))
                    lv[f'mean_{tag}'] = torch.empty(B * C, **f32)
                    lv[f'istd_{tag}'] = torch.empty(B * C, **f32)
                if lv['down' if tag == 'd' else 'up'].bias is not None and not (tag == 'u' and i == 0):
                    ws_bytes = max(ws_bytes, K.channel_sum_workspace_bytes(B * px, C))
            lv.update(P_d=pd, P_u=pu, P_gu=pgu, P_gd=pgd)
            # small-image levels: their weight gradients ride in one multi-problem launch (adn_wgrad_multi)
            # patch-staged levels: candidates for the shared-split launch (see _patch_groups below)
            if batching_patch and not edge0:
                if cd_in_p == cd_in and K.wgrad_patch_batch_workspace_bytes(T, B, [(hs, wsz, cd_out, 0, cd_in_p, 0)]) >= 0:
                    pshape_d[i] = (hs, wsz, cd_out, 0, cd_in_p, 0)
                if cu_out_p == cu_out and K.wgrad_patch_batch_workspace_bytes(T, B, [(hs, wsz, c_up0, c_up1, cu_out_p, 0)]) >= 0:
                    pshape_u[i] = (hs, wsz, c_up0, c_up1, cu_out_p, 0)
            # (class of the problem -- 0 = own launch, else it rides in the multi-problem launch -- and its norm partials)
            batching = T == torch.bfloat16 and not os.environ.get('ADN_NO_WGRAD_BATCH')
            lv['wb_d'], lv['wbq_d'] = (K.wgrad_batchable(T, B, hs, wsz, cd_out, 0, cd_in_p, 0)
                                       if batching and not edge0 and cd_in_p == cd_in else (0, 0))
            lv['wb_u'], lv['wbq_u'] = (K.wgrad_batchable(T, B, hs, wsz, c_up0, c_up1, cu_out_p, 0)
                                       if batching and not edge0 and cu_out_p == cu_out else (0, 0))
            for tag, bn, C in (('d', lv['bn_d'], cd_out), ('u', lv['bn_u'], cu_out)):
                if bn is None:
                    continue
                for nm in ('mean', 'istd', 'scale', 'shift'):
                    lv[f'{nm}_{tag}'] = torch.empty(C, **f32)
                lv[f'coef_{tag}'] = torch.empty(2 * C, **f32)
                lv[f'part_{tag}'] = torch.empty((pd if tag == 'd' else pu) * 2 * C, **f32)
        # backward stats partials: the tensor BN'd at (level i, tag) receives its final gradient from
        #   tag 'u' (zu[i], i>=1): dgrad of D(i-1)  -> P_gu of level i-1
        #   tag 'd' (zd[i], 1<=i<=n-2): dgrad of L(i+1) -> P_gd of level i+1
        for i, lv in enumerate(self.levels):
            if lv['bn_u'] is not None:
                lv['bpart_u'] = torch.empty(self.levels[i - 1]['P_gu'] * 2 * lv['cu_out'], **f32)
            if lv['bn_d'] is not None:
                lv['bpart_d'] = torch.empty(self.levels[i + 1]['P_gd'] * 2 * lv['cd_out'], **f32)
        # one flat T2 buffer + the layer table of adn_pack_t2_multi
        rows, t2_off, blk = [], 0, 0
        for lv in self.levels:
            for wk in ('down', 'up'):
                w = lv[wk].weight
                X, Y = w.shape[0], w.shape[1]
                rows.append([self.offset[id(w)], X, Y, t2_off, blk])
                lv[wk + '_t2_off'] = t2_off
                t2_off += 16 * X * Y
                blk += ((X + 63) // 64) * ((Y + 63) // 64) * 16
        self.t2_all = torch.empty(t2_off, dtype=T, device=dev)
        for lv in self.levels:
            for wk in ('down', 'up'):
                w = lv[wk].weight
                o = lv[wk + '_t2_off']
                lv[wk + '_t2'] = self.t2_all[o:o + 16 * w.shape[0] * w.shape[1]]
        # The patch-staged weight gradients of consecutive wide levels share ONE launch with 1/n of the pixel splits each
        # (adn_wgrad_patch_batch: n layers then write and re-read 1/n of the f32 slabs each): the down group L3, L2, L1 goes
        # out when L1's output gradient is final, the up group D1, D2, D3 when D3's is.
        def group(shapes):
            idx = sorted(shapes)[:4]
            ok = len(idx) >= 2 and idx == list(range(idx[0], idx[0] + len(idx)))
            return idx if ok else []
        self.pb_d, self.pb_u = group(pshape_d), group(pshape_u)
        self.pshape = {('d', i): pshape_d[i] for i in self.pb_d}
        self.pshape.update({('u', i): pshape_u[i] for i in self.pb_u})
        for tag, idx in (('d', self.pb_d), ('u', self.pb_u)):
            if idx:
                ws_bytes = max(ws_bytes, K.wgrad_patch_batch_workspace_bytes(T, B, [self.pshape[(tag, i)] for i in idx]))
        self._prepare_fused_norm(B, dev)
        if self.vae is not None:
            self._prepare_vae(B, dev)
        self.t2_table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.t2_layers, self.t2_blocks = len(rows), blk
        self.workspace = torch.empty(ws_bytes // 4 + 4, **f32)
        self.red_ws = torch.empty(4096, dtype=torch.float64, device=dev)
        self.weights_dirty = True
        self._shape_key = key
        self.B = B

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
        return L[i]['skip'], (L[i + 1]['ru'] if i < self.n - 1 else None)

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
        T = self.dtype
        self.sq_all = self.norm_ranges = None
        if os.environ.get('ADN_NO_FUSED_NORM'):
            return
        counts, covered = [], set()
        for i, lv in enumerate(self.levels):
            edge0 = i == 0 and self.edge_path
            hs, wsz = lv['hs'], lv['ws']
            c_up0, c_up1 = lv['cd_out'], lv['cu_in'] - lv['cd_out']
            nd = 0 if edge0 else K.wgrad_sq_count(T, B, hs, wsz, lv['cd_out'], 0, lv['down_ypad'], 0,
                                                  lv['cd_in'] if lv['down_ypad'] != lv['cd_in'] else 0)
            nu = 0 if edge0 else K.wgrad_sq_count(T, B, hs, wsz, c_up0, c_up1, lv['up_ypad'], 0,
                                                  lv['cu_out'] if lv['up_ypad'] != lv['cu_out'] else 0)
            if lv['wb_d']:                   # a problem of the multi-problem launch runs unsplit: its own partial count
                nd = lv['wbq_d']
            if lv['wb_u']:
                nu = lv['wbq_u']
            for wk, cnt in (('down', nd), ('up', nu)):
                counts.append((lv, wk, cnt))
                if cnt:
                    covered.add(id(lv[wk].weight))
        rows = []
        for p, off, numel in self.param_meta:
            if id(p) in covered:
                continue
            for o in range(0, numel, self.NORM_ROW):
                rows.append([off + o, (min(self.NORM_ROW, numel - o) + 3) // 4 * 4])   # the tail reads zero padding
        if not covered or len(rows) > 1024:
            return
        self.sq_all = torch.zeros(sum(c for _, _, c in counts), dtype=torch.float64, device=dev)
        o = 0
        for lv, wk, cnt in counts:
            lv[wk + '_sq'] = self.sq_all[o:o + cnt] if cnt else None
            o += cnt
        self.norm_ranges = torch.tensor(rows, dtype=torch.int64, device=dev).view(-1, 2) if rows else None

    # ------------------------------------------------------------------ forward
    def forward(self, x, training):
        if not x.is_cuda:
            raise RuntimeError('UnetGenerator.forward needs a HIP device tensor (libadn has no CPU path)')
        x = x.contiguous().float()
        self._prepare(x)
        if self.weights_dirty or self._packed_version != self._version_sum():
            self._pack_weights()
        T, B, n, L, ws = self.dtype, self.B, self.n, self.levels, self.workspace
        if self.edge_path:
            self._x_in, self._x_ver = x, x._version          # the first conv and its weight gradient read x itself
        else:
            K.nchw_to_nhwc(x, self.x_nhwc)
        self._drop_active = bool(training) and self.uses_dropout
        if self._drop_active:
            self._draw_masks()
        # ---- down path
        for i, lv in enumerate(L):
            src = self.x_nhwc if i == 0 else L[i - 1]['ad']
            C, hs, wsz = lv['cd_out'], lv['hs'], lv['ws']
            bn = lv['bn_d']
            if self._vae_level(i):
                K.igemm(T, GEMM_S2, B, hs, wsz, src, None, lv['down_s2'], C, EPI_RAW, [K.Seg(C, out0=self.vae_h)], ws)
                self._vae_forward(training)
            elif i == 0 and self.edge_path:
                K.l0_forward(x, self._flat_slice(self.flat_p, lv['down'].weight), B, hs, wsz, LEAKY, lv['ad'], lv['rd'])
            elif lv['in_d']:              # raw z (+ bias) through the identity form of the ACT epilogue, then the norm
                K.igemm(T, GEMM_S2, B, hs, wsz, src, None, lv['down_s2'], C, EPI_ACT,
                        [K.Seg(C, out0=lv['zd'], bias=lv['down'].bias, slope=1.0)], ws, algo_c=lv['cd_in'])
                K.inorm_fwd(lv['zd'], B, hs * wsz, C, lv['eps_d'], LEAKY, lv['mean_d'], lv['istd_d'], lv['ad'], lv['rd'], ws)
            elif bn is None:
                K.igemm(T, GEMM_S2, B, hs, wsz, src, None, lv['down_s2'], C, EPI_ACT,
                        [K.Seg(C, out0=lv['ad'], out1=lv['rd'], bias=lv['down'].bias, slope=LEAKY)], ws,
                        algo_c=lv['cd_in'])
            elif training:
                K.igemm(T, GEMM_S2, B, hs, wsz, src, None, lv['down_s2'], C, EPI_Z_STATS,
                        [K.Seg(C, out0=lv['zd'], partials=lv['part_d'])], ws)
                self._bn_forward(lv, 'd', bn, B * hs * wsz, lv['P_d'], lv['zd'], LEAKY, lv['ad'], lv['rd'])
            else:
                K.bn_eval_affine(bn.weight, bn.bias, bn.running_mean, bn.running_var, BN_EPS, lv['scale_d'],
                                 lv['shift_d'])
                K.igemm(T, GEMM_S2, B, hs, wsz, src, None, lv['down_s2'], C, EPI_ACT,
                        [K.Seg(C, out0=lv['ad'], out1=lv['rd'], scale=lv['scale_d'], shift=lv['shift_d'],
                               slope=LEAKY)], ws)
        # ---- up path
        for i in reversed(range(n)):
            lv = L[i]
            in0, in1 = self._up_inputs(i)
            C, hs, wsz = lv['cu_out'], lv['hs'], lv['ws']
            bn = lv['bn_u']
            if i == 0:
                bias = lv['up'].bias
                fa = self.final_act
                if self.n1_path:
                    K.convt_n1_forward(T, B, hs, wsz, in0, in1, self._flat_slice(self.flat_p, lv['up'].weight), bias,
                                       fa, lv['out'], ws, relu_in0=self._skip_relu(i))
                else:
                    K.igemm(T, GEMM_T2, B, hs, wsz, in0, in1, lv['up_t2'], C, EPI_FINAL,
                            [K.Seg(C, out0=lv['out'], bias=bias, final_act=fa)], ws)
            elif lv['in_u']:
                keep = lv['keep_u'] if self._drop_active else None
                K.igemm(T, GEMM_T2, B, hs, wsz, in0, in1, lv['up_t2'], C, EPI_ACT,
                        [K.Seg(C, out0=lv['zu'], bias=lv['up'].bias, slope=1.0)], ws)
                K.inorm_fwd(lv['zu'], B, 4 * hs * wsz, C, lv['eps_u'], 0.0, lv['mean_u'], lv['istd_u'], None, lv['ru'], ws,
                            keep=keep, keep_scale=1.0 / (1.0 - self.DROP_P))
            elif bn is None:
                K.igemm(T, GEMM_T2, B, hs, wsz, in0, in1, lv['up_t2'], C, EPI_ACT, [K.Seg(C, out1=lv['ru'])], ws)
                if lv['drop'] and self._drop_active:
                    K.dropout_apply(lv['ru'], lv['keep_u'], 1.0 / (1.0 - self.DROP_P))
            elif training:
                K.igemm(T, GEMM_T2, B, hs, wsz, in0, in1, lv['up_t2'], C, EPI_Z_STATS,
                        [K.Seg(C, out0=lv['zu'], partials=lv['part_u'])], ws)
                self._bn_forward(lv, 'u', bn, B * 4 * hs * wsz, lv['P_u'], lv['zu'], 0.0, None, lv['ru'])
                if lv['drop']:            # (dropout levels are <= 8 x 8 images: an unfused pass over ru)
                    K.dropout_apply(lv['ru'], lv['keep_u'], 1.0 / (1.0 - self.DROP_P))
            else:
                K.bn_eval_affine(bn.weight, bn.bias, bn.running_mean, bn.running_var, BN_EPS, lv['scale_u'],
                                 lv['shift_u'])
                K.igemm(T, GEMM_T2, B, hs, wsz, in0, in1, lv['up_t2'], C, EPI_ACT,
                        [K.Seg(C, out1=lv['ru'], scale=lv['scale_u'], shift=lv['shift_u'])], ws)
        out = L[0]['out']                                   # [B, H, W, Cout] f32
        Cout = L[0]['cu_out']
        if Cout == 1:
            return out.view(B, 1, out.shape[1], out.shape[2])
        res = torch.empty(B, Cout, out.shape[1], out.shape[2], dtype=torch.float32, device=out.device)
        K.nhwc_to_nchw(out, res)
        return res

    # tensors up to this many elements take the one-launch finalize + apply kernels (innermost levels: the two
    # separate launches cost 6-9 us each there, launch-latency bound)
    BN_FUSED_MAX = int(os.environ.get('ADN_BN_FUSED_MAX', 1 << 20))

    def _bn_forward(self, lv, tag, bn, count, P, z, slope, out_leaky, out_relu):
        """Train-mode BatchNorm + activation of a raw conv output: statistics finalize (+ running stats) and apply."""
        track = bn.track_running_stats and bn.running_mean is not None
        C = lv[f'mean_{tag}'].numel()
        args = (lv[f'part_{tag}'], P, C, count, bn.weight, bn.bias, BN_EPS,
                BN_MOMENTUM if bn.momentum is None else bn.momentum,
                bn.running_mean if track else None, bn.running_var if track else None,
                bn.num_batches_tracked if track else None,
                lv[f'mean_{tag}'], lv[f'istd_{tag}'], lv[f'scale_{tag}'], lv[f'shift_{tag}'])
        if count * C <= self.BN_FUSED_MAX and C % 32 == 0:
            K.bn_fwd_fused(*args, z, count, slope, out_leaky, out_relu)
        else:
            K.bn_fwd_finalize(*args)
            K.bn_act(z, count, C, lv[f'scale_{tag}'], lv[f'shift_{tag}'], slope, out_leaky, out_relu)

    def _bn_backward(self, lv, tag, bn, count, P, g, z):
        """BatchNorm backward of the tensor BN'd at (level, tag): dgamma / dbeta + dz in place of g."""
        C = lv[f'mean_{tag}'].numel()
        dg, db = self._flat_slice(self.flat_g, bn.weight), self._flat_slice(self.flat_g, bn.bias)
        if count * C <= self.BN_FUSED_MAX and C % 32 == 0:
            K.bn_bwd_fused(lv[f'bpart_{tag}'], P, C, count, dg, db, g, z, count, lv[f'scale_{tag}'], lv[f'mean_{tag}'],
                           lv[f'istd_{tag}'])
        else:
            K.bn_bwd_finalize(lv[f'bpart_{tag}'], P, C, count, dg, db, lv[f'coef_{tag}'])
            K.bn_bwd_apply(g, z, count, C, lv[f'scale_{tag}'], lv[f'mean_{tag}'], lv[f'istd_{tag}'], lv[f'coef_{tag}'])

    # ------------------------------------------------------------------ backward
    def _ready(self, param):
        if self.on_grad_ready is not None:
            off = self.offset[id(param)]
            _lib.record_py(lambda: self.on_grad_ready(off))

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
        # ---- up layers, outermost first
        # (weight gradients of the small-image levels are collected and launched together: nothing inside backward reads
        #  them, and their operands stay untouched until the end of the pass)
        batch = []                        # problems of either class (kernels.wgrad_multi)
        held_u, held_d = [], []           # patch-staged groups (see _prepare: pb_u / pb_d)
        # (the reducer's gradient-ready hook wants every dW as early as possible: the same problems then go out as
        #  one-problem launches of the same entry point -- same kernel form, unsplit --, so both modes produce identical bits)
        use_batch = self.on_grad_ready is None

        def flush():
            if batch:
                K.wgrad_multi(T, B, batch)
                del batch[:]
        for i in range(n):
            lv = L[i]
            hs, wsz = lv['hs'], lv['ws']
            gscale = 1.0 / (1.0 - self.DROP_P) if lv['drop'] and self._drop_active else 1.0
            if i == 0:
                dz = lv['dz0']
            elif lv['in_u']:
                K.inorm_bwd(lv['Gu'], lv['zu'], lv['mean_u'], lv['istd_u'], B, 4 * hs * wsz, lv['cu_out'], gscale, ws)
                dz = lv['Gu']
            elif lv['bn_u'] is None:
                dz = lv['Gu']                             # no norm: the masked gradient is dz
                if gscale != 1.0:
                    K.dropout_apply(dz, None, gscale)
            else:
                self._bn_backward(lv, 'u', lv['bn_u'], B * 4 * hs * wsz, L[i - 1]['P_gu'], lv['Gu'], lv['zu'])
                dz = lv['Gu']
                if gscale != 1.0:                         # BatchNorm backward is linear in g: the factor rides behind it
                    bn = lv['bn_u']
                    for t in (dz, self._flat_slice(self.flat_g, bn.weight), self._flat_slice(self.flat_g, bn.bias)):
                        K.dropout_apply(t, None, gscale)
            if i > 0 and lv['up'].bias is not None:       # (instance: every transposed conv has a bias)
                K.channel_sum(dz, B * 4 * hs * wsz, lv['cu_out'], lv['cu_out'], self._flat_slice(self.flat_g, lv['up'].bias), ws)
            in0, in1 = self._up_inputs(i)
            # (ref is only compared with 0: the LeakyReLU copy of level 0 gives the same mask as the ReLU copy)
            segs = [] if self._no_skip(i) else [K.Seg(lv['cd_out'], out0=lv['Gd'], ref=lv['skip'], slope=0.0)]
            if i < n - 1:
                nx = L[i + 1]
                if nx['bn_u'] is None:
                    segs.append(K.Seg(nx['cu_out'], out0=nx['Gu'], ref=nx['ru'], slope=0.0))
                else:
                    # (a dropped unit is a zero of ru: on a dropout level the mask must come from ref, never from z)
                    aff = {} if nx['drop'] else dict(scale=nx['scale_u'], shift=nx['shift_u'])
                    segs.append(K.Seg(nx['cu_out'], out0=nx['Gu'], ref=nx['ru'], slope=0.0, z=nx['zu'],
                                      mean=nx['mean_u'], istd=nx['istd_u'], partials=nx['bpart_u'], **aff))
            if i == 0 and self.edge_path:
                K.thin_wgrad(dz, in0, in1, B, hs, wsz, self._flat_slice(self.flat_g, lv['up'].weight), ws,
                             relu_plain0=self._skip_relu(i))
                self._ready(lv['up'].weight)
                K.d0_dgrad(dz, self._flat_slice(self.flat_p, lv['up'].weight), B, hs, wsz, segs[0], segs[1])
                continue
            if i in self.pb_u:
                held_u.append((hs, wsz, in0, in1, dz, None, self._flat_slice(self.flat_g, lv['up'].weight),
                               lv['up_sq'] if fused_norm else None))
                if i == self.pb_u[-1]:                    # the group's last (innermost) level: all of them in one launch
                    K.wgrad_patch_batch(T, B, held_u, ws)
                    self._ready(lv['up'].weight)
            elif lv['wb_u']:
                if len(batch) == 8:
                    flush()
                batch.append((hs, wsz, in0, in1, dz, None, self._flat_slice(self.flat_g, lv['up'].weight),
                              lv['up_sq'] if fused_norm else None))
                if not use_batch:
                    flush()
            else:
                K.wgrad(T, B, hs, wsz, in0, in1, dz, None, self._flat_slice(self.flat_g, lv['up'].weight), ws,
                        c_valid=lv['cu_out'] if (i == 0 and self.cout_pad != lv['cu_out']) else 0,
                        sq=lv['up_sq'] if fused_norm else None)
            if i not in self.pb_u:
                self._ready(lv['up'].weight)
            K.igemm(T, GEMM_S2, B, hs, wsz, dz, None, lv['up_s2'], lv['cu_in'], EPI_BWD, segs, ws,
                    algo_c=lv['cu_out'])
        if self.vae is not None:
            self._vae_backward()                          # Gd[n-1]: d h_recon -> d h
        # ---- down layers, innermost first
        for i in reversed(range(n)):
            lv = L[i]
            hs, wsz = lv['hs'], lv['ws']
            if lv['bn_d'] is not None:
                self._bn_backward(lv, 'd', lv['bn_d'], B * hs * wsz, L[i + 1]['P_gd'], lv['Gd'], lv['zd'])
            elif lv['in_d']:
                K.inorm_bwd(lv['Gd'], lv['zd'], lv['mean_d'], lv['istd_d'], B, hs * wsz, lv['cd_out'], 1.0, ws)
            if lv['down'].bias is not None:
                K.channel_sum(lv['Gd'], B * hs * wsz, lv['cd_out'], lv['cd_out'],
                              self._flat_slice(self.flat_g, lv['down'].bias), ws)
            src = self.x_nhwc if i == 0 else L[i - 1]['ad']
            if i == 0 and self.edge_path:
                if self._x_in._version != self._x_ver:
                    raise RuntimeError('the network input was modified in place between forward and backward')
                K.thin_wgrad(self._x_in, lv['Gd'], None, B, hs, wsz, self._flat_slice(self.flat_g, lv['down'].weight), ws)
            elif i in self.pb_d:
                flush()
                held_d.append((hs, wsz, lv['Gd'], None, src, None, self._flat_slice(self.flat_g, lv['down'].weight),
                               lv['down_sq'] if fused_norm else None))
                if i == self.pb_d[0]:                     # the group's last (outermost) level
                    K.wgrad_patch_batch(T, B, held_d, ws)
            elif lv['wb_d']:
                if len(batch) == 8:
                    flush()
                batch.append((hs, wsz, lv['Gd'], None, src, None, self._flat_slice(self.flat_g, lv['down'].weight),
                              lv['down_sq'] if fused_norm else None))
                if not use_batch:
                    flush()
            else:
                flush()                                   # back at the wide levels: the collected small ones go first
                K.wgrad(T, B, hs, wsz, lv['Gd'], None, src, None, self._flat_slice(self.flat_g, lv['down'].weight), ws,
                        c_valid=lv['cd_in'] if (i == 0 and self.cin_pad != lv['cd_in']) else 0,
                        sq=lv['down_sq'] if fused_norm else None)
            if i not in self.pb_d or i == self.pb_d[0]:
                self._ready(lv['down'].weight)
            if i > 0:
                pv = L[i - 1]
                acc = not self._no_skip(i - 1)            # no skip above the cVAE bottleneck: the only writer of Gd
                seg = K.Seg(pv['cd_out'], out0=pv['Gd'], ref=pv['ad'], slope=LEAKY, accumulate=acc)
                if pv['bn_d'] is not None:
                    seg = K.Seg(pv['cd_out'], out0=pv['Gd'], ref=pv['ad'], slope=LEAKY, accumulate=acc,
                                z=pv['zd'], mean=pv['mean_d'], istd=pv['istd_d'], partials=pv['bpart_d'],
                                scale=pv['scale_d'], shift=pv['shift_d'])
                K.igemm(T, GEMM_T2, B, hs, wsz, lv['Gd'], None, lv['down_t2'], lv['cd_in'], EPI_BWD, [seg], ws)
        flush()
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
