"""What the fused trainers share, none of it about one model: capture / replay of a fixed-shape step (GraphedStep), the
optimizer half of a step (OptimTail), and the single-output trainer of the U-Net and DoubleConv engines (FusedTrainer).
"""
from __future__ import annotations

import torch

from . import _lib
from . import kernels as K


class GraphedStep:
    """Launch-overhead removal of a fixed-shape step (a few hundred libadn launches, nothing synchronising with the
    host): after ``after_steps`` eager steps it is captured over static input buffers, either into ONE hipGraph
    (``enable_graph``) or as a launch plan, the list of prebuilt ctypes calls that ``_lib.replay`` walks
    (``_plan_after``), and replayed from then on.  Subclasses implement ``_step_impl(*inputs)`` (inputs may be None)
    and return device tensors that stay valid across replays; ``engine`` has weights_dirty / s2_fresh / pin_buffers, and,
    where it keeps packed copies of its parameters, _packed_version / _version_sum() / resync_mirror() (FlatParamEngine).
    Setting ``_plan, _plan_after = None, None`` drops a plan: the step is eager again and can be re-armed."""
    _graph = _graph_after = _plan = _plan_after = None
    _calls = 0

    def enable_graph(self, after_steps=3):
        self._graph_after = after_steps

    def _capture_ok(self):
        """Gate of the capture (not of the step count): a trainer that wants its first steps eager overrides it."""
        return True

    def _graphed(self, *inputs):
        self._calls += 1
        eng = self.engine
        versions = getattr(eng, '_version_sum', None)       # (an engine that packs no operand copies tracks no versions)
        if (self._plan is not None or self._graph is not None) and versions is not None \
                and eng._packed_version != versions():
            # somebody changed the parameters from outside since the engine last packed them (load_state_dict, an
            # in-place edit, a torch.optim step): the captured step holds the pack decisions of the step it was
            # recorded from (no re-cast of the bf16 mirror, T2 operands read from it) and would run on the old
            # operands.  Drop it; this very call captures again, over a mirror re-cast here, once, so that the new
            # capture records the same fast path (not a re-cast on every replay).
            self._graph = self._plan = None
            eng.resync_mirror()
        if self._plan is not None or self._graph is not None:
            for buf, t in zip(self._g_in, inputs):
                if (buf is None) != (t is None) or (buf is not None and buf.shape != t.shape):
                    return self._step_impl(*inputs)      # another batch shape: eager, on that shape's own buffer set
            for buf, t in zip(self._g_in, inputs):
                if buf is not None:
                    buf.copy_(t)
            if self._plan is not None:
                _lib.replay(self._plan)
            else:
                self._graph.replay()
            # the replayed optimizer step changes the weights behind Python's back: restore the engine's
            # "operands are stale" flags after every replay (an eval forward in between clears them)
            self.engine.weights_dirty, self.engine.s2_fresh = self._post_flags
            return self._g_out
        plan = self._plan_after is not None and self._calls > self._plan_after
        if (plan or (self._graph_after is not None and self._calls > self._graph_after)) and self._capture_ok():
            self._g_in = [None if t is None else t.contiguous().float().clone() for t in inputs]
            if plan:
                _lib.RECORD = []
                try:
                    self._g_out = self._step_impl(*self._g_in)
                    self._plan = _lib.RECORD
                finally:
                    _lib.RECORD = None
            else:
                torch.cuda.synchronize()
                self._graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._graph):
                    self._g_out = self._step_impl(*self._g_in)
            self.engine.pin_buffers()                    # the capture holds raw pointers into this shape's buffer set
            self._post_flags = (self.engine.weights_dirty, self.engine.s2_fresh)
            if not plan:
                self._graph.replay()        # a graph capture only records: run the step once for real
            return self._g_out
        return self._step_impl(*inputs)

    def _shape_scratch(self, key, make):
        """The trainer's scratch of one batch shape, built by ``make()`` on first use and never freed: a captured step
        holds raw pointers into it, and an eager step on another batch shape in between (a ragged last batch) must not
        hand those blocks back to the allocator."""
        sets = self.__dict__.setdefault('_scratch_sets', {})
        if key not in sets:
            sets[key] = make()
        return sets[key]


class OptimTail(GraphedStep):
    """The optimizer half of a fused step, the same for every trainer: hyper-parameters, lazily allocated state
    (``state`` = [step, 1 - beta1^step, 1 - beta2^step, grad norm, ...] f64, the two moments, ``norm_ws``), the
    data-parallel reducer, the checkpoint format, and ``_apply``: clip + optimizer + the engine's stale-operand flags.
    A trainer differs in ``_optim_offset`` / ``_optim_meta`` (what is optimised) and ``_attach_reducer``."""
    OPT = {'AdamW': 0, 'Adam': 1, 'SGD': 2}
    _ready = False
    _flat_id = None
    _captured_hyper = None
    _optim_offset = 0           # the optimised range is [offset:] of every flat buffer

    def _init_optim(self, engine, optimizer, lr, betas, eps, weight_decay, clip_norm, ddp):
        self.engine = engine
        self.opt_kind = self.OPT[optimizer]
        self.lr, self.betas, self.eps = float(lr), betas, float(eps)
        if weight_decay is None:                                           # torch defaults (train.py passes only lr)
            weight_decay = 0.01 if optimizer == 'AdamW' else 0.0
        self.weight_decay = float(weight_decay)
        self.clip_norm = clip_norm
        self.ddp = ddp                    # ddp.GradientAllReducer: one process per GPU, DataParallel semantics

    def enable_graph(self, after_steps=3):
        """Capture the whole step into one hipGraph after ``after_steps`` eager steps (fixed batch shape).  Not
        combined with the data-parallel reducer, whose collectives are host-side calls."""
        if self.ddp is not None:
            raise RuntimeError('graph capture of the step is only wired for single-process training')
        super().enable_graph(after_steps)

    def _hyper(self):
        """What adn_grad_norm / adn_optimizer_step take BY VALUE: a captured step has these frozen inside it."""
        return (self.lr, tuple(self.betas), self.eps, self.weight_decay, self.clip_norm)

    def _graphed(self, *inputs):
        """A hipGraph / launch plan replays the optimizer's by-value arguments of the step it was captured from, so a
        captured step whose hyper-parameters changed since (a per-epoch learning-rate schedule: ``trainer.lr = ...``) is
        dropped here and captured again by this very call, with the new values."""
        captured = self._graph is not None or self._plan is not None
        if captured and self._hyper() != self._captured_hyper:
            self._graph = self._plan = None
            captured = False
        out = super()._graphed(*inputs)
        if not captured and (self._graph is not None or self._plan is not None):
            self._captured_hyper = self._hyper()
        return out

    def _optim_meta(self):
        """(param, offset, numel) of the parameters the reference's optimizer holds, in its order."""
        return self.engine.param_meta

    def _attach_reducer(self):
        self.ddp.attach(self.engine)

    def _setup(self, dev):
        """Fresh optimizer state for the engine's current flat buffers."""
        eng = self.engine
        if not eng._bound():
            eng.bind_parameters()
        f64 = dict(dtype=torch.float64, device=dev)
        self.state = torch.zeros(8, **f64)
        self.norm_ws = torch.empty(1024 + 8, **f64)
        self.exp_avg = torch.zeros_like(eng.flat_p)
        self.exp_avg_sq = torch.zeros_like(eng.flat_p)
        self._flat_id = eng.flat_p.data_ptr()
        self.bucket_norm = None
        if self.ddp is not None:
            self._attach_reducer()
            if self.clip_norm is not None and eng.flat_g.is_cuda:
                self.bucket_norm = self.ddp.enable_bucket_norm()      # sums of squares per reduced bucket (ddp.finish)
        self._ready = True

    def _ensure_setup(self, dev):
        """First step, or the engine re-bound its flat buffers: the moments must match them."""
        eng = self.engine
        if not self._ready or self._flat_id != (eng.flat_p.data_ptr() if eng.flat_p is not None else None):
            self._setup(dev)

    def state_dict(self):
        """The checkpoint's 'optimizer' / 'optimizer_state_dict' entry in ``torch.optim`` format (optim_state.py): what
        ``torch.optim.AdamW(model.parameters(), ...).state_dict()`` would hold after the same steps, so the reference's
        ``optimizer.load_state_dict`` (train_binaural_attention.py:361) reads it and vice versa."""
        from . import optim_state
        eng = self.engine
        if not eng._bound():
            eng.bind_parameters()
        step = int(self.state[0].item()) if self._ready else 0
        return optim_state.export_state(self._optim_meta(), eng._view, self.exp_avg if self._ready else None,
                                        self.exp_avg_sq if self._ready else None, step, self.opt_kind, self.lr,
                                        self.betas, self.eps, self.weight_decay)

    def load_state_dict(self, sd, device):
        """Restore a ``torch.optim`` state dict (written by this class or by the reference's torch optimizer over the
        same parameters); the flat layout of round 1 ('exp_avg' / 'exp_avg_sq' / 'step')
        is re-sliced parameter by parameter (its alignment was 4 elements, today's is 8) or rejected."""
        from . import optim_state
        self._setup(device)
        if optim_state.is_torch_format(sd):
            step, group = optim_state.import_state(sd, self._optim_meta(), self.engine._view, self.exp_avg,
                                                   self.exp_avg_sq)
            optim_state.adopt_group(self, group)
            self._set_step(step)
        elif 'exp_avg' in sd:
            step = optim_state.import_legacy_flat(sd, self.engine.param_meta, self.exp_avg, self.exp_avg_sq)
            self._set_step(step)

    def _set_step(self, step):
        """state = [step, 1 - beta1^step, 1 - beta2^step, ...] (adn_optimizer_step advances all three)."""
        self.state[0] = float(step)
        self.state[1] = 1.0 - self.betas[0] ** step
        self.state[2] = 1.0 - self.betas[1] ** step

    def _finish_loss(self, finish, workspace, pix, sums, stats, pix_global, weights, terms):
        """Second half of a fused loss pass (``finish`` = adn_*_loss_finish): block sums in ``workspace`` -> ``sums`` ->
        weighted ``terms``.  ``stats`` is the tuple of statistics the family's finish takes in front of the global pixel
        count (may be empty).  Under the data-parallel reducer the sums are finished locally, all-reduced and finished
        again (one global-batch loss, as under DataParallel), and the reducer is armed for the backward pass."""
        if self.ddp is None:
            finish(workspace, pix, sums, *stats, pix_global, *weights, terms)
            return
        finish(workspace, pix, sums, *(None,) * len(stats), pix_global, *(0.0,) * len(weights), None)
        self.ddp.all_reduce_loss_stats(sums)
        finish(None, pix, sums, *stats, pix_global, *weights, terms)
        self.ddp.begin_backward()

    def _apply(self, fused_norm=False):
        """Clip and step flat_p[offset:] from flat_g[offset:].  The total norm comes from what the weight-gradient
        kernels left in the engine's ``sq_all`` (``fused_norm``), from the reducer's per-bucket sums, or from a pass
        over the gradients."""
        eng, off = self.engine, self._optim_offset
        g, clip = eng.flat_g[off:], self.clip_norm is not None
        if fused_norm:
            K.grad_norm_ranges(g, eng.norm_ranges, eng.sq_all, float(self.clip_norm), self.state, self.norm_ws)
        elif clip and self.bucket_norm is not None:
            K.grad_norm_ranges(g, None, self.bucket_norm, float(self.clip_norm), self.state, self.norm_ws)
        elif clip:
            K.grad_norm(g, float(self.clip_norm), self.state, self.norm_ws)
        K.optimizer_step(eng.flat_p[off:], g, self.exp_avg[off:], self.exp_avg_sq[off:], self.opt_kind, self.lr,
                         self.betas[0], self.betas[1], self.eps, self.weight_decay, clip, self.state,
                         bf16_copy=eng.flat_w16[off:] if eng.flat_w16 is not None else None)
        eng.weights_dirty = True
        # the optimizer just refreshed the bf16 S2 operands; a partly stepped mirror (the rest is still valid) is
        # re-cast as a whole to keep that path simple
        eng.s2_fresh = eng.flat_w16 is not None and off == 0


class FusedTrainer(OptimTail):
    """One fused training step: forward + masked loss + backward + (all-reduce) + clip + optimizer.

    Mirrors the hot loop of /root/reference/train.py:633-693 (and train_binaural_attention.py:394-433 when
    ``clip_norm`` is None and ``mask_mode`` is 'gt0'; train_rgb_depth.py:355-362 with criterion 'DepthLoss',
    where l1_weight / silog_weight carry lambda_l1 / lambda_smooth).  ``engine`` is a UNetEngine or a DCEngine
    (both expose forward / backward / flat_p / flat_g / flat_w16).  Everything stays on device; ``step`` returns the
    loss as a 0-dim device tensor (call .item() to reproduce the reference's per-step host sync).
    """
    CRIT = {'L1': 0, 'SIlog': 1, 'Combined': 2, 'DepthLoss': 3}

    def __init__(self, engine, criterion='Combined', l1_weight=0.5, silog_weight=0.5, silog_lambda=0.5,
                 max_depth=30.0, optimizer='AdamW', lr=0.002, betas=(0.9, 0.999), eps=1e-8, weight_decay=None,
                 clip_norm=1.0, mask_mode='ne0', ddp=None):
        if ddp is not None and not getattr(engine, 'batch_only', True):
            raise NotImplementedError('data-parallel training is wired for norm="batch" without dropout only '
                                      '(norm="instance" / "none" and use_dropout=True train on one GPU)')
        self._init_optim(engine, optimizer, lr, betas, eps, weight_decay, clip_norm, ddp)
        self.criterion = self.CRIT[criterion]
        self.l1_weight, self.silog_weight, self.silog_lambda = float(l1_weight), float(silog_weight), float(silog_lambda)
        self.scale = float(max_depth) if engine.depth_norm else 1.0       # train.py:649-652
        self.mask_mode = 0 if mask_mode == 'ne0' else 1
        self._gout_valid, self._last_pred_gt = True, None

    def enable_launch_plan(self, after_steps=3):
        """Record the step's launches once (after ``after_steps`` eager steps) and replay the prebuilt ctypes
        calls afterwards: the low-overhead eager mode used with the data-parallel reducer, whose collectives
        stay ordinary torch.distributed calls inside the plan."""
        self._plan_after = after_steps

    def _capture_ok(self):
        return self._ready          # the step that allocates the optimizer state and the loss buffers stays eager

    _g_audio = property(lambda self: self._g_in[0])       # the static input buffers of the captured step
    _g_gt = property(lambda self: self._g_in[1])

    def _setup(self, dev):
        super()._setup(dev)
        f64 = dict(dtype=torch.float64, device=dev)
        self.stats = torch.zeros(4, **f64)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.loss_ws = torch.empty(4096 + 8, **f64)
        self.gout = None
        if getattr(self.engine, 'uses_dropout', False):
            self.engine.step_counter = self.state     # device step count: a replayed step draws fresh dropout masks

    def step(self, audio, gt):
        return self._graphed(audio, gt)

    def loss_gradient(self):
        """d loss / d prediction of the last step (diagnostics, tests).  When the fused loss kernel wrote the gradient of
        the output's PRE-activation instead (adn_loss_finish_dz), it is recomputed here from that step's statistics."""
        if not self._gout_valid:
            pred, gt = self._last_pred_gt
            K.loss_finish(pred, gt, self.scale, self.mask_mode, 1e-6, self.stats, self.criterion, self.l1_weight,
                          self.silog_weight, self.silog_lambda, None, self.gout)
            self._gout_valid = True
        return self.gout

    def _step_impl(self, audio, gt):
        eng = self.engine
        self._ensure_setup(audio.device)
        pred = eng.forward(audio, True)
        gt = gt.contiguous().float()
        dz_ready = False
        self.gout = self._shape_scratch(tuple(pred.shape), lambda: torch.empty_like(pred))
        if self.criterion == 3:       # DepthLoss: unmasked L1 + total variation (train_rgb_depth.py:43-87)
            K.l1tv_stats(pred, gt, self.stats, self.loss_ws)
            if self.ddp is not None:
                _lib.record_py(lambda: self.ddp.all_reduce_loss_stats(self.stats))
            K.l1tv_finish(pred, gt, self.stats, self.ddp.world_size if self.ddp is not None else 1, self.l1_weight,
                          self.silog_weight, self.loss, self.gout)
        else:
            K.loss_stats(pred, gt, self.scale, self.mask_mode, 1e-6, self.stats, self.loss_ws)
            if self.ddp is not None:      # one global-batch loss, as under DataParallel
                _lib.record_py(lambda: self.ddp.all_reduce_loss_stats(self.stats))
            # U-Net with the thin last layer: the loss kernel writes d loss / d pre-activation and the bias gradient itself
            target = eng.dz_target() if self.criterion <= 2 else None
            if target is not None:
                dz, bias_grad, final_act = target
                K.loss_finish_dz(pred, gt, self.scale, self.mask_mode, 1e-6, self.stats, self.criterion, self.l1_weight,
                                 self.silog_weight, self.silog_lambda, self.loss, dz, final_act, bias_grad, self.loss_ws)
                dz_ready = True
            else:
                K.loss_finish(pred, gt, self.scale, self.mask_mode, 1e-6, self.stats, self.criterion, self.l1_weight,
                              self.silog_weight, self.silog_lambda, self.loss, self.gout)
        if self.ddp is not None:
            _lib.record_py(self.ddp.begin_backward)
        # single process: the weight-gradient kernels leave their share of the total norm behind (no pass over flat_g);
        # under the reducer the norm is that of the all-reduced gradients, taken afterwards
        fused = (self.clip_norm is not None and self.ddp is None and eng.supports_fused_norm
                 and eng.sq_all is not None)
        self._gout_valid, self._last_pred_gt = not dz_ready, (pred, gt)
        eng.backward(self.gout, fused_norm=fused, dz_ready=dz_ready)
        if self.ddp is not None:
            _lib.record_py(self.ddp.finish)
        self._apply(fused_norm=fused)
        return self.loss[0], pred
