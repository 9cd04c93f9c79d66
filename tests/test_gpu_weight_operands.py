"""The bf16 weight operands of a fused step, link by link and bit for bit: the optimizer's f32 update and the bf16 mirror
it writes (adn_optimizer_step), the T2 pack of every layer in one launch (adn_pack_t2_multi), and the Python state that
decides when those copies may be trusted (weights_dirty, s2_fresh, _packed_version, GraphedStep._post_flags).

Every link is a copy, a permutation or a round-to-nearest-even cast, so apart from the optimizer arithmetic everything here
compares integer views.  References: tests/weight_operand_cases.py (checked against torch on the CPU in
tests/test_weight_operand_cases.py).

  1. adn_optimizer_step: single steps from random states against the float64 restatement of torch's update, fed the
     f32-rounded hyper-parameters the kernel receives; bar rtol 2e-5 / atol 2e-6 (the suite's optimizer bar).  Measured on
     an MI355X, maximum over every size, step count and clip setting, as a fraction of that bar / as a relative error of
     the parameters with |p| >= 1e-3:
         AdamW   0.006 of the bar / 1.19e-05        Adam    0.006 of the bar / 1.19e-05
         Adam+L2 0.011 of the bar / 2.00e-05        SGD     0.003 of the bar / 6.00e-07
     With the two moments drawn independently of each other (see ``opt_states``) the figures were 0.069, 0.077 and, for
     Adam+L2, 1.18 of the bar on ONE of 8.4 M elements, whose update was hundreds of times |p|.
     The mirror equals torch's cast of the kernel's own f32 output on every element, and on the rounding edges (ties,
     -0.0, a denormal, the largest finite value, infinities) the bits RNE prescribes.
  2. adn_pack_t2_multi == the documented index permutation for f32 -> f32, f32 -> bf16 and bf16 -> bf16, ten layers of
     both kernel forms in one launch, NaN between the masters, sentinels around the outputs.
  3. After every event that can make them stale -- construction, fused steps, replayed steps, an in-place edit, a
     load_state_dict, a torch.optim step, a switch of the shape set, sample() -- the operands a forward reads equal the
     cast / permutation of the f32 masters.
  4. An edit between two replays of a captured step: the replaying trainer ends where the eager one does.
"""
import pytest
import torch

import weight_operand_cases as wc
from weight_operand_cases import bits

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16 = torch.float32, torch.bfloat16


def K():
    from audio_depth_estimation_amd import kernels
    return kernels


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ===================================================================================== 1. adn_optimizer_step + mirror
LR, B1, B2, EPS = (wc.f32r(x) for x in (1e-2, 0.9, 0.999, 1e-8))
COEF = 0.37
PAD = 8                                     # sentinel elements either side of the stepped range
P_SENT, M_SENT, V_SENT, W_SENT = -7.25, 3.5, 11.0, 0x5A5A
SIZES = (1, 3, 4, 5, 1027, 8192 * 1024 + 1029)          # the n & 3 tail of block 0; one group past the capped grid's first pass
_measured = {}


@pytest.fixture(scope='module')
def opt_states():
    """Random (p, g, m, v) per size, drawn once: every case clones them.  v >= m^2, as the two moments of one gradient
    stream have it up to their different decay rates.  Independent draws put |m| / sqrt(v) at 1e3 and beyond in a few of
    8 M elements; the update is then hundreds of times |p|, and the f32 rounding of such an update -- torch's own f32
    optimizer has it too -- is no longer small against a bar that is relative to |p|."""
    made = {}

    def get(n):
        if n not in made:
            g_ = torch.Generator(device=DEV).manual_seed(1000 + n % 9973)
            r = lambda: torch.randn(n, generator=g_, device=DEV)
            p, g, m = r(), r(), 0.1 * r()
            made[n] = (p, g, m, m * m + (0.1 * r()) ** 2)
        return made[n]
    yield get
    made.clear()


def _framed(x, fill, dtype=F32):
    """x between PAD sentinel elements each side; the view of the middle starts 8 elements in (32 / 16 bytes: aligned)."""
    buf = torch.full((x.numel() + 2 * PAD,), fill, dtype=dtype, device=DEV)
    buf[PAD:PAD + x.numel()] = x
    return buf


def _frame_intact(buf, n, fill):
    return bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all())


def _step(p0, g, m0, v0, kind, wd, use_clip, t, lr=LR, mirror=True):
    """One adn_optimizer_step on framed clones, called on [8:8+n] slices of all five buffers (the form OptimTail._apply
    passes: flat_p[off:]).  -> (p, m, v, w16 as int16 or None), frames checked."""
    n = p0.numel()
    p, m, v, gg = _framed(p0, P_SENT), _framed(m0, M_SENT), _framed(v0, V_SENT), _framed(g, 0.0)
    w = torch.full((n + 2 * PAD,), W_SENT, dtype=torch.int16, device=DEV)
    state = torch.zeros(8, dtype=torch.float64, device=DEV)
    state[0], state[1], state[2], state[4] = t - 1, 0.123, 0.456, COEF       # [1], [2]: stale, the kernel recomputes them
    mid = slice(PAD, PAD + n)
    K().optimizer_step(p[mid], gg[mid], m[mid], v[mid], kind, lr, B1, B2, EPS, wd, use_clip, state,
                       bf16_copy=w[mid].view(BF16) if mirror else None)
    assert int(state[0].item()) == t and float(state[4].item()) == COEF
    assert _frame_intact(p, n, P_SENT) and _frame_intact(m, n, M_SENT) and _frame_intact(v, n, V_SENT)
    assert _frame_intact(w, n, W_SENT)
    if not mirror:
        assert bool((w == W_SENT).all())
    return p[mid], m[mid], v[mid], (w[mid] if mirror else None)


def _within_bar(got, ref, what, key):
    d = (got.double() - ref).abs()
    frac = float((d / (wc.OPT_ATOL + wc.OPT_RTOL * ref.abs())).max())
    big = ref.abs() >= 1e-3
    rel = float((d[big] / ref.abs()[big]).max()) if bool(big.any()) else 0.0
    old = _measured.get(key, (0.0, 0.0))
    _measured[key] = (max(old[0], frac), max(old[1], rel))
    assert frac <= 1.0, (what, frac, rel)


@pytest.mark.parametrize('kind,wd', wc.KINDS, ids=[wc.KIND_NAME[k] for k in wc.KINDS])
def test_optimizer_step_against_float64_with_mirror_bits(kind, wd, opt_states):
    for n in SIZES:
        p0, g, m0, v0 = opt_states(n)
        for use_clip in (True, False):
            for t in (1, 2, 1000):
                p, m, v, w = _step(p0, g, m0, v0, kind, wd, use_clip, t)
                pr, mr, vr = wc.optimizer_reference(p0, g, m0, v0, kind, LR, B1, B2, EPS, wc.f32r(wd),
                                                    wc.f32r(COEF) if use_clip else 1.0, t)
                what = (wc.KIND_NAME[(kind, wd)], n, use_clip, t)
                _within_bar(p, pr, what + ('p',), (kind, wd))
                if kind == 2:
                    assert torch.equal(m, m0) and torch.equal(v, v0), what          # SGD leaves the moments alone
                else:
                    _within_bar(m, mr, what + ('m',), (kind, wd))
                    _within_bar(v, vr, what + ('v',), (kind, wd))
                # the mirror: torch's round-to-nearest-even cast of the kernel's OWN f32 output, every element
                assert torch.equal(w, bits(p.to(BF16))), what
        # without a mirror pointer the same f32 results and nothing else
        p2, m2, v2, _ = _step(p0, g, m0, v0, kind, wd, True, 2, mirror=False)
        p1, m1, v1, _ = _step(p0, g, m0, v0, kind, wd, True, 2)
        assert same_bits(p1, p2) and same_bits(m1, m2) and same_bits(v1, v2), n
    frac, rel = _measured[(kind, wd)]
    print(f'\nadn_optimizer_step {wc.KIND_NAME[(kind, wd)]}: max error = {frac:.3f} of the bar, max relative error {rel:.3e}')


def test_mirror_rounding_edges():
    """SGD with g = 0 and lr = 1 leaves p as it is: the mirror of every edge pattern, in the vector groups and in the tail."""
    names = list(wc.EDGE_BITS)
    seq = [names[(j + r) % len(names)] for r in range(4) for j in range(len(names))][:39]      # each edge in several lanes
    assert len(seq) & 3 == 3 and len({(k, i & 3) for i, k in enumerate(seq[:36])}) >= 2 * len(names)
    p0 = wc.f32_from_bits([wc.EDGE_BITS[k] for k in seq], DEV)
    zero = torch.zeros_like(p0)
    p, _, _, w = _step(p0, zero, zero, zero, 2, 0.0, False, 1, lr=1.0)
    want16 = bits(p0.cpu().to(BF16))                                                  # torch's CPU cast
    for i, k in enumerate(seq):
        if k == 'nan':
            assert bool(torch.isnan(p[i])) and bool(torch.isnan(w[i:i + 1].view(BF16)).all()), i
            continue
        assert int(bits(p)[i]) == int(bits(p0)[i]), (i, k)                            # p itself unchanged, -0.0 and denormal too
        got = int(w[i]) & 0xFFFF
        assert got == wc.EDGE_BF16[k] == int(want16[i]) & 0xFFFF, (i, k, hex(got))


def test_optimizer_step_refuses_a_misaligned_mirror():
    n = 64
    p0, g = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    for shift in (1, 2, 3):                                   # 2, 4, 6 bytes off: the kernel stores the mirror 8 bytes at a time
        p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        w = torch.full((n + 8,), W_SENT, dtype=torch.int16, device=DEV)
        state = torch.zeros(8, dtype=torch.float64, device=DEV)
        with pytest.raises(RuntimeError, match='bf16_copy must be 8-byte aligned'):
            K().optimizer_step(p, g, m, v, 0, LR, B1, B2, EPS, 0.1, False, state, bf16_copy=w[shift:shift + n].view(BF16))
        torch.cuda.synchronize()
        assert torch.equal(p, p0) and not m.any() and not v.any() and not state.any() and bool((w == W_SENT).all())


# ===================================================================================== 2. adn_pack_t2_multi
def _t2_problem():
    rows, m_total, t2_total, blocks = wc.t2_table()
    g_ = torch.Generator().manual_seed(11)
    master = torch.full((m_total,), float('nan'))
    for m_off, X, Y, _, _ in rows:
        master[m_off:m_off + 16 * X * Y] = torch.randn(16 * X * Y, generator=g_)
    return rows, master.to(DEV), t2_total, blocks


@pytest.mark.parametrize('src,dst', [(F32, F32), (F32, BF16), (BF16, BF16)], ids=['f32_f32', 'f32_bf16', 'bf16_bf16'])
def test_pack_t2_multi_is_the_index_permutation(src, dst):
    rows, master, t2_total, blocks = _t2_problem()
    flat = master if src == F32 else master.to(BF16)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    itype, sent = (torch.int32, 0x5A5A5A5A) if dst == F32 else (torch.int16, 0x5A5A)
    out = torch.full((t2_total + 64,), sent, dtype=itype, device=DEV)
    want = out.clone()
    for m_off, X, Y, t2_off, _ in rows:
        w = flat[m_off:m_off + 16 * X * Y].view(X, 16, Y).to(dst)                    # (bf16 -> bf16, f32 -> f32: the same bits)
        want[t2_off:t2_off + 16 * X * Y] = bits(wc.t2_reference(w)).flatten()
    K().pack_t2_multi(flat, table, len(rows), blocks, dst, out.view(dst))
    for m_off, X, Y, t2_off, _ in rows:
        sl = slice(t2_off, t2_off + 16 * X * Y)
        bad = (out[sl] != want[sl]).nonzero().flatten()
        assert bad.numel() == 0, ((X, Y), int(bad.numel()), bad[:8].tolist())
        if src == F32:                                        # ... and what adn_pack_weights gives for this layer alone
            alone = torch.full((16 * X * Y,), sent, dtype=itype, device=DEV)
            K().pack_weights(master[m_off:m_off + 16 * X * Y], X, Y, dst, None, alone.view(dst))
            assert torch.equal(alone, out[sl]), (X, Y)
    assert torch.equal(out, want)                             # every element of every layer, and nothing past the last one


def test_pack_t2_multi_refuses_a_bf16_master_for_an_f32_pack():
    rows, master, t2_total, blocks = _t2_problem()
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    out = torch.full((t2_total,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match='cannot feed'):
        K().pack_t2_multi(master.to(BF16), table, len(rows), blocks, F32, out.view(F32))
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A).all())


# ===================================================================================== 3. operands are current
def _cfg(depth_norm=False):
    from types import SimpleNamespace
    return SimpleNamespace(dataset=SimpleNamespace(depth_norm=bool(depth_norm), max_depth=30.0))


def _unet(ngf, dtype, seed=0):
    from audio_depth_estimation_amd.models.unetbaseline_model import define_G
    torch.manual_seed(seed)
    model = define_G(_cfg(), 2, 1, ngf, 'unet_128', gpu_ids=[])
    model.compute_dtype = dtype
    return model.to(DEV)


def _batch(B, C=2, S=128, seed=6):
    g_ = torch.Generator().manual_seed(seed + B)
    return torch.rand(B, C, S, S, generator=g_).to(DEV), (30 * torch.rand(B, 1, S, S, generator=g_)).to(DEV)


def _unet_trainer(model, **kw):
    from audio_depth_estimation_amd.engine import FusedTrainer
    return FusedTrainer(model.engine(), 'Combined', 0.237, 0.637, 0.869, lr=0.002, clip_norm=1.0, **kw)


def _forward(model, x, train):
    model.train(train)
    with torch.no_grad():
        out = model(x)
    return out[0] if isinstance(out, tuple) else out


def assert_operands_current(eng, where=''):
    """What the next GEMM of a UNetEngine would read, against the f32 masters: S2 = the cast master (zero padded channels),
    T2 = its permutation, and the mirror ranges the unpadded S2 operands view."""
    T = eng.dtype
    for i, lv in enumerate(eng.levels):
        for wk in ('down', 'up'):
            w = lv[wk].weight
            X, Y = w.shape[0], w.shape[1]
            cast = eng._flat_slice(eng.flat_p, w).view(X, 16, Y).to(T)
            yp = lv[wk + '_ypad']
            s2 = lv.get(wk + '_s2')
            if s2 is not None:
                assert same_bits(s2.reshape(X, 16, yp), wc.s2_reference(cast, yp)), (where, i, wk, 'S2')
            t2 = lv.get(wk + '_t2')
            if t2 is not None:
                assert same_bits(t2.view(4, Y, 4, X), wc.t2_reference(cast)), (where, i, wk, 'T2')
            if T == BF16 and yp == Y:
                assert same_bits(eng._flat_slice(eng.flat_w16, w).view(X, 16, Y), cast), (where, i, wk, 'mirror')


def assert_mirror_current(eng, where=''):
    """flat_w16 == bf16(flat_p) over every parameter range (the alignment gaps belong to nobody)."""
    for p, off, n in eng.param_meta:
        got, want = eng.flat_w16[off:off + n], eng.flat_p[off:off + n].to(BF16)
        assert same_bits(got, want), (where, off, n, int((bits(got) != bits(want)).sum()))


def _donor_state(model, seed=21):
    """A state dict of other values for the same architecture."""
    g_ = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        v = v.detach().cpu()
        if v.is_floating_point():
            r = torch.rand(v.shape, generator=g_)
            v = (0.5 + r) * v.abs() + 0.01 * r if k.endswith('running_var') else v * (0.5 + r) + 0.01 * (r - 0.5)
        sd[k] = v.clone()
    return sd


def _conv_weight(model):
    """The first conv weight of the trained network (AdaBins: of the student; the teacher comes first in parameters())."""
    root = getattr(model, 'audio_encoder', model)
    return next(p for p in root.parameters() if p.dim() == 4 and p.shape[0] > 1 and p.shape[1] > 1)


UNET_CASES = [(8, F32), (8, BF16), (4, BF16), (64, BF16)]
UNET_IDS = ['ngf8_f32', 'ngf8_bf16', 'ngf4_bf16', 'ngf64_bf16']


@pytest.mark.parametrize('ngf,dtype', UNET_CASES, ids=UNET_IDS)
def test_unet_operands_current_after_eager_events(ngf, dtype):
    x2, gt2 = _batch(2)
    x3, _ = _batch(3)
    for train in (True, False):                                      # (a) construction, train and eval mode
        model = _unet(ngf, dtype)
        _forward(model, x2, train)
        assert_operands_current(model.engine(), f'construction train={train}')
    eng = model.engine()
    tr = _unet_trainer(model)
    model.train()
    for _ in range(3):                                               # (b) three eager fused steps
        tr.step(x2, gt2)
    assert dtype == F32 or eng.s2_fresh
    _forward(model, x2, False)
    assert_operands_current(eng, 'fused steps, eval')
    model.train()
    tr.step(x2, gt2)
    _forward(model, x2, True)
    assert_operands_current(eng, 'fused step, train')
    tr.step(x2, gt2)                                                 # (d) in-place edit after a fused step
    with torch.no_grad():
        _conv_weight(model).mul_(1.5)
    _forward(model, x2, False)
    assert_operands_current(eng, 'in-place edit')
    model.train()
    tr.step(x2, gt2)                                                 # (e) load_state_dict after a fused step
    model.load_state_dict(_donor_state(model))
    _forward(model, x2, False)
    assert_operands_current(eng, 'load_state_dict')
    model.train()
    tr.step(x2, gt2)                                                 # (f) a torch.optim step through the autograd bridge
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    opt.zero_grad()
    (model(x2) - gt2).abs().mean().backward()
    opt.step()
    _forward(model, x2, True)
    assert_operands_current(eng, 'torch.optim step')
    tr.step(x2, gt2)                                                 # (g) B = 2 step, B = 3 forward (new shape set), B = 2 again
    _forward(model, x3, False)
    assert_operands_current(eng, 'new shape set')
    _forward(model, x2, False)
    assert_operands_current(eng, 'back on the first shape set')
    model.train()
    tr.step(x3, _batch(3)[1])                                        # ... and a fused step on one set, a forward on the other
    _forward(model, x2, False)
    assert_operands_current(eng, 'step on one set, forward on the other')


@pytest.mark.parametrize('mode', ['graph', 'plan'])
@pytest.mark.parametrize('ngf,dtype', UNET_CASES, ids=UNET_IDS)
def test_unet_operands_current_after_replayed_steps(ngf, dtype, mode):
    x2, gt2 = _batch(2)
    model = _unet(ngf, dtype).train()
    tr = _unet_trainer(model)
    tr.enable_graph(after_steps=1) if mode == 'graph' else tr.enable_launch_plan(after_steps=1)
    for _ in range(4):                                               # (c) eager, capture, two replays
        tr.step(x2, gt2)
    assert (tr._graph if mode == 'graph' else tr._plan) is not None
    _forward(model, x2, False)
    assert_operands_current(model.engine(), 'replayed steps, eval')
    model.train()
    tr.step(x2, gt2)                                                 # a replay after the eval forward cleared the flags
    _forward(model, x2, True)
    assert_operands_current(model.engine(), 'replay, train')


# ---- the other engines, by behaviour: eval prediction == a fresh model holding the same state_dict
def _cvae(seed):
    from audio_depth_estimation_amd.models.unet_cvae_model import define_G_cvae
    torch.manual_seed(seed)
    model = define_G_cvae(_cfg(True), 2, 1, 8, 'unet_128', latent_dim=24)
    model.compute_dtype = BF16
    return model.to(DEV)


def _rgb(seed, dtype=BF16):
    from audio_depth_estimation_amd.models.rgb_depth_model import RGBDepthNet
    torch.manual_seed(seed)
    model = RGBDepthNet(base_channels=8, bilinear=True, output_size=64, max_depth=30.0)
    model.compute_dtype = dtype
    return model.to(DEV)


def _adabins(seed):
    from audio_depth_estimation_amd.models.adabins_distillation_model import AdaBinsDistillationModel
    torch.manual_seed(seed)
    model = AdaBinsDistillationModel(128, 64, 32, 30.0)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.compute_dtype = BF16
    return model.to(DEV)


class _Family:
    """build(seed) -> model; steps(model) runs the fused steps of the case; predict(model) -> eval prediction."""

    def __init__(self, name):
        self.name = name
        if name == 'cvae':
            self.build, (self.x, self.gt) = _cvae, _batch(2)
            self.gt = self.gt / 30.0
        elif name == 'dc':
            self.build, (self.x, self.gt) = _rgb, _batch(2, 3, 64)
        else:
            self.build, (self.x, self.gt) = _adabins, _batch(2, 2, 32)
            self.rgb = _batch(2, 3, 32, seed=9)[0]

    def trainer(self, model):
        eng = model.engine()
        if self.name == 'cvae':
            from audio_depth_estimation_amd.cvae_engine import CVAETrainer
            return CVAETrainer(eng, 'Combined', 0.5, 0.5, 0.5, max_depth=30.0, lr=1e-3, kl_weight=1e-2)
        if self.name == 'dc':
            from audio_depth_estimation_amd.engine import FusedTrainer
            return FusedTrainer(eng, 'DepthLoss', 1.0, 0.1, optimizer='AdamW', lr=1e-3, weight_decay=0.01, clip_norm=None)
        from audio_depth_estimation_amd.adabins_engine import AdaBinsTrainer
        return AdaBinsTrainer(eng, lr=1e-3)

    def step(self, tr):
        return tr.step(self.x, self.rgb, self.gt) if self.name == 'adabins' else tr.step(self.x, self.gt)

    def steps(self, model, tr):
        model.train()
        for _ in range(3):
            self.step(tr)
        if self.name == 'cvae':                    # sample() runs on a shape set of its own and hands the flags back
            model.eval()
            model.sample(self.x, 2, seed=3)
            model.train()
            self.step(tr)

    def predict(self, model):
        model.eval()
        with torch.no_grad():
            if self.name == 'cvae':
                model.engine().eps_in = torch.zeros(2, 24, device=DEV)          # z = mu: no draw in the comparison
                return model(self.x)[0].clone()
            if self.name == 'dc':
                return model(self.x).clone()
            return model.forward_audio(self.x)['final_depth'].clone()


def _apply_event(model, event):
    if event == 'edit':
        with torch.no_grad():
            _conv_weight(model).mul_(1.5)
    elif event == 'load':
        model.load_state_dict(_donor_state(model))


@pytest.mark.parametrize('event', ['steps', 'edit', 'load'])
@pytest.mark.parametrize('family', ['cvae', 'dc', 'adabins'])
def test_other_engines_predict_from_current_operands(family, event):
    fam = _Family(family)
    model = fam.build(0)
    tr = fam.trainer(model)
    fam.steps(model, tr)
    _apply_event(model, event)
    got = fam.predict(model)
    assert_mirror_current(model.engine(), (family, event))
    if family == 'cvae':
        assert_operands_current(model.engine(), (family, event))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    fresh = fam.build(5)
    fresh.load_state_dict(sd)
    want = fam.predict(fresh)
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want), (family, event, float((got - want).abs().max()))


def test_a_partly_stepped_mirror_is_not_trusted():
    """AdaBinsTrainer steps the student only (_optim_offset != 0): the optimizer writes flat_w16[offset:] and nobody keeps
    the teacher's part, so the next pack has to re-cast the mirror -- whatever that part holds by then."""
    fam = _Family('adabins')
    model = fam.build(0)
    tr = fam.trainer(model)
    fam.steps(model, tr)
    eng = model.engine()
    assert tr._optim_offset > 0
    eng.flat_w16[:tr._optim_offset].fill_(float('nan'))
    fam.step(tr)
    fam.predict(model)
    assert_mirror_current(eng, 'teacher range')


# ===================================================================================== 4. edits between replays
def _part4_run(family, dtype, mode, edit, eval_between):
    if family == 'unet':
        model = _unet(8, dtype)
        x, gt = _batch(2)
        tr = _unet_trainer(model)
        predict = lambda: _forward(model, x, False)
    else:
        model = _rgb(0, dtype)
        x, gt = _batch(2, 3, 64)
        fam = _Family('dc')
        tr = fam.trainer(model)
        predict = lambda: fam.predict(model)
    if mode == 'graph':
        tr.enable_graph(after_steps=1)
    elif mode == 'plan':
        tr.enable_launch_plan(after_steps=1)
    model.train()
    for _ in range(3):
        tr.step(x, gt)
    if mode != 'eager':
        assert (tr._graph if mode == 'graph' else tr._plan) is not None          # the third step was a replay
    _apply_event(model, edit)
    if eval_between:
        predict()
        model.train()
    for _ in range(2):
        tr.step(x, gt)
    torch.cuda.synchronize()
    eng = model.engine()
    return eng.flat_p.clone(), (eng.flat_w16.clone() if eng.flat_w16 is not None else None)


_eager_runs = {}


@pytest.mark.parametrize('eval_between', [False, True], ids=['steps_at_once', 'eval_between'])
@pytest.mark.parametrize('edit', ['load', 'edit'])
@pytest.mark.parametrize('mode', ['graph', 'plan'])
@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('family', ['unet', 'dc'])
def test_edit_between_replays_graph_equals_eager(family, dtype, mode, edit, eval_between):
    """Three steps (the third replayed), an edit of the parameters from outside, two more steps: the replaying trainer and
    the eager one end on the same f32 masters and the same bf16 mirror.  f32 reads the masters directly: the control."""
    key = (family, dtype, edit, eval_between)
    if key not in _eager_runs:
        _eager_runs[key] = _part4_run(family, dtype, 'eager', edit, eval_between)
    want_p, want_w = _eager_runs[key]
    got_p, got_w = _part4_run(family, dtype, mode, edit, eval_between)
    diff = int((bits(got_p) != bits(want_p)).sum())
    assert diff == 0, (f'{diff} of {want_p.numel()} f32 masters differ from the eager run, max |d| = '
                       f'{float((got_p - want_p).abs().max()):.3e}')
    if want_w is not None:
        assert same_bits(got_w, want_w)
