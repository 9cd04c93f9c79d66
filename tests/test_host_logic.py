"""CPU-only host logic: config surface, module tree / state_dict layout, parameter flat layout."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def test_config_loader_matches_reference_dump():
    """tests/golden/config_dump.json was produced by the REFERENCE's load_config (make_golden flow)."""
    from audio_depth_estimation_amd.config_loader import load_config
    ref = json.load(open(os.path.join(GOLDEN, 'config_dump.json')))
    for key, parts in ref.items():
        ds, mode = key.split('/')
        cfg = load_config(ds, mode, 'exp')
        for part, vals in parts.items():
            assert vars(getattr(cfg, part)) == vals, (key, part)
    cfg = load_config('batvisionv2', 'train', 'x', model_name='does_not_exist')
    assert cfg.model.name == 'unet_baseline' and cfg.mode.batch_size == 256 and cfg.mode.l1_weight == 0.237


def test_state_dict_keys_and_init_match_reference():
    from audio_depth_estimation_amd.models.unetbaseline_model import define_G
    from oracle import unet_oracle
    z = np.load(os.path.join(GOLDEN, 'unet256_ngf4.npz'))
    cfg = SimpleNamespace(dataset=SimpleNamespace(depth_norm=False))
    torch.manual_seed(0)
    model = define_G(cfg, 2, 1, 4, 'unet_256')
    ref_keys = [k[4:] for k in z.files if k.startswith('sd0/')]
    assert list(model.state_dict().keys()) == ref_keys
    np.testing.assert_array_equal(model.state_dict()['model.model.0.weight'].numpy(), z['sd_init/model.model.0.weight'])
    assert [k for k, _ in model.named_parameters()] == unet_oracle.param_keys(8)
    full = define_G(cfg, 2, 1, 64, 'unet_256')
    assert sum(p.numel() for p in full.parameters()) == 54408833
    assert len(full.state_dict()) == 82
    with pytest.raises(NotImplementedError):
        define_G(cfg, 2, 1, 4, 'resnet_6blocks')
    levels = full._adn_levels()
    assert [lv['down'].weight.shape[0] for lv in levels] == [64, 128, 256, 512, 512, 512, 512, 512]
    assert levels[0]['bn_d'] is None and levels[7]['bn_d'] is None and levels[7]['bn_u'] is not None


def test_depth_norm_selects_sigmoid_head():
    from audio_depth_estimation_amd.models.unetbaseline_model import define_G
    m = define_G(SimpleNamespace(dataset=SimpleNamespace(depth_norm=True)), 2, 1, 4, 'unet_128')
    assert isinstance(m.model.model[-1], torch.nn.Sigmoid) and m._depth_norm
    m = define_G(SimpleNamespace(dataset=SimpleNamespace(depth_norm=False)), 2, 1, 4, 'unet_128')
    assert isinstance(m.model.model[-1], torch.nn.ReLU)


def test_cpu_model_call_raises():
    from audio_depth_estimation_amd.models.unetbaseline_model import define_G
    m = define_G(SimpleNamespace(dataset=SimpleNamespace(depth_norm=False)), 2, 1, 4, 'unet_128')
    with pytest.raises(RuntimeError, match='HIP'):
        m(torch.rand(1, 2, 128, 128))


def test_optimizer_state_is_torch_optim_format_and_round_trips():
    """optim_state.export_state writes what torch.optim.AdamW.state_dict() holds (so the reference's
    optimizer.load_state_dict reads it, train_binaural_attention.py:361) and import_state reads a state written by a
    REAL torch optimizer over the same parameters back into the flat, channels_last moment buffers."""
    import torch
    from audio_depth_estimation_amd import optim_state
    from audio_depth_estimation_amd.flat import FlatParamEngine
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(6, 4, 4, 4)), torch.nn.Parameter(torch.randn(6)),
              torch.nn.Parameter(torch.randn(5, 6, 3, 3))]
    # a real torch optimizer takes two steps
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0.01)
    for _ in range(2):
        for p in params:
            p.grad = torch.randn_like(p)
        opt.step()
    ref = opt.state_dict()
    # flat layout of flat.py: parameters() order, conv tensors in channels_last memory
    meta, total = [], 0
    for p in params:
        meta.append((p, total, p.numel()))
        total += (p.numel() + 7) // 8 * 8
    m, v = torch.zeros(total), torch.zeros(total)
    step, group = optim_state.import_state(ref, meta, FlatParamEngine._view, m, v)
    assert step == 2 and group['lr'] == 1e-3
    for i, (p, off, n) in enumerate(meta):
        assert torch.equal(FlatParamEngine._view(m, off, p), ref['state'][i]['exp_avg'])
        if p.dim() == 4:          # memory order of the flat slice is [X][kh][kw][Y]
            assert torch.equal(m[off:off + n].view(p.shape[0], p.shape[2], p.shape[3], p.shape[1]),
                               ref['state'][i]['exp_avg'].permute(0, 2, 3, 1))
    out = optim_state.export_state(meta, FlatParamEngine._view, m, v, step, 0, 1e-3, (0.9, 0.999), 1e-8, 0.01)
    assert optim_state.is_torch_format(out)
    assert set(out['param_groups'][0].keys()) == set(ref['param_groups'][0].keys())
    for i in range(len(params)):
        assert float(out['state'][i]['step']) == 2.0
        assert torch.equal(out['state'][i]['exp_avg'], ref['state'][i]['exp_avg'])
        assert torch.equal(out['state'][i]['exp_avg_sq'], ref['state'][i]['exp_avg_sq'])
    # ... and a fresh torch optimizer accepts it and continues exactly like the original
    opt2 = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1e-3, weight_decay=0.01)
    opt2.load_state_dict(out)
    gs = [torch.randn_like(p) for p in params]
    for p, q, g in zip(params, opt2.param_groups[0]['params'], gs):
        p.grad, q.grad = g.clone(), g.clone()
    opt.step()
    opt2.step()
    for p, q in zip(params, opt2.param_groups[0]['params']):
        assert torch.equal(p.detach(), q.detach())
    # a parameter list of another length is refused
    import pytest
    with pytest.raises(ValueError):
        optim_state.import_state(ref, meta[:2], FlatParamEngine._view, m, v)


def test_optim_state_groups_and_legacy_flat_layout():
    """optim_state: a checkpoint with several param_groups is rejected (the fused optimizer has one hyper-parameter set),
    the loaded group's betas / eps / weight_decay are adopted like torch's load_state_dict does, and a round-1 flat
    moment buffer (4-element alignment) is re-sliced parameter by parameter into today's 8-element layout."""
    import types

    import pytest
    import torch

    from audio_depth_estimation_amd import optim_state
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(1))]
    offs8, o = [], 0
    for p_ in ps:
        offs8.append(o)
        o += (p_.numel() + 7) // 8 * 8
    meta = [(p_, off, p_.numel()) for p_, off in zip(ps, offs8)]
    view = lambda flat, off, p_: flat[off:off + p_.numel()].view(p_.shape)
    m, v = torch.zeros(o), torch.zeros(o)
    opt = torch.optim.AdamW([{'params': ps[:2]}, {'params': ps[2:], 'lr': 1.0}], lr=0.1)
    with pytest.raises(ValueError, match='param_groups'):
        optim_state.import_state(opt.state_dict(), meta, view, m, v)
    opt1 = torch.optim.AdamW(ps, lr=0.05, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.2)
    _, group = optim_state.import_state(opt1.state_dict(), meta, view, m, v)
    tr = types.SimpleNamespace(lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    optim_state.adopt_group(tr, group)
    assert (tr.lr, tr.betas, tr.eps, tr.weight_decay) == (0.05, (0.8, 0.9), 1e-6, 0.2)
    # legacy flat buffers: 4-element alignment -> offsets 0, 4, 12, total 16
    legacy = torch.arange(16, dtype=torch.float32)
    step = optim_state.import_legacy_flat({'exp_avg': legacy, 'exp_avg_sq': legacy * 2, 'step': 7}, meta, m, v)
    assert step == 7
    assert m[0:3].tolist() == [0, 1, 2] and m[8:13].tolist() == [4, 5, 6, 7, 8] and m[16:17].tolist() == [12]
    assert v[8:13].tolist() == [8, 10, 12, 14, 16]
    with pytest.raises(ValueError, match='matches neither'):
        optim_state.import_legacy_flat({'exp_avg': torch.zeros(17), 'exp_avg_sq': torch.zeros(17), 'step': 1}, meta, m, v)


def _wgrad_plan_tool():
    import importlib.util
    path = os.path.join(os.path.dirname(GOLDEN), '..', 'tools', 'wgrad_plan_table.py')
    spec = importlib.util.spec_from_file_location('wgrad_plan_table', os.path.abspath(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wgrad_plans_match_recorded_table():
    """The weight-gradient plan queries (host only) answer what tests/golden/wgrad_plans.json recorded from the library
    before the tap-staged kernels of the two geometries were merged into one source (tools/wgrad_plan_table.py writes the
    table from any build).  Workspace bytes pin the split count, hence the summation order, hence the bits of dW."""
    tool = _wgrad_plan_tool()
    table = json.load(open(os.path.join(GOLDEN, 'wgrad_plans.json')))
    assert len(table['rows']) >= 80 and len(table['groups']) >= 2
    for r in table['rows']:
        got = tool.query_row(r)
        assert got == {k: r[k] for k in got}, r['name']
    for g, v in table['groups'].items():
        assert tool.query_group(v['rows']) == v['workspace_bytes'], g
    # the recorded table must itself hold what it is meant to pin
    by_name = {r['name']: r for r in table['rows']}
    assert table['groups']['patch_L3_L2_L1']['workspace_bytes'] > 0 and table['groups']['patch_D1_D2_D3']['workspace_bytes'] > 0
    assert table['groups']['not_patch_s1']['workspace_bytes'] == -1
    assert by_name['unet256_L1_bf16']['sq_count'] > 0 and by_name['unet256_L5_bf16']['batchable'] > 0
    for r in table['rows']:
        if r['ks']:
            assert (r['sq_count'], r['batchable'], r['batch_sq_count']) == (0, 0, 0), r['name']


def test_wgrad_plans_with_patch_kernels_off_match_recorded_table():
    """ADN_WGRAD_PATCH=0 (read once per process, hence the child): every layer takes the tap-staged plan."""
    import subprocess
    import sys
    table = json.load(open(os.path.join(GOLDEN, 'wgrad_plans.json')))
    tool = os.path.abspath(os.path.join(os.path.dirname(GOLDEN), '..', 'tools', 'wgrad_plan_table.py'))
    out = subprocess.run([sys.executable, tool, '--query', 'rows_patch_off'], env=dict(os.environ, ADN_WGRAD_PATCH='0'),
                         capture_output=True, text=True, check=True).stdout
    assert len(table['rows_patch_off']) >= 10
    assert json.loads(out) == table['rows_patch_off']
    on = {r['name']: r for r in table['rows']}
    assert any(r['workspace_bytes'] != on[r['name']]['workspace_bytes'] for r in table['rows_patch_off'])


def _igemm_plan_tool():
    import importlib.util
    path = os.path.join(os.path.dirname(GOLDEN), '..', 'tools', 'igemm_plan_table.py')
    spec = importlib.util.spec_from_file_location('igemm_plan_table', os.path.abspath(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _igemm_form(plan):
    """'ring bm=256 bn=128 nsplit=1 ...' -> 'ring 256x128' (direct: 'direct'; split-K: '... split')."""
    import re
    m = re.match(r'(\S+) bm=(\d+) bn=(\d+) nsplit=(\d+) ', plan)
    kind, bm, bn, ns = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
    return 'direct' if kind == 'direct' else '%s %dx%d%s' % (kind, bm, bn, ' split' if ns > 1 else '')


def test_igemm_plans_match_recorded_table():
    """adn_igemm_describe (host only) answers what tests/golden/igemm_plans.json recorded from the library before the
    planner was restructured around a kernel kind (tools/igemm_plan_table.py writes the table from any build): kernel form,
    tile, split count, grid, K-steps, partial rows and workspace bytes of every unet_256 layer, the benchmarked shapes, the
    shapes of the GPU tests and rows on both sides of every planning rule."""
    tool = _igemm_plan_tool()
    table = json.load(open(os.path.join(GOLDEN, 'igemm_plans.json')))
    assert len(table['rows']) >= 400
    for r in table['rows']:
        got = tool.query_row(r)
        assert got == {k: r[k] for k in got}, r['name']
        assert r['plan'].endswith('partials=%d ws=%d' % (r['num_partials'], r['workspace_bytes'])), r['name']
    # the recorded table must itself hold what it is meant to pin: every form, and both sides of the rule boundaries
    plan = {r['name']: r['plan'] for r in table['rows']}
    assert {p.split()[0] for p in plan.values()} == {'direct', 'tile', 'patch', 'patch-tall', 'patch-pair', 'ring'}
    assert all(p.split()[0] in ('direct', 'tile') for n, p in plan.items() if n.endswith('f32'))
    assert 'bn=128' in plan['rule_s2_t128_b127_n128_bf16'] and 'bn=64' in plan['rule_s2_t128_b128_n128_bf16']
    assert 'bn=64' in plan['rule_s2_t128_b255_n128_bf16'] and 'bn=128' in plan['rule_s2_t128_b128_n256_bf16']
    assert plan['rule_ring_s2_b191_bf16'].startswith('ring bm=256 bn=64') and plan['rule_ring_s2_b192_bf16'].startswith('ring bm=256 bn=128')
    assert plan['rule_ring_t2_b47_bf16'].startswith('ring bm=256 bn=64') and plan['rule_ring_t2_b48_bf16'].startswith('ring bm=256 bn=128')
    assert plan['rule_pair_b30_n256_bf16'].startswith('tile') and plan['rule_pair_b32_n256_bf16'].startswith('patch-pair')
    assert plan['rule_tall_t2_b127_bf16'].startswith('patch ') and plan['rule_tall_t2_b128_bf16'].startswith('patch-tall')
    assert [plan['rule_tinycap_b%d_n%d_bf16' % bn].split()[3] for bn in ((8, 128), (16, 512), (32, 512))] == ['nsplit=64', 'nsplit=32', 'nsplit=16']
    assert plan['unet256_D4_fwd_bf16'].startswith('patch-pair') and plan['unet256_D1_dgrad_bf16'].startswith('ring')


@pytest.mark.parametrize('section', ['rows_ring_off', 'rows_patch_off', 'rows_bn_t2_128'])
def test_igemm_plans_with_knobs_match_recorded_table(section):
    """ADN_IGEMM_RING=0 / ADN_IGEMM_PATCH=0 / ADN_IGEMM_BN_T2=128 (read once per process, hence the child)."""
    import subprocess
    import sys
    tool = _igemm_plan_tool()
    table = json.load(open(os.path.join(GOLDEN, 'igemm_plans.json')))
    out = subprocess.run([sys.executable, tool.__file__, '--query', section], env=dict(os.environ, **tool.KNOBS[section]),
                         capture_output=True, text=True, check=True).stdout
    assert len(table[section]) >= 30
    assert json.loads(out) == table[section]
    on = {r['name']: r['plan'] for r in table['rows']}
    assert any(r['plan'] != on[r['name']] for r in table[section])
    kinds = {r['plan'].split()[0] for r in table[section]}
    if section == 'rows_ring_off':
        assert 'ring' not in kinds
    if section == 'rows_patch_off':
        assert not any(k.startswith('patch') for k in kinds)


def test_igemm_gpu_test_shapes_reach_the_forms_they_name():
    """Every bf16 launch of the igemm tests of test_gpu_kernels.py runs the kernel form IGEMM_FORMS names for it, and the
    forms add up: each one is reached by a forward (RAW) launch and, where it can carry them, by a Z_STATS and a BWD launch."""
    import test_gpu_kernels as tg
    tool = _igemm_plan_tool()
    rows = tg.igemm_launches()
    assert {r['name'][:-5] for r in rows if r['dtype'] == 1} == set(tg.IGEMM_FORMS)
    reached = {}
    for r in rows:
        form = _igemm_form(tool.query_row(r)['plan'])
        if r['dtype'] == 1:
            assert form == tg.IGEMM_FORMS[r['name'][:-5]], r['name']
        reached.setdefault((form, r['geom']), set()).add(r['epi'])
    epis = lambda form, geoms=(0, 1): set().union(*[reached.get((form, g), set()) for g in geoms])
    for form in ('tile 128x128', 'tile 128x64', 'tile 256x64', 'tile 256x128', 'tile 128x128 split', 'tile 128x64 split', 'direct'):
        assert epis(form) >= {0, 1, 3}, form
    for geom in (0, 1):                                    # S2, T2
        assert epis('patch 128x64', (geom,)) >= {0, 1, 3}, geom
        for form in ('ring 256x64', 'ring 256x128'):       # (the ring kernel has no RAW epilogue)
            assert epis(form, (geom,)) >= {1, 3}, (form, geom)
    assert epis('patch 128x128', (0,)) >= {0}
    for form in ('patch-tall 256x64', 'patch-pair 128x128'):     # T2 only (the S2 pair form lost to split-K, tall needs T2 / S1)
        assert epis(form, (1,)) >= {0, 1, 3}, form
    # ACT (2) is the eval-mode forward of the same layers: every non-ring form must carry it too; FINAL (4) and ADD (5) must
    # reach the direct path, a split tile (both: the scalar epilogue), an unsplit tile and a patch form (the vector epilogue)
    for form in ('tile 128x128', 'tile 128x64', 'tile 256x64', 'tile 256x128', 'tile 128x128 split', 'tile 128x64 split', 'direct'):
        assert 2 in epis(form), form
    for geom in (0, 1):
        assert 2 in epis('patch 128x64', (geom,)), geom
    assert 2 in epis('patch 128x128', (0,))
    for form in ('patch-tall 256x64', 'patch-pair 128x128'):
        assert 2 in epis(form, (1,)), form
    by_epi = lambda epi: {form for (form, _), e in reached.items() if epi in e}
    for epi in (4, 5):
        forms = by_epi(epi)
        assert 'direct' in forms, epi
        assert any(f.startswith('tile') and f.endswith('split') for f in forms), epi
        assert any(f.startswith('tile') and not f.endswith('split') for f in forms), epi
        assert any(f.startswith('patch') for f in forms), epi
    # the patch kernel's stats epilogues run off the ring kernel's 16 x 16 grid, at the smallest B that plans unsplit
    for geom, B, C0, N in tg.PATCH_STATS_CASES:
        for b, want in ((B, 'patch'), (B - 1, 'tile')):
            r = dict(name='', dtype=1, geom=geom, B=b, Hs=tg.PATCH_HS, Ws=tg.PATCH_WS, C0=C0, C1=0, N=N, epi=1, segs=[N], ks=0)
            p = tool.query_row(r)['plan']
            assert p.split()[0] == want and ('nsplit=1 ' in p) == (b == B), p


def test_igemm_epilogue_s1_shapes_reach_the_forms_they_name():
    """The stride-1 launches of tests/test_gpu_igemm_epilogues.py (ACT and ADD; FINAL has no stride-1 user) run the kernel
    form their case table names, and every case of that module -- S2 / T2 ones included, which the test above and the plan
    table pin -- names a shape whose form the planner confirms.  ACT reaches every stride-1 form, ADD the unsplit 1 x 1
    tiles of the attention block, a 3 x 3 patch form, a split tile and the direct path."""
    import igemm_epilogue_cases as ec
    tool = _igemm_plan_tool()
    rows = ec.launch_rows(s1=True)
    assert len(rows) >= 20 and all(r['geom'] == 2 for r in rows)
    for r in rows + ec.launch_rows(s1=False):
        assert ec.plan_form(tool.query_row(r)['plan']) == r['form'], r['name']
    for epi, key_cases in ec.CASES.items():                       # the variant of every case exists and fits its shape
        for key, var in key_cases:
            sets = {ec.ACT: ec.ACT_VARIANTS, ec.ADD: ec.ADD_VARIANTS}.get(epi, {var: [None]})[var]
            assert len(sets) in (1, len(ec.SHAPES[key]['segs'])), (key, var)
            assert max(ec.SHAPES[key][d] for d in ('B', 'Hs', 'Ws')) <= 256
            assert ec.SHAPES[key]['B'] * ec.SHAPES[key]['Hs'] * ec.SHAPES[key]['Ws'] <= 16 * 64 * 64, key
    forms = lambda epi, ks: {r['form'] for r in rows if r['epi'] == epi and r['ks'] == ks}
    assert forms(ec.ACT, 3) >= {'direct', 'tile 128x128 split', 'tile 128x64', 'patch 128x64', 'patch 128x128', 'patch-tall 256x64'}
    assert forms(ec.ACT, 1) >= {'tile 128x64', 'tile 256x64', 'tile 128x128'}
    assert forms(ec.ADD, 1) >= {'tile 128x128', 'tile 128x64', 'tile 256x64'}
    assert forms(ec.ADD, 3) >= {'direct', 'tile 128x128 split', 'patch 128x64'}
    assert not forms(ec.FINAL, 1) and not forms(ec.FINAL, 3)
    # what the mutation checks of the module rely on: the gate, a two-segment slope pair, an out0-only launch, ACT with
    # shift and bias, and FINAL's identity each run behind the scalar epilogue AND the vector one
    scalar = lambda key: ec.SHAPES[key]['form'] == 'direct' or ec.SHAPES[key]['form'].endswith('split')
    for epi, pick in ((ec.ADD, lambda v: v in ('gate', 'gate_chan')), (ec.ACT, lambda v: v == 'slopes'),
                      (ec.ACT, lambda v: v in ('scale', 'qkv')), (ec.ACT, lambda v: v == 'full'),
                      (ec.FINAL, lambda v: v[0] == 2)):
        for dt in (ec.F32, ec.BF16):
            paths = {scalar(key) for key, var in ec.CASES[epi] if pick(var) and ec.SHAPES[key]['dtype'] == dt}
            assert paths == {False, True}, (epi, dt)


def test_launch_plan_capture_and_replay_state_machine():
    """GraphedStep's launch-plan path on CPU tensors: ``after_steps`` eager calls, one recording call, replays over the
    static input buffers with the engine flags restored, eager steps for any other input signature, and re-arming."""
    from audio_depth_estimation_amd import _lib
    from audio_depth_estimation_amd.trainer import GraphedStep

    class Engine:
        weights_dirty, s2_fresh, pins = False, False, 0
        _packed_version, version, resyncs = 0, 0, 0          # ``version``: bumped by an edit of the parameters from outside

        def pin_buffers(self):
            self.pins += 1

        def _version_sum(self):
            return self.version

        def resync_mirror(self):
            self.resyncs += 1
            self.weights_dirty, self.s2_fresh, self._packed_version = True, True, self.version

    class Step(GraphedStep):
        def __init__(self):
            self.engine, self.out, self.impl_calls = Engine(), torch.zeros(3), 0

        def _step_impl(self, a, b, c):
            self.impl_calls += 1

            def work():           # out = sum(a) + (sum(b) if given) + 10 * sum(c): everything goes through record_py
                self.out.fill_(float(a.sum()) + (float(b.sum()) if b is not None else 0.0) + 10.0 * float(c.sum()))
            _lib.record_py(work)
            self.engine.weights_dirty, self.engine.s2_fresh = True, True
            return self.out

    def value(a, b, c):
        return float(a.sum()) + (float(b.sum()) if b is not None else 0.0) + 10.0 * float(c.sum())

    mk = lambda seed, n=4: torch.arange(n, dtype=torch.float32) + seed
    for with_b in (True, False):                     # a None input is part of the captured signature
        t, after = Step(), 2
        eng = t.engine
        t._plan_after = after
        for i in range(after):                       # exactly ``after_steps`` eager calls
            a, b, c = mk(i), (mk(i + 1) if with_b else None), mk(i + 2)
            assert float(t._graphed(a, b, c)[0]) == value(a, b, c)
            assert t._plan is None and t.impl_calls == i + 1 and eng.pins == 0
        a, b, c = mk(7), (mk(8) if with_b else None), mk(9).double()       # the recording call; f64 is stored as f32
        out = t._graphed(a, b, c)
        assert out is t.out and float(out[0]) == value(a, b, c)
        assert t.impl_calls == after + 1 and eng.pins == 1 and _lib.RECORD is None
        assert len(t._plan) == 1 and t._plan[0][0] is None and t._plan[0][2] == 'py'
        assert [None if g is None else g.dtype for g in t._g_in] == [torch.float32, torch.float32 if with_b else None,
                                                                     torch.float32]
        assert t._g_in[0] is not a and (t._g_in[1] is None) == (not with_b)
        assert t._post_flags == (True, True)
        bufs = list(t._g_in)
        for i in range(3):                           # replays: inputs copied into the static buffers, same output object
            eng.weights_dirty, eng.s2_fresh = False, False          # (an eval forward in between clears the flags)
            a, b, c = mk(20 + i), (mk(30 + i) if with_b else None), mk(40 + i)
            out = t._graphed(a, b, c)
            assert out is t.out and float(out[0]) == value(a, b, c)
            assert t.impl_calls == after + 1                         # nothing ran but the plan
            assert all(g is h for g, h in zip(t._g_in, bufs)) and torch.equal(t._g_in[0], a) and torch.equal(t._g_in[2], c)
            assert (eng.weights_dirty, eng.s2_fresh) == (True, True)
        # another batch shape, or None where a tensor was captured (and the reverse): eager, the plan stays
        plan, n = t._plan, t.impl_calls
        odd = [(mk(1, 5), (mk(2, 5) if with_b else None), mk(3, 5)),
               (mk(1), (None if with_b else mk(2)), mk(3))]
        for a, b, c in odd:
            eng.weights_dirty = False
            assert float(t._graphed(a, b, c)[0]) == value(a, b, c)
            n += 1
            assert t.impl_calls == n and t._plan is plan and eng.pins == 1
            assert all(g is h for g, h in zip(t._g_in, bufs)) and not torch.equal(t._g_in[0][:4], a[:4])
        a, b, c = mk(50), (mk(51) if with_b else None), mk(52)
        assert float(t._graphed(a, b, c)[0]) == value(a, b, c) and t.impl_calls == n      # the plan still replays
        # the parameters changed from outside since the engine packed them: the plan holds the pack decisions of the step
        # it recorded, so it is dropped and recorded again by the same call, over a mirror re-cast once
        eng.version += 1
        a, b, c = mk(53), (mk(54) if with_b else None), mk(55)
        assert float(t._graphed(a, b, c)[0]) == value(a, b, c)
        n += 1
        assert t.impl_calls == n and t._plan is not None and t._plan is not plan and eng.pins == 2 and eng.resyncs == 1
        assert eng._packed_version == eng.version and t._g_in[0] is not bufs[0]
        a, b, c = mk(56), (mk(57) if with_b else None), mk(58)
        assert float(t._graphed(a, b, c)[0]) == value(a, b, c) and t.impl_calls == n      # ... and replays from then on
        assert eng.resyncs == 1
        plan, bufs = t._plan, list(t._g_in)
        eng.pins = 1
        # dropping the plan: eager again, and it can be re-armed
        t._plan, t._plan_after = None, None
        for i in range(2):
            a, b, c = mk(60 + i), (mk(61 + i) if with_b else None), mk(62 + i)
            assert float(t._graphed(a, b, c)[0]) == value(a, b, c)
            n += 1
            assert t.impl_calls == n and t._plan is None
        t._plan_after = 0
        a, b, c = mk(70, 6), (mk(71, 6) if with_b else None), mk(72, 6)      # re-armed on another shape
        assert float(t._graphed(a, b, c)[0]) == value(a, b, c)
        assert t.impl_calls == n + 1 and t._plan is not None and t._plan is not plan and eng.pins == 2
        assert t._g_in[0].shape == (6,) and t._g_in[0] is not bufs[0]
        a, b, c = mk(80, 6), (mk(81, 6) if with_b else None), mk(82, 6)
        assert float(t._graphed(a, b, c)[0]) == value(a, b, c) and t.impl_calls == n + 1

    class Gated(Step):               # the overridable capture gate: an armed trainer stays eager until it opens
        ok = False

        def _capture_ok(self):
            return self.ok

    t = Gated()
    t._plan_after = 0
    for i in range(2):
        t._graphed(mk(i), None, mk(i))
        assert t._plan is None and t.impl_calls == i + 1
    t.ok = True
    t._graphed(mk(5), None, mk(5))
    assert t._plan is not None and t.impl_calls == 3 and t.engine.pins == 1


def test_k4_rect_cases_reach_the_forms_they_name():
    """tests/k4_rect_cases.py (the shapes of tests/test_gpu_k4_rect.py): every igemm case runs the kernel form its table
    names for each epilogue it launches, every weight-gradient case gets the answers its table holds from the plan queries,
    every rectangular case stands beside its transposed twin, and the forms add up: each igemm form is reached by RAW
    (where it can carry it), Z_STATS and BWD on a power-of-two rectangle, on its transpose where the tiling rule allows
    one, and on a non-power-of-two grid; each weight-gradient route has a non-square and a non-power-of-two case."""
    import k4_rect_cases as kc
    itool, wtool = _igemm_plan_tool(), _wgrad_plan_tool()
    pow2 = lambda n: n & (n - 1) == 0
    is_pow2 = lambda c: pow2(c['Hs']) and pow2(c['Ws'])
    reached = {}                                   # (form, geom, epi) -> [case]
    assert len(kc.IGEMM) >= 100
    for key, c in kc.IGEMM.items():
        assert c['Hs'] != c['Ws'], key
        assert c['B'] * c['Hs'] * c['Ws'] <= 16 * 56 * 40 and max(c['Hs'], c['Ws']) <= 64, key
        twin = '%s/%s/%dx%dx%d/%s' % (key.split('/')[0], key.split('/')[1], c['B'], c['Ws'], c['Hs'], c['cset'])
        assert twin in kc.IGEMM, key
        assert any(f is not None for f in c['forms'].values()), key
        for epi, form in c['forms'].items():
            assert (form is None) == (kc.IGEMM[twin]['forms'][epi] is None), key
            if form is None:
                continue
            assert _igemm_form(itool.query_row(kc.igemm_row(key, epi))['plan']) == form, (key, epi)
            reached.setdefault((form, c['geom'], epi), []).append(c)
    for name, keys in (('accumulate', kc.BWD_ACCUMULATE), ('mask_from_z', kc.BWD_MASK_FROM_Z), ('sentinel', kc.SWAP_SENTINEL)):
        for key in keys:
            assert key in kc.IGEMM and (name == 'sentinel' or kc.IGEMM[key]['forms'][kc.BWD] is not None), (name, key)

    def covered(form, geoms, epis, transpose=True):
        for epi in epis:
            cs = [c for g in geoms for c in reached.get((form, g, epi), [])]
            p2 = [c for c in cs if is_pow2(c)]
            assert p2, (form, geoms, epi, 'no power-of-two rectangle')
            assert any(not is_pow2(c) for c in cs), (form, geoms, epi, 'no non-power-of-two grid')
            if transpose:
                shapes = {(c['Hs'], c['Ws']) for c in cs}
                assert any((w, h) in shapes for h, w in shapes), (form, geoms, epi, 'no transposed pair')

    all3 = (kc.RAW, kc.Z_STATS, kc.BWD)
    for form in ('direct', 'tile 128x128 split', 'tile 128x64 split', 'tile 128x64', 'tile 128x128', 'tile 256x64', 'tile 256x128'):
        covered(form, (0, 1), all3)
    # the patch kernel needs Hs % 8 == 0 and Ws % 16 == 0, so the transpose of an 8 x 16-tileable image that is not
    # 16 x 16-tileable runs another kernel; patch-tall and the ring need 16 on both sides: both orientations run them
    for geom in (0, 1):
        covered('patch 128x64', (geom,), all3, transpose=False)
        for form in ('ring 256x64', 'ring 256x128'):          # (the ring kernel has no RAW epilogue)
            covered(form, (geom,), (kc.Z_STATS, kc.BWD))
    covered('patch 128x128', (0,), all3, transpose=False)
    covered('patch-tall 256x64', (1,), all3)
    for form, geoms in (('patch 128x64', (0, 1)), ('patch 128x128', (0,))):        # ... and name what their transposes run
        for c in [c for g in geoms for c in reached[(form, g, kc.RAW)]]:
            if c['Hs'] % 16 or c['Ws'] % 16:
                twin = kc.IGEMM['%s/%s/%dx%dx%d/%s' % ('bf16', 'ST'[c['geom']] + '2', c['B'], c['Ws'], c['Hs'], c['cset'])]
                assert twin['forms'][kc.RAW].startswith('tile') and not twin['forms'][kc.RAW].endswith('split')
    # accumulate: one BWD launch per form and geometry that has a BWD case; mask_from_z: a ring and a patch case
    acc_forms = {(kc.IGEMM[k]['forms'][kc.BWD], kc.IGEMM[k]['dtype']) for k in kc.BWD_ACCUMULATE}
    for (form, geom, epi), cs in reached.items():
        if epi == kc.BWD:
            for dt in {c['dtype'] for c in cs}:
                assert (form, dt) in acc_forms, (form, dt)
    mz = {kc.IGEMM[k]['forms'][kc.BWD].split()[0] for k in kc.BWD_MASK_FROM_Z}
    assert mz >= {'ring', 'patch'}
    sent = {(kc.IGEMM[k]['forms'][kc.RAW], kc.IGEMM[k]['geom']) for k in kc.SWAP_SENTINEL if kc.IGEMM[k]['dtype'] == 1}
    assert {f for f, g, e in reached if e == kc.RAW and any(c['dtype'] == 1 for c in reached[(f, g, e)])} == {f for f, _ in sent}
    # two-segment BWD launches: sets B (as B2 / A2) and D
    assert {c['cset'] for c in kc.IGEMM.values() if len(c['segs']) == 2 and c['forms'][kc.BWD]} >= {'A2', 'B2', 'D'}
    # 1 x 2 and 2 x 1 (1 x 3, 3 x 1): a split tile, where the one-pixel form at 1 x 1 plans an unsplit T2 tile
    for hw in ((1, 2), (2, 1), (1, 3), (3, 1)):
        cs = [c for c in kc.IGEMM.values() if (c['Hs'], c['Ws']) == hw and c['B'] == 32]
        assert {c['geom'] for c in cs} == {0, 1} and all(f.endswith('split') for c in cs for f in c['forms'].values())
    onepx = dict(name='', dtype=1, geom=1, B=32, Hs=1, Ws=1, C0=128, C1=0, N=128, epi=0, segs=[128], ks=0)
    assert _igemm_form(itool.query_row(onepx)['plan']) == 'tile 128x64'

    # ---- weight gradient
    by_route = {}
    assert len(kc.WGRAD) >= 80
    for key, c in kc.WGRAD.items():
        assert c['Hs'] != c['Ws'] and c['B'] * c['Hs'] * c['Ws'] <= 16 * 56 * 40 and max(c['Hs'], c['Ws']) <= 64, key
        twin = '%s/%dx%dx%d/%s' % (key.split('/')[0], c['B'], c['Ws'], c['Hs'], key.split('/')[2])
        assert twin in kc.WGRAD and kc.WGRAD[twin]['route'] == c['route'], key
        got = wtool.query_row(kc.wgrad_row(c))
        assert (got['workspace_bytes'], got['sq_count'], got['batchable']) == c['answers'], (key, got)
        patch = wtool.query_group([kc.wgrad_row(c)])
        assert (patch >= 0) == c['patch'], (key, patch)
        ws, sq, cls = c['answers']
        want = {'fast': ws == 0 and sq > 0 and cls == 2, 'general': ws == 0 and sq > 0 and cls == 1,
                'direct': (ws, sq, cls) == (0, 0, 0), 'split': ws > 0 and sq > 0 and cls == 0 and patch < 0,
                'patch': patch == ws > 0 and sq > 0, 'f32 unsplit': ws == 0 and sq > 0 and cls == 0,
                'f32 split': ws > 0 and sq > 0}[c['route']]
        assert want and (c['dtype'] == 0) == (c['route'].startswith('f32') or c['route'] == 'direct' and key.startswith('f32')), key
        if c['route'] == 'fast':
            assert is_pow2(c)
        by_route.setdefault(c['route'], []).append(c)
    assert set(by_route) == set(kc.ROUTES)
    for route, cs in by_route.items():
        if route != 'fast':                                    # (the fast form exists for power-of-two images only)
            assert any(not is_pow2(c) for c in cs), route
        assert any(c['C1'] for c in cs) or route in ('direct', 'split', 'f32 split'), route      # a second gathered source
    assert any(c['C1'] and c['route'] == 'patch' for c in kc.WGRAD.values())
    # the two batch launches: every problem has the class of its launch; groups stand beside their transposes
    flip = lambda probs: sorted((w, h) + tuple(r) for h, w, *r in probs)
    for B, cls, probs in kc.WGRAD_BATCH:
        assert any(flip(probs) == sorted(q) for b, k, q in kc.WGRAD_BATCH if (b, k) == (B, cls))
        assert any(not (pow2(h) and pow2(w)) for h, w, *_ in probs) == (cls == 1) and all(h != w for h, w, *_ in probs)
        for prob in probs:
            got = wtool.query_row(kc.batch_row(B, prob))
            assert got['batchable'] == cls and got['batch_sq_count'] > 0, prob
    assert {cls for _, cls, _ in kc.WGRAD_BATCH} == {1, 2}
    for probs, nbytes in kc.WGRAD_PATCH_BATCH:
        assert any(flip(probs) == sorted(q) for q, _ in kc.WGRAD_PATCH_BATCH)
        assert wtool.query_group([kc.batch_row(kc.PATCH_BATCH_B, p) for p in probs]) == nbytes, probs
        assert any(not (pow2(h) and pow2(w)) for h, w, *_ in probs)


def _attn_fake_desc(row, family, bwd):
    """The descriptor tests/test_gpu_attention.py builds for a row, with made-up pointers of the same alignment: every buffer
    starts 256-byte aligned, the views start where attn_cases.view_offsets puts them.  Nothing is dereferenced."""
    import attn_cases as ac
    from audio_depth_estimation_amd import _lib
    d = _lib.AdnAttnDesc()
    d.dtype, d.B2, d.N, d.dqk, d.dv, d.kv_shift = row['dtype'], row['B2'], row['N'], row['dqk'], row['dv'], row['kv_shift']
    d.scale = ac.scale_of(row, family)
    offs = ac.view_offsets(row)
    base = {b: 0x7f0000000000 + 0x10000000 * i for i, b in enumerate(sorted(ac.layout(row)[0]))}
    addr = lambda op: base[offs[op][0]] + offs[op][1] * ac.ESIZE[row['dtype']]
    d.q, d.k, d.v, d.o = addr('q'), addr('k'), addr('v'), addr('o')
    d.ld_q, d.ld_k, d.ld_v, d.ld_o = (offs[op][2] for op in ('q', 'k', 'v', 'o'))
    d.lse = 0x7e0000000000 + 4 * ac.GUARD_F32
    if bwd:
        d.dout, d.dq, d.dk, d.dvp = addr('dout'), addr('dq'), addr('dk'), addr('dv')
        d.ld_do, d.ld_dq, d.ld_dk, d.ld_dv = (offs[op][2] for op in ('dout', 'dq', 'dk', 'dv'))
        d.workspace = 0x7d0000000000 + 4 * ac.GUARD_F32
        d.workspace_bytes = row['B2'] * row['N'] * 4
    return d


def test_attn_cases_reach_the_forms_they_name():
    """tests/attn_cases.py (the cases of tests/test_gpu_attention.py): adn_attn_form, the launches' own dispatch predicate,
    answers the form every row names, forward and backward, for every family the row runs with; the table holds what the
    issue of the module asks of it; descriptors the launches refuse are refused with a message."""
    import ctypes
    import attn_cases as ac
    from audio_depth_estimation_amd import _lib
    lib = _lib.load()
    code = {ac.GENERIC: 0, ac.MFMA: 1}
    for name, row in ac.ROWS.items():
        for family in row['families']:
            for bwd in (0, 1):
                got = lib.adn_attn_form(ctypes.byref(_attn_fake_desc(row, family, bwd)), bwd)
                assert got == code[ac.form_of(row, family, bwd)], (name, family, bwd, got, lib.adn_last_error())
        # eight distinct strides; multiples of 8 wherever the form is (or is one change away from) MFMA
        lds = [ld for _, _, ld in ac.view_offsets(row).values()]
        if row['recipe'] != 'fused':
            assert len(set(lds)) == 8, name
        if row['recipe'] == 'aligned':
            assert all(ld % 8 == 0 for ld in lds), name
        for op, (_, off, ld) in ac.view_offsets(row).items():
            assert off % ld + ac.width_of(row, op) <= ld, (name, op)
    rows = ac.ROWS.values()
    mfma = [r for r in rows if r['form'] == (ac.MFMA, ac.MFMA)]
    assert all(r['dtype'] == ac.BF16 for r in mfma) and len(mfma) == len(ac.MFMA_ROWS)
    for dims, ns in zip(ac.MFMA_DIMS, ((128, 384), (128, 384), (64, 192))):
        mine = [r for r in mfma if (r['dqk'], r['dv']) == dims]
        assert {r['N'] for r in mine} == set(ns), dims
        assert {(r['B2'], r['kv_shift']) for r in mine} >= {(3, 1), (3, 2)}, dims
        assert any(r['recipe'] == 'fused' for r in mine), dims
        assert any(r['families'] == ('neg-scale',) and (r['dqk'], r['dv']) == dims for r in rows), dims
    assert {(r['B2'], r['kv_shift']) for r in mfma} == set(ac.SHIFTS)
    # fallback rows: the MFMA row with one thing changed
    base = ac.ROWS[ac.FALLBACK_OF]
    changed = lambda r: [k for k in ('B2', 'N', 'dqk', 'dv', 'kv_shift', 'dtype', 'recipe', 'families') if r[k] != base[k]]
    for name, key in (('f16-192-n', 'N'), ('f16-128-ldq', 'recipe'), ('f16-128-koff', 'recipe'), ('f16-128-dooff', 'recipe'),
                      ('f16-128-neg', 'families')):
        assert changed(ac.ROWS[name]) == [key], name
    assert ac.ROWS['f16-128-dooff']['form'] == (ac.MFMA, ac.GENERIC)
    assert ac.view_offsets(ac.ROWS['f16-128-ldq'])['q'][2] % 8 == 4
    assert ac.view_offsets(ac.ROWS['f16-128-koff'])['k'][1] % 8 == 4 and ac.view_offsets(ac.ROWS['f16-128-dooff'])['dout'][1] % 8 == 4
    # generic rows: both dtypes, every N and head-dim pair, 1, 2 and 3 dead waves, the limits at N = 16 and 70, the long rowdot
    for dt in (ac.F32, ac.BF16):
        gen = [r for r in rows if r['dtype'] == dt and r['recipe'] in ('ragged', 'fused') and r['form'] == (ac.GENERIC, ac.GENERIC)]
        assert {r['N'] for r in gen} >= {1, 3, 5, 63, 65, 130}
        assert {(-r['N']) % 4 for r in gen if r['N'] > 1} == {0, 1, 2, 3} and all(r['N'] % 4 or r['N'] == 16 for r in gen)
        assert {(r['dqk'], r['dv']) for r in gen} >= set(ac.GENERIC_DIMS)
        assert {r['N'] for r in gen if (r['dqk'], r['dv']) == (128, 1024)} == {16, 70}
        assert {(r['B2'], r['kv_shift']) for r in gen} >= set(ac.SHIFTS)
        assert any(r['B2'] * r['N'] > 4096 * 4 and (r['B2'], r['N'], r['dqk'], r['dv']) == (16, 1030, 2, 8) for r in gen)
    for name in list(ac.OFFSET_ROWS) + list(ac.CHAINED_ROWS) + list(ac.MFMA_ROWS):
        assert name in ac.ROWS, name
    assert {(ac.ROWS[n]['dqk'], ac.ROWS[n]['dv']) for n in ac.OFFSET_ROWS} == set(ac.MFMA_DIMS) | set(ac.GENERIC_DIMS)
    assert {ac.ROWS[n]['form'][0] for n in ac.CHAINED_ROWS} == {ac.MFMA, ac.GENERIC}

    # ---- refusals: a negative answer and a message
    def refused(bwd, **change):
        d = _attn_fake_desc(base, 'soft', bwd)
        for k, v in change.items():
            setattr(d, k, v)
        lib.adn_attn_form(ctypes.byref(_attn_fake_desc(base, 'soft', bwd)), bwd)       # (a good call in between)
        rc = lib.adn_attn_form(ctypes.byref(d), bwd)
        return rc < 0 and lib.adn_last_error().startswith(b'adn_attn')
    assert lib.adn_attn_form(ctypes.byref(_attn_fake_desc(base, 'soft', 1)), 1) == 1
    for bwd in (0, 1):
        assert refused(bwd, dqk=129), bwd
        assert refused(bwd, dv=1025, ld_v=2048, ld_o=2048, ld_do=2048, ld_dv=2048), bwd
        assert refused(bwd, kv_shift=base['B2']), bwd
        assert refused(bwd, kv_shift=-1), bwd
        assert refused(bwd, ld_v=base['dv'] - 1), bwd
    assert refused(1, workspace_bytes=base['B2'] * base['N'] * 4 - 4)
    assert not refused(0, workspace_bytes=0)                                           # (the forward has no workspace)
    assert lib.adn_attn_form(None, 0) < 0
