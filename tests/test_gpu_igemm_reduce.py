"""The split-K / direct slab reduce of adn_igemm: the vector form (igemm_reduce_vec_kernel, 16-byte accesses, every row of a
block in flight) against the scalar form (igemm_reduce_kernel), bit for bit, and the reduce against a CPU sum of the slabs.

ADN_IGEMM_REDUCE is read once per process, so the launches run in two fresh child processes (this file run as a script),
'scalar' (the reference: igemm_reduce_kernel everywhere) first, then 'vector', each under its own time limit; a child that
fails ends the run.  Each child asserts, through adn_igemm_describe, that every case has the plan it is there for (kind, split
count, rows per reduce block, whether the last row block is a partial one), launches every case and writes every output,
every partial row and (for the two cases of test_reduce_matches_cpu_sum_of_slabs) the workspace to one .npz.  The parent
process compares the two files byte for byte.

rb, the rows of a reduce block, is not part of the plan line; it is reduce_rows() of csrc/igemm.hip, restated in rows_per_block()
and tied to the plan line through partials == ceil(mout / rb).

Cases (bf16 unless marked; inputs seeded, both signs, so both sides of the LeakyReLU mask occur):
  d4_bwd        S2 B=32 8x8 C=64 N=512+512: rb 8, 4 splits, two segments, BWD with statistics and accumulate
  t2_zstats     T2 B=8 8x8 C=128 N=64: rb 2, N below one block's 256 channels, Z_STATS (with bias), four phases
  tail_b25      S2 B=25 8x8 C=64 N=1024: rb 6, 1600 rows: the last row block holds 4 rows; Z_STATS without bias
  odd_b24       S2 B=24 8x8 C=64 N=1024: 5 splits (odd: 4 + 1 in the grouped walk); BWD without accumulate, statistics on
                one segment only
  odd_b18       S2 B=18 8x8 C=64 N=512+512: 7 splits (4 + 2 + 1: every group size of the walk below 8); Z_STATS with bias
  ns64          S2 B=2 2x2 C=512 N=512: 64 splits (8 groups of 8), rb 1; Z_STATS
  l7_act        S2 B=32 1x1 C=512 N=512: 1 x 1 images, ACT with scale, shift, bias, both outputs
  raw / final / add  the t2_zstats shape: f32 outputs (RAW, FINAL sigmoid + bias), ADD with bias, scale, ref and accumulate
  f32_*         the t2_zstats shape in f32: Z_STATS, BWD with statistics and accumulate
  direct_n16    Direct kind, T2 B=4 24x24 C=6 N=16: rb 9 (> 8: a block walks its rows in two passes); Z_STATS and BWD
  direct_n10    Direct kind, S2 B=2 4x4 C=6 N=10: N is no multiple of 8, so BOTH modes run the scalar kernel (there is no
                vector path to compare: the case pins that the fallback is taken and still agrees)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 'f32', 'bf16'
S2, T2 = 0, 1
RAW, Z_STATS, ACT, BWD, FINAL, ADD = range(6)
MODES = ('scalar', 'vector')       # ADN_IGEMM_REDUCE of the two children (any value but 'scalar' leaves the default)
CHILD_TIMEOUT = 120           # seconds per child: a python start, ~20 small launches


def rows_per_block(mout, N):
    """reduce_rows() of csrc/igemm.hip."""
    return max(1, min(64, mout * (-(-N // 256)) // 1024))


def _case(dtype, geom, B, Hs, Ws, C, segs, epi, kind, nsplit, rb, tail=False, keep_ws=False, **opt):
    return dict(dtype=dtype, geom=geom, B=B, Hs=Hs, Ws=Ws, C=C, segs=segs, epi=epi, kind=kind, nsplit=nsplit, rb=rb,
                tail=tail, keep_ws=keep_ws, opt=opt)


_T2 = (T2, 8, 8, 8, 128, [64])
CASES = {
    'd4_bwd': _case(BF16, S2, 32, 8, 8, 64, [512, 512], BWD, 'tile', 4, 8, stats=(True, True), accumulate=True),
    't2_zstats': _case(BF16, *_T2, Z_STATS, 'tile', None, 2, bias=True),
    'tail_b25': _case(BF16, S2, 25, 8, 8, 64, [1024], Z_STATS, 'tile', None, 6, tail=True, keep_ws=True, bias=False),
    'odd_b24': _case(BF16, S2, 24, 8, 8, 64, [512, 512], BWD, 'tile', 5, 6, stats=(False, True), accumulate=False),
    'odd_b18': _case(BF16, S2, 18, 8, 8, 64, [512, 512], Z_STATS, 'tile', 7, 4, bias=True),
    'ns64': _case(BF16, S2, 2, 2, 2, 512, [512], Z_STATS, 'tile', 64, 1, bias=True),
    'l7_act': _case(BF16, S2, 32, 1, 1, 512, [512], ACT, 'tile', None, 1),
    'raw': _case(BF16, *_T2, RAW, 'tile', None, 2, keep_ws=True),
    'final': _case(BF16, *_T2, FINAL, 'tile', None, 2),
    'add': _case(BF16, *_T2, ADD, 'tile', None, 2),
    'f32_zstats': _case(F32, *_T2, Z_STATS, 'tile', None, 2, bias=True),
    'f32_bwd': _case(F32, *_T2, BWD, 'tile', None, 2, stats=(True,), accumulate=True),
    'direct_n16_zstats': _case(BF16, T2, 4, 24, 24, 6, [16], Z_STATS, 'direct', 1, 9, bias=True),
    'direct_n16_bwd': _case(BF16, T2, 4, 24, 24, 6, [16], BWD, 'direct', 1, 9, stats=(True,), accumulate=True),
    'direct_n10': _case(BF16, S2, 2, 4, 4, 6, [10], BWD, 'direct', 1, 1, stats=(True,), accumulate=True),
}
PROPERTY = {      # test -> its cases
    'rb8_two_segments_bwd': ['d4_bwd'],
    'rb2_narrow_zstats_four_phases': ['t2_zstats'],
    'partial_last_block_and_odd_splits': ['tail_b25', 'odd_b24', 'odd_b18'],
    'nsplit64_grouped_walk': ['ns64'],
    'onepx_act': ['l7_act'],
    'raw_final_add': ['raw', 'final', 'add'],
    'f32': ['f32_zstats', 'f32_bwd'],
    'direct_rb9_two_passes': ['direct_n16_zstats', 'direct_n16_bwd'],
    'scalar_fallback': ['direct_n10'],
}


# ---- child process: launches every case in one reduce mode ------------------------------------------------------------
def _child(out_path):
    import re
    import zlib

    import torch

    from audio_depth_estimation_amd import kernels as k

    dev = 'cuda'

    def rnd(g, *shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    out = {}
    for name, c in CASES.items():
        dtype = torch.bfloat16 if c['dtype'] == BF16 else torch.float32
        B, Hs, Ws, C, segs, epi, opt = c['B'], c['Hs'], c['Ws'], c['C'], c['segs'], c['epi'], c['opt']
        N = sum(segs)
        phases = 4 if c['geom'] == T2 else 1
        mout = B * Hs * Ws * phases
        # the plan has the property the case is there for
        plan = k.igemm_describe(dtype, c['geom'], B, Hs, Ws, C, 0, N, segs, epi=epi)
        m = re.match(r'(\S+) bm=\d+ bn=\d+ nsplit=(\d+) .* partials=(\d+) ws=(\d+)$', plan)
        kind, nsplit, P, ws_bytes = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
        assert kind == c['kind'], (name, plan)
        assert (nsplit > 1) == (kind == 'tile'), (name, plan)             # never an unsplit tile kernel: the reduce runs
        assert c['nsplit'] is None or nsplit == c['nsplit'], (name, plan)
        rb = rows_per_block(mout, N)
        assert rb == c['rb'] and P == -(-mout // rb), (name, plan, rb)
        assert (mout % rb != 0) == c['tail'], (name, mout, rb)
        assert ws_bytes == nsplit * mout * N * 4, (name, plan)
        # operands
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
        if c['geom'] == S2:
            x = rnd(g, B, 2 * Hs, 2 * Ws, C)
            X, Y, which = N, C, 0
        else:
            x = rnd(g, B, Hs, Ws, C)
            X, Y, which = C, N, 1
        master = rnd(g, X, 4, 4, Y, scale=0.1).to(dev)
        packs = (torch.empty(X, 16, Y, dtype=dtype, device=dev), torch.empty(4, Y, 4, X, dtype=dtype, device=dev))
        k.pack_weights(master, X, Y, dtype, *packs)
        in0 = x.to(dtype).to(dev)
        ws = torch.zeros(max(ws_bytes, 16) // 4, dtype=torch.float32, device=dev)
        seg_objs, keep = [], []
        for si, ch in enumerate(segs):
            def t(scale=1.0):
                return rnd(g, mout, ch, scale=scale).to(dtype).to(dev)

            def vec(lo, hi):
                return (torch.linspace(lo, hi, ch) + 0.2 * rnd(g, ch)).float().to(dev)
            part = torch.full((P, 2, ch), float('nan'), device=dev)
            odt = torch.float32 if epi in (RAW, FINAL) else dtype
            out0 = torch.full((mout, ch), float('nan'), dtype=odt, device=dev)
            kw, outs = {}, {'out0': out0}
            if epi == Z_STATS:
                kw = dict(partials=part, bias=vec(0.9, -0.7) if opt['bias'] else None)
                outs['partials'] = part
            elif epi == ACT:
                out1 = torch.full((mout, ch), float('nan'), dtype=dtype, device=dev)
                kw = dict(out1=out1, scale=vec(-1.5, 1.5), shift=vec(-0.8, 0.6), bias=vec(0.9, -0.7), slope=0.2)
                outs['out1'] = out1
            elif epi == BWD:
                kw = dict(ref=t(), slope=0.2, accumulate=opt['accumulate'])
                if opt['accumulate']:
                    out0.copy_(t(2.0))
                if opt['stats'][si]:
                    kw.update(z=t(), mean=vec(-0.3, 0.3), istd=vec(0.5, 2.0), partials=part)
                    outs['partials'] = part
            elif epi == FINAL:
                kw = dict(bias=vec(0.9, -0.7), final_act=1)
            elif epi == ADD:
                out0.copy_(t(2.0))
                kw = dict(bias=vec(0.9, -0.7), scale=vec(-1.5, 1.5), ref=t(), accumulate=True)
            seg_objs.append(k.Seg(ch, out0=out0, **kw))
            keep.append(outs)
        k.igemm(dtype, c['geom'], B, Hs, Ws, in0, None, packs[which], N, epi, seg_objs, ws)
        torch.cuda.synchronize()
        for si, outs in enumerate(keep):
            for key, ten in outs.items():
                out['%s/seg%d/%s' % (name, si, key)] = ten.cpu().contiguous().view(torch.uint8).numpy()
        if c['keep_ws']:
            out['%s/ws' % name] = ws.cpu().numpy().reshape(nsplit, mout, N)
    np.savez(out_path, **out)


# ---- parent process ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """{mode: arrays}: one child per mode, one after the other."""
    tmp = tmp_path_factory.mktemp('igemm_reduce')
    got = {}
    for mode in MODES:
        path = os.path.join(tmp, mode + '.npz')
        env = dict(os.environ, ADN_IGEMM_REDUCE=mode, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
        assert r.returncode == 0, '%s child failed (rc %d)\n%s\n%s' % (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        with np.load(path) as f:
            got[mode] = {key: f[key] for key in f.files}
    assert set(got['scalar']) == set(got['vector'])
    return got


def _same_bytes(runs, cases):
    checked = 0
    for key in sorted(runs['scalar']):
        if key.split('/')[0] not in cases or key.endswith('/ws'):
            continue
        a = runs['scalar'][key]
        for mode in MODES[1:]:
            b = runs[mode][key]
            assert a.dtype == np.uint8 and a.shape == b.shape and a.size > 0, key
            diff = int((a != b).sum())
            print('%s: %d bytes, %d differ in mode %s' % (key, a.size, diff, mode))
            assert diff == 0, (key, mode)
        checked += 1
    assert checked >= len(cases)
    return checked


def _f32(a):
    return a.view(np.float32)


def _written(runs, cases):
    """Nothing stayed at its NaN fill: every element of every output and partial row was written (in both modes: the
    bytes are equal).  bf16 NaN: exponent all ones, mantissa non-zero."""
    for key, a in runs['vector'].items():
        if key.split('/')[0] not in cases or key.endswith('/ws'):
            continue
        case = CASES[key.split('/')[0]]
        as_f32 = key.endswith('partials') or case['dtype'] == F32 or (key.endswith('out0') and case['epi'] in (RAW, FINAL))
        if as_f32:
            assert not np.isnan(_f32(a)).any(), key
        else:
            h = a.view(np.uint16)
            assert not (((h & 0x7f80) == 0x7f80) & ((h & 0x007f) != 0)).any(), key


def _check(runs, prop):
    """out0, out1 and every partial row of the property's cases: the same bytes from both kernels, all of them written."""
    _same_bytes(runs, PROPERTY[prop])
    _written(runs, PROPERTY[prop])


def test_rb8_two_segments_bwd_stats_accumulate(runs):
    _check(runs, 'rb8_two_segments_bwd')


def test_rb2_narrow_zstats_four_phases(runs):
    _check(runs, 'rb2_narrow_zstats_four_phases')


def test_partial_last_block_and_odd_split_counts(runs):
    _check(runs, 'partial_last_block_and_odd_splits')


def test_nsplit64_grouped_split_walk(runs):
    _check(runs, 'nsplit64_grouped_walk')


def test_onepx_act_scale_shift(runs):
    _check(runs, 'onepx_act')


def test_raw_final_add(runs):
    _check(runs, 'raw_final_add')


def test_f32_element_type(runs):
    _check(runs, 'f32')


def test_direct_kind_rb9_two_passes(runs):
    _check(runs, 'direct_rb9_two_passes')


def test_scalar_fallback_agrees(runs):
    _check(runs, 'scalar_fallback')


def test_scalar_fallback_case_has_no_vector_path():
    """direct_n10 is there for the fallback: its N is no multiple of 8, which the launch requires of the vector form."""
    assert sum(CASES['direct_n10']['segs']) % 8 != 0
    assert all(sum(c['segs']) % 8 == 0 and all(s % 8 == 0 for s in c['segs']) for n, c in CASES.items() if n != 'direct_n10')


def _bf16_rne(x):
    """float32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = x.astype(np.float32).view(np.uint32)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


@pytest.mark.parametrize('mode', MODES)
def test_reduce_matches_cpu_sum_of_slabs(runs, mode):
    """Independent of both kernels: the slabs adn_igemm left in the caller's workspace, summed on the CPU in float32 in split
    order from 0, rounded to bf16 (RNE), must equal the device z (Z_STATS without bias) / the f32 RAW output exactly, on every
    element.  The column sums of the partial rows must match the float64 column sums of v and v^2: a partial row is a
    float32 sum of rb <= 6 terms from 0 (error <= 6 * 2^-24 of the sum of the terms' magnitudes), the rows are added here in
    float64, so 1e-5 of sum|v| resp. sum v^2 per column is a bound with a margin of > 20x."""
    arr = runs[mode]
    for name in ('tail_b25', 'raw'):
        slabs = arr['%s/ws' % name]
        v = np.zeros(slabs.shape[1:], dtype=np.float32)
        for s in range(slabs.shape[0]):
            v = (v + slabs[s]).astype(np.float32)
        assert np.isfinite(v).all() and float(np.abs(v).max()) > 0.1
        if name == 'raw':
            got = _f32(arr['raw/seg0/out0']).reshape(v.shape)
            assert got.size == v.size and int((got.view(np.uint32) != v.view(np.uint32)).sum()) == 0
            continue
        got = arr['tail_b25/seg0/out0'].view(np.uint16).reshape(v.shape)
        assert got.size == v.size
        mism = int((got != _bf16_rne(v)).sum())
        print('%s %s: %d of %d elements differ' % (mode, name, mism, v.size))
        assert mism == 0
        part = _f32(arr['tail_b25/seg0/partials']).reshape(-1, 2, v.shape[1]).astype(np.float64).sum(0)
        v64 = v.astype(np.float64)
        e1 = np.abs(part[0] - v64.sum(0)) / np.abs(v64).sum(0)
        e2 = np.abs(part[1] - (v64 * v64).sum(0)) / (v64 * v64).sum(0)
        print('%s %s: column sums rel. err %.3e / %.3e' % (mode, name, e1.max(), e2.max()))
        assert e1.max() <= 1e-5 and e2.max() <= 1e-5


if __name__ == '__main__':
    _child(sys.argv[1])
