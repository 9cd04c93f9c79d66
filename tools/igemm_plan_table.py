"""Records which kernel form and tiling the implicit-GEMM planner picks for a table of descriptors (host only, no GPU).

    ADN_LIB=/path/to/libadn.so python tools/igemm_plan_table.py > tests/golden/igemm_plans.json
    python tools/igemm_plan_table.py --query rows_ring_off      (prints the answers of one section of the committed table)

Every row holds the line adn_igemm_describe writes (kernel form, tile, split count, grid, K-steps) beside the two older
queries (partial rows, workspace bytes).  The table pins the plans of the library it was recorded from;
tests/test_host_logic.py asserts that the built library still answers the same.  The `rows_*` knob sections are queried
with ADN_IGEMM_RING=0 / ADN_IGEMM_PATCH=0 / ADN_IGEMM_BN_T2=128 (read once per process: a process of their own).
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, 'tests', 'golden', 'igemm_plans.json')
F32, BF16 = 0, 1
S2, T2, S1 = 0, 1, 2
RAW, Z_STATS, ACT, BWD, FINAL, ADD = range(6)
KNOBS = {'rows_ring_off': {'ADN_IGEMM_RING': '0'}, 'rows_patch_off': {'ADN_IGEMM_PATCH': '0'},
         'rows_bn_t2_128': {'ADN_IGEMM_BN_T2': '128'}}


def row(name, dtype, geom, B, Hs, C0, C1, N, epi=RAW, segs=None, ks=0, Ws=None):
    return dict(name=name, dtype=dtype, geom=geom, B=B, Hs=Hs, Ws=Hs if Ws is None else Ws, C0=C0, C1=C1, N=N, epi=epi,
                segs=segs or [N], ks=ks)


def gpu_test_shapes():
    """The launches of the igemm tests of tests/test_gpu_kernels.py and tests/test_gpu_igemm_epilogues.py
    (igemm_launches() of the former builds them)."""
    import importlib.util
    sys.path.insert(0, os.path.join(ROOT, 'tests'))          # (the module imports its case tables from beside it)
    spec = importlib.util.spec_from_file_location('test_gpu_kernels', os.path.join(ROOT, 'tests', 'test_gpu_kernels.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.igemm_launches()


def cases():
    rows = []
    for dt, tag in ((BF16, 'bf16'), (F32, 'f32')):
        # ---- unet_256, ngf 64, B = 32: every layer with its real epilogue (forward, input gradient) ----
        cpad = 8 if dt == BF16 else 4                       # the outermost layers' thin operand, padded to a 16-byte chunk
        chans = [(cpad, 64), (64, 128), (128, 256), (256, 512), (512, 512), (512, 512), (512, 512), (512, 512)]
        for i, (cin, cout) in enumerate(chans):
            hs = 128 >> i
            inner = i == 7
            fwd_epi = ACT if i == 0 or inner else Z_STATS    # no BatchNorm on the outermost and innermost down convs
            rows.append(row(f'unet256_L{i}_fwd_{tag}', dt, S2, 32, hs, cin, 0, cout, fwd_epi))
            if i > 0:
                rows.append(row(f'unet256_L{i}_dgrad_{tag}', dt, T2, 32, hs, cout, 0, cin, BWD))
            # up path: input = [down activation | up output of the level below] (innermost: the down activation alone)
            c0, c1 = cout, 0 if inner else (cout if i < 7 else 0)
            n_up = cpad if i == 0 else cin
            if i > 0:
                rows.append(row(f'unet256_D{i}_fwd_{tag}', dt, T2, 32, hs, c0, c1, n_up, Z_STATS))
            rows.append(row(f'unet256_D{i}_dgrad_{tag}', dt, S2, 32, hs, n_up, 0, c0 + c1, BWD,
                            segs=[c0, c1] if c1 else [c0]))
        # ---- tools/gemm_bench.py: IGEMM and DEEP (Z_STATS; *_dgrad also with --bwd-epi), S1_IGEMM ----
        bench = [('L1_fwd', 0, 64, 64, 0, 128), ('L2_fwd', 0, 32, 128, 0, 256), ('L3_fwd', 0, 16, 256, 0, 512),
                 ('L4_fwd', 0, 8, 512, 0, 512), ('D1_fwd', 1, 64, 128, 128, 64), ('D2_fwd', 1, 32, 256, 256, 128),
                 ('D3_fwd', 1, 16, 512, 512, 256), ('D4_fwd', 1, 8, 512, 512, 512), ('D1_dgrad', 0, 64, 64, 0, 256),
                 ('D2_dgrad', 0, 32, 128, 0, 512), ('L2_dgrad', 1, 32, 256, 0, 128), ('L1_dgrad', 1, 64, 128, 0, 64),
                 ('L5_fwd', 0, 4, 512, 0, 512), ('L6_fwd', 0, 2, 512, 0, 512), ('L7_fwd', 0, 1, 512, 0, 512),
                 ('D7_fwd', 1, 1, 512, 0, 512), ('D6_fwd', 1, 2, 512, 512, 512), ('D5_fwd', 1, 4, 512, 512, 512),
                 ('D5_dgrad', 0, 4, 512, 0, 1024), ('D6_dgrad', 0, 2, 512, 0, 1024), ('L5_dgrad', 1, 4, 512, 0, 512)]
        for name, geom, hs, c0, c1, n in bench:
            rows.append(row(f'bench_{name}_{tag}', dt, geom, 32, hs, c0, c1, n, Z_STATS))
            if name.endswith('dgrad'):
                rows.append(row(f'bench_{name}_bwd_{tag}', dt, geom, 32, hs, c0, c1, n, BWD))
        for name, h, c0, c1, n in [('inc2_fwd', 256, 64, 0, 64), ('up4c1_fwd', 256, 64, 64, 64),
                                   ('up4c1_dgrad', 256, 64, 0, 128), ('d1c2_fwd', 128, 128, 0, 128),
                                   ('up3c1_fwd', 128, 128, 128, 128), ('d2c2_fwd', 64, 256, 0, 256),
                                   ('d3c2_fwd', 32, 512, 0, 512)]:
            rows.append(row(f'bench_s1_{name}_{tag}', dt, S1, 32, h, c0, c1, n, Z_STATS, ks=3))
        # ---- rule boundaries ----
        # S2 t128 = ceil(M / 128) * (N / 128) in [256, 512) -> 64 columns: 255, 256, 511, 512 (B x 16 x 16 images, N = 128 / 256)
        for b, n in ((127, 128), (128, 128), (255, 128), (128, 256), (129, 256)):
            rows.append(row(f'rule_s2_t128_b{b}_n{n}_{tag}', dt, S2, b, 16, 64, 0, n, RAW))
        # the same rule and the tall rule of the 3 x 3 stride-1 convs (M / 256 * (N / 64) >= 512)
        for b, hs, n in ((32, 32, 128), (64, 32, 128), (8, 16, 128), (127, 16, 128), (128, 16, 128), (32, 8, 128)):
            rows.append(row(f'rule_s1_b{b}_h{hs}_n{n}_{tag}', dt, S1, b, hs, 64, 0, n, Z_STATS, ks=3, Ws=16 if hs == 8 else None))
        # ring: M / 256 * (N / 128) * phases < 192 -> 64-column tiles (S2: B = 191 / 192 at 16 x 16; T2: B = 47 / 48)
        for b in (191, 192):
            rows.append(row(f'rule_ring_s2_b{b}_{tag}', dt, S2, b, 16, 64, 0, 128, Z_STATS))
        for b in (47, 48):
            rows.append(row(f'rule_ring_t2_b{b}_{tag}', dt, T2, b, 16, 128, 0, 128, Z_STATS))
        # ring needs Z_STATS / BWD, T2 a multiple of 128 gathered channels, N = 64 or a multiple of 128, 16 x 16 tiles
        rows.append(row(f'rule_ring_epi_act_{tag}', dt, S2, 64, 16, 64, 0, 128, ACT))
        rows.append(row(f'rule_ring_t2_c64_{tag}', dt, T2, 64, 16, 64, 0, 128, Z_STATS))
        rows.append(row(f'rule_ring_n64_{tag}', dt, S2, 64, 32, 64, 0, 64, Z_STATS))
        rows.append(row(f'rule_ring_n192_{tag}', dt, S2, 64, 32, 64, 0, 192, Z_STATS))
        rows.append(row(f'rule_ring_8x16_{tag}', dt, S2, 64, 8, 64, 0, 128, Z_STATS, Ws=16))
        # pair: M / 128 * (N / 128) * 4 >= 128 on 8 x 8 images, even B (N = 256: B = 30 / 32; odd B; N = 64)
        for b, n in ((30, 256), (32, 256), (33, 256), (64, 128), (62, 128), (64, 64)):
            rows.append(row(f'rule_pair_b{b}_n{n}_{tag}', dt, T2, b, 8, 128, 0, n, Z_STATS))
        rows.append(row(f'rule_pair_s2_{tag}', dt, S2, 32, 8, 128, 0, 256, Z_STATS))
        # patch tall: T2 M / 256 * (N / 64) * 4 >= 512 on images of 16 x 16 tiles (B = 127 / 128 at 16 x 16, N = 64)
        for b in (127, 128):
            rows.append(row(f'rule_tall_t2_b{b}_{tag}', dt, T2, b, 16, 64, 0, 64, RAW))
        # split-K: the cap of 16 slabs, lifted while the slabs fit in 4 MB (tinycap), the K-step bound, >= 256 tiles
        for b, hs, n in ((32, 1, 512), (32, 2, 512), (32, 4, 512), (64, 4, 512), (128, 4, 512), (32, 8, 512), (2, 16, 128),
                         (1, 2, 64)):
            rows.append(row(f'rule_split_b{b}_h{hs}_n{n}_{tag}', dt, S2, b, hs, 128, 0, n, RAW))
            rows.append(row(f'rule_split_t2_b{b}_h{hs}_n{n}_{tag}', dt, T2, b, hs, 128, 0, n, RAW))
        # tinycap: more than 16 slabs (bf16) while they stay within 4 MB: 64, 32, 16 splits
        for b, n in ((8, 128), (16, 512), (32, 512)):
            rows.append(row(f'rule_tinycap_b{b}_n{n}_{tag}', dt, S2, b, 2, 512, 0, n, RAW))
        # 256-row tiles: >= 256 of them and (64 columns or >= 32 K-steps)
        # (64 x 72 images: the patch kernel cannot tile them, so bf16 runs the tile kernel too)
        for b, c0, n in ((16, 64, 128), (16, 128, 128), (16, 64, 64), (14, 64, 64)):
            rows.append(row(f'rule_bm256_b{b}_c{c0}_n{n}_{tag}', dt, S2, b, 64, c0, 0, n, ACT, Ws=72))
        # images that are no power of two / not tileable, narrow channels (several taps per K-step), the direct path
        rows.append(row(f'npow2_s2_{tag}', dt, S2, 4, 6, 64, 0, 128, RAW, Ws=10))
        rows.append(row(f'npow2_t2_{tag}', dt, T2, 4, 6, 64, 64, 64, Z_STATS, Ws=10))
        rows.append(row(f'npow2_24x48_{tag}', dt, S2, 16, 24, 64, 0, 128, Z_STATS, Ws=48))
        rows.append(row(f'npow2_48x48_{tag}', dt, T2, 16, 48, 128, 0, 128, Z_STATS))
        rows.append(row(f'npow2_s1_{tag}', dt, S1, 2, 6, 64, 0, 128, ACT, ks=3, Ws=10))
        for c0 in (8, 16, 32):
            rows.append(row(f'narrow_s2_c{c0}_{tag}', dt, S2, 8, 32, c0, 0, 64, ACT))
            rows.append(row(f'narrow_t2_c{c0}_{tag}', dt, T2, 8, 32, c0, 0, 64, ACT))
        rows.append(row(f'narrow_s1_c8_{tag}', dt, S1, 8, 32, 8, 0, 64, ACT, ks=3))
        rows.append(row(f'narrow_f32_c4_{tag}', dt, S2, 8, 32, 4, 0, 64, ACT))
        rows.append(row(f's1_k1_{tag}', dt, S1, 8, 32, 128, 0, 256, ADD, ks=1))
        rows.append(row(f'direct_n10_{tag}', dt, S2, 2, 4, 6, 0, 10, RAW))
        rows.append(row(f'direct_two_src_{tag}', dt, T2, 1, 5, 3, 5, 1, RAW))
        rows.append(row(f'direct_seg96_{tag}', dt, S2, 4, 16, 64, 0, 192, BWD, segs=[96, 96]))
        rows.append(row(f'direct_s1_{tag}', dt, S1, 2, 8, 5, 0, 6, RAW, ks=3))
    rows += gpu_test_shapes()
    names = [r['name'] for r in rows]
    assert len(set(names)) == len(names), 'duplicate row names'
    pick = lambda *keys: [r for r in rows if r['dtype'] == BF16 and any(k in r['name'] for k in keys)]
    knob_rows = {'rows_ring_off': pick('unet256_', 'rule_ring_', 'bench_D1_dgrad'),
                 'rows_patch_off': pick('unet256_', 'rule_pair_', 'rule_tall_', 'bench_s1_'),
                 'rows_bn_t2_128': pick('unet256_', 'rule_pair_', 'rule_tall_', 'rule_split_t2')}
    return rows, knob_rows


def fill(d, r):
    d.dtype, d.geom, d.B, d.Hs, d.Ws, d.C0, d.C1, d.N = r['dtype'], r['geom'], r['B'], r['Hs'], r['Ws'], r['C0'], r['C1'], r['N']
    d.epi, d.ks = r['epi'], r['ks']
    d.in0 = d.w = 1                          # host-only queries: operands only have to be non-null
    d.in1 = 1 if r['C1'] else None
    for k in range(2):
        d.seg[k].channels = r['segs'][k] if k < len(r['segs']) else 0
        d.seg[k].out0 = d.seg[k].ref = 1


def query_row(r):
    from audio_depth_estimation_amd import _lib
    lib = _lib.load()
    d = _lib.AdnIgemmDesc()
    fill(d, r)
    buf = C.create_string_buffer(160)
    rc = lib.adn_igemm_describe(C.byref(d), buf, len(buf))
    return dict(plan=buf.value.decode() if rc == 0 else 'error %d' % rc,
                num_partials=int(lib.adn_igemm_num_partials(C.byref(d))),
                workspace_bytes=int(lib.adn_igemm_workspace_bytes(C.byref(d))))


def query_section(table, section):
    """The answers of the loaded library for one section of a table, in the table's form."""
    return [dict(r, **query_row(r)) for r in table[section]]


def query_in_child(section, rows):
    """The knob sections: the environment is read once per process, so the answers come from a child."""
    code = ('import json, sys; sys.path.insert(0, %r); import igemm_plan_table as t; '
            'json.dump([dict(r, **t.query_row(r)) for r in json.load(sys.stdin)], sys.stdout)' % os.path.dirname(os.path.abspath(__file__)))
    child = subprocess.run([sys.executable, '-c', code], input=json.dumps(rows), env=dict(os.environ, **KNOBS[section]),
                           capture_output=True, text=True, check=True)
    return json.loads(child.stdout)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == '--query':
        table = json.load(open(TABLE))
        json.dump(query_section(table, sys.argv[2]), sys.stdout)
        return
    rows, knob_rows = cases()
    out = dict(rows=query_section(dict(rows=rows), 'rows'))
    for section, sel in knob_rows.items():
        strip = [{k: v for k, v in r.items() if k not in ('plan', 'num_partials', 'workspace_bytes')} for r in sel]
        out[section] = query_in_child(section, strip)
    print('{')
    print(',\n'.join(' %s: [\n  ' % json.dumps(s) + ',\n  '.join(json.dumps(r) for r in v) + '\n ]' for s, v in out.items()))
    print('}')


if __name__ == '__main__':
    main()
