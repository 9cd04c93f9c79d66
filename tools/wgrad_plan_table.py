"""Records what the weight-gradient plan queries answer for a table of descriptors (host only, no GPU).

    ADN_LIB=/path/to/libadn.so python tools/wgrad_plan_table.py > tests/golden/wgrad_plans.json
    python tools/wgrad_plan_table.py --query rows_patch_off      (prints the answers of one section of the committed table)

The table pins the plans (workspace bytes = split count x dW size, norm partial counts, batch classes) of the library it
was recorded from; tests/test_host_logic.py asserts that the built library still answers the same.  The `rows_patch_off`
section is queried with ADN_WGRAD_PATCH=0 (read once per process, so it needs a process of its own).
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, 'tests', 'golden', 'wgrad_plans.json')
F32, BF16 = 0, 1


def row(name, dtype, B, Hs, R0, R1, C0, C1, c_valid=0, ks=0, Ws=None):
    return dict(name=name, dtype=dtype, B=B, Hs=Hs, Ws=Hs if Ws is None else Ws, R0=R0, R1=R1, C0=C0, C1=C1,
                c_valid=c_valid, ks=ks)


def cases():
    rows = []
    # unet_256, ngf 64, B = 32: the six benchmarked shapes (tools/gemm_bench.py WGRAD) ...
    big = [('L1', 64, 128, 0, 64), ('L2', 32, 256, 0, 128), ('L3', 16, 512, 0, 256),
           ('D1', 64, 128, 128, 64), ('D2', 32, 256, 256, 128), ('D3', 16, 512, 512, 256)]
    # ... and the small levels below them (conv L4-L7, transposed conv D4-D7)
    small = [('L4', 8, 512, 0, 512), ('L5', 4, 512, 0, 512), ('L6', 2, 512, 0, 512), ('L7', 1, 512, 0, 512),
             ('D7', 1, 512, 0, 512), ('D6', 2, 512, 512, 512), ('D5', 4, 512, 512, 512), ('D4', 8, 512, 512, 512)]
    for dt, tag in ((BF16, 'bf16'), (F32, 'f32')):
        for name, hs, r0, r1, c in big + small:
            rows.append(row(f'unet256_{name}_{tag}', dt, 32, hs, r0, r1, c, 0))
        # outermost layers: two channels padded to a 16-byte chunk (c_valid < C), one gathered channel
        rows.append(row(f'unet256_L0_cvalid_{tag}', dt, 32, 128, 64, 0, 8, 0, c_valid=2))
        rows.append(row(f'unet256_D0_{tag}', dt, 32, 128, 64, 64, 1, 0))
        rows.append(row(f'cvalid_mfma_{tag}', dt, 4, 16, 128, 0, 64, 0, c_valid=48))
        # WG_SHAPES of tests/test_gpu_kernels.py: (B, R0, R1, Cg, Hs)
        for k, (b, r0, r1, cg, hs) in enumerate([(2, 128, 0, 64, 8), (2, 128, 128, 128, 4), (4, 128, 0, 64, 32),
                                                 (2, 64, 128, 96, 64), (16, 64, 0, 32, 16), (2, 8, 0, 6, 4),
                                                 (1, 4, 4, 1, 8)]):
            rows.append(row(f'wg_shape{k}_{tag}', dt, b, hs, r0, r1, cg, 0))
        # two gathered sources (k4: fast only when every column tile lies in one source), non-power-of-two image
        rows.append(row(f'k4_two_gath_{tag}', dt, 8, 4, 128, 0, 128, 128))
        rows.append(row(f'k4_two_gath64_{tag}', dt, 8, 4, 128, 0, 64, 64))
        rows.append(row(f'k4_npow2_{tag}', dt, 4, 6, 128, 0, 64, 0, Ws=10))
        # S1_WGRAD of tools/gemm_bench.py (RGBDepthNet, 256 x 256, B = 32): name, H, R, C0, C1
        for name, h, r, c0, c1 in [('inc2', 256, 64, 64, 0), ('up4c1', 256, 64, 64, 64), ('d1c2', 128, 128, 128, 0),
                                   ('up3c1', 128, 128, 128, 128), ('d2c2', 64, 256, 256, 0), ('d3c2', 32, 512, 512, 0)]:
            rows.append(row(f's1_{name}_{tag}', dt, 32, h, r, 0, c0, c1, ks=3))
        # stride 1 beyond the patch kernel: 1 x 1, tiles that straddle taps / sources (MIXED), R = 64 (HALF), odd images
        rows.append(row(f's1_k1_{tag}', dt, 32, 64, 128, 0, 256, 0, ks=1))
        rows.append(row(f's1_k1_half_{tag}', dt, 8, 32, 64, 0, 64, 0, ks=1))
        rows.append(row(f's1_c96_{tag}', dt, 4, 16, 128, 0, 96, 0, ks=3))
        rows.append(row(f's1_mixed_{tag}', dt, 4, 16, 128, 0, 64, 32, ks=3))
        rows.append(row(f's1_half_small_{tag}', dt, 2, 4, 64, 0, 64, 0, ks=3))
        rows.append(row(f's1_npow2_{tag}', dt, 2, 6, 128, 0, 64, 0, ks=3, Ws=10))
        rows.append(row(f's1_direct_{tag}', dt, 2, 8, 6, 0, 5, 0, ks=3))
        rows.append(row(f's1_cvalid_{tag}', dt, 8, 32, 64, 0, 8, 0, c_valid=3, ks=3))
    by_name = {r['name']: r for r in rows}
    groups = {
        'patch_L3_L2_L1': ['unet256_L3_bf16', 'unet256_L2_bf16', 'unet256_L1_bf16'],
        'patch_D1_D2_D3': ['unet256_D1_bf16', 'unet256_D2_bf16', 'unet256_D3_bf16'],
        'patch_pair': ['unet256_L1_bf16', 'unet256_D1_bf16'],
        'not_patch_small_level': ['unet256_L1_bf16', 'unet256_L5_bf16'],
        'not_patch_f32': ['unet256_L1_f32', 'unet256_L2_f32'],
        'not_patch_s1': ['s1_inc2_bf16', 's1_d1c2_bf16'],
    }
    off = ['unet256_L1_bf16', 'unet256_L3_bf16', 'unet256_D1_bf16', 'unet256_D3_bf16', 'unet256_L4_bf16',
           'wg_shape2_bf16', 'wg_shape3_bf16', 'wg_shape4_bf16', 's1_inc2_bf16', 's1_up4c1_bf16', 's1_d3c2_bf16',
           'unet256_L1_f32']
    return rows, {g: [by_name[n] for n in names] for g, names in groups.items()}, [by_name[n] for n in off]


def fill(d, r):
    from audio_depth_estimation_amd._lib import GEMM_S1
    d.dtype, d.B, d.Hs, d.Ws, d.R0, d.R1, d.C0, d.C1 = r['dtype'], r['B'], r['Hs'], r['Ws'], r['R0'], r['R1'], r['C0'], r['C1']
    d.c_valid = r['c_valid']
    d.geom, d.ks = (GEMM_S1, r['ks']) if r['ks'] else (0, 0)
    d.plain0 = d.gath0 = d.dw = 1            # host-only queries: operands only have to be non-null
    d.plain1 = 1 if r['R1'] else None
    d.gath1 = 1 if r['C1'] else None


def query_row(r):
    from audio_depth_estimation_amd import _lib
    lib = _lib.load()
    d = _lib.AdnWgradDesc()
    fill(d, r)
    return dict(workspace_bytes=int(lib.adn_wgrad_workspace_bytes(C.byref(d))),
                sq_count=int(lib.adn_wgrad_sq_count(C.byref(d))),
                batchable=int(lib.adn_wgrad_batchable(C.byref(d))),
                batch_sq_count=int(lib.adn_wgrad_batch_sq_count(C.byref(d))))


def query_group(rows):
    from audio_depth_estimation_amd import _lib
    arr = (_lib.AdnWgradDesc * len(rows))()
    for d, r in zip(arr, rows):
        fill(d, r)
    return int(_lib.load().adn_wgrad_patch_batch_workspace_bytes(arr, len(rows)))


def query_section(table, section):
    """The answers of the loaded library for one section of a table, in the table's form."""
    if section == 'groups':
        return {g: dict(rows=v['rows'], workspace_bytes=query_group(v['rows'])) for g, v in table['groups'].items()}
    return [dict(r, **query_row(r)) for r in table[section]]


def main():
    if len(sys.argv) == 3 and sys.argv[1] == '--query':
        table = json.load(open(TABLE))
        json.dump(query_section(table, sys.argv[2]), sys.stdout)
        return
    rows, groups, off = cases()
    table = dict(rows=rows, groups={g: dict(rows=v) for g, v in groups.items()}, rows_patch_off=off)
    out = dict(rows=query_section(table, 'rows'), groups=query_section(table, 'groups'))
    # ADN_WGRAD_PATCH is read once per process: the switched-off answers come from a child
    env = dict(os.environ, ADN_WGRAD_PATCH='0')
    code = ('import json, sys; sys.path.insert(0, %r); import wgrad_plan_table as t; '
            'json.dump([dict(r, **t.query_row(r)) for r in json.load(sys.stdin)], sys.stdout)' % os.path.dirname(os.path.abspath(__file__)))
    child = subprocess.run([sys.executable, '-c', code], input=json.dumps(off), env=env, capture_output=True, text=True,
                           check=True)
    out['rows_patch_off'] = json.loads(child.stdout)
    print('{')
    print(' "rows": [\n  ' + ',\n  '.join(json.dumps(r) for r in out['rows']) + '\n ],')
    print(' "groups": {\n  ' + ',\n  '.join('%s: %s' % (json.dumps(g), json.dumps(v)) for g, v in out['groups'].items())
          + '\n },')
    print(' "rows_patch_off": [\n  ' + ',\n  '.join(json.dumps(r) for r in out['rows_patch_off']) + '\n ]')
    print('}')


if __name__ == '__main__':
    main()
