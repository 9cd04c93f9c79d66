"""Per-kernel resource and instruction census of one csrc/*.hip source, for before / after tables (no GPU needed).

    python tools/isa_kernel_census.py igemm [--csrc OTHER/csrc] [--match igemm_]

Compiles the source to gfx950 assembly the way tools/isa_lds_waits.py does and prints, per kernel symbol: VGPRs, AGPRs,
SGPRs, scratch bytes, static LDS bytes, occupancy (waves per SIMD) as the assembler reports them, the instruction count, and
the counts of MFMA / ds_read / buffer-load-to-LDS / s_barrier instructions in the whole kernel and between its first and last
s_barrier (the K loop plus a little of the epilogue, see isa_lds_waits.py).  --csrc points at another checkout's csrc.
"""
import argparse
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO = {'NumVgprs': 'vgpr', 'NumAgprs': 'agpr', 'TotalNumSgprs': 'sgpr', 'ScratchSize': 'scratch', 'LDSByteSize': 'lds',
        'Occupancy': 'occ'}


def parse(path):
    out, cur, last = {}, None, None
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        t = line.strip()
        if m:
            cur = last = m.group(1)
            out[cur] = dict(lines=[])
        elif cur is not None:
            if t and not t.startswith(';') and not t.startswith('.'):
                out[cur]['lines'].append(t)
            if t.startswith('s_endpgm'):
                cur = None
        elif last is not None:
            m = re.match(r'^;\s*(\w+):\s*(\d+)', t)
            if m and m.group(1) in INFO and INFO[m.group(1)] not in out[last]:
                out[last][INFO[m.group(1)]] = int(m.group(2))
    return out


def count(lines):
    c = dict(mfma=0, ds_read=0, dma=0, barrier=0)
    for ln in lines:
        o = ln.split()[0]
        c['mfma'] += o.startswith('v_mfma')
        c['ds_read'] += o.startswith('ds_read')
        c['dma'] += o.startswith('buffer_load') and ' lds' in ln
        c['barrier'] += o == 's_barrier'
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('name')
    ap.add_argument('--csrc', default=os.path.join(ROOT, 'audio-depth-estimation_amd', 'csrc'))
    ap.add_argument('--match', default='')
    args = ap.parse_args()
    filt = shutil.which('c++filt') or shutil.which('llvm-cxxfilt') or '/opt/rocm/llvm/bin/llvm-cxxfilt'
    s = os.path.join(tempfile.mkdtemp(), args.name + '.s')
    subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=fast',
                    '--cuda-device-only', '-S', '-o', s, os.path.join(args.csrc, args.name + '.hip'), '-I', args.csrc,
                    '-I', os.path.join(os.path.dirname(os.path.dirname(args.csrc)), 'include')], check=True,
                   stderr=subprocess.DEVNULL)
    print('vgpr agpr sgpr scratch    lds occ  insts | mfma ds_read  dma barrier | loop: mfma ds_read  dma  kernel')
    rows = []
    for k, v in parse(s).items():
        name = subprocess.run([filt, k], capture_output=True, text=True).stdout.strip()
        name = name.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
        if args.match not in name:
            continue
        lines = v['lines']
        a = count(lines)
        bars = [i for i, ln in enumerate(lines) if ln.split()[0] == 's_barrier']
        b = count(lines[bars[0]:bars[-1]]) if len(bars) >= 2 else dict(mfma=0, ds_read=0, dma=0)
        rows.append((name, '%4d %4d %4d %7d %6d %3d %6d | %4d %7d %4d %7d | %10d %7d %4d  %s' % (
            v.get('vgpr', -1), v.get('agpr', -1), v.get('sgpr', -1), v.get('scratch', -1), v.get('lds', -1), v.get('occ', -1),
            len(lines), a['mfma'], a['ds_read'], a['dma'], a['barrier'], b['mfma'], b['ds_read'], b['dma'], name)))
    for _, r in sorted(rows):
        print(r)


if __name__ == '__main__':
    main()
