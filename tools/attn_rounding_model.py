"""CPU models of the ROUNDINGS of the attention kernels, for the cases of tests/attn_cases.py and against the float64 reference
and the bounds of tests/test_gpu_attention.py.  Host only; not the kernels: the models hold the reference arithmetic at the
kernels' precision, so a case a model already misses has inputs the reference arithmetic cannot meet the bound on (change
the inputs, not the bound), and a case only the GPU misses points at the kernel.

  generic  everything in float32 (scores, exp, sums; dP summed in another order than D), outputs rounded to the storage dtype
  mfma     float64 with only the bf16 roundings of the MFMA path: P and dS as bf16 MFMA operands, bf16 outputs

    python tools/attn_rounding_model.py [row-name-substring]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import attn_cases as ac  # noqa: E402
import test_gpu_attention as tg  # noqa: E402


def bf(x):
    return x.to(torch.bfloat16).double()


def model(name, family, form):
    row, r = ac.ROWS[name], tg.reference(name, family)
    dt = tg.TORCH_DTYPE[row['dtype']]
    out = {x: torch.empty_like(r[x]) for x in ('o', 'dq', 'dk', 'dv')}
    lse = r['lse'].clone()
    for b in range(row['B2']):
        kb = (b + row['kv_shift']) % row['B2']
        if form == ac.GENERIC:
            q, k, v, do = (r[x].float() for x in ('q', 'k', 'v', 'dout'))
            sc = torch.tensor(r['scale']).float()
            S = (q[b] @ k[kb].t()) * sc
            m = S.max(-1, keepdim=True).values
            E = torch.exp(S - m)
            out['o'][b] = ((E @ v[kb]) / E.sum(-1, keepdim=True)).to(dt).double()
            lse[b] = (m[:, 0] + torch.log(E.sum(-1))).double()
            P = torch.exp(S - r['lse_in'][b][:, None])
            D = (do[b] * r['o_in'][b].float()).sum(-1)
            dS = P * ((do[b].double() @ v[kb].double().t()).float() - D[:, None]) * sc
            out['dq'][b], out['dk'][kb], out['dv'][kb] = ((dS @ k[kb]).to(dt).double(), (dS.t() @ q[b]).to(dt).double(),
                                                         (P.t() @ do[b]).to(dt).double())
        else:
            q, k, v, do, sc = r['q'], r['k'], r['v'], r['dout'], r['scale']
            S = (q[b] @ k[kb].t()) * sc
            E = torch.exp(S - S.max(-1, keepdim=True).values)
            out['o'][b] = bf((bf(E) @ v[kb]) / E.sum(-1, keepdim=True))
            P = torch.exp(S - r['lse_in'][b].double()[:, None])
            dS = bf(P * (do[b] @ v[kb].t() - r['dsum'][b][:, None]))          # unscaled, as the kernels hold it
            out['dq'][b], out['dk'][kb], out['dv'][kb] = bf(dS @ k[kb] * sc), bf(dS.t() @ q[b] * sc), bf(bf(P).t() @ do[b])
    bd = tg.bounds(row, r)
    e = {x: tg.batch_err(out[x], r[x]) for x in out}
    el = float((lse - r['lse']).abs().max())
    backward = family not in ('offset+', 'offset-')                         # the offset families run the forward only
    miss = e['o'] > bd['o'] or el > bd['lse'] or (backward and max(e['dq'], e['dk'], e['dv']) > bd['grad'])
    print('%-15s %-9s %-7s eff %5.2f  o %.1e / %.1e  lse %.1e / %.1e  dq %.1e dk %.1e dv %.1e / %.1e%s'
          % (name, family, form, r['eff_keys'], e['o'], bd['o'], el, bd['lse'], e['dq'], e['dk'], e['dv'], bd['grad'],
             '   MISSES' if miss else ''))
    return miss


if __name__ == '__main__':
    pick = sys.argv[1] if len(sys.argv) > 1 else ''
    missed = [c for c in tg.FWD_CASES if pick in c[0] and model(c[0], c[1], ac.form_of(ac.ROWS[c[0]], c[1], True))]
    print('%d case(s) beyond a bound in the model' % len(missed), missed)
