"""The host-side references of tests/test_gpu_weight_operands.py against torch itself, on the CPU: a reference that is
wrong would make the GPU tests wrong in the same way, so each is pinned to something that does not share its code."""
import numpy as np
import pytest
import torch

import weight_operand_cases as wc


@pytest.mark.parametrize('kind,wd', wc.KINDS)
@pytest.mark.parametrize('t', [1, 2, 1000])
def test_optimizer_reference_is_torch_optim(kind, wd, t):
    """One step of torch.optim (float64 parameters, state preset to step t - 1) == optimizer_reference."""
    g_ = torch.Generator().manual_seed(7 + t)
    n = 257
    p0, g = torch.randn(n, generator=g_, dtype=torch.float64), torch.randn(n, generator=g_, dtype=torch.float64)
    m0 = 0.1 * torch.randn(n, generator=g_, dtype=torch.float64)
    v0 = (0.1 * torch.randn(n, generator=g_, dtype=torch.float64)) ** 2
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    p = torch.nn.Parameter(p0.clone())
    if kind == 2:
        opt = torch.optim.SGD([p], lr=lr)
    else:
        cls = torch.optim.AdamW if kind == 0 else torch.optim.Adam
        opt = cls([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        opt.state[p] = {'step': torch.tensor(float(t - 1)), 'exp_avg': m0.clone(), 'exp_avg_sq': v0.clone()}
    coef = 0.37
    p.grad = g * coef
    opt.step()
    pr, mr, vr = wc.optimizer_reference(p0, g, m0, v0, kind, lr, b1, b2, eps, wd, coef, t)
    torch.testing.assert_close(pr, p.detach(), rtol=1e-12, atol=1e-14)
    if kind != 2:
        torch.testing.assert_close(mr, opt.state[p]['exp_avg'], rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(vr, opt.state[p]['exp_avg_sq'], rtol=1e-12, atol=1e-14)
    else:
        assert mr is not None and torch.equal(mr, m0) and torch.equal(vr, v0)


def test_every_term_of_the_update_clears_the_bar():
    """At the GPU test's hyper-parameters (lr 1e-2, wd 0.1, clip coefficient 0.37) leaving out the decay, the L2 term, the
    clip coefficient or a bias correction moves more than 95 % of the parameters past the bar and the worst one by at least
    40 bars: no element-wise comparison at that bar can let a missing term through."""
    g_ = torch.Generator().manual_seed(3)
    n = 4096
    p0, g = torch.randn(n, generator=g_), torch.randn(n, generator=g_)
    m0 = 0.1 * torch.randn(n, generator=g_)
    v0 = m0 ** 2 + (0.1 * torch.randn(n, generator=g_)) ** 2          # the GPU test's states: v >= m^2
    lr, b1, b2, eps = (wc.f32r(x) for x in (1e-2, 0.9, 0.999, 1e-8))

    def moved(a, b):          # the worst element, in bars, once more than 95 % of the elements are past the bar
        r = (a - b).abs() / (wc.OPT_ATOL + wc.OPT_RTOL * a.abs())
        return float(r.max()) if float((r > 1.0).float().mean()) >= 0.95 else 0.0

    for t in (1, 2, 1000):
        ref = lambda kind, wd, coef=0.37, tt=t: wc.optimizer_reference(p0, g, m0, v0, kind, lr, b1, b2, eps, wd, coef, tt)[0]
        assert moved(ref(0, 0.1), ref(0, 0.0)) >= 40          # decoupled decay
        assert moved(ref(1, 0.1), ref(1, 0.0)) >= 40          # L2 term
        for kind, wd in wc.KINDS:
            assert moved(ref(kind, wd), ref(kind, wd, coef=1.0)) >= 40       # clip coefficient
        assert moved(ref(1, 0.0), ref(1, 0.0, tt=t + 1 if t < 1000 else 10 * t)) >= 40      # bias corrections (step count)


def test_t2_reference_is_the_documented_permutation():
    X, Y = 6, 10
    w = torch.arange(X * Y * 16, dtype=torch.float32).view(X, Y, 4, 4)                 # torch layout [X, Y, kh, kw]
    master = w.permute(0, 2, 3, 1).reshape(X, 16, Y)                                   # channels_last memory
    t2 = wc.t2_reference(master)
    assert t2.shape == (4, Y, 4, X)
    for ph in range(2):
        for pw in range(2):
            for ty in range(2):
                for tx in range(2):
                    for x in range(X):
                        for y in range(Y):
                            assert t2[ph * 2 + pw, y, ty * 2 + tx, x] == w[x, y, wc.KH[(ph, ty)], wc.KH[(pw, tx)]]
    assert sorted(t2.flatten().tolist()) == sorted(master.flatten().tolist())          # a permutation
    # ... and the transposed convolution it serves: output row 2*i + ph takes input row i + dy through kernel row kh
    assert sorted(wc.KH.values()) == [0, 1, 2, 3]
    for (ph, t), kh in wc.KH.items():
        assert (kh - 1 - ph) % 2 == 0                      # oy = 2*iy - 1 + kh  =>  kh - 1 - ph even
    s2 = wc.s2_reference(master, 16)
    assert torch.equal(s2[:, :, :Y], master) and not s2[:, :, Y:].any()


def test_t2_table_layout():
    rows, m_total, t2_total, blocks = wc.t2_table()
    assert len(rows) == len(wc.T2_LAYERS)
    forms = set()
    for (m_off, X, Y, t2_off, blk), nxt in zip(rows, rows[1:] + [[m_total, 0, 0, t2_total, blocks]]):
        assert m_off % wc.ALIGN == 0 and X <= nxt[0] - (m_off + 16 * X * Y) < X + wc.ALIGN     # the gap the GPU test poisons
        assert nxt[3] == t2_off + 16 * X * Y
        assert nxt[4] - blk == 16 * -(-X // 64) * -(-Y // 64)
        forms.add(((X | Y) & 7 == 0, X % 64 != 0, Y % 64 != 0))
    assert {f[0] for f in forms} == {False, True}                          # scalar and vector form
    assert {(True, a, b) for a in (False, True) for b in (False, True)} <= forms     # full and partial tiles each way
    assert (4, 8) in wc.T2_LAYERS and 4 & 7 and not 8 & 7                            # X alone breaks the vector form


def test_bf16_reference_cast_is_round_to_nearest_even():
    names = [k for k in wc.EDGE_BITS if k != 'nan']
    b = np.array([wc.EDGE_BITS[k] for k in names], dtype=np.uint32)
    want = np.array([wc.EDGE_BF16[k] for k in names], dtype=np.uint16)
    np.testing.assert_array_equal(wc.bf16_rne_bits(b), want)
    got = wc.bits(wc.f32_from_bits(b).to(torch.bfloat16)).numpy().view(np.uint16)     # torch's cast: the GPU tests' reference
    np.testing.assert_array_equal(got, want)
    assert torch.isnan(wc.f32_from_bits([wc.EDGE_BITS['nan']]).to(torch.bfloat16)).all()
    rng = np.random.default_rng(0)
    r = rng.integers(0, 1 << 32, size=1 << 16, dtype=np.uint64).astype(np.uint32)
    r = r[(r & 0x7F800000) != 0x7F800000]                                              # finite ones
    got = wc.bits(wc.f32_from_bits(r).to(torch.bfloat16)).numpy().view(np.uint16)
    np.testing.assert_array_equal(got, wc.bf16_rne_bits(r))
    trunc = (r >> 16).astype(np.uint16)
    assert (trunc != got).mean() > 0.4                                                  # truncation is not this cast
