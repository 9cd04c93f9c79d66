"""Every form the kernels of csrc/adabins.hip and csrc/baseres.hip can take, against torch-CPU float64 on the same inputs.

bf16 cases round the inputs to bf16 first (what the kernel reads); gradients come from autograd; every output (and
every workspace) is filled with NaN before the launch, so an element the kernel skips fails the comparison.

Bounds: f32 outputs <= 2e-5 of max|ref|, bf16-stored outputs <= 6e-3 of max|ref|; a reduced sum is bounded per output
element by 2e-5 * sum|summands| (absolute sum in float64, the scale test_relu_bwd_stats uses; the longest f32 chain of
rowsum_partial is ~260 terms, 260 * 2^-24 = 1.6e-5).  HW <= 5000 in the reduction cases: one dropped or doubled row
moves a sum by >= 2e-4 of sum|x|.  The loss kernels run on a grid of multiples of 0.25, where every difference is
exactly 0 or >= 0.25 (asserted), so sign() and the clamp's pass band have no near-ties.

Branch reached by each case (pool_parts / blocks_for / the dispatch of adn_bins_fwd in csrc/adabins.hip):

pool (B, HW, C, ld), each in f32 and bf16, nq = 1 (mean) and nq = 3 (sums for the feature cosine):
  (2, 60, 24, 24)        P = 1, 8-channel vector path, rpi = 85 (the shape test_gpu_adabins.py has)
  (2, 65, 8, 8)          P = 2, rpi = 256 (one channel group, every thread a row)
  (3, 130, 192, 192)     P = 3, rpb = 44, ragged last part (42 rows), rpi = 10 with 16 idle threads
  (2, 4097, 64, 64)      P capped at 64, rpb = 65, last part of 2 rows
  (1, 5000, 128, 136)    ld > C on the vector path, P capped
  (2, 200, 2048, 2048)   rpi = 1 (256 channel groups), P = 4
  (1, 70, 2056, 2056)    C > 2048: the scalar rowsum path, channel loop of 9 passes, P = 2
  (2, 333, 5, 5)         scalar rowsum path (C % 8 != 0), P = 6, ragged
  (2, 129, 12, 20)       scalar rowsum path with ld > C, P = 3
bins_fwd / bins_bwd (B, HW, nb), f32 and bf16, backward with dmean and with dmean = None:
  (2, 63, 128)           bf16: bins_fwd_vec_kernel<16>; f32: generic kernel, lanes u = 0, 1; backward P = 1
  (2, 63, 64)            bf16: bins_fwd_vec_kernel<8>
  (3, 130, 64)           bins_fwd_vec_kernel<8> with a dead tail (390 pixels, 32 per block); backward P = 3, ragged
  (2, 4100, 128)         backward P capped at 64, rpb = 65
  (2, 77, 100)           the bf16 generic bins kernel (nb not 64 / 128), u = 1 partly masked
  (2, 77, 16)            nb < 64: lanes >= nb masked in u = 0
  (1, 70, 256)           nb = kMaxBins, lanes u = 2, 3
  (2, 5, 1)              one bin: softmax == 1, base == centre
  forward only (2, 33001, 128) bf16      grid-stride loop of the vector kernel (66 002 pixels > 65 536)
  forward only (1, 16500, 100) both      grid-stride loop of the generic kernel (16 500 pixels > 16 384), f32 and bf16
  forward, bf16 nb = 128 on a view 2 bytes past a 16-byte boundary: must take the generic kernel
binpred_fwd / binpred_bwd (B, Cb, Hd, nb), with a dropout mask and without:
  (3, 512, 256, 128)     the model's shape
  (2, 1024, 256, 256)    the limits kMaxBott / kMaxHid / kMaxBins that size the LDS arrays
  (5, 100, 37, 5)        sizes that are no multiple of 64 or 256; nb < 64: one-wave softmax
  (1, 64, 64, 64)        exactly one wave of everything
  Cb = 1025, Hd = 257, nb = 257: RuntimeError, nothing written
bcast_add / featcos_grad (B, HW, C), f32 and bf16, bcast_add with accumulate on and off:
  (2, 60, 24)            one pass
  (3, 1, 128)            HW = 1: the engine's view(-1, 1, 1, C) form
  (2, 4200, 64)          537 600 elements, 2100 blocks: more than half of the grid cap
  (2, 4200, 128)         1 075 200 elements > 4096 x 256: the grid-stride loop (the (2, 4200, 64) case stays under it)
  (1, 7, 5)              less than one block
  featcos_grad (2, 60, 24) with a dead channel in a and another in r (the eps branches of F.normalize)
distill_pix_stats / distill_pix_grad / baseres_stats / baseres_grad / clamp_add, n =
  128                    one block
  2049                   nbk = 2
  70 000                 nbk = 35, 274 blocks in the gradient kernel
  2 097 152 + 3*2048 + 5 nbk capped at 1024 (stride loop of 3 passes), gradient kernel over its 4096-block cap
  2049 all invalid       N = 0: NaN terms, gradients exactly 0 (distill) / g_final routed by the clamp only (baseres)
distill_small (B, nb): (2, 16), (3, 128), (1, 256) = kMaxBins, (4, 100), feature channels 8, 12, 5, 64, 300 (B * C over
  and under one 256-thread pass)

One-line mutations of the kernels that these cases catch and the one-shape tests of test_gpu_adabins.py cannot
(reasoned from the code, never run):
  * rowsum_partial, ``r1 = r0 + rpb`` without the clamp to HW: pool (3, 130, 192, 192) has rpb = 44, so the last part
    would also sum rows 130 and 131 -- the next sample's first two rows -- and move every mean by ~2/130 of sum|x|;
    at HW = 60 there is one part with rpb == HW and the clamp never acts.  bins_bwd (3, 130, 64) does the same for dcent.
  * adn_pool handing rowsum_final the uncapped cdiv(HW, 64) = 65 instead of P = 64: pool (2, 4097, 64, 64) then strides
    the partials by 65 per sample, so sample 0 also adds sample 1's first part (65 rows too many); P = 1 at HW = 60.
  * bins_fwd_vec_kernel with NB fixed at 128 (or the <8> launch sized like <16>): (2, 63, 64) and (3, 130, 64) in bf16
    read every pixel's bins at twice their stride; only nb = 128 ran before.
  * sum4_kernel / baseres_total_kernel given the uncapped cdiv(n, 2048) = 1028: the n = 2 103 301 case sums four rows of
    the workspace no block wrote (NaN-filled here); at n = 128 there is one block.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
F32, BF16 = torch.float32, torch.bfloat16
TOL = {F32: 2e-5, BF16: 6e-3}
SUM_TOL = 2e-5
DTYPES = [F32, BF16]


def K():
    from audio_depth_estimation_amd import kernels
    return kernels


def gen(seed):
    return torch.Generator().manual_seed(seed)


def nans(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def f64(t):
    return t.detach().cpu().double()


def max_err(got, ref):
    return float((f64(got).reshape(ref.shape) - ref).abs().max())


def check_max(got, ref, tol, what=''):
    """max|got - ref| <= tol * max|ref| (NaN in got fails)."""
    err, scale = max_err(got, ref), float(ref.abs().max())
    assert err <= tol * scale, (what, err, tol * scale)


def check_sum(got, ref, abs_sum, what=''):
    """Every element of a reduced sum within SUM_TOL of the absolute sum of its summands."""
    err = (f64(got).reshape(ref.shape) - ref).abs()
    ok = err <= SUM_TOL * abs_sum
    assert bool(ok.all()), (what, float((err / abs_sum.clamp_min(1e-300)).nan_to_num(nan=float('inf')).max()))


# ---- pool ---------------------------------------------------------------------------------------------------------
POOL_CASES = [(2, 60, 24, 24), (2, 65, 8, 8), (3, 130, 192, 192), (2, 4097, 64, 64), (1, 5000, 128, 136),
              (2, 200, 2048, 2048), (1, 70, 2056, 2056), (2, 333, 5, 5), (2, 129, 12, 20)]


@pytest.mark.parametrize('nq', [1, 3])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,HW,C,ld', POOL_CASES)
def test_pool(B, HW, C, ld, dtype, nq):
    g = gen(100 + HW)
    x = torch.randn(B, HW, C, generator=g).to(dtype)
    y = (0.5 * x.float() + torch.randn(B, HW, C, generator=g)).to(dtype)

    def padded(t):                                  # [B, HW, ld] with NaN in the columns the kernel must not read
        buf = torch.full((B, HW, ld), NAN, dtype=dtype)
        buf[..., :C] = t
        return buf.to(DEV)

    k = K()
    ws = nans(k.pool_workspace_bytes(B, HW, C, nq) // 4)
    xd, yd = x.double(), y.double()
    if nq == 1:
        out = nans(B, C)
        k.pool(padded(x), None, B, HW, C, 1, 1.0 / HW, out, ws)
        check_sum(out, xd.sum(1) / HW, xd.abs().sum(1) / HW, 'mean')
        return
    out = nans(B, 3, C)
    k.pool(padded(x), padded(y), B, HW, C, 3, 1.0, out, ws)
    ref = torch.stack([(xd * xd).sum(1), (yd * yd).sum(1), (xd * yd).sum(1)], 1)
    check_sum(out, ref, torch.stack([ref[:, 0], ref[:, 1], (xd * yd).abs().sum(1)], 1), 'sums')
    st = f64(out)
    cos = (F.normalize(xd, dim=1) * F.normalize(yd, dim=1)).sum(1)
    check_max(st[:, 2] / (st[:, 0].sqrt() * st[:, 1].sqrt()), cos, 2e-5, 'cosine')


def test_pool_refuses_a_channel_sliced_view():
    """kernels.pool takes the row stride from x.shape[-1]: buf[..., :C] would be summed with the wrong stride."""
    k = K()
    buf = torch.randn(2, 60, 32, device=DEV)
    out, ws = nans(2, 24), nans(k.pool_workspace_bytes(2, 60, 24, 3) // 4)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.pool(buf[..., :24], None, 2, 60, 24, 1, 1.0, out, ws)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.pool(buf, buf.transpose(0, 1).contiguous().transpose(0, 1), 2, 60, 24, 3, 1.0, nans(2, 3, 24), ws)
    with pytest.raises(RuntimeError):
        k.pool(buf, buf[:1], 2, 60, 24, 3, 1.0, nans(2, 3, 24), ws)       # y of another shape
    assert bool(torch.isnan(out).all())
    k.pool(buf, None, 2, 60, 24, 1, 1.0 / 60, out, ws)                     # the whole buffer with Cc = 24 is the way
    check_sum(out, f64(buf)[..., :24].sum(1) / 60, f64(buf)[..., :24].abs().sum(1) / 60)


# ---- soft binning ---------------------------------------------------------------------------------------------------
BINS_CASES = [(2, 63, 128), (2, 63, 64), (3, 130, 64), (2, 4100, 128), (2, 77, 100), (2, 77, 16), (1, 70, 256), (2, 5, 1)]


def _bins_inputs(B, HW, nb, dtype):
    g = gen(200 + HW + nb)
    logits = (2 * torch.randn(B, 1, HW, nb, generator=g)).to(dtype)
    cent = torch.rand(B, nb, generator=g).cumsum(1)
    return logits, cent


def _bins_ref(logits, cent):
    p = torch.softmax(logits.double(), -1)
    return p, (p * cent.double()[:, None, None, :]).sum(-1)


def _bins_fwd(logits_dev, cent):
    B, _, HW, _ = logits_dev.shape
    base = nans(B * HW)
    K().bins_fwd(logits_dev, cent.to(DEV), base)
    return base


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,HW,nb', BINS_CASES + [(1, 16500, 100)])
def test_bins_fwd(B, HW, nb, dtype):
    logits, cent = _bins_inputs(B, HW, nb, dtype)
    _, ref = _bins_ref(logits, cent)
    check_max(_bins_fwd(logits.to(DEV), cent), ref.reshape(-1), 2e-5, 'base')       # the output is f32 in both dtypes


def test_bins_fwd_vector_kernel_grid_stride():
    logits, cent = _bins_inputs(2, 33001, 128, BF16)
    _, ref = _bins_ref(logits, cent)
    check_max(_bins_fwd(logits.to(DEV), cent), ref.reshape(-1), 2e-5, 'base')


def test_bins_fwd_bf16_view_off_the_16_byte_boundary():
    """Element offset 1 of a flat bf16 buffer: 16-byte loads would be misaligned, the generic kernel must run."""
    B, HW, nb = 2, 63, 128
    logits, cent = _bins_inputs(B, HW, nb, BF16)
    _, ref = _bins_ref(logits, cent)
    n = logits.numel()
    flat = torch.zeros(n + 8, dtype=BF16, device=DEV)
    view = flat[1:1 + n].view(B, 1, HW, nb)
    view.copy_(logits)
    assert view.data_ptr() % 16 == 2 and view.is_contiguous()
    off, aligned = _bins_fwd(view, cent), _bins_fwd(logits.to(DEV), cent)
    scale = float(ref.abs().max())
    check_max(off, ref.reshape(-1), 2e-5, 'off-boundary view')
    assert float((off - aligned).abs().max()) <= 2e-5 * scale


@pytest.mark.parametrize('with_dmean', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,HW,nb', BINS_CASES)
def test_bins_bwd(B, HW, nb, dtype, with_dmean):
    logits, cent = _bins_inputs(B, HW, nb, dtype)
    g = gen(300 + HW + nb)
    dbase = torch.randn(B, HW, generator=g)
    dmean = torch.randn(B, nb, generator=g) if with_dmean else None
    lg = logits.double().requires_grad_(True)
    ct = cent.double().requires_grad_(True)
    p = torch.softmax(lg, -1)
    loss = ((p * ct[:, None, None, :]).sum(-1).view(B, HW) * dbase.double()).sum()
    if with_dmean:
        loss = loss + (lg.mean((1, 2)) * dmean.double()).sum()
    loss.backward()
    k = K()
    ld = logits.to(DEV)
    base = _bins_fwd(ld, cent)
    dl = nans(B, 1, HW, nb, dtype=dtype)
    dc = nans(B, nb)
    ws = nans(k.bins_bwd_workspace_bytes(B, HW, nb) // 4)
    k.bins_bwd(ld, cent.to(DEV), base, dbase.reshape(-1).to(DEV), dmean.to(DEV) if with_dmean else None, dl, dc, ws)
    check_max(dl, lg.grad, TOL[dtype], 'dlogits')
    check_sum(dc, ct.grad, (p.detach().view(B, HW, nb) * dbase.double()[:, :, None]).abs().sum(1), 'dcent')


def test_bins_and_pointwise_wrappers_refuse_strided_operands():
    k = K()
    B, HW, nb = 2, 6, 16
    wide = torch.randn(B, 1, HW, 2 * nb, device=DEV)
    lg, cent, base = wide[..., :nb].contiguous(), torch.rand(B, nb, device=DEV), nans(B * HW)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.bins_fwd(wide[..., :nb], cent, base)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.bins_fwd(lg, torch.rand(nb, B, device=DEV).t(), base)
    assert bool(torch.isnan(base).all())
    k.bins_fwd(lg, cent, base)
    dl, dc = nans(B, 1, HW, nb), nans(B, nb)
    ws = nans(k.bins_bwd_workspace_bytes(B, HW, nb) // 4)
    db = torch.randn(B * HW, device=DEV)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.bins_bwd(wide[..., :nb], cent, base, db, None, dl, dc, ws)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.bins_bwd(lg, cent, base, db, None, nans(B, 1, HW, 2 * nb)[..., :nb], dc, ws)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.bins_bwd(lg, cent, base, db, torch.rand(nb, B, device=DEV).t(), dl, dc, ws)
    assert bool(torch.isnan(dl).all()) and bool(torch.isnan(dc).all())
    gx, dg = nans(B, 1, HW, 2 * nb), torch.randn(B, nb, device=DEV)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.bcast_add(gx[..., :nb], dg, 1.0, False)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.bcast_add(dl, torch.randn(nb, B, device=DEV).t(), 1.0, False)
    assert bool(torch.isnan(gx).all()) and bool(torch.isnan(dl).all())
    st = torch.ones(B, 3, nb, device=DEV)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.featcos_grad(wide[..., :nb], lg, st, 1.0, dl)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.featcos_grad(lg, wide[..., nb:], st, 1.0, dl)
    with pytest.raises(RuntimeError, match='contiguous'):
        k.featcos_grad(lg, lg, st, 1.0, gx[..., :nb])
    assert bool(torch.isnan(gx).all()) and bool(torch.isnan(dl).all())


# ---- bin predictor ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_mask', [True, False])
@pytest.mark.parametrize('B,Cb,Hd,nb', [(3, 512, 256, 128), (2, 1024, 256, 256), (5, 100, 37, 5), (1, 64, 64, 64)])
def test_binpred(B, Cb, Hd, nb, with_mask):
    g = gen(400 + Cb + nb)
    maxd, p = 30.0, 0.1
    r = lambda *s: torch.randn(*s, generator=g)
    gf, W1, b1 = r(B, Cb), r(Hd, Cb) * (1.6 / Cb ** 0.5), r(Hd) * 0.1
    W2, b2 = r(nb, Hd) * (1.6 / Hd ** 0.5), r(nb) * 0.1
    mask = torch.rand(B, Hd, generator=g) > p
    dc = r(B, nb)
    leaves = [t.double().requires_grad_(True) for t in (gf, W1, b1, W2, b2)]
    g_, W1_, b1_, W2_, b2_ = leaves
    h = F.relu(F.linear(g_, W1_, b1_))
    if with_mask:
        h = h * mask.double() / (1.0 - p)
    w = torch.softmax(F.linear(h, W2_, b2_), 1)
    edges = torch.cat([torch.zeros(B, 1, dtype=torch.float64), torch.cumsum(w, 1)], 1) * maxd
    cent = (edges[:, :-1] + edges[:, 1:]) / 2
    cent.backward(dc.double())
    k = K()
    dev = [t.to(DEV) for t in (gf, W1, b1, W2, b2)]
    md = mask.to(torch.uint8).to(DEV) if with_mask else None
    h1, wd, cd = nans(B, Hd), nans(B, nb), nans(B, nb)
    k.binpred_fwd(*dev, md, p, maxd, h1, wd, cd)
    check_max(h1, h.detach(), 2e-5, 'h1')
    check_max(wd, w.detach(), 2e-5, 'widths')
    check_max(cd, cent.detach(), 2e-5, 'centres')
    dW2p, db2p, dW1p, db1p, dg = nans(B, nb * Hd), nans(B, nb), nans(B, Hd * Cb), nans(B, Hd), nans(B, Cb)
    k.binpred_bwd(dc.to(DEV), wd, h1, dev[0], dev[1], dev[3], with_mask, p, maxd, dW2p, db2p, dW1p, db1p, dg)
    check_max(f64(dW2p).sum(0), W2_.grad.reshape(-1), 5e-5, 'dW2')
    check_max(f64(db2p).sum(0), b2_.grad, 5e-5, 'db2')
    check_max(f64(dW1p).sum(0), W1_.grad.reshape(-1), 5e-5, 'dW1')
    check_max(f64(db1p).sum(0), b1_.grad, 5e-5, 'db1')
    check_max(dg, g_.grad, 5e-5, 'dg')


@pytest.mark.parametrize('Cb,Hd,nb', [(1025, 256, 256), (1024, 257, 256), (1024, 256, 257)])
def test_binpred_over_its_limits_raises_and_writes_nothing(Cb, Hd, nb):
    k = K()
    B = 2
    z = lambda *s: torch.zeros(*s, device=DEV)
    gf, W1, b1, W2, b2 = z(B, Cb), z(Hd, Cb), z(Hd), z(nb, Hd), z(nb)
    h1, wd, cd = nans(B, Hd), nans(B, nb), nans(B, nb)
    with pytest.raises(RuntimeError):
        k.binpred_fwd(gf, W1, b1, W2, b2, None, 0.1, 30.0, h1, wd, cd)
    outs = [nans(B, nb * Hd), nans(B, nb), nans(B, Hd * Cb), nans(B, Hd), nans(B, Cb)]
    with pytest.raises(RuntimeError):
        k.binpred_bwd(z(B, nb), z(B, nb), z(B, Hd), gf, W1, W2, False, 0.1, 30.0, *outs)
    torch.cuda.synchronize()
    for t in [h1, wd, cd] + outs:
        assert bool(torch.isnan(t).all())


# ---- bcast_add / featcos_grad -------------------------------------------------------------------------------------------
POINT_CASES = [(2, 60, 24), (3, 1, 128), (2, 4200, 64), (2, 4200, 128), (1, 7, 5)]


@pytest.mark.parametrize('accumulate', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,HW,C', POINT_CASES)
def test_bcast_add(B, HW, C, dtype, accumulate):
    g = gen(500 + HW + C)
    gx0 = torch.randn(B, 1, HW, C, generator=g).to(dtype)
    dg = torch.randn(B, C, generator=g)
    scale = 0.37
    ref = (dg.double() * scale)[:, None, None, :].expand(B, 1, HW, C)
    gx = gx0.to(DEV) if accumulate else nans(B, 1, HW, C, dtype=dtype)
    if accumulate:
        ref = ref + gx0.double()
    K().bcast_add(gx, dg.to(DEV), scale, accumulate)
    check_max(gx, ref, TOL[dtype])


def _featcos(B, HW, C, dtype, dead):
    g = gen(600 + HW + C)
    a = torch.randn(B, 1, HW, C, generator=g)
    r = 0.5 * a + torch.randn(B, 1, HW, C, generator=g)
    if dead:
        a[..., 3] = 0.0                       # ReLU features have dead channels: |a| = 0 in every sample
        r[..., 7] = 0.0
    a, r = a.to(dtype), r.to(dtype)
    ga0 = torch.randn(B, 1, HW, C, generator=g).to(dtype)
    coef = -1.0 / (B * C)
    ad = a.double().requires_grad_(True)
    rd = r.double()
    af, rf = F.normalize(ad.view(B, HW, C), dim=1), F.normalize(rd.view(B, HW, C), dim=1)     # over the pixels
    ((af * rf).sum(1).sum() * coef).backward()
    st = torch.stack([(ad.detach() ** 2).sum((1, 2)), (rd ** 2).sum((1, 2)), (ad.detach() * rd).sum((1, 2))], 1)
    want = ga0.double() + ad.grad
    ga = ga0.clone().to(DEV)
    K().featcos_grad(a.to(DEV), r.to(DEV), st.float().contiguous().to(DEV), coef, ga)
    return f64(ga), want


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,HW,C', POINT_CASES)
def test_featcos_grad(B, HW, C, dtype):
    """Float64 autograd through F.normalize over the pixels (utils_distillation_loss.py:72-98; the NHWC tensors are
    [B, 1, HW, C], so the reference's dim=2 of [B, C, HW] is dim 1 of the [B, HW, C] view here)."""
    got, want = _featcos(B, HW, C, dtype, dead=False)
    check_max(got, want, TOL[dtype])


@pytest.mark.parametrize('dtype', DTYPES)
def test_featcos_grad_dead_channels(dtype):
    """A channel of a that is 0 everywhere: F.normalize divides by eps = 1e-12, the gradient is coef * r / (eps |r|)
    (~1e10 here) -- compared on its own scale, so that it does not hide the live channels.  A dead channel of r: 0."""
    got, want = _featcos(2, 60, 24, dtype, dead=True)
    live = [c for c in range(24) if c != 3]
    check_max(got[..., live], want[..., live], TOL[dtype], 'live')
    check_max(got[..., 3], want[..., 3], TOL[dtype], 'dead a')
    assert float(want[..., 3].abs().max()) > 1e6
    assert float((got[..., 7] - want[..., 7]).abs().max()) <= TOL[dtype] * float(want[..., live].abs().max())


# ---- loss kernels on the 0.25 grid ----------------------------------------------------------------------------------------
N_CASES = [128, 2049, 70000, 2097152 + 3 * 2048 + 5]
MAXD = 30.0
LAM = (1.0, 0.5, 0.3, 0.2, 0.1)


def quarter(n, lo, hi, g):
    return torch.randint(int(lo * 4), int(hi * 4) + 1, (n,), generator=g).float() / 4


def assert_on_grid(*diffs):
    for d in diffs:
        a = d.abs()
        assert not bool(((a > 0) & (a < 0.25)).any())


def _pix_inputs(n, seed, all_invalid=False):
    """base, resid, gt, second map (teacher / structural target) on the 0.25 grid with the clamp's edges planted."""
    g = gen(seed)
    base, resid = quarter(n, -1, 31, g), quarter(n, -2, 2, g)
    gt, other = quarter(n, 0, 30, g), quarter(n, 0, 30, g)
    gt[gt < 5] = 0
    for o in (0, n - 16):                  # in the first and in the last block
        gt[o:o + 12] = 12.0
        base[o + 0], resid[o + 0] = 0.0, 0.0             # base + resid == 0 exactly, resid == 0
        base[o + 1], resid[o + 1] = 29.0, 1.0            # == max_depth exactly
        base[o + 2], resid[o + 2] = -1.0, 0.5            # below 0
        base[o + 3], resid[o + 3] = 30.5, 0.25           # above max_depth
        base[o + 4], resid[o + 4] = 10.0, 0.0            # resid == 0
        base[o + 5], resid[o + 5] = 11.5, 0.5            # final == gt
        base[o + 6], resid[o + 6] = 0.5, -0.5            # == 0 from a negative residual
        base[o + 7], resid[o + 7], other[o + 7] = 8.0, 1.0, 9.0      # final == teacher
        base[o + 8], other[o + 8] = 14.0, 14.0           # base == structural target
        base[o + 9], resid[o + 9], gt[o + 9] = 31.0, 1.0, 0.0        # out of range and invalid
        base[o + 10], resid[o + 10], gt[o + 10] = 30.0, 0.0, 0.0     # on the bound and invalid
    if all_invalid:
        gt.zero_()
    return base, resid, gt, other


def _small_inputs(B, nb, chans, seed):
    g = gen(seed)
    ms, mt = torch.randn(B, nb, generator=g), torch.randn(B, nb, generator=g)
    cs, ct = torch.rand(B, nb, generator=g).cumsum(1), torch.rand(B, nb, generator=g).cumsum(1)
    fa = [torch.randn(B, C, 2, 2, generator=g) for C in chans]
    fr = [0.5 * a + torch.randn(B, C, 2, 2, generator=g) for a, C in zip(fa, chans)]
    return ms, mt, cs, ct, fa, fr


def _distill(n, B, nb, chans, teacher, seed, all_invalid=False):
    """adn_distill_pix_stats -> adn_distill_small -> adn_distill_pix_grad against oracle.distillation_loss in float64."""
    from oracle import dcnet_oracle
    base, resid, gt, tfin = _pix_inputs(n, seed, all_invalid)
    ms, mt, cs, ct, fa, fr = _small_inputs(B, nb, chans, seed + 1)
    fin32 = torch.clamp(base + resid, 0, MAXD)
    assert_on_grid(fin32 - gt, fin32 - tfin, resid)
    shp = (1, 1, 1, n)
    D = lambda t: t.double().view(shp)
    bd, rd = D(base).requires_grad_(True), D(resid).requires_grad_(True)
    msd, csd = ms.double().requires_grad_(True), cs.double().requires_grad_(True)
    final = torch.clamp(bd + rd, 0, MAXD)
    feats = lambda fs: {f'x{i + 1}': f.double() for i, f in enumerate(fs)}
    spread = lambda m: m[:, :, None, None].expand(B, nb, 2, 2)
    out = {'audio': {'final_depth': final, 'features': feats(fa), 'bin_logits': spread(msd), 'bin_centers': csd,
                     'residual': rd},
           'rgb': {'final_depth': D(tfin), 'features': feats(fr), 'bin_logits': spread(mt.double()),
                   'bin_centers': ct.double()} if teacher else None}
    valid = D(gt) > 0
    total, parts = dcnet_oracle.distillation_loss(out, D(gt), valid, *LAM, 4.0)
    total.backward()
    want = torch.stack([parts[q].detach() for q in ('task', 'response', 'feature', 'bin', 'bin_centers', 'sparse')] +
                       [total.detach()])
    k = K()
    dev = lambda t: t.contiguous().to(DEV)
    stats = nans(4, dtype=torch.float64)
    ws = nans(8192 + 64)                   # 1024 block rows + NaN rows behind them
    fo = nans(n)
    bD, rD, gD, tD = dev(base), dev(resid), dev(gt), (dev(tfin) if teacher else None)
    k.distill_pix_stats(bD, rD, gD, tD, MAXD, fo, stats, ws)
    fst = []
    for a, r in zip(fa, fr):
        a2, r2 = a.double().flatten(2), r.double().flatten(2)
        fst.append(dev(torch.stack([(a2 * a2).sum(2), (r2 * r2).sum(2), (a2 * r2).sum(2)], 1).float()))
    terms, dmean, dcent = nans(8), nans(B, nb), nans(B, nb)
    k.distill_small(dev(ms), dev(mt) if teacher else None, dev(cs), dev(ct) if teacher else None, fst, list(chans), stats,
                    4.0, LAM, terms, dmean, dcent)
    db, dr = nans(n), nans(n)
    k.distill_pix_grad(bD, rD, gD, tD, MAXD, stats, LAM[0], LAM[1] if teacher else 0.0, LAM[4], db, dr)
    return dict(final=fo, final_ref=fin32, terms=f64(terms), want=want, n_valid=int((gt > 0).sum()), db=db, dr=dr,
                db_ref=bd.grad.view(-1), dr_ref=rd.grad.view(-1), dmean=dmean, dcent=dcent, dmean_ref=msd.grad,
                dcent_ref=csd.grad)


def _check_distill(o, teacher):
    assert torch.equal(o['final'].cpu(), o['final_ref'])               # exact on the grid
    torch.testing.assert_close(o['terms'][:7], o['want'], rtol=2e-5, atol=2e-6)
    assert float(o['terms'][7]) == o['n_valid']
    check_max(o['db'], o['db_ref'], 2e-5, 'dbase')
    check_max(o['dr'], o['dr_ref'], 2e-5, 'dres')
    if teacher:
        check_max(o['dmean'], o['dmean_ref'], 2e-5, 'dmean')
        check_max(o['dcent'], o['dcent_ref'], 2e-5, 'dcent')
    else:
        assert float(o['dmean'].abs().max()) == 0.0 and float(o['dcent'].abs().max()) == 0.0


@pytest.mark.parametrize('teacher', [True, False])
@pytest.mark.parametrize('n', N_CASES)
def test_distill_pixel_terms(n, teacher):
    _check_distill(_distill(n, 2, 16, (4, 4, 4, 4, 4), teacher, seed=700 + n % 1000), teacher)


@pytest.mark.parametrize('teacher', [True, False])
@pytest.mark.parametrize('B,nb', [(2, 16), (3, 128), (1, 256), (4, 100)])
def test_distill_small(B, nb, teacher):
    _check_distill(_distill(128, B, nb, (8, 12, 5, 64, 300), teacher, seed=800 + nb), teacher)


@pytest.mark.parametrize('teacher', [True, False])
def test_distill_all_invalid(teacher):
    """gt == 0 everywhere: the masked means are 0 / 0 (NaN, as the reference's mean over an empty selection), N = 0,
    and no pixel carries a gradient."""
    o = _distill(2049, 2, 16, (4, 4, 4, 4, 4), teacher, seed=900, all_invalid=True)
    t = o['terms']
    assert torch.equal(o['final'].cpu(), o['final_ref'])
    assert bool(torch.isnan(t[0])) and bool(torch.isnan(t[5])) and bool(torch.isnan(t[6]))
    assert bool(torch.isnan(t[1])) == teacher and (teacher or float(t[1]) == 0.0)
    assert float(t[7]) == 0.0
    assert bool((o['db'] == 0).all()) and bool((o['dr'] == 0).all())
    if teacher:                                      # the terms that do not depend on the mask keep their values
        torch.testing.assert_close(t[2:5], o['want'][2:5], rtol=2e-5, atol=2e-6)
        check_max(o['dmean'], o['dmean_ref'], 2e-5)
        check_max(o['dcent'], o['dcent_ref'], 2e-5)


# ---- Base + Residual loss kernels --------------------------------------------------------------------------------------------
LBASE, LSPARSE, RECON = 1.2, 0.05, 0.75


def _baseres(n, seed, all_invalid=False):
    """adn_baseres_stats / adn_baseres_grad against oracle.base_residual_loss in float64 with the reconstruction term held
    out (lambda_recon = 0; d loss / d final enters as g_final, its value as the device scalar ``recon``).  The oracle
    computes its structural target from gt; with k = 1 that target is gt itself, so it is handed base - struct + gt
    (exact on the grid) in place of base: |base' - gt| = |base - struct| with an INDEPENDENT struct."""
    from oracle import dcnet_oracle
    base, resid, gt, strct = _pix_inputs(n, seed, all_invalid)
    gfin = torch.randn(n, generator=gen(seed + 2))
    assert_on_grid(base - strct, resid)
    shp = (1, 1, 1, n)
    D = lambda t: t.double().view(shp)
    bd, rd = D(base).requires_grad_(True), D(resid).requires_grad_(True)
    final = torch.clamp(bd + rd, 0, MAXD)
    total, (_, lb, ls) = dcnet_oracle.base_residual_loss(bd - D(strct) + D(gt), rd, final, D(gt), D(gt) > 0, 0.0, LBASE,
                                                         LSPARSE, k=1)
    if not all_invalid:
        (LBASE * lb + LSPARSE * ls + (final * D(gfin)).sum()).backward()
    k = K()
    dev = lambda t: t.contiguous().to(DEV)
    bD, rD, sD, gD, fD = dev(base), dev(resid), dev(strct), dev(gt), dev(gfin)
    recon = torch.tensor([RECON], device=DEV)
    stats, terms, ws = nans(4, dtype=torch.float64), nans(4), nans(8192 + 64)
    k.baseres_stats(bD, rD, sD, gD, recon, 1.0, LBASE, LSPARSE, stats, terms, ws)
    db, dr = nans(n), nans(n)
    k.baseres_grad(bD, rD, sD, gD, fD, MAXD, stats, LBASE, LSPARSE, db, dr)
    s = base + resid
    routed = torch.where((s >= 0) & (s <= MAXD), gfin, torch.zeros(()))
    return dict(terms=f64(terms), lb=lb.detach(), ls=ls.detach(), n_valid=int((gt > 0).sum()), stats=f64(stats), db=db,
                dr=dr, db_ref=bd.grad, dr_ref=rd.grad, routed=routed)


@pytest.mark.parametrize('n', N_CASES)
def test_baseres_stats_and_grad(n):
    o = _baseres(n, seed=1000 + n % 1000)
    t = o['terms']
    assert float(t[0]) == RECON and float(o['stats'][0]) == o['n_valid']
    want = torch.stack([o['lb'], o['ls'], RECON + LBASE * o['lb'] + LSPARSE * o['ls']])
    torch.testing.assert_close(t[1:4], want, rtol=2e-5, atol=2e-6)
    check_max(o['db'], o['db_ref'].view(-1), 2e-5, 'dbase')
    check_max(o['dr'], o['dr_ref'].view(-1), 2e-5, 'dres')
    s = o['routed']
    assert float(s.abs().max()) > 0 and bool((s == 0).any())


def test_baseres_all_invalid():
    o = _baseres(2049, seed=1100, all_invalid=True)
    t = o['terms']
    assert float(t[0]) == RECON and bool(torch.isnan(t[1:4]).all()) and float(o['stats'][0]) == 0.0
    assert torch.equal(o['db'].cpu(), o['routed']) and torch.equal(o['dr'].cpu(), o['routed'])


@pytest.mark.parametrize('n', N_CASES)
def test_clamp_add_is_torch_clamp_bit_for_bit(n):
    base, resid, _, _ = _pix_inputs(n, 1200 + n % 1000)
    g = gen(1300)
    for a, b in ((base, resid), (20 * torch.randn(n, generator=g), 20 * torch.randn(n, generator=g))):
        out = nans(n)
        K().clamp_add(a.to(DEV), b.to(DEV), MAXD, out)
        assert torch.equal(out.cpu(), torch.clamp(a + b, 0, MAXD))
