"""CPU-only checks of the dual-regression coarse-depth family: module mirror, loss mirror, refusals, ABI, command line and
the host-side plan of the fusion conv."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from audio_depth_estimation_amd.models.coarse_depth_model import DualRegressionLoss, DualRegressionModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'dualreg32_bc64.npz')


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()


def _build():
    torch.manual_seed(0)
    return DualRegressionModel(2, 64, 32)


def test_initial_state_dict_matches_reference_bits():
    ref = np.load(GOLDEN)
    m = _build()
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in ref['sd_init_keys']]
    assert [_sha(v) for v in sd.values()] == [str(h) for h in ref['sd_init_sha']]
    assert [n for n, _ in m.named_children()] == ['inc', 'down1', 'down2', 'down3', 'down4', 'coarse_up1', 'coarse_up2',
                                                   'coarse_up3', 'coarse_up4', 'coarse_head', 'offset_up1', 'offset_up2',
                                                   'offset_up3', 'offset_up4', 'offset_fusion', 'offset_head']
    assert m.get_num_params() == 25173570 == int(ref['num_params'])
    assert [int(v) for v in ref['kinks']] == [0, 0, 0]          # the fixture's batch has no pixel next to an L1 kink


def test_refusals():
    with pytest.raises(NotImplementedError, match='bilinear'):
        DualRegressionModel(2, 64, 32, bilinear=False)
    m = _build()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 2, 32, 32))                     # CPU tensor: there is no CPU path
    with pytest.raises(RuntimeError):
        m.predict_depth(torch.zeros(1, 2, 32, 32))
    eng = m.engine()                                     # the engine's shape check runs before any device work
    for shape in ((1, 2, 64, 64), (1, 2, 32, 64), (1, 2, 64, 32)):
        with pytest.raises(NotImplementedError, match='output_size'):
            eng.check_input(shape)
    with pytest.raises(RuntimeError, match='channels'):
        eng.check_input((1, 3, 32, 32))
    eng.check_input((5, 2, 32, 32))
    m.plane_channels = 12                                # not a multiple of a 16-byte chunk
    assert m.engine() is not eng
    with pytest.raises(ValueError, match='plane_channels'):
        m.engine()._plane_width()


def test_factory_still_refuses_and_points_at_the_class():
    from audio_depth_estimation_amd.models import coarse_depth_model as M
    with pytest.raises(NotImplementedError, match='DualRegressionModel directly'):
        M.define_coarse_depth_model('dual_reg')
    for mt in ('lite', 'hybrid'):
        with pytest.raises(NotImplementedError):
            M.define_coarse_depth_model(mt)


def _by_hand(coarse, offset, final, gt, cw, fw, rw):
    m = (gt > 0).double()
    n = m.sum()
    if n == 0:
        m, n = torch.ones_like(m), torch.tensor(float(gt.numel()), dtype=torch.float64)
    lc = (m * (coarse.double() - gt.double()).abs()).sum() / n
    lf = (m * (final.double() - gt.double()).abs()).sum() / n
    lo = offset.double().abs().sum() / offset.numel()
    return lc, lf, lo, cw * lc + fw * lf + rw * lo


@pytest.mark.parametrize('all_invalid', [False, True])
def test_loss_module_on_cpu_tensors(all_invalid):
    g = torch.Generator().manual_seed(3)
    coarse = torch.rand(2, 1, 5, 7, generator=g) * 30
    offset = torch.randn(2, 1, 5, 7, generator=g)
    final = coarse + offset
    gt = torch.rand(2, 1, 5, 7, generator=g) * 30
    gt[gt < 3] = 0
    if all_invalid:
        gt.zero_()
    for w in ((1.0, 1.0, 0.01), (0.5, 2.0, 0.1)):
        total, d = DualRegressionLoss(*w)(coarse, offset, final, gt)
        assert list(d) == ['total', 'coarse', 'final', 'offset_reg'] and d['total'] is total
        lc, lf, lo, lt = _by_hand(coarse, offset, final, gt, *w)
        for got, want in ((d['coarse'], lc), (d['final'], lf), (d['offset_reg'], lo), (total, lt)):
            assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want))
    c = DualRegressionLoss()
    assert (c.coarse_weight, c.final_weight, c.offset_reg_weight) == (1.0, 1.0, 0.01)


def test_abi_lists_dualreg_symbols_and_rejects_null_planes():
    from audio_depth_estimation_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'adn.h')).read()
    for name in ('adn_dualreg_loss', 'adn_dualreg_loss_finish', 'adn_dualreg_loss_workspace_bytes'):
        assert re.search(r'\b' + name + r'\(', text)
        assert name in _lib.symbol_names()
    lib = _lib.load()
    assert lib.adn_dualreg_loss_workspace_bytes(0) == -1 and lib.adn_dualreg_loss_workspace_bytes(-5) == -1
    assert lib.adn_dualreg_loss_workspace_bytes(1) == 24
    assert lib.adn_dualreg_loss_workspace_bytes(600001) == 2048 * 24       # the grid is capped at 2 048 blocks
    d = _lib.AdnDualRegLoss()
    d.pixels = 4
    assert lib.adn_dualreg_loss(ctypes.byref(d), None) == -1                # null planes: rejected before any launch
    assert b'adn_dualreg_loss' in lib.adn_last_error()
    d.coarse = d.offset = d.final_depth = d.gt = 16                         # a target without gradient planes / workspace
    assert lib.adn_dualreg_loss(ctypes.byref(d), None) == -1
    assert b'adn_dualreg_loss' in lib.adn_last_error()
    assert lib.adn_dualreg_loss_finish(None, 4, None, None, 4, 1.0, 1.0, 0.01, None, None) == -1
    assert b'adn_dualreg_loss_finish' in lib.adn_last_error()


def test_train_coarse_depth_dual_reg_without_synthetic_says_why():
    from audio_depth_estimation_amd import train_dc
    with pytest.raises(NotImplementedError, match='file decoding that is not available'):
        train_dc.main_coarse(['--model_type', 'dual_reg'])


def _plan(dtype, B, H, W, C0, C1, N, segs, epi):
    """(kernel kind, workspace bytes) of a 3x3 S1 implicit GEMM, host-only (the descriptor of kernels.igemm_query)."""
    from audio_depth_estimation_amd import _lib
    from audio_depth_estimation_amd import kernels as K
    d = _lib.AdnIgemmDesc()
    d.ks = 3
    d.dtype, d.geom, d.B, d.Hs, d.Ws, d.C0, d.C1, d.N = K.dtype_code(dtype), _lib.GEMM_S1, B, H, W, C0, C1, N
    d.in0 = d.w = 1
    d.in1 = 1 if C1 else None
    d.epi = epi
    for i, c in enumerate(segs):
        d.seg[i].channels = c
        d.seg[i].out0 = d.seg[i].ref = 1
    buf = ctypes.create_string_buffer(256)
    assert _lib.load().adn_igemm_describe(ctypes.byref(d), buf, 256) == 0
    ws = K.igemm_query(dtype, _lib.GEMM_S1, B, H, W, C0, C1, N, segs, ks=3, epi=epi)[1]
    return buf.value.decode().split()[0], ws


def test_fusion_conv_plan_stays_off_the_generic_path():
    """Host-only plan check of the [64 decoder + plane] -> 64 fusion conv (forward with the Z + stats epilogue, and its
    input gradient) at base 64 with the default plane width.  The generic kernel's signature is a B*H*W*N*4-byte slab
    (tests/test_abi.py::test_plan_queries_cover_unet256_shapes).  At the fixture's 2 x 32 x 32 the MFMA tile kernel splits K
    into slabs of its own -- it does so for every 64-channel 3x3 layer of that size, the plain [64, 64] -> 64 skip conv
    included -- so there the check is the plan's kind and a workspace that is not the generic slab; at the trained shape
    (16 x 256 x 256) no workspace at all.  The one-chunk plane gets the generic kernel at both."""
    from audio_depth_estimation_amd._lib import EPI_ADD, EPI_Z_STATS
    eng = _build().engine()
    eng.dtype = torch.bfloat16
    plane = eng._plane_width()
    assert plane == 64
    for dtype in (torch.bfloat16, torch.float32):
        for B, S in ((2, 32), (16, 256)):
            slab = B * S * S * 64 * 4
            for kind, ws in (_plan(dtype, B, S, S, 64, plane, 64, [64], EPI_Z_STATS),
                             _plan(dtype, B, S, S, 64, 0, 64 + plane, [64, plane], EPI_ADD)):
                assert kind != 'direct' and ws != slab and ws % slab == 0, (dtype, B, S, kind, ws)
                if S == 256:
                    assert ws == 0
    eng.requested_plane = 'epc'
    assert eng._plane_width() == 8
    for B, S in ((2, 32), (16, 256)):
        assert _plan(torch.bfloat16, B, S, S, 64, 8, 64, [64], EPI_Z_STATS) == ('direct', B * S * S * 64 * 4)
        assert _plan(torch.bfloat16, B, S, S, 64, 0, 72, [64, 8], EPI_ADD) == ('direct', B * S * S * 72 * 4)
    eng.dtype = torch.float32
    assert eng._plane_width() == 4
