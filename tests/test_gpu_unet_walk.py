"""CVAEEngine.sample walks the layers with the launches of an eval forward(): the down path once, the up path once per draw.

The two share one implementation of each walk step (engine.UNetEngine._down_conv / _up_conv); this pins the result from the
outside, on the recorded launch plans: entry names and scalar arguments, descriptor fields included (pointers left out)."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _scalars(v):
    """The non-pointer content of one recorded ctypes argument."""
    if hasattr(v, '_obj'):                                   # byref(descriptor)
        v = v._obj
    if isinstance(v, ctypes.Structure):
        return {k: _scalars(getattr(v, k)) for k, t in v._fields_ if t is not ctypes.c_void_p}
    if isinstance(v, ctypes.Array):
        return [_scalars(e) for e in v]
    return v


def _plan(fn):
    """[(entry name, scalar arguments)] of the launches ``fn`` makes."""
    from audio_depth_estimation_amd import _lib
    _lib.RECORD = []
    try:
        fn()
    finally:
        rec, _lib.RECORD = _lib.RECORD, None
    return [(name, [_scalars(v) for v, t in zip(args, f.argtypes) if t is not ctypes.c_void_p])
            for f, args, name, _ in rec if f is not None]


def _cvae(dtype):
    from audio_depth_estimation_amd.models import unet_cvae_model as VM
    from audio_depth_estimation_amd.models.unetbaseline_model import get_norm_layer
    torch.manual_seed(3)
    cfg = SimpleNamespace(dataset=SimpleNamespace(depth_norm=False, max_depth=30.0))
    m = VM.init_net(VM.UnetGeneratorVAE(cfg, 2, 1, 5, ngf=4, norm_layer=get_norm_layer('batch'), latent_dim=16),
                    'normal', 0.02, [])
    m.compute_dtype = dtype
    return m.to(DEV).eval()


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_sample_walks_the_eval_forward(dtype):
    m = _cvae(dtype)
    x = torch.rand(2, 2, 32, 32, generator=torch.Generator().manual_seed(13)).to(DEV)
    with torch.no_grad():
        fwd = _plan(lambda: m(x))
        smp = _plan(lambda: m.sample(x, 3, seed=7))
    # set aside: the weight pack in front of a walk on a fresh buffer set, and the eval affines (sample issues the up
    # path's once for all draws)
    aside = ('adn_pack_weights', 'adn_pack_t2_multi', 'adn_bn_eval_affine')
    fwd = [e for e in fwd if e[0] not in aside]
    smp = [e for e in smp if e[0] not in aside]
    names = [e[0] for e in fwd]
    cut = names.index('adn_vae_fwd')
    down, up = fwd[:cut], fwd[cut + 1:]
    assert len(down) == 1 + 5 and len(up) == 5               # the input conversion + one launch per conv
    at = [e[0] for e in smp].index('adn_vae_sample')
    assert smp[:at] == down
    assert smp[-1][0] == 'adn_sample_stats'
    assert smp[at + 1:-1] == up * 3
