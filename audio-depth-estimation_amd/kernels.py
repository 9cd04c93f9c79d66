"""Tensor-level wrappers over the libadn C ABI (one Python function per entry point).

Everything here only *launches* HIP kernels on torch's current stream; tensors are
allocated by the caller (PyTorch's caching allocator).  No CPU fallbacks.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib
from ._lib import AdnAttnDesc, AdnCoarseDecode, AdnCoarseEvalStats, AdnCoarseLoss, AdnDistillSmall, AdnDualRegLoss, AdnHybridLoss  # noqa: E402
from ._lib import (ADN_BF16, ADN_F32, EPI_ACT, EPI_ADD, EPI_BWD, EPI_FINAL, EPI_RAW, EPI_Z_STATS, GEMM_S1, GEMM_S2, GEMM_T2,
                   AdnEpiSeg, AdnIgemmDesc, AdnMx8ConvDesc, AdnWgradDesc, ptr)

__all__ = ['dtype_code', 'Seg', 'igemm', 'igemm_query', 'wgrad', 'wgrad_workspace_bytes', 'pack_weights',
           'nchw_to_nhwc', 'nhwc_to_nchw', 'bn_fwd_finalize', 'bn_eval_affine', 'bn_act', 'bn_bwd_finalize',
           'bn_bwd_apply', 'loss_stats', 'loss_finish', 'final_act_bwd', 'sum_to_scalar', 'grad_norm', 'grad_norm_ranges', 'wgrad_sq_count',
           'optimizer_step', 'compute_errors', 'frontend', 'convt_n1_forward', 'convt_n1_workspace_bytes', 'vae_fwd',
           'vae_bwd', 'vae_bwd_workspace_bytes']


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional per-launch timing of the GEMM kernels (bench.py): when PROFILE is a list, every igemm/wgrad
# launch appends (label, algorithmic_flops, start_event, end_event); events are recorded on the stream the
# kernel is launched on (torch's current stream), nothing synchronises.
PROFILE = None


def _prof_begin():
    if PROFILE is None:
        return None
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    return ev


def _prof_end(ev0, label, flops):
    if ev0 is None:
        return
    ev1 = torch.cuda.Event(enable_timing=True)
    ev1.record()
    PROFILE.append((label, flops, ev0, ev1))


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return ADN_F32
    if dt == torch.bfloat16:
        return ADN_BF16
    raise TypeError(f'libadn supports float32 and bfloat16 activations, got {dt}')


def _dev(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('libadn kernels need CUDA/HIP device tensors (no CPU fallback)')


class Seg:
    """One output channel segment of an implicit GEMM (mirrors AdnEpiSeg)."""

    def __init__(self, channels, out0=None, out1=None, ref=None, z=None, mean=None, istd=None, scale=None,
                 shift=None, bias=None, partials=None, slope=0.0, accumulate=False, final_act=0):
        self.channels = channels
        self.tensors = (out0, out1, ref, z, mean, istd, scale, shift, bias, partials)
        self.slope, self.accumulate, self.final_act = slope, accumulate, final_act

    def fill(self, s: AdnEpiSeg):
        _dev(*self.tensors)
        (s.out0, s.out1, s.ref, s.z, s.mean, s.istd, s.scale, s.shift, s.bias, s.partials) = [ptr(t) for t in
                                                                                                 self.tensors]
        s.channels = self.channels
        s.slope = float(self.slope)
        s.accumulate = int(bool(self.accumulate))
        s.final_act = int(self.final_act)


def _igemm_desc(dtype, geom, B, Hs, Ws, in0, in1, w, N, epi, segs, workspace=None, ks=0):
    d = AdnIgemmDesc()
    d.ks = ks
    d.dtype, d.geom, d.B, d.Hs, d.Ws = dtype_code(dtype), geom, B, Hs, Ws
    d.C0 = in0.shape[-1]
    d.C1 = in1.shape[-1] if in1 is not None else 0
    d.N = N
    _dev(in0, in1, w, workspace)
    d.in0, d.in1, d.w = ptr(in0), ptr(in1), ptr(w)
    d.epi = epi
    segs[0].fill(d.seg[0])
    if len(segs) > 1:
        segs[1].fill(d.seg[1])
    d.workspace = ptr(workspace)
    d.workspace_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    return d


def _launch(label, flops, entry, *args):
    """Call ``entry`` on the current stream, annotate the recorded launch with its label and algorithmic FLOPs, time it
    under PROFILE."""
    ev = _prof_begin()
    _lib.call(entry, *args, _stream())
    _lib.annotate(label=label, flops=flops)
    if ev is not None:
        _prof_end(ev, label, flops)


def _igemm_shape_desc(dtype, geom, B, Hs, Ws, C0, C1, N, seg_channels, ks, epi):
    """A descriptor of the shape alone for the host-only queries (dummy non-null operands: they only validate and plan)."""
    d = AdnIgemmDesc()
    d.ks = ks
    d.dtype, d.geom, d.B, d.Hs, d.Ws, d.C0, d.C1, d.N = dtype_code(dtype), geom, B, Hs, Ws, C0, C1, N
    d.in0 = d.w = 1
    d.in1 = 1 if C1 else None
    d.epi = epi
    for i in (0, 1):
        d.seg[i].channels = seg_channels[i] if i < len(seg_channels) else 0
        d.seg[i].out0 = d.seg[i].ref = 1
    return d


def igemm_query(dtype, geom, B, Hs, Ws, C0, C1, N, seg_channels, ks=0, epi=EPI_RAW):
    """(num stats partial rows, workspace bytes) for a shape, without touching the GPU.  ``epi``: the epilogue the launch
    will use -- the kernel choice (and with it the number of partial rows of the Z_STATS / BWD epilogues) depends on it."""
    d = _igemm_shape_desc(dtype, geom, B, Hs, Ws, C0, C1, N, seg_channels, ks, epi)
    lib = _lib.load()
    p = lib.adn_igemm_num_partials(C.byref(d))
    wsb = lib.adn_igemm_workspace_bytes(C.byref(d))
    if p < 0 or wsb < 0:
        raise RuntimeError('adn_igemm query failed: ' + lib.adn_last_error().decode())
    return p, wsb


def igemm_describe(dtype, geom, B, Hs, Ws, C0, C1, N, seg_channels, ks=0, epi=EPI_RAW):
    """The plan line of adn_igemm_describe for a shape ('ring bm=256 ...'; the first word is the kernel form), host only."""
    d = _igemm_shape_desc(dtype, geom, B, Hs, Ws, C0, C1, N, seg_channels, ks, epi)
    buf = C.create_string_buffer(256)
    lib = _lib.load()
    if lib.adn_igemm_describe(C.byref(d), buf, len(buf)) != 0:
        raise RuntimeError('adn_igemm_describe failed: ' + lib.adn_last_error().decode())
    return buf.value.decode()


def igemm(dtype, geom, B, Hs, Ws, in0, in1, w, N, epi, segs, workspace=None, algo_c=None, ks=0):
    """algo_c: real (unpadded) gathered channel count, only used for the algorithmic FLOP count."""
    d = _igemm_desc(dtype, geom, B, Hs, Ws, in0, in1, w, N, epi, segs, workspace, ks)
    # algorithmic FLOPs 2*M_out*N*K, K = taps*Cin  (S2: 16 taps on B*Hs*Ws pixels; T2: 4 taps on 4x the pixels;
    # S1: ks*ks taps on B*Hs*Ws pixels)
    flops = 2.0 * B * Hs * Ws * N * (ks * ks if geom == GEMM_S1 else 16) * (algo_c if algo_c else d.C0 + d.C1)
    _launch('igemm', flops, 'adn_igemm', C.byref(d))


def _wgrad_desc(dtype, B, Hs, Ws, plain0, plain1, gath0, gath1, dw, workspace, c_valid=0, ks=0):
    d = AdnWgradDesc()
    d.c_valid = c_valid
    d.geom, d.ks = (GEMM_S1, ks) if ks else (0, 0)
    d.dtype, d.B, d.Hs, d.Ws = dtype_code(dtype), B, Hs, Ws
    _dev(plain0, plain1, gath0, gath1, dw, workspace)
    d.plain0, d.plain1 = ptr(plain0), ptr(plain1)
    d.R0 = plain0.shape[-1]
    d.R1 = plain1.shape[-1] if plain1 is not None else 0
    d.gath0, d.gath1 = ptr(gath0), ptr(gath1)
    d.C0 = gath0.shape[-1]
    d.C1 = gath1.shape[-1] if gath1 is not None else 0
    d.dw = ptr(dw)
    d.workspace = ptr(workspace)
    d.workspace_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    return d


def _wgrad_shape_desc(dtype, B, Hs, Ws, R0, R1, C0, C1, c_valid=0, ks=0, d=None):
    """A descriptor of the shape alone for the host-only queries (``d``: fill this slot of a descriptor array)."""
    d = AdnWgradDesc() if d is None else d
    d.c_valid = c_valid
    d.geom, d.ks = (GEMM_S1, ks) if ks else (0, 0)
    d.dtype, d.B, d.Hs, d.Ws, d.R0, d.R1, d.C0, d.C1 = dtype_code(dtype), B, Hs, Ws, R0, R1, C0, C1
    d.plain0 = d.gath0 = d.dw = 1
    d.plain1 = 1 if R1 else None
    d.gath1 = 1 if C1 else None
    return d


def wgrad_workspace_bytes(dtype, B, Hs, Ws, R0, R1, C0, C1, c_valid=0, ks=0):
    d = _wgrad_shape_desc(dtype, B, Hs, Ws, R0, R1, C0, C1, c_valid, ks)
    lib = _lib.load()
    n = lib.adn_wgrad_workspace_bytes(C.byref(d))
    if n < 0:
        raise RuntimeError('adn_wgrad query failed: ' + lib.adn_last_error().decode())
    return n


def wgrad_batchable(dtype, B, Hs, Ws, R0, R1, C0, C1, c_valid=0):
    """(class, norm partials) of this k4 weight gradient as a problem of a wgrad_batch launch; class 0 = not batchable,
    problems of one launch share their class (host-only query)."""
    d = _wgrad_shape_desc(dtype, B, Hs, Ws, R0, R1, C0, C1, c_valid)
    lib = _lib.load()
    return int(lib.adn_wgrad_batchable(C.byref(d))), int(lib.adn_wgrad_batch_sq_count(C.byref(d)))


def _wgrad_problems(dtype, B, problems, workspace):
    """(descriptor array, algorithmic FLOPs) of a list of (Hs, Ws, plain0, plain1, gath0, gath1, dw, sq) k4 problems."""
    arr = (AdnWgradDesc * len(problems))()
    flops = 0.0
    for slot, (Hs, Ws, p0, p1, g0, g1, dw, sq) in zip(arr, problems):
        d = _wgrad_desc(dtype, B, Hs, Ws, p0, p1, g0, g1, dw, workspace)
        d.sq_partials = ptr(sq)
        C.memmove(C.byref(slot), C.byref(d), C.sizeof(AdnWgradDesc))
        flops += 2.0 * B * Hs * Ws * (d.R0 + d.R1) * 16 * (d.C0 + d.C1)
    return arr, flops


def wgrad_batch(dtype, B, problems, entry='adn_wgrad_batch'):
    """problems: list of (Hs, Ws, plain0, plain1, gath0, gath1, dw, sq): up to 8 weight gradients of ONE class in one
    launch."""
    arr, flops = _wgrad_problems(dtype, B, problems, None)
    _launch('wgrad', flops, entry, arr, len(problems))


def wgrad_multi(dtype, B, problems):
    """As wgrad_batch for problems of either class (adn_wgrad_multi): longest problem first inside the launch, the
    small-image levels in the small-image fast form, dead taps of 1x1 images stored as zeros."""
    wgrad_batch(dtype, B, problems, entry='adn_wgrad_multi')


def wgrad_patch_batch_workspace_bytes(dtype, B, shapes):
    """shapes: list of (Hs, Ws, R0, R1, C0, C1).  Bytes of slab scratch of one wgrad_patch_batch launch over them, or -1 when
    some layer is not a patch-staged one (host-only query)."""
    arr = (AdnWgradDesc * len(shapes))()
    for slot, shape in zip(arr, shapes):
        _wgrad_shape_desc(dtype, B, *shape, d=slot)
    return int(_lib.load().adn_wgrad_patch_batch_workspace_bytes(arr, len(shapes)))


def wgrad_patch_batch(dtype, B, problems, workspace):
    """problems: list of (Hs, Ws, plain0, plain1, gath0, gath1, dw, sq): 2 .. 4 patch-staged weight gradients in one launch
    with 1/n of the pixel splits each (+ one slab sum per problem)."""
    arr, flops = _wgrad_problems(dtype, B, problems, workspace)
    _launch('wgrad', flops, 'adn_wgrad_patch_batch', arr, len(problems))


def wgrad_sq_count(dtype, B, Hs, Ws, R0, R1, C0, C1, c_valid=0, ks=0):
    """Partial sums of dW^2 adn_wgrad leaves behind when asked to (``sq=``); 0 = this layer's kernel has no fused form."""
    d = _wgrad_shape_desc(dtype, B, Hs, Ws, R0, R1, C0, C1, c_valid, ks)
    return int(_lib.load().adn_wgrad_sq_count(C.byref(d)))


def wgrad(dtype, B, Hs, Ws, plain0, plain1, gath0, gath1, dw, workspace=None, c_valid=0, ks=0, sq=None):
    """ks=0: the k4 s2 p1 pair (gathered tensor on the 2x grid); ks in {1,3}: stride-1 ks x ks conv (same grid).
    sq (optional, f64, wgrad_sq_count(...) elements): receives the partial sums of dW^2 for the fused gradient norm."""
    d = _wgrad_desc(dtype, B, Hs, Ws, plain0, plain1, gath0, gath1, dw, workspace, c_valid, ks)
    if sq is not None:
        _dev(sq)
        if sq.dtype != torch.float64:
            raise TypeError('wgrad: sq must be float64')
        d.sq_partials = ptr(sq)
    flops = 2.0 * B * Hs * Ws * (d.R0 + d.R1) * (ks * ks if ks else 16) * (c_valid if c_valid else d.C0 + d.C1)
    _launch('wgrad', flops, 'adn_wgrad', C.byref(d))


def pack_weights(master, X, Y, dtype, s2_out=None, t2_out=None, y_pad=None):
    """master f32 [X][16][Y] -> s2 [X][16][y_pad] (zero padded) and/or t2 [4][Y][4][X]."""
    _dev(master, s2_out, t2_out)
    _lib.call('adn_pack_weights', ptr(master), X, Y, Y if y_pad is None else y_pad, dtype_code(dtype), ptr(s2_out),
              ptr(t2_out), _stream())


def s1_row_stride(dtype, taps, cin):
    """Elements per packed S1 weight row: taps*cin rounded up to the 128-byte K-step of the GEMM."""
    bk = 128 // (2 if dtype == torch.bfloat16 else 4)
    return -(-taps * cin // bk) * bk


def pack_rows(master, X, taps, Y, out, y_pad=None):
    """master f32 [X][taps][Y] -> out [X][row_stride] = [X][taps][y_pad] + zero tail (S1 forward operand)."""
    _dev(master, out)
    _lib.call('adn_pack_rows', ptr(master), X, taps, Y, Y if y_pad is None else y_pad,
              out.stride(0) if out.dim() > 1 else 1, dtype_code(out.dtype), ptr(out), _stream())


def pack_transpose_taps(master, X, taps, Y, out, flip=True):
    """master f32 [X][taps][Y] -> out [Y][row_stride], out[y][t'*X+x] = master[x][t][y] (S1 dgrad operand)."""
    _dev(master, out)
    _lib.call('adn_pack_transpose_taps', ptr(master), X, taps, Y, int(flip), out.stride(0), dtype_code(out.dtype),
              ptr(out), _stream())


# ---- block-scaled fp8 (MX e4m3) 3 x 3 convolution path (csrc/mx8.hip) ------------------------------------------------------
def mx8_quantize(src, dst8, scales):
    """src bf16 [..., C] -> dst8 uint8 (e4m3 bits, same shape) + scales uint8 (E8M0) [..., C/32]."""
    _dev(src, dst8, scales)
    if src.dtype != torch.bfloat16 or dst8.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise TypeError('mx8_quantize: src bf16, dst / scales uint8')
    Cc = src.shape[-1]
    _lib.call('adn_mx8_quantize', ptr(src), src.numel() // Cc, Cc, ptr(dst8), ptr(scales), _stream())


def bn_act_mx8(z, pixels, Cc, scale, shift, out_relu, out8, out_scales):
    """bn_act (BN affine + ReLU, bf16) that also writes the MX-fp8 copy of its output."""
    _dev(z, scale, shift, out_relu, out8, out_scales)
    _lib.call('adn_bn_act_mx8', ptr(z), pixels, Cc, ptr(scale), ptr(shift), ptr(out_relu), ptr(out8), ptr(out_scales),
              _stream())


def bn_bwd_apply_mx8(g, z, pixels, Cc, scale, mean, istd, coef, out8, out_scales):
    """bn_bwd_apply (in place on g, bf16) that also writes the MX-fp8 copy of the resulting d loss / d z."""
    _dev(g, z, scale, mean, istd, coef, out8, out_scales)
    _lib.call('adn_bn_bwd_apply_mx8', ptr(g), ptr(z), pixels, Cc, ptr(scale), ptr(mean), ptr(istd), ptr(coef), ptr(out8),
              ptr(out_scales), _stream())


def mx8_pack_shapes(X, Y, transpose):
    """(w8 shape, wsc shape) of the packed MX operand of a [X,Y,3,3] conv weight."""
    rows, kc = (Y, X) if transpose else (X, Y)
    return (rows, 10, kc), (rows, kc // 64, 5, 4)


def mx8_pack(master, X, Y, transpose, w8, wsc):
    """master f32 [X][9][Y] -> w8 / wsc (see include/adn.h adn_mx8_pack)."""
    _dev(master, w8, wsc)
    _lib.call('adn_mx8_pack', ptr(master), X, Y, int(transpose), ptr(w8), ptr(wsc), _stream())


def _mx8_shape_desc(B, H, W, N, C0, C1):
    """A descriptor of the shape alone for the host-only queries (dummy non-null operands: they only validate and plan)."""
    d = AdnMx8ConvDesc()
    d.B, d.H, d.W, d.C0, d.C1, d.N = B, H, W, C0, C1, N
    d.in0 = d.sc0 = d.w = d.wsc = 1
    d.in1 = d.sc1 = 1 if C1 else None
    d.epi = EPI_Z_STATS
    d.seg[0].channels, d.seg[0].out0 = N, 1
    return d


def conv3x3_mx8_num_partials(B, H, W, N=128, C0=64, C1=0):
    """Stats partial rows the kernel writes for this shape (queried from the library: 128 or 256 pixels per workgroup)."""
    d = _mx8_shape_desc(B, H, W, N, C0, C1)
    lib = _lib.load()
    n = lib.adn_conv3x3_mx8_num_partials(C.byref(d))
    if n < 0:
        raise RuntimeError('adn_conv3x3_mx8 query failed: ' + lib.adn_last_error().decode())
    return n


def conv3x3_mx8_describe(B, H, W, N=128, C0=64, C1=0):
    """The form line of adn_conv3x3_mx8_describe for a shape ('mx bm=128 bn=64 tiles_m=.. tiles_n=..'), host only."""
    d = _mx8_shape_desc(B, H, W, N, C0, C1)
    buf = C.create_string_buffer(128)
    lib = _lib.load()
    if lib.adn_conv3x3_mx8_describe(C.byref(d), buf, len(buf)) != 0:
        raise RuntimeError('adn_conv3x3_mx8_describe failed: ' + lib.adn_last_error().decode())
    return buf.value.decode()


def conv3x3_mx8(B, H, W, in0, sc0, in1, sc1, w8, wsc, N, epi, segs):
    """3 x 3 stride-1 conv on MX-fp8 operands; outputs / epilogue operands of ``segs`` are bf16 (as igemm)."""
    d = AdnMx8ConvDesc()
    d.B, d.H, d.W = B, H, W
    d.C0 = in0.shape[-1]
    d.C1 = in1.shape[-1] if in1 is not None else 0
    d.N = N
    _dev(in0, sc0, in1, sc1, w8, wsc)
    d.in0, d.sc0, d.in1, d.sc1, d.w, d.wsc = ptr(in0), ptr(sc0), ptr(in1), ptr(sc1), ptr(w8), ptr(wsc)
    d.epi = epi
    segs[0].fill(d.seg[0])
    if len(segs) > 1:
        segs[1].fill(d.seg[1])
    _launch('conv3x3_mx8', 2.0 * B * H * W * N * 9 * (d.C0 + d.C1), 'adn_conv3x3_mx8', C.byref(d))


def nchw_to_nhwc(src, dst):
    """src f32 [B,C,H,W] -> dst [B,H,W,Cpad] (Cpad = dst.shape[-1] >= C, extra channels zero)."""
    B, Cc, H, W = src.shape
    _dev(src, dst)
    _lib.call('adn_nchw_to_nhwc', ptr(src), ptr(dst), B, Cc, dst.shape[-1], H, W, dtype_code(dst.dtype), _stream())


def nhwc_to_nchw(src, dst):
    B, Cc, H, W = dst.shape
    _dev(src, dst)
    _lib.call('adn_nhwc_to_nchw', ptr(src), ptr(dst), B, Cc, H, W, dtype_code(src.dtype), _stream())


BN_REDUCE_ROWS, BN_REDUCE_SLICES = 2048, 64


def _bn_prereduce(partials, P, Cc, scratch):
    """Layers with thousands of partial rows: coalesced pre-reduction to 64 rows in ``scratch`` (f32 [>= 64 * 2 * C])."""
    if scratch is None or P < BN_REDUCE_ROWS or Cc % 32 != 0 or scratch.numel() < BN_REDUCE_SLICES * 2 * Cc:
        return partials, P
    _dev(partials, scratch)
    _lib.call('adn_bn_partials_reduce', ptr(partials), P, Cc, BN_REDUCE_SLICES, ptr(scratch), _stream())
    return scratch, BN_REDUCE_SLICES


def bn_fwd_finalize(partials, P, Cc, count, gamma, beta, eps, momentum, running_mean, running_var, nbt, mean,
                    istd, scale, shift, scratch=None):
    partials, P = _bn_prereduce(partials, P, Cc, scratch)
    _dev(partials, mean, istd, scale, shift)
    _lib.call('adn_bn_fwd_finalize', ptr(partials), P, Cc, count, ptr(gamma), ptr(beta), eps, momentum,
              ptr(running_mean), ptr(running_var), ptr(nbt), ptr(mean), ptr(istd), ptr(scale), ptr(shift),
              _stream())


def bn_fwd_fused(partials, P, Cc, count, gamma, beta, eps, momentum, running_mean, running_var, nbt, mean, istd, scale,
                 shift, z, pixels, slope, out_leaky, out_relu):
    """bn_fwd_finalize + bn_act in one launch (small tensors, C % 32 == 0)."""
    _dev(partials, mean, istd, scale, shift, z, out_leaky, out_relu)
    _lib.call('adn_bn_fwd_fused', ptr(partials), P, Cc, count, ptr(gamma), ptr(beta), eps, momentum, ptr(running_mean),
              ptr(running_var), ptr(nbt), ptr(mean), ptr(istd), ptr(scale), ptr(shift), ptr(z), pixels,
              dtype_code(z.dtype), float(slope), ptr(out_leaky), ptr(out_relu), _stream())


def bn_bwd_fused(partials, P, Cc, count, dgamma, dbeta, g, z, pixels, scale, mean, istd):
    """bn_bwd_finalize + bn_bwd_apply (g in place) in one launch (small tensors, C % 32 == 0)."""
    _dev(partials, g, z, scale, mean, istd)
    _lib.call('adn_bn_bwd_fused', ptr(partials), P, Cc, count, ptr(dgamma), ptr(dbeta), ptr(g), ptr(z), pixels,
              dtype_code(g.dtype), ptr(scale), ptr(mean), ptr(istd), _stream())


def bn_eval_affine(gamma, beta, running_mean, running_var, eps, scale, shift):
    _dev(running_mean, scale)
    _lib.call('adn_bn_eval_affine', ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), eps,
              running_mean.numel(), ptr(scale), ptr(shift), _stream())


def bn_act(z, pixels, Cc, scale, shift, slope, out_leaky=None, out_relu=None):
    _dev(z, scale, shift, out_leaky, out_relu)
    _lib.call('adn_bn_act', ptr(z), pixels, Cc, dtype_code(z.dtype), ptr(scale), ptr(shift), slope, ptr(out_leaky),
              ptr(out_relu), _stream())


def bn_bwd_finalize(partials, P, Cc, count, dgamma, dbeta, coef, scratch=None):
    partials, P = _bn_prereduce(partials, P, Cc, scratch)
    _dev(partials, coef)
    _lib.call('adn_bn_bwd_finalize', ptr(partials), P, Cc, count, ptr(dgamma), ptr(dbeta), ptr(coef), _stream())


def bn_bwd_apply(g, z, pixels, Cc, scale, mean, istd, coef):
    _dev(g, z)
    _lib.call('adn_bn_bwd_apply', ptr(g), ptr(z), pixels, Cc, dtype_code(g.dtype), ptr(scale), ptr(mean), ptr(istd),
              ptr(coef), _stream())


def loss_stats(pred, gt, scale, mask_mode, eps, stats, workspace):
    _dev(pred, gt, stats, workspace)
    _lib.call('adn_loss_stats', ptr(pred), ptr(gt), pred.numel(), scale, mask_mode, eps, ptr(stats), ptr(workspace),
              workspace.numel() * workspace.element_size(), _stream())


def loss_finish(pred, gt, scale, mask_mode, eps, stats, criterion, l1_weight, silog_weight, silog_lambda, loss_out,
                grad):
    _dev(pred, gt, stats, loss_out, grad)
    _lib.call('adn_loss_finish', ptr(pred), ptr(gt), pred.numel(), scale, mask_mode, eps, ptr(stats), criterion,
              l1_weight, silog_weight, silog_lambda, ptr(loss_out), ptr(grad), _stream())


def loss_finish_dz(pred, gt, scale, mask_mode, eps, stats, criterion, l1_weight, silog_weight, silog_lambda, loss_out, dz,
                   final_act, bias_grad, workspace):
    """loss_finish + final_act_bwd + the last layer's bias gradient in one pass (1-channel prediction = activation output)."""
    _dev(pred, gt, stats, loss_out, dz, bias_grad, workspace)
    _lib.call('adn_loss_finish_dz', ptr(pred), ptr(gt), pred.numel(), scale, mask_mode, eps, ptr(stats), criterion,
              l1_weight, silog_weight, silog_lambda, ptr(loss_out), ptr(dz), final_act, ptr(bias_grad), ptr(workspace),
              workspace.numel() * workspace.element_size(), _stream())


def final_act_bwd(gout, out, final_act, dz):
    """dz [pixels, Cpad]: channel 0 = gout * act'(out), padded channels zero."""
    _dev(gout, out, dz)
    _lib.call('adn_final_act_bwd', ptr(gout), ptr(out), out.numel(), final_act, dtype_code(dz.dtype),
              dz.numel() // out.numel(), ptr(dz), _stream())


def convt_n1_workspace_bytes(B, Hs, Ws):
    return _lib.load().adn_convt_n1_workspace_bytes(B, Hs, Ws)


N1_RELU_IN0, N1_TWO_LAUNCH = 1, 2          # adn.h: flags of adn_convt_n1_forward_ex


def convt_n1_forward(dtype, B, Hs, Ws, in0, in1, w_master, bias, final_act, out, workspace, relu_in0=False, bn1=None,
                     two_launch=None):
    """Last transposed conv (Cout = 1).  ``relu_in0``: in0 holds the values before the ReLU (a LeakyReLU copy), the
    kernel clamps it on load.  ``bn1`` = (scale, shift): in1 holds the raw conv output of a train-mode BatchNorm + ReLU
    layer, the kernel applies both on load (adn_convt_n1_forward_bn).  ADN_CONVT_N1_FUSED=0 (or ``two_launch``) takes the
    two-launch form (tap products through the workspace)."""
    sc1, sh1 = bn1 if bn1 is not None else (None, None)
    _dev(in0, in1, w_master, bias, out, workspace, sc1, sh1)
    ev = _prof_begin()
    if two_launch is None:
        two_launch = os.environ.get('ADN_CONVT_N1_FUSED') == '0'
    flags = (N1_RELU_IN0 if relu_in0 else 0) | (N1_TWO_LAUNCH if two_launch else 0)
    args = (dtype_code(dtype), B, Hs, Ws, ptr(in0), in0.shape[-1], ptr(in1), in1.shape[-1] if in1 is not None else 0,
            ptr(w_master), ptr(bias), final_act, ptr(out), ptr(workspace), workspace.numel() * workspace.element_size(),
            flags)
    if bn1 is None:
        _lib.call('adn_convt_n1_forward_ex', *args, _stream())
    else:
        _lib.call('adn_convt_n1_forward_bn', *args, ptr(sc1), ptr(sh1), _stream())
    if ev is not None:
        cin = in0.shape[-1] + (in1.shape[-1] if in1 is not None else 0)
        _prof_end(ev, 'convt_n1', 2.0 * B * Hs * Ws * 16 * cin)


def l0_forward(x, w_master, B, Hs, Ws, slope, out_leaky, out_relu):
    """First conv (2 -> 64 channels) of the bf16 path: x f32 NCHW [B,2,2Hs,2Ws], w f32 [64][16][2] (parameter memory)."""
    _dev(x, w_master, out_leaky, out_relu)
    _lib.call('adn_l0_forward', ptr(x), ptr(w_master), B, Hs, Ws, x.shape[1], w_master.numel() // (16 * x.shape[1]),
              float(slope), ptr(out_leaky), ptr(out_relu), _stream())
    _lib.annotate(label='edge', flops=2.0 * B * Hs * Ws * 64 * 16 * x.shape[1])


def l0_forward_stats_num_partials(B, Hs, Ws):
    n = _lib.load().adn_l0_forward_stats_num_partials(B, Hs, Ws)
    if n < 0:
        raise RuntimeError(f'adn_l0_forward_stats: bad shape B={B} Hs={Hs} Ws={Ws} (Ws % 16)')
    return n


def l0_forward_stats(x, w_master, bias, B, Hs, Ws, z, partials):
    """First conv (2 -> 64 channels) in front of a train-mode BatchNorm: z bf16 [B,Hs,Ws,64] = conv(x) + bias and
    l0_forward_stats_num_partials rows [2][64] of sum z / sum z^2 (the EPI_Z_STATS convention)."""
    _dev(x, w_master, bias, z, partials)
    _lib.call('adn_l0_forward_stats', ptr(x), ptr(w_master), ptr(bias), B, Hs, Ws, x.shape[1],
              w_master.numel() // (16 * x.shape[1]), ptr(z), ptr(partials), _stream())
    _lib.annotate(label='edge', flops=2.0 * B * Hs * Ws * 64 * 16 * x.shape[1])


def d0_dgrad_num_partials(B, Hs, Ws):
    return _lib.load().adn_d0_dgrad_num_partials(B, Hs, Ws)


def d0_dgrad(dz, w_master, B, Hs, Ws, seg0, seg1):
    """Input gradient of the last transposed conv (128 -> 1): dz f32 [B,1,2Hs,2Ws], segments = skip / up half.  seg1
    without ``ref``: masked by the BatchNorm + ReLU of its z (scale, shift), the activation that was not materialised."""
    _dev(dz, w_master)
    s0, s1 = AdnEpiSeg(), AdnEpiSeg()
    seg0.fill(s0)
    seg1.fill(s1)
    _lib.call('adn_d0_dgrad', ptr(dz), ptr(w_master), B, Hs, Ws, C.byref(s0), C.byref(s1), _stream())
    _lib.annotate(label='edge', flops=2.0 * B * Hs * Ws * 128 * 16)


def thin_wgrad_workspace_bytes(B, Hs, Ws, ct, c0, c1):
    return _lib.load().adn_thin_wgrad_workspace_bytes(B, Hs, Ws, ct, c0, c1)


def thin_wgrad(thin, plain0, plain1, B, Hs, Ws, dw, workspace, relu_plain0=False, bn1=None):
    """dw[c][tap*ct + t] = sum plain[.., c] * thin window; thin f32 [B,ct,2Hs,2Ws] planar, plain bf16 NHWC.
    ``relu_plain0`` (ct = 1): plain0 holds the values before the ReLU, the kernel clamps it after the load.
    ``bn1`` = (scale, shift) (ct = 1): plain1 holds the raw conv output of a train-mode BatchNorm + ReLU layer, the kernel
    applies both after the load (adn_thin_wgrad_bn)."""
    sc1, sh1 = bn1 if bn1 is not None else (None, None)
    _dev(thin, plain0, plain1, dw, workspace, sc1, sh1)
    ct = thin.shape[1]
    c0 = plain0.shape[-1]
    c1 = plain1.shape[-1] if plain1 is not None else 0
    args = (ptr(thin), ct, ptr(plain0), c0, ptr(plain1), c1, B, Hs, Ws, ptr(dw), ptr(workspace),
            workspace.numel() * workspace.element_size(), 1 if relu_plain0 else 0)
    if bn1 is None:
        _lib.call('adn_thin_wgrad_ex', *args, _stream())
    else:
        _lib.call('adn_thin_wgrad_bn', *args, ptr(sc1), ptr(sh1), _stream())
    _lib.annotate(label='edge', flops=2.0 * B * Hs * Ws * (c0 + c1) * 16 * ct)


def sum_to_scalar(x, out, workspace):
    _dev(x, out, workspace)
    _lib.call('adn_sum_to_scalar', ptr(x), x.numel(), dtype_code(x.dtype), ptr(out), ptr(workspace),
              workspace.numel() * workspace.element_size(), _stream())


def grad_norm(grads, max_norm, state, workspace):
    _dev(grads, state, workspace)
    _lib.call('adn_grad_norm', ptr(grads), grads.numel(), max_norm, ptr(state), ptr(workspace),
              workspace.numel() * workspace.element_size(), _stream())


def grad_sqsum_count(n):
    """Number of f64 partial sums adn_grad_sqsum_partials writes for n elements."""
    return _lib.load().adn_grad_norm_workspace_bytes(n) // 8


def grad_sqsum_partials(grads, partials):
    """partials f64[grad_sqsum_count(n)] <- sums of squares of the f32 slice ``grads`` (one all-reduce bucket)."""
    _dev(grads, partials)
    _lib.call('adn_grad_sqsum_partials', ptr(grads), grads.numel(), ptr(partials), _nbytes(partials), _stream())


def grad_norm_ranges(grads, ranges, extra, max_norm, state, workspace):
    """Total gradient norm + clip coefficient from (a) ``ranges`` (int64 [n, 2] rows (offset, length <= 8192), both
    multiples of 4) of ``grads`` and (b) ``extra``: partial sums of squares the gradient kernels already wrote."""
    _dev(grads, ranges, extra, state, workspace)
    nr = 0 if ranges is None else ranges.shape[0]
    ne = 0 if extra is None else extra.numel()
    _lib.call('adn_grad_norm_ranges', ptr(grads), ptr(ranges), nr, ptr(extra), ne, max_norm, ptr(state), ptr(workspace),
              workspace.numel() * workspace.element_size(), _stream())


def optimizer_step(params, grads, exp_avg, exp_avg_sq, kind, lr, beta1, beta2, eps, weight_decay, use_clip, state,
                   bf16_copy=None):
    _dev(params, grads, state, bf16_copy)
    _lib.call('adn_optimizer_step', ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), kind, lr,
              beta1, beta2, eps, weight_decay, int(use_clip), ptr(state), ptr(bf16_copy), _stream())


def pack_t2_multi(flat_master, table, layers, total_blocks, dtype, t2_base):
    """flat_master: the f32 masters or their bf16 mirror (same offsets)."""
    _dev(flat_master, table, t2_base)
    _lib.call('adn_pack_t2_multi', ptr(flat_master), dtype_code(flat_master.dtype), ptr(table), layers, total_blocks,
              dtype_code(dtype), ptr(t2_base), _stream())


def edge_loss(pred, gt, lambdas, stats, terms, grad, workspace):
    """Edge-aware / smoothness loss (adn_edge_loss): pred, gt f32 [B,1,H,W]; lambdas = (recon, edge, smooth)."""
    _dev(pred, gt, stats, terms, grad, workspace)
    B, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
    _lib.call('adn_edge_loss', ptr(pred), ptr(gt), B, H, W, float(lambdas[0]), float(lambdas[1]), float(lambdas[2]),
              ptr(stats), ptr(terms), ptr(grad), ptr(workspace), workspace.numel() * workspace.element_size(), _stream())


def edge_loss_workspace_bytes(B, H, W):
    return _lib.load().adn_edge_loss_workspace_bytes(B, H, W)


def compute_errors(gt, pred, out7):
    """gt/pred [samples, pixels] f32 -> out7 [samples, 7]."""
    _dev(gt, pred, out7)
    _lib.call('adn_compute_errors', ptr(gt), ptr(pred), gt.shape[0], gt.shape[1], ptr(out7), None, 0, _stream())


def frontend(wave, mode, S, antialias, out, workspace):
    _dev(wave, out, workspace)
    B, _, T = wave.shape
    _lib.call('adn_frontend', ptr(wave), B, T, mode, S, int(antialias), ptr(out), ptr(workspace),
              workspace.numel() * workspace.element_size(), _stream())


def resize_bilinear_bwd(gout, H, W, gin):
    """gout f32 [planes, S, S] -> gin f32 [planes, H, W]: adjoint of resize_bilinear(antialias=False)."""
    _dev(gout, gin)
    planes, S, _ = gout.shape
    _lib.call('adn_resize_bilinear_bwd', ptr(gout), planes, H, W, S, ptr(gin), _stream())


def clamp_range(x, max_depth, out, g=None):
    """out = clamp(x, 0, max_depth), or with ``g``: g masked to 0 <= x <= max_depth (the clamp's backward)."""
    _dev(x, out, g)
    _lib.call('adn_clamp_range', ptr(x), ptr(g), x.numel(), float(max_depth), ptr(out), _stream())


def frontend_workspace_bytes(B, T, mode):
    return _lib.load().adn_frontend_workspace_bytes(B, T, mode)


def resize_bilinear(src, S, antialias, out):
    """src f32 [planes, H, W] -> out f32 [planes, S, S] (align_corners=False, optional antialias)."""
    _dev(src, out)
    planes, H, W = src.shape
    _lib.call('adn_resize_bilinear', ptr(src), planes, H, W, S, int(antialias), ptr(out), _stream())


# ---- DoubleConv U-Net family (csrc/dcnet.hip) -------------------------------------------------------
def maxpool2_fwd(src, dst):
    """src [B,H,W,C] -> dst [B,H//2,W//2,C] (nn.MaxPool2d(2))."""
    B, H, W, Cc = src.shape
    _dev(src, dst)
    _lib.call('adn_maxpool2_fwd', ptr(src), ptr(dst), B, H, W, Cc, dtype_code(src.dtype), _stream())


def maxpool2_fwd_mx8(src, dst, out8, out_scales):
    """maxpool2_fwd (bf16) that also writes the MX-fp8 copy of dst."""
    B, H, W, Cc = src.shape
    _dev(src, dst, out8, out_scales)
    _lib.call('adn_maxpool2_fwd_mx8', ptr(src), ptr(dst), B, H, W, Cc, ptr(out8), ptr(out_scales), _stream())


def upsample2x_fwd_mx8(src, dst, out8, out_scales):
    """upsample2x_fwd (bf16) that also writes the MX-fp8 copy of dst."""
    B, Hi, Wi, Cc = src.shape
    _dev(src, dst, out8, out_scales)
    _lib.call('adn_upsample2x_fwd_mx8', ptr(src), ptr(dst), B, Hi, Wi, dst.shape[1], dst.shape[2], Cc, ptr(out8),
              ptr(out_scales), _stream())


def maxpool2_bwd(gdst, y, gsrc, accumulate):
    B, H, W, Cc = y.shape
    _dev(gdst, y, gsrc)
    _lib.call('adn_maxpool2_bwd', ptr(gdst), ptr(y), ptr(gsrc), B, H, W, Cc, int(bool(accumulate)),
              dtype_code(y.dtype), _stream())


def tail_stats_blocks(work, Cc):
    """Partial rows the tail-fused backward kernels write for ``work`` thread items (0: this channel count is not fusable)."""
    return _lib.load().adn_tail_stats_blocks(work, Cc)


def maxpool2_bwd_tail(gdst, y, gsrc, accumulate, z, mean, istd, partials):
    """maxpool2_bwd that is the last writer of gsrc: + ReLU mask of y and BN-backward partial sums."""
    B, H, W, Cc = y.shape
    _dev(gdst, y, gsrc, z, mean, istd, partials)
    _lib.call('adn_maxpool2_bwd_tail', ptr(gdst), ptr(y), ptr(gsrc), B, H, W, Cc, int(bool(accumulate)), dtype_code(y.dtype),
              ptr(z), ptr(mean), ptr(istd), ptr(partials), _stream())


def upsample2x_bwd_tail(gdst, gsrc, accumulate, y, z, mean, istd, partials):
    B, Hi, Wi, Cc = gsrc.shape
    _dev(gdst, gsrc, y, z, mean, istd, partials)
    _lib.call('adn_upsample2x_bwd_tail', ptr(gdst), ptr(gsrc), B, Hi, Wi, gdst.shape[1], gdst.shape[2], Cc,
              int(bool(accumulate)), dtype_code(gsrc.dtype), ptr(y), ptr(z), ptr(mean), ptr(istd), ptr(partials), _stream())


def upsample2x_fwd(src, dst):
    """Bilinear x2 (align_corners=True) of src [B,Hi,Wi,C], zero padded into dst [B,Ho,Wo,C]."""
    B, Hi, Wi, Cc = src.shape
    _dev(src, dst)
    _lib.call('adn_upsample2x_fwd', ptr(src), ptr(dst), B, Hi, Wi, dst.shape[1], dst.shape[2], Cc,
              dtype_code(src.dtype), _stream())


def upsample2x_bwd(gdst, gsrc, accumulate=False):
    B, Hi, Wi, Cc = gsrc.shape
    _dev(gdst, gsrc)
    _lib.call('adn_upsample2x_bwd', ptr(gdst), ptr(gsrc), B, Hi, Wi, gdst.shape[1], gdst.shape[2], Cc,
              int(bool(accumulate)), dtype_code(gsrc.dtype), _stream())


def pixel_shuffle2(packed, spatial, inverse=False):
    """packed [B,H,W,4*C] (tap-major) <-> spatial [B,2H,2W,C]: the scatter of ConvTranspose2d(k 2, s 2) / the gather of
    its gradient (inverse)."""
    B, H, W, C4 = packed.shape
    assert spatial.shape == (B, 2 * H, 2 * W, C4 // 4) and packed.dtype == spatial.dtype
    _dev(packed, spatial)
    src, dst = (spatial, packed) if inverse else (packed, spatial)
    _lib.call('adn_pixel_shuffle2', ptr(src), ptr(dst), B, H, W, C4 // 4, int(bool(inverse)), dtype_code(packed.dtype),
              _stream())


def relu_bwd_stats_num_partials(pixels, Cc):
    return _lib.load().adn_relu_bwd_stats_num_partials(pixels, Cc)


def relu_bwd_stats(g, y, z, mean, istd, pixels, Cc, partials):
    _dev(g, y, z, mean, istd, partials)
    _lib.call('adn_relu_bwd_stats', ptr(g), ptr(y), ptr(z), ptr(mean), ptr(istd), pixels, Cc, dtype_code(g.dtype),
              ptr(partials), _stream())


def head1x1_fwd(x, w, bias, act, max_depth, zpre, out):
    """x [..., C] NHWC, w f32 [C], bias f32 [1] or None -> zpre/out f32 [pixels]."""
    Cc = x.shape[-1]
    _dev(x, w, bias, zpre, out)
    _lib.call('adn_head1x1_fwd', ptr(x), ptr(w), ptr(bias), x.numel() // Cc, Cc, dtype_code(x.dtype), act,
              float(max_depth), ptr(zpre), ptr(out), _stream())


def head1x1_bwd_workspace_bytes(pixels, Cc):
    return _lib.load().adn_head1x1_bwd_workspace_bytes(pixels, Cc)


def head1x1_bwd(gout, zpre, x, w, act, max_depth, gx, dw, db, workspace):
    Cc = x.shape[-1]
    _dev(gout, zpre, x, w, gx, dw, db, workspace)
    _lib.call('adn_head1x1_bwd', ptr(gout), ptr(zpre), ptr(x), ptr(w), x.numel() // Cc, Cc, dtype_code(x.dtype), act,
              float(max_depth), ptr(gx), ptr(dw), ptr(db), ptr(workspace),
              workspace.numel() * workspace.element_size(), _stream())


def l1tv_workspace_bytes(n):
    return _lib.load().adn_l1tv_workspace_bytes(n)


def l1tv_stats(pred, gt, stats, workspace):
    B, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
    _dev(pred, gt, stats, workspace)
    _lib.call('adn_l1tv_stats', ptr(pred), ptr(gt), B, H, W, ptr(stats), ptr(workspace),
              workspace.numel() * workspace.element_size(), _stream())


def l1tv_finish(pred, gt, stats, replicas, lambda_l1, lambda_smooth, loss_out, grad):
    B, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
    _dev(pred, gt, stats, loss_out, grad)
    _lib.call('adn_l1tv_finish', ptr(pred), ptr(gt), B, H, W, ptr(stats), int(replicas), float(lambda_l1),
              float(lambda_smooth), ptr(loss_out), ptr(grad), _stream())


# ---- binaural cross-attention (csrc/attn.hip, attn_mfma.hip) -----------------------------------------------
def nchw_slice_to_nhwc(src, c_lo, Cc, dst):
    """Channels [c_lo, c_lo + Cc) of src f32 [B,Ct,H,W] -> dst [B,H,W,Cpad] (extra channels zero)."""
    B, Ct, H, W = src.shape
    _dev(src, dst)
    _lib.call('adn_nchw_slice_to_nhwc', ptr(src), ptr(dst), B, Ct, c_lo, Cc, dst.shape[-1], H, W, dtype_code(dst.dtype),
              _stream())


def _esz(t):
    return t.element_size()


def _attn_desc(q, k, v, o, lse, dqk, dv, kv_shift, scale, dout=None, dq=None, dk=None, dvg=None, workspace=None):
    """q/k/v/o (and gradients) are [B2, N, *] views whose last-dim stride is 1 and row stride = stride(1)."""
    d = AdnAttnDesc()
    B2, N = q.shape[0], q.shape[1]
    d.dtype, d.B2, d.N, d.dqk, d.dv, d.kv_shift = dtype_code(q.dtype), B2, N, dqk, dv, kv_shift
    for t in (q, k, v, o, dout, dq, dk, dvg):
        if t is not None:
            assert t.stride(-1) == 1 and t.stride(0) == N * t.stride(1), 'attention operands must be [B2,N,ld] row views'
    _dev(q, k, v, o, lse, dout, dq, dk, dvg, workspace)
    d.q, d.k, d.v, d.o, d.lse = ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse)
    d.ld_q, d.ld_k, d.ld_v, d.ld_o = q.stride(1), k.stride(1), v.stride(1), o.stride(1)
    d.scale = float(scale)
    if dout is not None:
        d.dout, d.dq, d.dk, d.dvp = ptr(dout), ptr(dq), ptr(dk), ptr(dvg)
        d.ld_do, d.ld_dq, d.ld_dk, d.ld_dv = dout.stride(1), dq.stride(1), dk.stride(1), dvg.stride(1)
        d.workspace = ptr(workspace)
        d.workspace_bytes = workspace.numel() * workspace.element_size()
    return d


def attn_fwd(q, k, v, o, lse, dqk, dv, kv_shift, scale):
    d = _attn_desc(q, k, v, o, lse, dqk, dv, kv_shift, scale)
    _lib.call('adn_attn_fwd', C.byref(d), _stream())
    _lib.annotate(label='attn_fwd', flops=2.0 * d.B2 * d.N * d.N * (dqk + dv))


def attn_bwd(q, k, v, o, lse, dqk, dv, kv_shift, scale, dout, dq, dk, dvg, workspace):
    d = _attn_desc(q, k, v, o, lse, dqk, dv, kv_shift, scale, dout, dq, dk, dvg, workspace)
    _lib.call('adn_attn_bwd', C.byref(d), _stream())
    _lib.annotate(label='attn_bwd', flops=2.0 * d.B2 * d.N * d.N * (3 * dqk + 2 * dv))


def attn_form(q, k, v, o, lse, dqk, dv, kv_shift, scale, dout=None, dq=None, dk=None, dvg=None, workspace=None):
    """Kernel form of attn_fwd (no dout) / attn_bwd (with the gradient operands) on these operands: 'mfma' or 'generic'."""
    d = _attn_desc(q, k, v, o, lse, dqk, dv, kv_shift, scale, dout, dq, dk, dvg, workspace)
    form = _lib.load().adn_attn_form(C.byref(d), int(dout is not None))
    if form < 0:
        _lib.check(form, 'adn_attn_form')
    return ('generic', 'mfma')[form]


def channel_sum_workspace_bytes(rows, Cc):
    return _lib.load().adn_channel_sum_workspace_bytes(rows, Cc)


def channel_sum(x, rows, Cc, ld, out, workspace):
    _dev(x, out, workspace)
    _lib.call('adn_channel_sum', ptr(x), rows, Cc, ld, dtype_code(x.dtype), ptr(out), ptr(workspace),
              workspace.numel() * workspace.element_size(), _stream())


def gate_bwd(t, att, gamma, gsum, bias, Cc, dgamma, dbias, dw, workspace):
    _dev(t, att, gamma, gsum, bias, dgamma, dbias, dw, workspace)
    _lib.call('adn_gate_bwd', ptr(t), ptr(att), t.numel(), dtype_code(t.dtype), ptr(gamma), ptr(gsum), ptr(bias), Cc,
              ptr(dgamma), ptr(dbias), ptr(dw), dw.numel() if dw is not None else 0, ptr(workspace),
              workspace.numel() * workspace.element_size(), _stream())


# ---- AdaBins distillation model (csrc/adabins.hip) -----------------------------------------------------------
def _nbytes(t):
    return t.numel() * t.element_size()


def pool_workspace_bytes(B, HW, Cc, nq=1):
    return _lib.load().adn_pool_workspace_bytes(B, HW, Cc, nq)


def _contiguous(who, **named):
    """The AdaBins kernels index by shape alone: a strided view would be read (or written) at the wrong addresses."""
    for name, t in named.items():
        if t is not None and not t.is_contiguous():
            raise RuntimeError(f'{who}: {name} must be contiguous, got shape {tuple(t.shape)} with strides {tuple(t.stride())}')


def pool(x, y, B, HW, Cc, nq, scale, out, workspace):
    """x (and y) [B,HW,ld] contiguous NHWC tensors, ld = x.shape[-1] >= Cc (the first Cc channels of every row are
    summed) -> out f32 [B,Cc] (nq=1: scale*sum x) or [B,3,Cc] (sum x^2, y^2, x*y).  A channel-sliced view such as
    buf[..., :Cc] is refused: pass buf itself."""
    _dev(x, y, out, workspace)
    _contiguous('pool', x=x, y=y, out=out)
    if x.numel() != B * HW * x.shape[-1] or (y is not None and (y.shape != x.shape or y.dtype != x.dtype)):
        raise RuntimeError(f'pool: x has shape {tuple(x.shape)} for B={B}, HW={HW} (y: {None if y is None else tuple(y.shape)})')
    _lib.call('adn_pool', ptr(x), ptr(y), B, HW, Cc, x.shape[-1], nq, dtype_code(x.dtype), float(scale), ptr(out),
              ptr(workspace), _nbytes(workspace), _stream())


def binpred_fwd(g, W1, b1, W2, b2, mask, drop_p, max_depth, h1, widths, centers):
    B, Cb = g.shape
    Hd, nb = W1.shape[0], W2.shape[0]
    _dev(g, W1, b1, W2, b2, mask, h1, widths, centers)
    _lib.call('adn_binpred_fwd', ptr(g), ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(mask), float(drop_p), float(max_depth),
              B, Cb, Hd, nb, ptr(h1), ptr(widths), ptr(centers), _stream())


def binpred_bwd(dcent, widths, h1, g, W1, W2, has_mask, drop_p, max_depth, dW2p, db2p, dW1p, db1p, dg):
    B, Cb = g.shape
    Hd, nb = W1.shape[0], W2.shape[0]
    _dev(dcent, widths, h1, g, W1, W2, dW2p, db2p, dW1p, db1p, dg)
    _lib.call('adn_binpred_bwd', ptr(dcent), ptr(widths), ptr(h1), ptr(g), ptr(W1), ptr(W2), int(bool(has_mask)),
              float(drop_p), float(max_depth), B, Cb, Hd, nb, ptr(dW2p), ptr(db2p), ptr(dW1p), ptr(db1p), ptr(dg), _stream())


def dropout_mask(mask, p, seed, counter=None):
    _dev(mask, counter)
    _lib.call('adn_dropout_mask', ptr(mask), mask.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(counter),
              _stream())


# ---- InstanceNorm2d + activation (+ dropout) (csrc/inorm.hip) -------------------------------------------------
INORM_FORMS = {1: 'resident', 2: 'streaming', 3: 'resident-plain', 4: 'streaming-plain'}


def inorm_workspace_bytes(B, HW, Cc):
    n = _lib.load().adn_inorm_workspace_bytes(B, HW, Cc)
    if n < 0:
        raise ValueError('adn_inorm_workspace_bytes: ' + _lib.load().adn_last_error().decode())
    return n


def inorm_form(HW, Cc, dtype):
    """Host only: the kernel form the two launches take for this shape (a key of INORM_FORMS)."""
    form = _lib.load().adn_inorm_form(HW, Cc, dtype_code(dtype))
    if form < 0:
        raise ValueError('adn_inorm_form: ' + _lib.load().adn_last_error().decode())
    return INORM_FORMS[form]


def inorm_fwd(z, B, HW, Cc, eps, slope, mean, istd, out_leaky, out_relu, workspace, keep=None, keep_scale=1.0):
    """z [B, HW, Cc] (any contiguous NHWC view of it) -> mean / istd [B, Cc] and the activated copies."""
    _dev(z, mean, istd, out_leaky, out_relu, keep, workspace)
    _contiguous('inorm_fwd', z=z, out_leaky=out_leaky, out_relu=out_relu, keep=keep)
    if z.numel() != B * HW * Cc or mean.numel() != B * Cc or istd.numel() != B * Cc:
        raise RuntimeError(f'inorm_fwd: z {tuple(z.shape)} / mean {tuple(mean.shape)} for B={B}, HW={HW}, C={Cc}')
    for t in (out_leaky, out_relu):
        if t is not None and (t.numel() != z.numel() or t.dtype != z.dtype):
            raise RuntimeError('inorm_fwd: an output does not match z')
    if keep is not None and (keep.numel() != z.numel() or keep.dtype != torch.uint8):
        raise RuntimeError('inorm_fwd: keep must be a uint8 mask of the shape of z')
    _lib.call('adn_inorm_fwd', ptr(z), B, HW, Cc, dtype_code(z.dtype), float(eps), float(slope), ptr(mean), ptr(istd),
              ptr(out_leaky), ptr(out_relu), ptr(keep), float(keep_scale), ptr(workspace), _nbytes(workspace), _stream())


def dropout_apply(x, keep, scale):
    """x <- x * (keep ? scale : 0) in place; keep None: x * scale."""
    _dev(x, keep)
    _contiguous('dropout_apply', x=x, keep=keep)
    if keep is not None and (keep.numel() != x.numel() or keep.dtype != torch.uint8):
        raise RuntimeError('dropout_apply: keep must be a uint8 mask of the shape of x')
    _lib.call('adn_dropout_apply', ptr(x), ptr(keep), x.numel(), dtype_code(x.dtype), float(scale), _stream())


def inorm_bwd(g, z, mean, istd, B, HW, Cc, gscale, workspace):
    """g (masked upstream gradient, same layout and dtype as z) <- dz, in place."""
    _dev(g, z, mean, istd, workspace)
    _contiguous('inorm_bwd', g=g, z=z)
    if z.numel() != B * HW * Cc or g.numel() != z.numel() or g.dtype != z.dtype or mean.numel() != B * Cc \
            or istd.numel() != B * Cc:
        raise RuntimeError(f'inorm_bwd: g {tuple(g.shape)} / z {tuple(z.shape)} for B={B}, HW={HW}, C={Cc}')
    _lib.call('adn_inorm_bwd', ptr(g), ptr(z), ptr(mean), ptr(istd), B, HW, Cc, dtype_code(z.dtype), float(gscale),
              ptr(workspace), _nbytes(workspace), _stream())


def _vae_shapes(who, B, Cc, L, **named):
    """Every operand of the VAE kernels must hold exactly its [rows, cols] (contiguous): the kernels index by B, C, L."""
    for name, (t, numel) in named.items():
        if t is None:
            continue
        short = t.numel() < numel if name == 'counter' else t.numel() != numel      # counter: reads element 0
        if short or not t.is_contiguous():
            raise RuntimeError(f'{who}: {name} has shape {tuple(t.shape)} (contiguous: {t.is_contiguous()}), expected '
                               f'{numel} contiguous elements for B={B}, C={Cc}, L={L}')
        if name in ('out_relu', 'g_rec', 'dh'):
            dtype_code(t.dtype)
        elif name == 'counter':
            if t.dtype != torch.float64:
                raise RuntimeError(f'{who}: counter must be float64')
        elif t.dtype != torch.float32:
            raise RuntimeError(f'{who}: {name} must be float32, got {t.dtype}')


def vae_fwd(h, w_mu, b_mu, w_lv, b_lv, w_dec, b_dec, seed, counter, eps_in, mu, logvar, eps, z, kl_img, kl, out_relu):
    """VAE bottleneck forward (adn_vae_fwd): h f32 [B, C]; weights f32 in nn.Linear layout; out_relu [B, C] in the
    compute dtype (bf16 or f32) receives ReLU(fc_dec(z)).  eps_in (f32 [B, L]) replaces the in-kernel draw when given."""
    B, Cc = h.shape[0], h.numel() // h.shape[0]
    L = mu.shape[-1]
    _vae_shapes('vae_fwd', B, Cc, L, h=(h, B * Cc), w_mu=(w_mu, L * Cc), b_mu=(b_mu, L), w_lv=(w_lv, L * Cc),
                b_lv=(b_lv, L), w_dec=(w_dec, Cc * L), b_dec=(b_dec, Cc), counter=(counter, 1), eps_in=(eps_in, B * L),
                mu=(mu, B * L), logvar=(logvar, B * L), eps=(eps, B * L), z=(z, B * L), kl_img=(kl_img, B), kl=(kl, 1),
                out_relu=(out_relu, B * Cc))
    _dev(h, w_mu, b_mu, w_lv, b_lv, w_dec, b_dec, counter, eps_in, mu, logvar, eps, z, kl_img, kl, out_relu)
    _lib.call('adn_vae_fwd', ptr(h), B, Cc, L, ptr(w_mu), ptr(b_mu), ptr(w_lv), ptr(b_lv), ptr(w_dec), ptr(b_dec),
              int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(counter), ptr(eps_in), ptr(mu), ptr(logvar), ptr(eps), ptr(z), ptr(kl_img),
              ptr(kl), dtype_code(out_relu.dtype), ptr(out_relu), _stream())


VAE_DRAW, VAE_MEAN = 0, 1                   # adn.h: mode of adn_vae_sample


def vae_sample(h, w_mu, b_mu, w_lv, b_lv, w_dec, b_dec, seed, eps_in, mu, logvar, eps, z, kl_img, kl, out_relu,
               mode=VAE_DRAW):
    """K draws from one bottleneck (adn_vae_sample): mu / logvar [B, L] once; eps, z f32 [K, B, L]; out_relu [K * B, C]
    (compute dtype) = ReLU(fc_dec(z)), row k * B + b.  eps_in (f32 [K, B, L]) replaces the draw; mode VAE_MEAN decodes
    z = mu (K = 1)."""
    B, Cc = h.shape[0], h.numel() // h.shape[0]
    L = mu.shape[-1]
    Kn = z.shape[0]
    if z.dim() != 3 or Kn < 1:
        raise RuntimeError(f'vae_sample: z must be [K, B, L] with K >= 1, got {tuple(z.shape)}')
    _vae_shapes('vae_sample', B, Cc, L, h=(h, B * Cc), w_mu=(w_mu, L * Cc), b_mu=(b_mu, L), w_lv=(w_lv, L * Cc),
                b_lv=(b_lv, L), w_dec=(w_dec, Cc * L), b_dec=(b_dec, Cc), eps_in=(eps_in, Kn * B * L), mu=(mu, B * L),
                logvar=(logvar, B * L), eps=(eps, Kn * B * L), z=(z, Kn * B * L), kl_img=(kl_img, B), kl=(kl, 1),
                out_relu=(out_relu, Kn * B * Cc))
    _dev(h, w_mu, b_mu, w_lv, b_lv, w_dec, b_dec, eps_in, mu, logvar, eps, z, kl_img, kl, out_relu)
    _lib.call('adn_vae_sample', ptr(h), B, Cc, L, Kn, mode, ptr(w_mu), ptr(b_mu), ptr(w_lv), ptr(b_lv), ptr(w_dec),
              ptr(b_dec), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(eps_in), ptr(mu), ptr(logvar), ptr(eps), ptr(z), ptr(kl_img),
              ptr(kl), dtype_code(out_relu.dtype), ptr(out_relu), _stream())


def sample_stats(samples, mean, std):
    """Per-element mean and unbiased std over dim 0 of ``samples`` (f32 [K, ...], contiguous) -> mean, std (f32, the
    trailing shape): adn_sample_stats.  std is 0 for K = 1."""
    Kn = samples.shape[0]
    N = samples.numel() // max(Kn, 1)
    for name, t, numel in (('samples', samples, Kn * N), ('mean', mean, N), ('std', std, N)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel:
            raise RuntimeError(f'sample_stats: {name} must be contiguous float32 with {numel} elements, got '
                               f'{tuple(t.shape)} {t.dtype}')
    _dev(samples, mean, std)
    _lib.call('adn_sample_stats', ptr(samples), Kn, N, ptr(mean), ptr(std), _stream())


def vae_bwd_workspace_bytes(B, L):
    return _lib.load().adn_vae_bwd_workspace_bytes(B, L)


def vae_bwd(g_rec, h, mu, logvar, eps, z, w_mu, w_lv, w_dec, g_kl, dw_mu, db_mu, dw_lv, db_lv, dw_dec, db_dec, dh,
            workspace, kl=None, loss=None):
    """VAE bottleneck backward (adn_vae_bwd): g_rec [B, C] (compute dtype) = d loss / d h_recon after the ReLU mask;
    g_kl device f32 [1]; dh [B, C] (compute dtype, may be g_rec itself).  With ``loss``: loss[0] += g_kl * kl."""
    B, Cc = h.shape[0], h.numel() // h.shape[0]
    L = mu.shape[-1]
    _vae_shapes('vae_bwd', B, Cc, L, g_rec=(g_rec, B * Cc), h=(h, B * Cc), mu=(mu, B * L), logvar=(logvar, B * L),
                eps=(eps, B * L), z=(z, B * L), w_mu=(w_mu, L * Cc), w_lv=(w_lv, L * Cc), w_dec=(w_dec, Cc * L),
                g_kl=(g_kl, 1), dw_mu=(dw_mu, L * Cc), db_mu=(db_mu, L), dw_lv=(dw_lv, L * Cc), db_lv=(db_lv, L),
                dw_dec=(dw_dec, Cc * L), db_dec=(db_dec, Cc), dh=(dh, B * Cc), kl=(kl, 1), loss=(loss, 1))
    if g_rec.dtype != dh.dtype:
        raise RuntimeError('vae_bwd: g_rec and dh must share the compute dtype')
    _dev(g_rec, h, mu, logvar, eps, z, w_mu, w_lv, w_dec, g_kl, dw_mu, db_mu, dw_lv, db_lv, dw_dec, db_dec, dh, workspace,
         kl, loss)
    _lib.call('adn_vae_bwd', ptr(g_rec), dtype_code(g_rec.dtype), B, Cc, L, ptr(h), ptr(mu), ptr(logvar), ptr(eps), ptr(z),
              ptr(w_mu), ptr(w_lv), ptr(w_dec), ptr(g_kl), ptr(dw_mu), ptr(db_mu), ptr(dw_lv), ptr(db_lv), ptr(dw_dec),
              ptr(db_dec), ptr(kl), ptr(loss), ptr(dh), ptr(workspace), _nbytes(workspace), _stream())


def bcast_add(gx, dg, scale, accumulate):
    B, H, W, Cc = gx.shape
    _dev(gx, dg)
    _contiguous('bcast_add', gx=gx, dg=dg)
    _lib.call('adn_bcast_add', ptr(gx), ptr(dg), B, H * W, Cc, float(scale), int(bool(accumulate)), dtype_code(gx.dtype),
              _stream())


def bins_fwd(logits, centers, base):
    B, H, W, nb = logits.shape
    _dev(logits, centers, base)
    _contiguous('bins_fwd', logits=logits, centers=centers, base=base)
    _lib.call('adn_bins_fwd', ptr(logits), ptr(centers), B, H * W, nb, dtype_code(logits.dtype), ptr(base), _stream())


def bins_bwd_workspace_bytes(B, HW, nb):
    return _lib.load().adn_bins_bwd_workspace_bytes(B, HW, nb)


def bins_bwd(logits, centers, base, dbase, dmean, dlogits, dcent, workspace):
    B, H, W, nb = logits.shape
    _dev(logits, centers, base, dbase, dmean, dlogits, dcent, workspace)
    _contiguous('bins_bwd', logits=logits, centers=centers, base=base, dbase=dbase, dmean=dmean, dlogits=dlogits, dcent=dcent)
    _lib.call('adn_bins_bwd', ptr(logits), ptr(centers), ptr(base), ptr(dbase), ptr(dmean), B, H * W, nb,
              dtype_code(logits.dtype), ptr(dlogits), ptr(dcent), 0, ptr(workspace), _nbytes(workspace), _stream())


def distill_pix_stats(base, resid, gt, teacher, max_depth, final_out, stats, workspace):
    _dev(base, resid, gt, teacher, final_out, stats, workspace)
    _lib.call('adn_distill_pix_stats', ptr(base), ptr(resid), ptr(gt), ptr(teacher), base.numel(), float(max_depth),
              ptr(final_out), ptr(stats), ptr(workspace), _nbytes(workspace), _stream())


def distill_pix_grad(base, resid, gt, teacher, max_depth, stats, lt, lr, ls, dbase, dres):
    _dev(base, resid, gt, teacher, stats, dbase, dres)
    _lib.call('adn_distill_pix_grad', ptr(base), ptr(resid), ptr(gt), ptr(teacher), base.numel(), float(max_depth),
              ptr(stats), float(lt), float(lr), float(ls), ptr(dbase), ptr(dres), _stream())


def featcos_grad(a, r, stats, coef, ga):
    B, H, W, Cc = a.shape
    _dev(a, r, stats, ga)
    _contiguous('featcos_grad', a=a, r=r, stats=stats, ga=ga)
    _lib.call('adn_featcos_grad', ptr(a), ptr(r), ptr(stats), B, H * W, Cc, dtype_code(a.dtype), float(coef), ptr(ga),
              _stream())


def distill_small(mean_s, mean_t, cent_s, cent_t, feat_stats, feat_channels, pix_stats, temperature, lambdas, terms,
                  dmean, dcent):
    """lambdas = (task, response, feature, bin, sparse); feat_stats: 5 tensors [B,3,C] or None (no teacher)."""
    d = AdnDistillSmall()
    has_t = mean_t is not None
    _dev(mean_s, mean_t, cent_s, cent_t, pix_stats, terms, dmean, dcent)
    d.mean_student, d.mean_teacher, d.centers_student, d.centers_teacher = ptr(mean_s), ptr(mean_t), ptr(cent_s), ptr(cent_t)
    for i in range(5):
        d.feat_stats[i] = ptr(feat_stats[i]) if has_t else None
        d.feat_channels[i] = feat_channels[i] if has_t else 0
    d.pix_stats = ptr(pix_stats)
    d.B, d.nb, d.has_teacher = mean_s.shape[0], mean_s.shape[1], int(has_t)
    d.temperature = float(temperature)
    (d.lambda_task, d.lambda_response, d.lambda_feature, d.lambda_bin, d.lambda_sparse) = [float(v) for v in lambdas]
    d.terms, d.dmean, d.dcent = ptr(terms), ptr(dmean), ptr(dcent)
    _lib.call('adn_distill_small', C.byref(d), _stream())


def resize_nearest(src, S):
    """src f32 [..., H, W] -> new tensor [..., S, S], F.interpolate(mode='nearest')."""
    _dev(src)
    src = src.contiguous()
    out = torch.empty(src.shape[:-2] + (S, S), dtype=torch.float32, device=src.device)
    planes = src.numel() // (src.shape[-1] * src.shape[-2])
    _lib.call('adn_resize_nearest', ptr(src), planes, src.shape[-2], src.shape[-1], S, ptr(out), _stream())
    return out


def resize_nearest_bwd(gout, H, W):
    """gout f32 [..., S, S] -> gradient of the nearest-resized source, new tensor [..., H, W]."""
    _dev(gout)
    gout = gout.contiguous()
    S = gout.shape[-1]
    out = torch.empty(gout.shape[:-2] + (H, W), dtype=torch.float32, device=gout.device)
    planes = gout.numel() // (S * S)
    _lib.call('adn_resize_nearest_bwd', ptr(gout), planes, H, W, S, ptr(out), _stream())
    return out


def image_prepare(src, S, out):
    """src uint8 [B,H,W,3] BGR (decoded camera frames) -> out f32 [B,3,S,S] RGB in [0,1] (cv2 INTER_LINEAR resize)."""
    _dev(src, out)
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[-1] != 3:
        raise TypeError('image_prepare: src must be uint8 [B,H,W,3]')
    B, H, W, _ = src.shape
    _lib.call('adn_image_prepare', ptr(src), B, H, W, S, ptr(out), _stream())


def depth_prepare(src, S, max_depth, norm, out):
    """Raw depth maps in mm [planes,H,W] (float32 / uint16 / int32) -> metres, cleaned, clipped, nearest-resized."""
    code = {torch.float32: 0, torch.uint16: 1, torch.int32: 2}[src.dtype]
    planes, H, W = src.shape
    _dev(src, out)
    _lib.call('adn_depth_prepare', ptr(src), code, planes, H, W, S, float(max_depth or 0.0), float(norm or 0.0), ptr(out),
              _stream())


# ---- Base + Residual model (csrc/baseres.hip) --------------------------------------------------------------------
def lowpass_workspace_bytes(B, H, W, k):
    return _lib.load().adn_lowpass_workspace_bytes(B, H, W, k)


def lowpass(gt, k, out, workspace):
    """gt f32 [B,1,H,W] -> avg_pool2d(k, 1, k//2) + bilinear resize back to H x W."""
    B, H, W = gt.shape[0], gt.shape[-2], gt.shape[-1]
    _dev(gt, out, workspace)
    _lib.call('adn_lowpass', ptr(gt), B, H, W, k, ptr(out), ptr(workspace), _nbytes(workspace), _stream())


def clamp_add(a, b, max_depth, out):
    _dev(a, b, out)
    _lib.call('adn_clamp_add', ptr(a), ptr(b), a.numel(), float(max_depth), ptr(out), _stream())


def baseres_stats(base, resid, strct, gt, recon, lrecon, lbase, lsparse, stats, terms, workspace):
    _dev(base, resid, strct, gt, recon, stats, terms, workspace)
    _lib.call('adn_baseres_stats', ptr(base), ptr(resid), ptr(strct), ptr(gt), base.numel(), ptr(recon), float(lrecon),
              float(lbase), float(lsparse), ptr(stats), ptr(terms), ptr(workspace), _nbytes(workspace), _stream())


def baseres_grad(base, resid, strct, gt, gfinal, max_depth, stats, lbase, lsparse, dbase, dres):
    _dev(base, resid, strct, gt, gfinal, stats, dbase, dres)
    _lib.call('adn_baseres_grad', ptr(base), ptr(resid), ptr(strct), ptr(gt), ptr(gfinal), base.numel(), float(max_depth),
              ptr(stats), float(lbase), float(lsparse), ptr(dbase), ptr(dres), _stream())


# ---- coarse-depth classification family (csrc/coarse.hip) ---------------------------------------------------------
CE_MODES = {'soft': 0, 'focal': 1, 'ce': 2}


def coarse_targets_workspace_bytes(n):
    return _lib.load().adn_coarse_targets_workspace_bytes(n)


def coarse_targets(depth, edges, bins, stats, workspace):
    """depth f32 [n]; edges f32 = the n_bins - 1 interior bin edges; bins int32 [n] or None (valid count alone);
    stats f64[>= 1]: stats[0] = count of depth > 0."""
    _dev(depth, edges, bins, stats, workspace)
    if depth.dtype != torch.float32 or not depth.is_contiguous():
        raise RuntimeError('coarse_targets: depth must be contiguous float32')
    nb = 0
    if bins is not None:
        if edges is None or bins.dtype != torch.int32 or bins.numel() != depth.numel() or edges.dtype != torch.float32:
            raise RuntimeError('coarse_targets: bins must be int32 with one entry per depth value, edges float32')
        nb = edges.numel() + 1
    _lib.call('adn_coarse_targets', ptr(depth), depth.numel(), ptr(edges), nb, ptr(bins), ptr(stats), ptr(workspace),
              _nbytes(workspace), _stream())


def coarse_loss_workspace_bytes(pixels):
    return _lib.load().adn_coarse_loss_workspace_bytes(pixels)


def coarse_loss(logits, nb, centers, depth, bins=None, gt=None, n_valid=None, pixels_global=None, ce_mode=0, sigma=2.0,
                gamma=2.0, ce_weight=1.0, reg_weight=0.5, argmax=None, dlogits=None, workspace=None):
    """logits [..., ld] (bf16 / f32, ld >= nb), centers f32 [nb], depth f32 [pixels] out; see adn_coarse_loss."""
    ld = logits.shape[-1]
    pixels = logits.numel() // ld
    _dev(logits, centers, depth, bins, gt, n_valid, argmax, dlogits, workspace)
    for name, t, dt in (('centers', centers, torch.float32), ('depth', depth, torch.float32), ('bins', bins, torch.int32),
                        ('gt', gt, torch.float32), ('n_valid', n_valid, torch.float64), ('argmax', argmax, torch.int32),
                        ('dlogits', dlogits, logits.dtype)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise RuntimeError(f'coarse_loss: {name} must be contiguous {dt}')
    for name, t in (('depth', depth), ('bins', bins), ('gt', gt), ('argmax', argmax)):
        if t is not None and t.numel() != pixels:
            raise RuntimeError(f'coarse_loss: {name} has {t.numel()} elements for {pixels} pixels')
    if centers.numel() != nb or not logits.is_contiguous() or (dlogits is not None and dlogits.shape != logits.shape):
        raise RuntimeError('coarse_loss: centers must hold n_bins values; logits / dlogits contiguous and same shape')
    d = AdnCoarseLoss()
    d.logits, d.dtype, d.nb, d.ld, d.ce_mode = ptr(logits), dtype_code(logits.dtype), nb, ld, int(ce_mode)
    d.pixels, d.pixels_global = pixels, int(pixels_global if pixels_global is not None else pixels)
    d.centers, d.bins, d.gt, d.n_valid = ptr(centers), ptr(bins), ptr(gt), ptr(n_valid)
    d.sigma, d.gamma, d.ce_weight, d.reg_weight = float(sigma), float(gamma), float(ce_weight), float(reg_weight)
    d.depth, d.argmax, d.dlogits = ptr(depth), ptr(argmax), ptr(dlogits)
    d.workspace, d.workspace_bytes = ptr(workspace), (_nbytes(workspace) if workspace is not None else 0)
    _lib.call('adn_coarse_loss', C.byref(d), _stream())


def coarse_loss_finish(workspace, pixels, sums, n_valid, pixels_global, ce_weight, reg_weight, terms):
    """workspace None: sums f64[2] are taken as given (all-reduced); terms f32[3] = ce, regression, total (or None)."""
    _dev(workspace, sums, n_valid, terms)
    _lib.call('adn_coarse_loss_finish', ptr(workspace), int(pixels), ptr(sums), ptr(n_valid), int(pixels_global),
              float(ce_weight), float(reg_weight), ptr(terms), _stream())


EVAL_SUMS, EVAL_OUT = 41, 39          # f64 lengths of adn_coarse_eval_finish's sums and out (include/adn.h)
EVAL_FIELDS = ('n_valid', 'top1', 'within1', 'mean_bin_error', 'mean_std', 'mean_entropy', 'mean_confidence',
               'std_error_corr', 'ece')                     # out[:9]; out[9:] is the reliability table [10][3]


def coarse_decode(logits, nb, centers, mean=None, hard=None, std=None, entropy=None, confidence=None, argmax=None):
    """logits [..., ld] (bf16 / f32, ld >= nb), centers f32 [nb] -> the given planes, f32 [pixels] (argmax int32), each
    optional; see adn_coarse_decode."""
    ld = logits.shape[-1]
    pixels = logits.numel() // ld
    _dev(logits, centers, mean, hard, std, entropy, confidence, argmax)
    for name, t, dt in (('centers', centers, torch.float32), ('mean', mean, torch.float32), ('hard', hard, torch.float32),
                        ('std', std, torch.float32), ('entropy', entropy, torch.float32),
                        ('confidence', confidence, torch.float32), ('argmax', argmax, torch.int32)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise RuntimeError(f'coarse_decode: {name} must be contiguous {dt}')
        if t is not None and name != 'centers' and t.numel() != pixels:
            raise RuntimeError(f'coarse_decode: {name} has {t.numel()} elements for {pixels} pixels')
    if centers.numel() != nb or not logits.is_contiguous():
        raise RuntimeError('coarse_decode: centers must hold n_bins values; logits contiguous')
    d = AdnCoarseDecode()
    d.logits, d.dtype, d.nb, d.ld, d.pixels = ptr(logits), dtype_code(logits.dtype), nb, ld, pixels
    d.centers, d.mean, d.hard, d.stdev = ptr(centers), ptr(mean), ptr(hard), ptr(std)
    d.entropy, d.confidence, d.argmax = ptr(entropy), ptr(confidence), ptr(argmax)
    _lib.call('adn_coarse_decode', C.byref(d), _stream())


def coarse_eval_stats_workspace_bytes(pixels):
    return _lib.load().adn_coarse_eval_stats_workspace_bytes(pixels)


def coarse_eval_stats(argmax, bins, confidence, std, entropy, mean, gt, workspace):
    """The planes of coarse_decode, the target bins (int32) and gt (f32), [pixels] each -> per-block partials in
    ``workspace``; see adn_coarse_eval_stats."""
    pixels = gt.numel()
    _dev(argmax, bins, confidence, std, entropy, mean, gt, workspace)
    for name, t, dt in (('argmax', argmax, torch.int32), ('bins', bins, torch.int32), ('confidence', confidence, torch.float32),
                        ('std', std, torch.float32), ('entropy', entropy, torch.float32), ('mean', mean, torch.float32),
                        ('gt', gt, torch.float32)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != pixels:
            raise RuntimeError(f'coarse_eval_stats: {name} must be contiguous {dt} with {pixels} elements')
    d = AdnCoarseEvalStats()
    d.argmax, d.bins, d.confidence, d.stdev = ptr(argmax), ptr(bins), ptr(confidence), ptr(std)
    d.entropy, d.mean, d.gt, d.pixels = ptr(entropy), ptr(mean), ptr(gt), pixels
    d.workspace, d.workspace_bytes = ptr(workspace), _nbytes(workspace)
    _lib.call('adn_coarse_eval_stats', C.byref(d), _stream())


def coarse_eval_finish(workspace, pixels, sums, out=None):
    """workspace None: sums f64[EVAL_SUMS] are taken as given (added up over batches by the caller); out f64[EVAL_OUT] or
    None."""
    _dev(workspace, sums, out)
    for name, t, n in (('sums', sums, EVAL_SUMS), ('out', out, EVAL_OUT)):
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or t.numel() < n):
            raise RuntimeError(f'coarse_eval_finish: {name} must be contiguous float64 with {n} elements')
    _lib.call('adn_coarse_eval_finish', ptr(workspace), int(pixels), ptr(sums), ptr(out), _stream())


# ---- dual-regression coarse-depth family (csrc/dualreg.hip) --------------------------------------------------------
def dualreg_loss_workspace_bytes(pixels):
    return _lib.load().adn_dualreg_loss_workspace_bytes(pixels)


def dualreg_loss(coarse, offset, final, gt=None, n_valid=None, pixels_global=None, coarse_weight=1.0, final_weight=1.0,
                 offset_reg_weight=0.01, dcoarse=None, doffset=None, workspace=None):
    """coarse / offset f32 [pixels] -> final = coarse + offset; with gt also dcoarse / doffset and the per-block partials in
    ``workspace``; see adn_dualreg_loss."""
    pixels = coarse.numel()
    _dev(coarse, offset, final, gt, n_valid, dcoarse, doffset, workspace)
    for name, t in (('coarse', coarse), ('offset', offset), ('final', final), ('gt', gt), ('dcoarse', dcoarse),
                    ('doffset', doffset)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != pixels):
            raise RuntimeError(f'dualreg_loss: {name} must be contiguous float32 with {pixels} elements')
    if n_valid is not None and n_valid.dtype != torch.float64:
        raise RuntimeError('dualreg_loss: n_valid must be float64')
    d = AdnDualRegLoss()
    d.coarse, d.offset, d.gt, d.n_valid = ptr(coarse), ptr(offset), ptr(gt), ptr(n_valid)
    d.pixels, d.pixels_global = pixels, int(pixels_global if pixels_global is not None else pixels)
    d.coarse_weight, d.final_weight, d.offset_reg_weight = float(coarse_weight), float(final_weight), float(offset_reg_weight)
    d.final_depth, d.dcoarse, d.doffset = ptr(final), ptr(dcoarse), ptr(doffset)
    d.workspace, d.workspace_bytes = ptr(workspace), (_nbytes(workspace) if workspace is not None else 0)
    _lib.call('adn_dualreg_loss', C.byref(d), _stream())


def dualreg_loss_finish(workspace, pixels, sums, n_valid, pixels_global, coarse_weight, final_weight, offset_reg_weight,
                        terms):
    """workspace None: sums f64[3] are taken as given (all-reduced); terms f32[4] = coarse, final, offset_reg, total (or
    None)."""
    _dev(workspace, sums, n_valid, terms)
    _lib.call('adn_dualreg_loss_finish', ptr(workspace), int(pixels), ptr(sums), ptr(n_valid), int(pixels_global),
              float(coarse_weight), float(final_weight), float(offset_reg_weight), ptr(terms), _stream())


# ---- hybrid coarse-depth family (csrc/hybrid.hip) -------------------------------------------------------------------
REG_MODES = {'l1': 0, 'l2': 1}


def hybrid_loss_workspace_bytes(pixels):
    return _lib.load().adn_hybrid_loss_workspace_bytes(pixels)


def hybrid_loss(logits, nb, centers, coarse, offset, bins, gt, final, dlogits, doffset, workspace, pixels_global=None,
                ce_weight=1.0, reg_weight=1.0, offset_reg_weight=0.1, label_smoothing=0.0, reg_mode=0):
    """logits [..., ld] (bf16 / f32, ld >= nb), centers f32 [nb], coarse / offset / gt f32 [pixels], bins int32 [pixels] ->
    final = coarse + offset, dlogits (the logits' dtype and shape), doffset f32 [pixels] and the per-block partials in
    ``workspace``; see adn_hybrid_loss."""
    ld = logits.shape[-1]
    pixels = logits.numel() // ld
    _dev(logits, centers, coarse, offset, bins, gt, final, dlogits, doffset, workspace)
    for name, t, dt in (('centers', centers, torch.float32), ('coarse', coarse, torch.float32),
                        ('offset', offset, torch.float32), ('bins', bins, torch.int32), ('gt', gt, torch.float32),
                        ('final', final, torch.float32), ('doffset', doffset, torch.float32),
                        ('dlogits', dlogits, logits.dtype)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise RuntimeError(f'hybrid_loss: {name} must be contiguous {dt}')
    for name, t in (('coarse', coarse), ('offset', offset), ('bins', bins), ('gt', gt), ('final', final),
                    ('doffset', doffset)):
        if t is not None and t.numel() != pixels:
            raise RuntimeError(f'hybrid_loss: {name} has {t.numel()} elements for {pixels} pixels')
    if ((centers is not None and centers.numel() != nb) or not logits.is_contiguous() or
            (dlogits is not None and dlogits.shape != logits.shape)):
        raise RuntimeError('hybrid_loss: centers must hold n_bins values; logits / dlogits contiguous and same shape')
    d = AdnHybridLoss()
    d.logits, d.dtype, d.nb, d.ld, d.reg_mode = ptr(logits), dtype_code(logits.dtype), nb, ld, int(reg_mode)
    d.pixels, d.pixels_global = pixels, int(pixels_global if pixels_global is not None else pixels)
    d.centers, d.coarse, d.offset, d.bins, d.gt = ptr(centers), ptr(coarse), ptr(offset), ptr(bins), ptr(gt)
    d.ce_weight, d.reg_weight, d.offset_reg_weight = float(ce_weight), float(reg_weight), float(offset_reg_weight)
    d.label_smoothing = float(label_smoothing)
    d.final_depth, d.dlogits, d.doffset = ptr(final), ptr(dlogits), ptr(doffset)
    d.workspace, d.workspace_bytes = ptr(workspace), (_nbytes(workspace) if workspace is not None else 0)
    _lib.call('adn_hybrid_loss', C.byref(d), _stream())


def hybrid_loss_finish(workspace, pixels, sums, pixels_global, ce_weight, reg_weight, offset_reg_weight, terms):
    """workspace None: sums f64[4] are taken as given (all-reduced); terms f32[5] = ce, regression, offset_reg, coarse_l1,
    total (or None)."""
    _dev(workspace, sums, terms)
    _lib.call('adn_hybrid_loss_finish', ptr(workspace), int(pixels), ptr(sums), int(pixels_global), float(ce_weight),
              float(reg_weight), float(offset_reg_weight), ptr(terms), _stream())
