"""Tensor-level wrappers over the C ABI (include/wesup_hip.h).

Each wrapper checks on the HOST that operand shapes/dtypes/devices match what
the kernel and its grid assume (a faulting kernel can reset the GPU), then calls
the entry on torch's current stream.  torch is only used for device memory and
streams here.  No CPU fallback: a CPU tensor raises.
"""
import ctypes
import struct

import torch

from . import _lib

RELU_IN, RELU_OUT, ACCUM, MASK = 1, 2, 4, 8
# Stream-K tail of the NT GEMM family (the tiles of a short last round cut along K over all block slots + a fix-up launch): a
# kernel ALONE on the GPU gains 6-7 % from it, inside the 3-stream training step the other streams fill a short round anyway and
# the fix-up launches sit on the chain (17.52 vs 17.34 ms, round 2).  The step never uses it; a single-stream caller (a tool, an
# inference experiment, the tests of the path) switches it on for its own calls with set_streamk(True).
STREAMK = False


def set_streamk(on):
    global STREAMK
    STREAMK = bool(on)


if hasattr(torch._C, '_cuda_getCurrentRawStream') and hasattr(torch._C, '_cuda_getDevice'):
    def _stream():
        # the raw handle of torch's current stream on the current device (torch.cuda.current_stream().cuda_stream builds a Stream
        # object per call: 2.5 us, ~500 times per training step -- a quarter of the host time of a step at batch 1).  The engine
        # checks once per forward that the current device is the model's.
        return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
else:                                                  # a torch build without the private accessors
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# TIMING-ONLY diagnostics (bench.py --diag-skip, results wrong): 'tout' leaves out the separate output transforms of the K = 512
# Winograd layers, 'tin' the input transforms of the forward -- what those launches cost the step
DIAG = set()


# Optional HIP-event timing of the kernel classes that are launched outside the engine's schedule (superpixel
# preprocessing, label propagation + loss, SGD): bench.py hands the engine's KernelTimer over; None = no events.
_timer = None


def set_timer(timer):
    global _timer
    _timer = timer


def _tbegin(tag):
    return _timer.begin(tag) if _timer is not None else None


def _tend(tok, work):
    if tok is not None:
        _timer.end(tok, work)


def _chk(t, dtype=torch.float32, name='tensor'):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.WesupHipError(f'{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback)')
    if t.dtype != dtype:
        raise _lib.WesupHipError(f'{name}: expected {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise _lib.WesupHipError(f'{name}: expected a contiguous tensor')
    return t


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_ws_cache = {}
_ws_first = {}         # key -> size of the first request
_ws_retired = []       # buffers replaced by a growth: kept for a while (another stream's queued kernels may still use them)
ws_generation = 0      # bumped whenever a workspace is (re)allocated: a recorded step plan holds the old addresses


ws_headroom = 1        # 2 once the step runner has met a second shape (set_workspace_headroom): see workspace()


def set_workspace_headroom(factor):
    global ws_headroom
    ws_headroom = max(1, int(factor))


def workspace(nbytes, device, tag='default'):
    """Grow-only byte workspace per (device, tag), served exactly while a run has one shape (``ws_headroom`` 1: the benchmark
    configurations pay nothing extra).  Once the step runner has met a second shape it sets the headroom to 2: from then on a
    workspace that has to grow becomes twice what is asked for and, in the same go, every other workspace of the device at least
    twice its first size.  Every growth bumps ``ws_generation`` and with it drops every recorded step plan and every plan waiting
    for its twin; under multi-scale training (utils/data.py:98-101: shapes within a factor 1.8 of each other in area) exact-fit
    growth did that once per new largest shape and tag, spread over the first dozens of shapes -- a shape's first recording hardly
    ever met its twin (3.4 -> 2.2 recordings per shape over the 94-shape rotation; the cold line itself moves with the box, 262 ... 297 img/s)."""
    global ws_generation
    key = (str(device), tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        regrow = buf is not None and ws_headroom > 1
        buf = None                                       # (the tag's own stream orders the release behind its queued kernels)
        _ws_cache.pop(key, None)
        _ws_first.setdefault(key, int(nbytes))
        buf = torch.empty(max((ws_headroom if regrow else 1) * int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
        if regrow:
            for k2 in [k for k in _ws_cache if k[0] == key[0] and k != key]:
                if _ws_cache[k2].numel() < ws_headroom * _ws_first.get(k2, 0):
                    _ws_retired.append(_ws_cache.pop(k2))      # (ITS stream may still run kernels of this very walk on it)
                    _ws_cache[k2] = torch.empty(ws_headroom * _ws_first[k2], dtype=torch.uint8, device=device)
        del _ws_retired[:-64]
        ws_generation += 1
    return buf


def _nt_workspace(nbytes, device):
    """Stream-K workspace of the NT GEMM family: one per stream, because launches on different streams overlap."""
    if not nbytes:
        return None
    return workspace(nbytes, device, 'nt%x' % torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------- input pipeline
def augment(img_u8, mask_u8, params, n_classes=2, elastic=None):
    """img (B,H,W,3) uint8, mask (B,H,W) uint8 class index or None, params (B,12) fp32 -> img f32 (B,3,H,W) in [0,1],
    one-hot mask uint8 (B,C,H,W) or None.  elastic = (field (B,2,hc,wc) fp32, params (B,12) fp32, cell): the displacement
    field of ElasticTransform on a coarse grid (utils.data.elastic_field) for the images whose params row has on = 1."""
    _chk(img_u8, torch.uint8, 'img'); _chk(params, name='params')
    B, H, W, three = img_u8.shape
    assert three == 3 and params.shape == (B, 12)
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=img_u8.device)
    om = None
    if mask_u8 is not None:
        _chk(mask_u8, torch.uint8, 'mask'); assert mask_u8.shape == (B, H, W)
        om = torch.empty(B, n_classes, H, W, dtype=torch.uint8, device=img_u8.device)
    ef = ep = None
    hc = wc = cell = 0
    if elastic is not None:
        ef, ep, cell = elastic
        _chk(ef, name='elastic field'); _chk(ep, name='elastic params')
        hc, wc = ef.shape[2:]
        assert ef.shape == (B, 2, hc, wc) and ep.shape == (B, 12) and cell > 0 and hc * cell >= H and wc * cell >= W
    _lib.call('wesup_augment', _p(img_u8), _p(mask_u8), _p(params), _p(ef), _p(ep), hc, wc, int(cell), _p(out), _p(om), B, H, W,
              n_classes, _stream())
    return out, om


def appearance(img_u8, params):
    """img (B,H,W,3) uint8, params (B,8) fp32 {alpha, beta, hue, sat, val, clahe_clip, blur, 0} -> (B,H,W,3) uint8 after
    HueSaturationValue, RandomBrightnessContrast, CLAHE and Blur(3) in the reference's order."""
    _chk(img_u8, torch.uint8, 'img'); _chk(params, name='params')
    B, H, W, three = img_u8.shape
    assert three == 3 and params.shape == (B, 8)
    out = torch.empty_like(img_u8)
    nb = _lib.load().wesup_appearance_workspace_bytes(B, H, W)
    ws = workspace(nb, img_u8.device, 'appearance')
    _lib.call('wesup_appearance', _p(img_u8), _p(params), _p(out), B, H, W, _p(ws), nb, _stream())
    return out


# ---------------------------------------------------------------- packing
def pack_input(img, out=None):
    _chk(img, name='img')
    B, C, H, W = img.shape
    assert C == 3
    if out is None:
        out = torch.empty(B, H, W, 4, dtype=torch.float32, device=img.device)
    _lib.call('wesup_pack_input', _p(img), _p(out), B, H, W, _stream())
    return out


def conv3x3_kpad(Ci):
    return _lib.load().wesup_conv3x3_kpad(int(Ci))


def pack_conv3x3_weight(w, w_fwd=None, w_dgrad=None, need_dgrad=True, need_fwd=True):
    _chk(w, name='w')
    Co, Ci, kh, kw = w.shape
    assert kh == 3 and kw == 3 and (need_fwd or need_dgrad)
    if need_fwd and w_fwd is None:
        w_fwd = torch.empty(Co, conv3x3_kpad(Ci), dtype=torch.float32, device=w.device)
    if need_dgrad and w_dgrad is None:
        w_dgrad = torch.empty(Ci, 9 * Co, dtype=torch.float32, device=w.device)
    _lib.call('wesup_pack_conv3x3_weight', _p(w), _p(w_fwd) if need_fwd else None, _p(w_dgrad) if need_dgrad else None,
              Co, Ci, _stream())
    return w_fwd, w_dgrad


def transpose(a, out=None):
    _chk(a, name='a')
    r, c = a.shape
    if out is None:
        out = torch.empty(c, r, dtype=torch.float32, device=a.device)
    _lib.call('wesup_transpose', _p(a), _p(out), r, c, _stream())
    return out


TRANSPOSE_MAX = 40      # items per wesup_transpose_batched launch (csrc/spatial.hip)


def transpose_batched(pairs):
    """[(a (r, c), out (c, r)), ...]: every out = a^T, TRANSPOSE_MAX pairs per launch (a batch of 32 images at 480 x 480 hands over
    64 interpolation-pooling matrices: two launches)."""
    for a, out in pairs:
        _chk(a, name='a'); _chk(out, name='out')
        assert out.shape == (a.shape[1], a.shape[0])
    for i0 in range(0, len(pairs), TRANSPOSE_MAX):
        part = pairs[i0:i0 + TRANSPOSE_MAX]
        n = len(part)
        arr = (_lib.TransposeItem * n)()
        for i, (a, out) in enumerate(part):
            arr[i].src, arr[i].dst, arr[i].rows, arr[i].cols = a.data_ptr(), out.data_ptr(), a.shape[0], a.shape[1]
        _lib.call('wesup_transpose_batched', ctypes.cast(arr, ctypes.c_void_p), n, _stream())


def scale_rows_by_area(x, area):
    """x (B,Kmax,C) *= 1 / area (B,Kmax) per row, in place (0 for rows of area 0): the pre-scaled form of the side-branch gradient
    rows that conv3x3_dgrad_winograd_gather(area_new=None) gathers."""
    _chk(x, name='x'); _chk(area, torch.int32, 'area')
    assert x.dim() == 3 and area.shape == x.shape[:2]
    _lib.call('wesup_scale_rows_by_area', _p(x), _p(area), x.shape[0] * x.shape[1], x.shape[2], _stream())
    return x


def winograd_fused_min_blocks():
    """The process-wide rule behind wesup_winograd_fused_route: grids below this many blocks take the two-kernel route."""
    return int(_lib.load().wesup_winograd_set_fused_min_blocks(-1))


# ---------------------------------------------------------------- sync edges / step plans (csrc/plan.hip)
def sync_record(slot, stream=None):
    """Mark the work queued so far on ``stream`` (raw handle; None: torch's current stream) in event slot ``slot``."""
    _lib.call('wesup_sync_record', int(slot), _stream() if stream is None else ctypes.c_void_p(stream))


def sync_wait(slot, stream=None):
    """``stream`` waits for the latest mark of ``slot``."""
    _lib.call('wesup_sync_wait', int(slot), _stream() if stream is None else ctypes.c_void_p(stream))


# ---------------------------------------------------------------- conv 3x3
def conv3x3_fwd(x, w_fwd, bias, Cout, relu_in, out=None, out_relu=None, side=None):
    """side = (side_w (Cout/2, Cout), side_bias or None, side_out 2-D view with row stride >= Cout/2): the layer's 1x1
    side conv computed in the conv's epilogue (Cout 64 / 128 only)."""
    _chk(x, name='x'); _chk(w_fwd, name='w_fwd')
    B, H, W, Cin = x.shape
    assert w_fwd.shape == (Cout, conv3x3_kpad(Cin)), (w_fwd.shape, Cout, Cin)
    if bias is not None:
        _chk(bias, name='bias'); assert bias.numel() == Cout
    if out is None:
        out = torch.empty(B, H, W, Cout, dtype=torch.float32, device=x.device)
    assert out.shape == (B, H, W, Cout) and out.is_contiguous()
    if out_relu is not None:
        _chk(out_relu, name='out_relu'); assert out_relu.shape == out.shape
    if side is not None:
        sw, sbias, sout = side
        _chk(sw, name='side_w'); assert sw.shape == (Cout // 2, Cout)
        if sbias is not None:
            _chk(sbias, name='side_bias'); assert sbias.numel() == Cout // 2
        assert sout.dtype == torch.float32 and sout.is_cuda and sout.dim() == 2 and sout.stride(1) == 1
        assert sout.shape == (B * H * W, Cout // 2) and sout.stride(0) >= Cout // 2
        _lib.call('wesup_conv3x3_fwd_side', _p(x), _p(w_fwd), _p(bias), _p(out), _p(out_relu), _p(sw), _p(sbias), _p(sout),
                  sout.stride(0), B, H, W, Cin, Cout, int(relu_in), _stream())
        return out
    nb = _lib.load().wesup_conv3x3_workspace_bytes(B, H, W, Cin, Cout) if STREAMK else 0
    _lib.call('wesup_conv3x3_fwd', _p(x), _p(w_fwd), _p(bias), _p(out), _p(out_relu), B, H, W, Cin, Cout, int(relu_in),
              _p(_nt_workspace(nb, x.device)), nb, _stream())
    return out


def conv3x3_dgrad(dy, w_dgrad, Cin, mask_src=None, out=None, accumulate=False):
    _chk(dy, name='dy'); _chk(w_dgrad, name='w_dgrad')
    B, H, W, Cout = dy.shape
    assert w_dgrad.shape == (Cin, 9 * Cout)
    if mask_src is not None:
        _chk(mask_src, name='mask_src'); assert mask_src.shape == (B, H, W, Cin)
    if out is None:
        assert not accumulate
        out = torch.empty(B, H, W, Cin, dtype=torch.float32, device=dy.device)
    assert out.shape == (B, H, W, Cin) and out.is_contiguous()
    nb = _lib.load().wesup_conv3x3_workspace_bytes(B, H, W, Cout, Cin) if STREAMK else 0
    _lib.call('wesup_conv3x3_dgrad', _p(dy), _p(w_dgrad), _p(mask_src), _p(out), B, H, W, Cin, Cout, int(accumulate),
              _p(_nt_workspace(nb, dy.device)), nb, _stream())
    return out


def conv3x3_wgrad(x, dy, Ci, relu_in, dw=None, db=None, ws_tag='default'):
    _chk(x, name='x'); _chk(dy, name='dy')
    B, H, W, Cx = x.shape
    Cout = dy.shape[3]
    assert dy.shape[:3] == (B, H, W) and Cx == (4 if Ci == 3 else Ci)
    if dw is None:
        dw = torch.empty(Cout, Ci, 3, 3, dtype=torch.float32, device=x.device)
    if db is None:
        db = torch.empty(Cout, dtype=torch.float32, device=x.device)
    assert dw.is_contiguous() and dw.numel() == Cout * Ci * 9 and db.numel() == Cout
    nb = _lib.load().wesup_conv3x3_wgrad_workspace_bytes(B, H, W, Ci, Cout)
    ws = workspace(nb, x.device, ws_tag)
    _lib.call('wesup_conv3x3_wgrad', _p(x), _p(dy), _p(dw), _p(db), B, H, W, Ci, Cout, int(relu_in), _p(ws), nb, _stream())
    return dw, db


def winograd_positions(m=2):
    """Positions of the F(m x m, 3x3) domain: (m+2)^2 = 16 for m = 2, 36 for m = 4."""
    assert m in (2, 4), m
    return (m + 2) * (m + 2)


def winograd_pack_weight(w, need_fwd=True, need_dgrad=True, u_fwd=None, u_dgrad=None, m=2):
    """w (Cout,Cin,3,3) -> (u_fwd (P,Cout,Cin), u_dgrad (P,Cin,Cout)): G g G^T per channel pair, the second from the
    rotated filter; P = (m+2)^2 positions of F(m x m, 3x3)."""
    _chk(w, name='w')
    Cout, Cin = w.shape[:2]
    P = winograd_positions(m)
    if need_fwd and u_fwd is None:
        u_fwd = torch.empty(P, Cout, Cin, dtype=torch.float32, device=w.device)
    if need_dgrad and u_dgrad is None:
        u_dgrad = torch.empty(P, Cin, Cout, dtype=torch.float32, device=w.device)
    for u, shape in ((u_fwd if need_fwd else None, (P, Cout, Cin)), (u_dgrad if need_dgrad else None, (P, Cin, Cout))):
        if u is not None:
            _chk(u, name='u'); assert u.shape == shape, (u.shape, shape)
    _lib.call('wesup_winograd_pack_weight', _p(w), _p(u_fwd if need_fwd else None),
              _p(u_dgrad if need_dgrad else None), Cout, Cin, m, _stream())
    return u_fwd if need_fwd else None, u_dgrad if need_dgrad else None


def winograd_pack_weights(items):
    """[(w (Cout,Cin,3,3), u_fwd (36,Cout,Cin) or None, u_dgrad (36,Cin,Cout) or None), ...]: the F(4x4,3x3) filters of
    several layers in one launch (at most 32 panels)."""
    n = len(items)
    arr = (_lib.WinoFilter * n)()
    for i, (w, uf, ud) in enumerate(items):
        _chk(w, name='w')
        Cout, Cin = w.shape[:2]
        for u, shape in ((uf, (36, Cout, Cin)), (ud, (36, Cin, Cout))):
            if u is not None:
                _chk(u, name='u'); assert u.shape == shape, (u.shape, shape)
        arr[i].w, arr[i].u_fwd, arr[i].u_dgrad = w.data_ptr(), (uf.data_ptr() if uf is not None else None), (ud.data_ptr() if ud is not None else None)
        arr[i].Cout, arr[i].Cin = Cout, Cin
    _lib.call('wesup_winograd_pack_weights', ctypes.cast(arr, ctypes.c_void_p), n, _stream())


def winograd_tiles(B, H, W, m=2):
    return B * ((H + m - 1) // m) * ((W + m - 1) // m)


def winograd_input_transform(x, relu=False, out=None, m=2):
    """x (B,H,W,C) -> V (P, tiles, C) = B^T d B of every (m+2) x (m+2) input patch."""
    _chk(x, name='x')
    B, H, W, C = x.shape
    T, P = winograd_tiles(B, H, W, m), winograd_positions(m)
    if out is None:
        out = torch.empty(P, T, C, dtype=torch.float32, device=x.device)
    assert out.shape == (P, T, C) and out.is_contiguous()
    _lib.call('wesup_winograd_input_transform', _p(x), _p(out), 0, B, H, W, C, int(relu), m, _stream())
    return out


def winograd_outgrad_transform(dy, out=None, m=2, db=None):
    """dy (B,H,W,C) -> dM (P, tiles, C) = A dY A^T of every m x m output tile.  db (C,), m = 4 only: also the bias gradient
    sum_pixels dy (m = 2 gets it from winograd_filter_grad: position (1,1) of dM)."""
    _chk(dy, name='dy')
    B, H, W, C = dy.shape
    T, P = winograd_tiles(B, H, W, m), winograd_positions(m)
    if out is None:
        out = torch.empty(P, T, C, dtype=torch.float32, device=dy.device)
    assert out.shape == (P, T, C) and out.is_contiguous()
    ws, nb = None, 0
    if db is not None:
        _chk(db, name='db'); assert db.numel() == C and m == 4
        nb = _lib.load().wesup_winograd_outgrad_workspace_bytes(B, H, W, C, m)
        ws = workspace(nb, dy.device, 'wino_outgrad')
    _lib.call('wesup_winograd_outgrad_transform', _p(dy), _p(out), _p(db), B, H, W, C, m, _p(ws), nb, _stream())
    return out


def winograd_output_transform(Mt, B, H, W, bias=None, mask_src=None, out=None, out_relu=None, out_pool=None, pool_relu=False,
                              accumulate=False, m=2):
    """Mt (P, tiles, C) -> y (B,H,W,C) = A^T M A + bias [masked by mask_src > 0] [+ old y]."""
    _chk(Mt, name='Mt')
    C = Mt.shape[2]
    assert Mt.shape == (winograd_positions(m), winograd_tiles(B, H, W, m), C)
    if out is None:
        assert not accumulate
        out = torch.empty(B, H, W, C, dtype=torch.float32, device=Mt.device)
    assert out.shape == (B, H, W, C) and out.is_contiguous()
    for t, shape in ((out_relu, out.shape), (mask_src, out.shape), (out_pool, (B, H // 2, W // 2, C))):
        if t is not None:
            _chk(t, name='operand'); assert t.shape == shape, (t.shape, shape)
    _lib.call('wesup_winograd_output_transform', _p(Mt), 0, _p(bias), _p(mask_src), _p(out), _p(out_relu), _p(out_pool),
              int(pool_relu), B, H, W, C, int(accumulate), m, _stream())
    return out


def winograd_gemm_output_transform(V, U, B, H, W, bias=None, mask_src=None, out=None, out_pool=None, pool_relu=False,
                                   accumulate=False, unpool=None):
    """V (36, tiles, K) x U (36, N, K) -> y (B,H,W,N) = A^T (V_p . U_p^T) A + epilogue, in one kernel (F(4x4,3x3); K = 64 or
    128, N % 64 == 0).  unpool = (src, dst) (B,Hu,Wu,N): the max-pool backward as the epilogue instead of the store."""
    _chk(V, name='V'); _chk(U, name='U')
    P, T, K = V.shape
    N = U.shape[1]
    assert P == 36 and U.shape == (36, N, K) and T == winograd_tiles(B, H, W, 4)
    Hu = Wu = 0
    us = ud = None
    if unpool is not None:
        us, ud = unpool
        _chk(us, name='unpool_src'); _chk(ud, name='unpool_dst')
        _, Hu, Wu, _ = us.shape
        assert us.shape == (B, Hu, Wu, N) == ud.shape and (Hu // 2, Wu // 2) == (H, W) and out is None
    else:
        if out is None:
            assert not accumulate
            out = torch.empty(B, H, W, N, dtype=torch.float32, device=V.device)
        assert out.shape == (B, H, W, N) and out.is_contiguous()
    for t, shape in ((mask_src, (B, H, W, N)), (out_pool, (B, H // 2, W // 2, N))):
        if t is not None:
            _chk(t, name='operand'); assert t.shape == shape, (t.shape, shape)
    _lib.call('wesup_winograd_gemm_output_transform', _p(V), 0, _p(U), _p(bias), _p(mask_src), _p(out), _p(out_pool), int(pool_relu),
              _p(us), _p(ud), Hu, Wu, B, H, W, K, N, int(accumulate), _stream())
    return ud if unpool is not None else out


def gemm_nt_batched(A, Bw, out=None):
    """out[b] = A[b] @ Bw[b]^T for contiguous (nbatch, M, K) x (nbatch, N, K) -> (nbatch, M, N), one launch."""
    _chk(A, name='A'); _chk(Bw, name='B')
    nb, M, K = A.shape
    N = Bw.shape[1]
    assert Bw.shape == (nb, N, K)
    if out is None:
        out = torch.empty(nb, M, N, dtype=torch.float32, device=A.device)
    assert out.shape == (nb, M, N) and out.is_contiguous()
    _lib.call('wesup_gemm_nt_batched', _p(A), K, M * K, _p(Bw), K, N * K, _p(out), N, M * N, nb, M, N, K, _stream())
    return out


def gemm_nt_group(As, Bs, biases, outs):
    """outs[i] = As[i] @ Bs[i]^T + biases[i] for equally shaped 2-D operands that sit at a constant element stride from
    each other (row-strided views allowed: column slices of one buffer, parameters of one flat buffer): ONE launch.
    Returns False -- and launches nothing -- when the operands are not equally spaced; the caller then loops."""
    n = len(As)
    M, K = As[0].shape
    N = Bs[0].shape[0]

    def stride(ts):
        if any(t.shape != ts[0].shape or t.stride() != ts[0].stride() or t.dtype != torch.float32 or not t.is_cuda for t in ts):
            return None
        d = [(ts[i + 1].data_ptr() - ts[i].data_ptr()) for i in range(n - 1)]
        if any(v != d[0] for v in d) or d[0] % 16:
            return None
        return d[0] // 4
    sA, sB, sC = stride(As), stride(Bs), stride(outs)
    sb = 0 if biases is None else stride(biases)
    if n < 2 or None in (sA, sB, sC, sb) or K % 32 or min(sA, sB, sC) < 0:
        return False
    for t in (As[0], Bs[0], outs[0]):
        assert t.dim() == 2 and t.stride(1) == 1
    assert Bs[0].shape == (N, K) and outs[0].shape == (M, N)
    _lib.call('wesup_gemm_nt_batched_bias', _p(As[0]), As[0].stride(0), sA, _p(Bs[0]), Bs[0].stride(0), sB,
              _p(None if biases is None else biases[0]), sb, _p(outs[0]), outs[0].stride(0), sC, n, M, N, K, _stream())
    return True


def winograd_filter_grad(slabs, dw=None, db=None, m=2):
    """slabs (P, S, Cout*Cin + Cout): split-K partial products of the P transformed filter gradients, each followed by
    the column sums of its dM operand -> (dw (Cout,Cin,3,3) = G^T (sum over S) G, db (Cout) from position (1,1): m = 2
    only, pass None for m = 4 -- winograd_outgrad_transform(db=...) has it there).  Cout, Cin are taken from dw."""
    _chk(slabs, name='slabs'); _chk(dw, name='dw')
    Cout, Cin = dw.shape[:2]
    S = slabs.shape[1]
    assert slabs.shape == (winograd_positions(m), S, Cout * Cin + Cout) and slabs.is_contiguous()
    assert dw.shape == (Cout, Cin, 3, 3)
    if db is not None:
        _chk(db, name='db'); assert db.numel() == Cout and m == 2
    _lib.call('wesup_winograd_filter_grad', _p(slabs), slabs.stride(1), slabs.stride(0), S, _p(dw), _p(db), Cout, Cin, m,
              _stream())
    return dw, db


class _NullTimer:
    def begin(self, tag): return None
    def end(self, tok, work): pass


_NULL_TIMER = _NullTimer()


def _winograd_conv(inp, u, m, ws_tag, timer, V=None, v_ready=False, relu_in=False, relu_bits_out=None, after_transform=None,
                   bias=None, mask_src=None, mask_bits=None, out=None, out_relu=None, out_pool=None, pool_relu=False,
                   pool_code_out=None, accumulate=False, unpool=None, gather=None):
    """Every Winograd-domain conv with an epilogue: inp (B,H,W,Cin) x u (P,Cout,Cin) -> the epilogue's destination.  The one
    place that decides the route, splits the workspace, brackets the timer classes and reads DIAG.
    Stage 1, the operand: V (P,tiles,Cin) is handed in transformed (v_ready) or produced by the input transform, into V when
    given (the forward's v_keep), else into the head of the workspace; relu_bits_out: the sign bits of inp ride along.
    after_transform is then called once (the engine queues the previous layer's side branch there).
    Stage 2, the product: ONE kernel for the products and the output transform (short products on a grid that fills the chip),
    or the P batched NT GEMMs into the tail of the workspace and the output transform.
    unpool = (src, code, dst): the max-pool backward as the epilogue, into dst (B,Hu,Wu,Cout), decided by src or by the codes;
    gather = (side, new_row, area_new): the destination's old content replaced by the gathered side gradient.  The compact
    forms (mask_bits, pool_code_out, codes) and the gather exist on the one-kernel route only.
    timer (engine.KernelTimer-like, optional): the transforms and the product are bracketed as classes of their own."""
    B, H, W, Cin = inp.shape
    Cout = u.shape[1]
    lib = _lib.load()
    nb = lib.wesup_conv3x3_winograd_workspace_bytes(B, H, W, Cin, Cout, m)
    if not nb:
        raise _lib.WesupHipError(f'winograd conv: unsupported shape {(B, H, W, Cin, Cout, m)}')
    if timer is None:
        timer = _NULL_TIMER
    T, P = winograd_tiles(B, H, W, m), winograd_positions(m)
    us, ucode, udst = unpool or (None, None, None)
    Hu, Wu = udst.shape[1:3] if unpool else (0, 0)
    side, new_row, area_new = gather or (None, None, None)
    # the route: a caller that hands over a compact form or the gather has chosen the one-kernel route; otherwise the size of
    # the grid decides (wesup_winograd_fused_route).  Level 1 of that route has the forward's epilogues only.
    compact = mask_bits is not None or pool_code_out is not None or ucode is not None
    chosen = compact or gather is not None
    fused = 0 if out_relu is not None else (lib.wesup_winograd_fused_supported(Cin, Cout, m) if chosen
                                            else lib.wesup_winograd_fused_route(Cin, Cout, m, T))
    backward = mask_src is not None or mask_bits is not None or accumulate or unpool is not None or gather is not None
    one_kernel = fused == 2 or (fused == 1 and not backward)
    if chosen and not one_kernel:
        raise _lib.WesupHipError(f'winograd conv {Cin} -> {Cout}: compact masks / pooling codes / the gathered side gradient '
                                 'need the one-kernel product route')
    # the workspace: [V: P T Cin][Mt: P T Cout]; a finished operand on the one-kernel route needs neither part
    if not (v_ready and one_kernel):
        ws = workspace(nb, inp.device, ws_tag)
        if V is None:
            V = ws
    st = _stream()

    # stage 1: the operand
    if not v_ready and 'tin' not in DIAG:
        tok = timer.begin('winograd_transform')
        if relu_bits_out is not None:      # the sign bits of the input ride along (the ReLU mask of the layer below, for its backward)
            _lib.call('wesup_winograd_input_transform_bits', _p(inp), _p(V), 0, _p(relu_bits_out), B, H, W, Cin, int(relu_in), st)
        else:
            _lib.call('wesup_winograd_input_transform', _p(inp), _p(V), 0, B, H, W, Cin, int(relu_in), m, st)
        # bytes: read x, write the P / m^2-fold expansion (4x for m = 2, 2.25x for m = 4)
        timer.end(tok, 4.0 * (B * H * W + P * T) * Cin)
    if after_transform is not None:
        after_transform()

    # stage 2: the product
    tok = timer.begin('winograd_gemm')
    if one_kernel:
        # (three entries to one launcher, csrc/wino_fused.hip: _ex takes every option, the other two are its older subsets)
        if compact or (unpool is not None and v_ready and gather is None):
            pooled = unpool is not None
            _lib.call('wesup_winograd_gemm_output_transform_ex', _p(V), 0, _p(u), _p(bias), _p(mask_src), _p(mask_bits),
                      _p(None if pooled else out), _p(out_pool), int(pool_relu), _p(pool_code_out), _p(us), _p(ucode), _p(udst),
                      Hu, Wu, _p(side), _p(new_row), _p(area_new), side.shape[1] if gather else 0, B, H, W, Cin, Cout,
                      int(accumulate), st)
        elif gather is not None:
            _lib.call('wesup_winograd_gemm_output_transform_gather', _p(V), 0, _p(u), _p(mask_src), _p(udst if unpool else out),
                      _p(us), Hu, Wu, _p(side), _p(new_row), _p(area_new), side.shape[1], B, H, W, Cin, Cout, st)
        else:
            _lib.call('wesup_winograd_gemm_output_transform', _p(V), 0, _p(u), _p(bias), _p(mask_src), _p(out), _p(out_pool),
                      int(pool_relu), _p(us), _p(udst), Hu, Wu, B, H, W, Cin, Cout, int(accumulate), st)
        timer.end(tok, 2.0 * P * T * Cin * Cout)
        return
    Mt = ws[(P * T * Cin * 4 + 255) // 256 * 256:]
    _lib.call('wesup_gemm_nt_batched', _p(V), Cin, T * Cin, _p(u), Cin, Cout * Cin, _p(Mt), Cout, T * Cout, P, T, Cout, Cin, st)
    timer.end(tok, 2.0 * P * T * Cin * Cout)
    if 'tout' in DIAG:
        return
    tok = timer.begin('winograd_transform')
    if unpool is not None:
        _lib.call('wesup_winograd_output_transform_unpool', _p(Mt), 0, _p(bias), _p(mask_src), _p(us), _p(udst), B, H, W, Hu, Wu,
                  Cout, m, st)
        # bytes: the transformed gradient in, the windows of the pre-pool activations, one position of four read and re-written
        timer.end(tok, 4.0 * (P * T + (4 + 2) * B * H * W) * Cout)
    else:
        _lib.call('wesup_winograd_output_transform', _p(Mt), 0, _p(bias), _p(mask_src), _p(out), _p(out_relu), _p(out_pool),
                  int(pool_relu), B, H, W, Cout, int(accumulate), m, st)
        n_io = 1 + (out_relu is not None) + (mask_src is not None) + bool(accumulate) + (0.25 if out_pool is not None else 0)
        timer.end(tok, 4.0 * (P * T + n_io * B * H * W) * Cout)


def conv3x3_fwd_winograd(x, u_fwd, bias, relu_in, out=None, out_relu=None, v_keep=None, ws_tag='default', timer=None,
                         out_pool=None, pool_relu=False, m=2, relu_bits_out=None, pool_code_out=None, after_transform=None):
    """conv3x3_fwd through the Winograd F(m x m, 3x3) domain (deep layers); v_keep (P, tiles, Cin) receives the transformed
    input; out_pool (B, H//2, W//2, Cout) the 2x2 max-pool of the output (ReLU'd if pool_relu), written by the output
    transform."""
    _chk(x, name='x'); _chk(u_fwd, name='u_fwd')
    B, H, W, Cin = x.shape
    Cout = u_fwd.shape[1]
    assert u_fwd.shape == (winograd_positions(m), Cout, Cin)
    if bias is not None:
        _chk(bias, name='bias'); assert bias.numel() == Cout
    if out is None:
        out = torch.empty(B, H, W, Cout, dtype=torch.float32, device=x.device)
    assert out.shape == (B, H, W, Cout) and out.is_contiguous()
    if out_relu is not None:
        _chk(out_relu, name='out_relu'); assert out_relu.shape == out.shape
    if v_keep is not None:
        _chk(v_keep, name='v_keep'); assert v_keep.numel() == winograd_positions(m) * winograd_tiles(B, H, W, m) * Cin
    if out_pool is not None:
        _chk(out_pool, name='out_pool'); assert out_pool.shape == (B, H // 2, W // 2, Cout) and out_pool.is_contiguous()
    # relu_bits_out (B,H,W,Cin/4) uint8: the sign bits of x; pool_code_out (B,H/2,W/2,Cout/4) int16: the pooling's decisions
    # (include/wesup_hip.h: wesup_winograd_input_transform_bits, wesup_winograd_gemm_output_transform_ex)
    if relu_bits_out is not None:
        assert m == 4 and relu_bits_out.dtype == torch.uint8 and relu_bits_out.shape == (B, H, W, Cin // 4) and relu_bits_out.is_contiguous()
    if pool_code_out is not None:
        assert (out_pool is not None and pool_code_out.dtype == torch.int16
                and pool_code_out.shape == (B, H // 2, W // 2, Cout // 4) and pool_code_out.is_contiguous())
    _winograd_conv(x, u_fwd, m, ws_tag, timer, V=v_keep, relu_in=relu_in, relu_bits_out=relu_bits_out,
                   after_transform=after_transform, bias=bias, out=out, out_relu=out_relu, out_pool=out_pool, pool_relu=pool_relu,
                   pool_code_out=pool_code_out)
    return out


def conv3x3_dgrad_winograd(dy, u_dgrad, mask_src=None, out=None, accumulate=False, ws_tag='default', timer=None, m=2,
                           mask_bits=None, v_pre=None):
    _chk(dy, name='dy'); _chk(u_dgrad, name='u_dgrad')
    B, H, W, Cout = dy.shape
    Cin = u_dgrad.shape[1]
    assert u_dgrad.shape == (winograd_positions(m), Cin, Cout)
    if mask_src is not None:
        _chk(mask_src, name='mask_src'); assert mask_src.shape == (B, H, W, Cin)
    if mask_bits is not None:
        assert mask_bits.dtype == torch.uint8 and mask_bits.shape == (B, H, W, Cin // 4) and mask_bits.is_contiguous()
    if out is None:
        assert not accumulate
        out = torch.empty(B, H, W, Cin, dtype=torch.float32, device=dy.device)
    assert out.shape == (B, H, W, Cin) and out.is_contiguous()
    # v_pre (P,tiles,Cout): dy's input transform, done already (winograd_dual_transform): only the products and the way back
    if v_pre is not None:
        _chk(v_pre, name='v_pre'); assert v_pre.shape == (winograd_positions(m), winograd_tiles(B, H, W, m), Cout)
    _winograd_conv(dy, u_dgrad, m, ws_tag, timer, V=v_pre, v_ready=v_pre is not None, mask_src=mask_src, mask_bits=mask_bits,
                   out=out, accumulate=accumulate)
    return out


def conv3x3_dgrad_winograd_unpool(dy, u_dgrad, unpool_src, unpool_dst, ws_tag='default', timer=None, m=4, unpool_code=None,
                                  v_pre=None):
    """Input gradient of a layer that follows a 2x2 max-pool, added straight into the gradient of the PRE-pool activations:
    dy (B,H,W,Cout) at pooled resolution, unpool_src / unpool_dst (B,Hu,Wu,Cin) with H == Hu // 2, W == Wu // 2.  Equals
    conv3x3_dgrad_winograd(out=dxp) followed by maxpool2_bwd(unpool_src, dxp, unpool_dst, accumulate=True).
    unpool_code (B,H,W,Cin/4) int16: the pooling's decisions as codes (conv3x3_fwd_winograd(pool_code_out=...)) instead of a read
    of unpool_src; v_pre (P,tiles,Cout): dy's input transform, done already (winograd_dual_transform)."""
    _chk(dy, name='dy'); _chk(u_dgrad, name='u_dgrad'); _chk(unpool_dst, name='unpool_dst')
    B, H, W, Cout = dy.shape
    Cin = u_dgrad.shape[1]
    assert m == 4 and u_dgrad.shape == (winograd_positions(m), Cin, Cout)
    _, Hu, Wu, _ = unpool_dst.shape
    assert unpool_dst.shape == (B, Hu, Wu, Cin) and (Hu // 2, Wu // 2) == (H, W)
    if unpool_code is not None:
        assert unpool_code.dtype == torch.int16 and unpool_code.shape == (B, H, W, Cin // 4) and unpool_code.is_contiguous()
        unpool_src = None
    else:
        _chk(unpool_src, name='unpool_src'); assert unpool_src.shape == unpool_dst.shape
    if v_pre is not None:
        _chk(v_pre, name='v_pre'); assert v_pre.shape == (winograd_positions(m), winograd_tiles(B, H, W, m), Cout)
    _winograd_conv(dy, u_dgrad, m, ws_tag, timer, V=v_pre, v_ready=v_pre is not None, unpool=(unpool_src, unpool_code, unpool_dst))
    return unpool_dst


def winograd_fused_supported(K, N, m=4, tiles=0):
    """0: the products of this shape go through the batched GEMM + output transform; 1 / 2: through the one-kernel route in the
    forward / in every pass (wesup_winograd_fused_supported).  tiles > 0: ... of a problem of that many tiles (0 when the
    one-kernel route's grid would be too small, wesup_winograd_fused_route)."""
    return int(_lib.load().wesup_winograd_fused_route(K, N, m, int(tiles)))


def conv3x3_dgrad_winograd_gather(dy, u_dgrad, side, new_row, area_new, out, mask_src=None, unpool_src=None,
                                  ws_tag='default', timer=None, mask_bits=None, unpool_code=None, v_pre=None):
    """conv3x3_dgrad_winograd(accumulate=True) / conv3x3_dgrad_winograd_unpool (unpool_src given) with out's old content
    replaced by the gather side[b][new_row[b][pixel]] / area_new[...] (side (B,Kmax,Cin): the commuted side-branch gradient of
    a native-resolution layer): out is written, never read.  m = 4, shapes of the one-kernel product route only."""
    for t, n in ((dy, 'dy'), (u_dgrad, 'u_dgrad'), (side, 'side'), (out, 'out')):
        _chk(t, name=n)
    _chk(new_row, torch.int32, 'new_row')
    if area_new is not None:       # None: the rows of side are divided by their areas already (scale_rows_by_area)
        _chk(area_new, torch.int32, 'area_new')
    B, H, W, Cout = dy.shape
    Cin = u_dgrad.shape[1]
    Kmax = side.shape[1]
    assert u_dgrad.shape == (36, Cin, Cout) and side.shape == (B, Kmax, Cin) and (area_new is None or area_new.shape == (B, Kmax))
    unpool = None
    if unpool_src is not None or unpool_code is not None:
        _, Hu, Wu, _ = out.shape
        assert out.shape == (B, Hu, Wu, Cin) and (Hu // 2, Wu // 2) == (H, W) and Hu % 2 == 0 and Wu % 2 == 0
        assert mask_src is None and mask_bits is None and new_row.shape == (B, Hu * Wu)
        if unpool_code is not None:
            assert unpool_code.dtype == torch.int16 and unpool_code.shape == (B, H, W, Cin // 4) and unpool_code.is_contiguous()
            unpool_src = None
        else:
            _chk(unpool_src, name='unpool_src'); assert unpool_src.shape == out.shape
        unpool = (unpool_src, unpool_code, out)
    else:
        assert out.shape == (B, H, W, Cin) and new_row.shape == (B, H * W)
        if mask_bits is not None:
            assert mask_bits.dtype == torch.uint8 and mask_bits.shape == (B, H, W, Cin // 4) and mask_bits.is_contiguous()
            mask_src = None
        elif mask_src is not None:
            _chk(mask_src, name='mask_src'); assert mask_src.shape == out.shape
    if v_pre is not None:      # dy's input transform, done already (winograd_dual_transform)
        _chk(v_pre, name='v_pre'); assert v_pre.shape == (36, winograd_tiles(B, H, W, 4), Cout)
    _winograd_conv(dy, u_dgrad, 4, ws_tag, timer, V=v_pre, v_ready=v_pre is not None, mask_src=mask_src, mask_bits=mask_bits,
                   out=out, unpool=unpool, gather=(side, new_row, area_new))
    return out


def winograd_bias_rows(B, H, W, C):
    """Rows of per-block column sums the F(4x4) gradient transforms leave for the bias gradient (0: C is not covered)."""
    return int(_lib.load().wesup_winograd_bias_rows(B, H, W, C))


def winograd_dual_transform(dy, V, dM, bias_part=None):
    """One pass over dy (B,H,W,C) for both of its F(4x4) transforms: V (36,tiles,C) = B^T dY B (input of the layer's input
    gradient) and dM (36,tiles,C) = A dY A^T (operand of its weight gradient); bias_part (winograd_bias_rows, C): per-block
    column sums of dy for conv3x3_wgrad_winograd_pre."""
    _chk(dy, name='dy'); _chk(V, name='V'); _chk(dM, name='dM')
    B, H, W, C = dy.shape
    T = winograd_tiles(B, H, W, 4)
    assert V.shape == (36, T, C) == dM.shape
    if bias_part is not None:
        _chk(bias_part, name='bias_part'); assert bias_part.shape == (winograd_bias_rows(B, H, W, C), C) and bias_part.shape[0] > 0
    _lib.call('wesup_winograd_dual_transform', _p(dy), _p(V), _p(dM), _p(bias_part), B, H, W, C, _stream())
    return V, dM


def winograd_dual_transform_unpool(side, dp, code, V, dM, bias_part=None, new_row=None):
    """winograd_dual_transform of dy = side + maxpool2_bwd(dp), with dy never written: dp (B,H/2,W/2,C) the gradient at pooled
    resolution, code (B,H/2,W/2,C/4) int16 the forward's pooling decisions (conv3x3_fwd_winograd(pool_code_out=...)), H and W
    even.  side: the side-branch gradient, dense (B,H,W,C), or with new_row (B,H*W) int32 the rows (B,Kmax,C) it gathers per
    pixel (divided by their areas already: scale_rows_by_area).  Bit for bit what the dual transform makes of the tensor
    conv3x3_dgrad_winograd_unpool / conv3x3_dgrad_winograd_gather(unpool_code=...) leave."""
    _chk(side, name='side'); _chk(dp, name='dp'); _chk(V, name='V'); _chk(dM, name='dM')
    B, Hp, Wp, C = dp.shape
    H, W = 2 * Hp, 2 * Wp
    T = winograd_tiles(B, H, W, 4)
    assert V.shape == (36, T, C) == dM.shape
    assert code.dtype == torch.int16 and code.shape == (B, Hp, Wp, C // 4) and code.is_contiguous()
    Kmax = 0
    if new_row is not None:
        _chk(new_row, torch.int32, 'new_row')
        Kmax = side.shape[1]
        assert side.shape == (B, Kmax, C) and new_row.shape == (B, H * W)
    else:
        assert side.shape == (B, H, W, C)
    if bias_part is not None:
        _chk(bias_part, name='bias_part'); assert bias_part.shape == (winograd_bias_rows(B, H, W, C), C) and bias_part.shape[0] > 0
    _lib.call('wesup_winograd_dual_transform_unpool', _p(side), _p(new_row), Kmax, _p(dp), _p(code), _p(V), _p(dM), _p(bias_part),
              B, H, W, C, _stream())
    return V, dM


def conv3x3_wgrad_winograd_pre(v_pre, dm_pre, bias_part, B, H, W, dw, db=None, ws_tag='default'):
    """The F(4x4) weight gradient from operands that exist: v_pre (36,tiles,Ci) kept by the forward, dm_pre (36,tiles,Cout) and
    bias_part from winograd_dual_transform.  dw (Cout,Ci,3,3); db (Cout) needs bias_part."""
    _chk(v_pre, name='v_pre'); _chk(dm_pre, name='dm_pre'); _chk(dw, name='dw')
    T = winograd_tiles(B, H, W, 4)
    Ci, Cout = v_pre.shape[2], dm_pre.shape[2]
    assert v_pre.shape == (36, T, Ci) and dm_pre.shape == (36, T, Cout) and dw.shape == (Cout, Ci, 3, 3)
    rows = 0
    if db is not None:
        _chk(db, name='db'); _chk(bias_part, name='bias_part')
        rows = bias_part.shape[0]
        assert db.numel() == Cout and bias_part.shape == (winograd_bias_rows(B, H, W, Cout), Cout)
    nb = _lib.load().wesup_conv3x3_wgrad_winograd_workspace_bytes(B, H, W, Ci, Cout, 4)
    ws = workspace(nb, v_pre.device, ws_tag)
    _lib.call('wesup_conv3x3_wgrad_winograd_pre', _p(v_pre), _p(dm_pre), _p(bias_part if db is not None else None), rows, _p(dw),
              _p(db), B, H, W, Ci, Cout, _p(ws), nb, _stream())
    return dw, db


def conv3x3_wgrad_winograd(x, dy, relu_in, dw=None, db=None, ws_tag='default', v_pre=None, m=2):
    """The same (dw, db) as conv3x3_wgrad through the Winograd F(m x m, 3x3) domain: 2.25x (m = 2) / 4x (m = 4) fewer
    multiply-adds, 4x / 2.25x the operand bytes; for the wide layers (Ci, Cout >= 128)."""
    _chk(x, name='x'); _chk(dy, name='dy')
    B, H, W, Ci = x.shape
    Cout = dy.shape[3]
    assert dy.shape[:3] == (B, H, W)
    if dw is None:
        dw = torch.empty(Cout, Ci, 3, 3, dtype=torch.float32, device=x.device)
    if db is None:
        db = torch.empty(Cout, dtype=torch.float32, device=x.device)
    assert dw.is_contiguous() and dw.numel() == Cout * Ci * 9 and db.numel() == Cout
    nb = _lib.load().wesup_conv3x3_wgrad_winograd_workspace_bytes(B, H, W, Ci, Cout, m)
    if not nb:
        raise _lib.WesupHipError(f'conv3x3_wgrad_winograd: unsupported shape {(B, H, W, Ci, Cout, m)}')
    ws = workspace(nb, x.device, ws_tag)
    if v_pre is not None:
        _chk(v_pre, name='v_pre'); assert v_pre.numel() == winograd_positions(m) * winograd_tiles(B, H, W, m) * Ci
    _lib.call('wesup_conv3x3_wgrad_winograd', _p(x), _p(v_pre), _p(dy), _p(dw), _p(db), B, H, W, Ci, Cout, int(relu_in), m,
              _p(ws), nb, _stream())
    return dw, db


# ---------------------------------------------------------------- GEMMs
def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1
    return t.stride(0)


def gemm_nt(A, Bw, bias=None, out=None, mask=None, flags=0, streamk=None):
    """out[M][N] = epi(A[M][K] @ Bw[N][K]^T + bias).  A/out/mask may be row-strided 2-D views.
    streamk: True / False overrides ops.STREAMK for this call."""
    for t, n in ((A, 'A'), (Bw, 'B')):
        if not t.is_cuda or t.dtype != torch.float32:
            raise _lib.WesupHipError(f'{n}: expected float32 CUDA/HIP tensor')
    M, K = A.shape
    N, K2 = Bw.shape
    assert K == K2 and K % 32 == 0, (A.shape, Bw.shape)
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    assert out.shape == (M, N) and out.is_cuda
    ldmask = 0
    if mask is not None:
        assert mask.shape == (M, N) and mask.is_cuda
        ldmask = _ld(mask)
        flags |= MASK
    if bias is not None:
        _chk(bias, name='bias'); assert bias.numel() == N
    nb = _lib.load().wesup_gemm_nt_workspace_bytes(M, N, K) if (STREAMK if streamk is None else streamk) else 0
    _lib.call('wesup_gemm_nt', _p(A), _ld(A), _p(Bw), _ld(Bw), _p(bias), _p(out), _ld(out), _p(mask), ldmask, M, N, K,
              flags, _p(_nt_workspace(nb, A.device)), nb, _stream())
    return out


def gemm_tn(A, Bm, out=None, relu_b=False, ws_tag='default', colsum=None):
    """out[M][N] = A[K][M]^T @ Bm[K][N]  (deterministic split-K); colsum (M,), optional: also sum_k A[k][m]."""
    K, M = A.shape
    K2, N = Bm.shape
    assert K == K2 and A.is_cuda and Bm.is_cuda
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    assert out.shape == (M, N)
    nb = _lib.load().wesup_gemm_tn_workspace_bytes(M, N, K)
    ws = workspace(nb, A.device, ws_tag)      # one workspace per stream that may run concurrently
    if colsum is not None:
        _chk(colsum, name='colsum'); assert colsum.numel() == M
    _lib.call('wesup_gemm_tn', _p(A), _ld(A), _p(Bm), _ld(Bm), _p(out), _ld(out), _p(colsum), M, N, K, int(relu_b),
              _p(ws), nb, _stream())
    return out


def gemm_tn_batched(A, Bm, out, ws_tag='default'):
    """out[b] = A[b]^T @ Bm[b] for 3-D operands (nb,K,M), (nb,K,N) -> (nb,M,N); the last two dims may be row-strided
    views (unit stride along the last), the batch stride is free.  One launch + one reduce for all nb products."""
    nb, K, M = A.shape
    nb2, K2, N = Bm.shape
    assert nb == nb2 and K == K2 and out.shape == (nb, M, N)
    for t in (A, Bm, out):
        assert t.is_cuda and t.dtype == torch.float32 and t.stride(2) == 1
    nbytes = _lib.load().wesup_gemm_tn_batched_workspace_bytes(nb, M, N, K)
    ws = workspace(nbytes, A.device, ws_tag)
    _lib.call('wesup_gemm_tn_batched', _p(A), A.stride(1), A.stride(0), _p(Bm), Bm.stride(1), Bm.stride(0), _p(out),
              out.stride(1), out.stride(0), nb, M, N, K, 0, _p(ws), nbytes, _stream())
    return out


def colsum(A, out=None, ws_tag='colsum'):
    M, N = A.shape
    assert A.is_cuda
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=A.device)
    nb = _lib.load().wesup_colsum_workspace_bytes(M, N)
    ws = workspace(nb, A.device, ws_tag)
    _lib.call('wesup_colsum', _p(A), _ld(A), _p(out), M, N, _p(ws), nb, _stream())
    return out


# ---------------------------------------------------------------- pooling / upsampling
def maxpool2_fwd(y, out=None, relu=False):
    _chk(y, name='y')
    B, H, W, C = y.shape
    if out is None:
        out = torch.empty(B, H // 2, W // 2, C, dtype=torch.float32, device=y.device)
    assert out.shape == (B, H // 2, W // 2, C)
    _lib.call('wesup_maxpool2_fwd', _p(y), _p(out), B, H, W, C, int(relu), _stream())
    return out


def maxpool2_bwd(y, dyp, dy=None, accumulate=False):
    _chk(y, name='y'); _chk(dyp, name='dyp')
    B, H, W, C = y.shape
    assert dyp.shape == (B, H // 2, W // 2, C)
    if dy is None:
        assert not accumulate
        dy = torch.empty_like(y)
    assert dy.shape == y.shape and dy.is_contiguous()
    _lib.call('wesup_maxpool2_bwd', _p(y), _p(dyp), _p(dy), B, H, W, C, int(accumulate), _stream())
    return dy


def upsample_fwd(s, fm, coff):
    _chk(s, name='s'); _chk(fm, name='fm')
    B, h, w, C = s.shape
    B2, H, W, ldf = fm.shape
    assert B == B2 and coff + C <= ldf
    _lib.call('wesup_upsample_fwd', _p(s), _p(fm), B, h, w, H, W, C, ldf, coff, _stream())
    return fm


def upsample_bwd(dfm, coff, h, w, C, out=None):
    _chk(dfm, name='dfm')
    B, H, W, ldf = dfm.shape
    assert coff + C <= ldf
    if out is None:
        out = torch.empty(B, h, w, C, dtype=torch.float32, device=dfm.device)
    assert out.shape == (B, h, w, C)
    _lib.call('wesup_upsample_bwd', _p(dfm), None, None, _p(out), B, h, w, H, W, C, ldf, coff, 0, _stream())
    return out


def upsample_bwd_fused(g, new_row, area_new, H, W, coff, h, w, C, out=None):
    """pool-backward fused in: reads g[B][Kmax][ldf] through new_row instead of a materialised dfm."""
    _chk(g, name='g'); _chk(new_row, torch.int32, 'new_row'); _chk(area_new, torch.int32, 'area_new')
    B, Kmax, ldf = g.shape
    assert new_row.shape == (B, H * W) and area_new.shape == (B, Kmax) and coff + C <= ldf
    if out is None:
        out = torch.empty(B, h, w, C, dtype=torch.float32, device=g.device)
    assert out.shape == (B, h, w, C)
    _lib.call('wesup_upsample_bwd', _p(g), _p(new_row), _p(area_new), _p(out), B, h, w, H, W, C, ldf, coff, Kmax, _stream())
    return out


def upsample_bwd_fused_group(gs, new_row, area_new, H, W, h, w, outs):
    """upsample_bwd_fused for up to three layers of one coarse resolution in one launch: gs[i] (B,Kmax,C_i) dense ->
    outs[i] (B,h,w,C_i).  The window scan per coarse cell is shared by the layers."""
    n = len(gs)
    assert 1 <= n <= 3 and len(outs) == n and (h, w) != (H, W)
    B, Kmax = gs[0].shape[:2]
    _chk(new_row, torch.int32, 'new_row'); _chk(area_new, torch.int32, 'area_new')
    assert new_row.shape == (B, H * W) and area_new.shape == (B, Kmax)
    for g, o in zip(gs, outs):
        _chk(g, name='g'); _chk(o, name='out')
        assert g.is_contiguous() and o.is_contiguous() and g.shape[:2] == (B, Kmax) and o.shape == (B, h, w, g.shape[2])
    assert sum(g.shape[2] for g in gs) <= 768
    pg = [_p(g) for g in gs] + [_p(None)] * (3 - n)
    po = [_p(o) for o in outs] + [_p(None)] * (3 - n)
    cs = [g.shape[2] for g in gs] + [0] * (3 - n)
    _lib.call('wesup_upsample_bwd_group', *pg, *po, *cs, n, _p(new_row), _p(area_new), B, h, w, H, W, Kmax, _stream())
    return outs


# ---------------------------------------------------------------- superpixels
class SuperpixelMeta:
    """Device-side result of wesup_sp_preprocess for a batch of label maps (padded to Kmax rows per image)."""
    __slots__ = ('B', 'H', 'W', 'C', 'Kmax', 'labels', 'mask', 'n_sp', 'n_l', 'perm', 'inv_perm', 'area_new',
                 'sp_labels', 'new_row', 'row_start', 'pix_sorted', 'status', 'n_sp_host', 'seg_start', 'unit_row',
                 'Umax', 'counts', 'tiles')

    def check(self):
        """Host sync: raise on label-map errors the reference would turn into NaNs (models/wesup.py:57-61)."""
        st = self.status.cpu()
        if int(st.max()) != 0:
            bad = [(b, int(v)) for b, v in enumerate(st.tolist()) if v]
            raise ValueError(f'invalid label map (image, code): {bad}; 1 = id >= Kmax, 2 = empty id below the '
                             'maximum id (ids must be contiguous 0..K-1)')


def sp_preprocess(labels, mask, Kmax, n_classes=2, n_sp_host=None, into=None, counts=None):
    """labels (B,H,W) int32; mask (B,C,H,W) uint8 or None.  ``into``: a SuperpixelMeta of the same (B,H,W,C,Kmax) whose
    buffers are written again (a recorded step plan needs every buffer at a fixed address); ``counts``: an int32 (3,B) tensor
    that receives n_sp | n_l | status (the runner's read-back block)."""
    _chk(labels, torch.int32, 'labels')
    B, H, W = labels.shape
    HW = H * W
    dev = labels.device
    C = n_classes
    Kmax = int(Kmax)
    if mask is not None:
        _chk(mask, torch.uint8, 'mask')
        assert mask.shape == (B, C, H, W)
    m = into
    if m is None or (m.B, m.H, m.W, m.C, m.Kmax) != (B, H, W, C, Kmax) or m.n_sp.device != dev:
        m = SuperpixelMeta()
        m.B, m.H, m.W, m.C, m.Kmax = B, H, W, C, Kmax
        i32 = dict(dtype=torch.int32, device=dev)
        # n_sp | n_l | status side by side: the trainer reads the three back with one copy
        if counts is not None:
            assert counts.shape == (3, B) and counts.dtype == torch.int32 and counts.is_contiguous()
        m.counts = counts if counts is not None else torch.empty(3, B, **i32)
        m.n_sp, m.n_l, m.status = m.counts[0], m.counts[1], m.counts[2]
        m.perm = torch.empty(B, Kmax, **i32); m.inv_perm = torch.empty(B, Kmax, **i32)
        m.area_new = torch.empty(B, Kmax, **i32)
        m.sp_labels = torch.empty(B, Kmax, C, dtype=torch.float32, device=dev)
        m.new_row = torch.empty(B, HW, **i32); m.row_start = torch.empty(B, Kmax + 1, **i32)
        m.pix_sorted = torch.empty(B, HW, **i32)
        # segment table (rows cut into <= 512-pixel segments) for the load-balanced pooling kernels
        m.Umax = _lib.load().wesup_sp_max_units(HW, Kmax)
        m.seg_start = torch.empty(B, Kmax + 1, **i32)
        m.unit_row = torch.empty(B, m.Umax, **i32)
        m.tiles = None
    m.labels, m.mask, m.n_sp_host = labels, mask, n_sp_host
    nb = _lib.load().wesup_sp_preprocess_workspace_bytes(B, HW, C, Kmax)
    ws = workspace(nb, dev, 'sp')
    tok = _tbegin('sp_preprocess')
    _lib.call('wesup_sp_preprocess', _p(labels), _p(mask), B, HW, C, Kmax, _p(m.n_sp), _p(m.n_l), _p(m.perm),
              _p(m.inv_perm), _p(m.area_new), _p(m.sp_labels), _p(m.new_row), _p(m.row_start), _p(m.pix_sorted),
              _p(m.status), _p(m.seg_start), _p(m.unit_row), m.Umax, _p(ws), nb, _stream())
    # algorithmic bytes: the label map and the mask in, the row of every pixel and the row-sorted pixel list out
    _tend(tok, float(B) * HW * (4 + (C if mask is not None else 0) + 4 + 4))
    return m


def spmaps_to_labels(sp_maps):
    _chk(sp_maps, name='sp_maps')
    N, H, W = sp_maps.shape
    labels = torch.empty(1, H, W, dtype=torch.int32, device=sp_maps.device)
    _lib.call('wesup_spmaps_to_labels', _p(sp_maps), _p(labels), N, H * W, _stream())
    return labels


def sp_pool_fwd(fm, meta, C=None, out=None):
    _chk(fm, name='fm')
    B, H, W, ldf = fm.shape
    C = ldf if C is None else C
    assert (B, H, W) == (meta.B, meta.H, meta.W)
    if out is None:
        out = torch.empty(B, meta.Kmax, C, dtype=torch.float32, device=fm.device)
    assert out.shape == (B, meta.Kmax, C) and out.is_contiguous()
    nb = _lib.load().wesup_sp_pool_workspace_bytes(B, meta.Umax, C)
    ws = workspace(nb, fm.device, 'pool')
    _lib.call('wesup_sp_pool_fwd', _p(fm), _p(meta.pix_sorted), _p(meta.row_start), _p(meta.seg_start), _p(meta.unit_row),
              _p(out), B, H * W, ldf, C, meta.Kmax, meta.Umax, _p(ws), nb, _stream())
    return out


def sp_pool_upsample_fwd(s, meta, out, coff):
    """Fused upsample + scatter-mean of one side output s (B,h,w,C) into out[..., coff:coff+C] (out: (B,Kmax,ldo))."""
    _chk(s, name='s'); _chk(out, name='out')
    B, h, w, C = s.shape
    assert out.shape[:2] == (B, meta.Kmax) and B == meta.B and coff + C <= out.shape[2]
    nb = _lib.load().wesup_sp_pool_workspace_bytes(B, meta.Umax, C)
    ws = workspace(nb, s.device, 'pool_up')
    _lib.call('wesup_sp_pool_upsample_fwd', _p(s), _p(meta.pix_sorted), _p(meta.row_start), _p(meta.seg_start),
              _p(meta.unit_row), _p(out), B, h, w, meta.H, meta.W, C, out.shape[2], coff, meta.Kmax, meta.Umax, _p(ws), nb,
              _stream())
    return out


def sp_interp_matrix(meta, h, w, out=None):
    """Wm (B,Kmax,h*w): upsample-to-(H,W)-then-average-over-superpixel as a matrix over the coarse cells."""
    B, Kmax = meta.B, meta.Kmax
    assert 0 < h <= meta.H and 0 < w <= meta.W and h * w <= 8192
    if out is None:
        out = torch.empty(B, Kmax, h * w, dtype=torch.float32, device=meta.pix_sorted.device)
    _chk(out, name='out')
    assert out.shape == (B, Kmax, h * w)
    _lib.call('wesup_sp_interp_matrix', _p(meta.pix_sorted), _p(meta.row_start), _p(out), B, meta.H, meta.W, h, w, Kmax,
              _stream())
    return out


def sp_pool_mat_sparse(Kmax, hw):
    """True where the products of a (Kmax, hw) interpolation-pooling matrix walk its non-zeros, False where they are the dense
    batched GEMMs (the size rule of csrc/pool_mat_route.hpp; WESUP_POOL_MAT_SPARSE_MIN moves it, read at every call)."""
    return bool(_lib.load().wesup_sp_pool_mat_route(Kmax, hw))


def _pool_mat_args(Wm, WmT, x, sp, off):
    B, Kmax, hw = Wm.shape
    C = x.shape[2]
    for t, n in ((Wm, 'Wm'), (WmT, 'WmT'), (x, 's / ds'), (sp, 'sp')):
        _chk(t, name=n)
    assert WmT.shape == (B, hw, Kmax) and x.shape == (B, hw, C) and sp.dim() == 3 and sp.shape[:2] == (B, Kmax)
    return B, Kmax, hw, C, sp.shape[2]


def sp_pool_mat_fwd(Wm, WmT, s, sp, off, ws_tag='default'):
    """sp[:, :, off:off + C] = Wm . s per image: Wm (B,Kmax,hw), WmT its transpose (B,hw,Kmax), s (B,hw,C), sp (B,Kmax,ld).
    Dense (gemm_tn_batched on WmT, bit for bit) below the size rule, by Wm's non-zeros in ascending cell order above it."""
    B, Kmax, hw, C, ld = _pool_mat_args(Wm, WmT, s, sp, off)
    ws, nbytes = None, 0
    if not sp_pool_mat_sparse(Kmax, hw):
        nbytes = _lib.load().wesup_gemm_tn_batched_workspace_bytes(B, Kmax, C, hw)
        ws = workspace(nbytes, Wm.device, ws_tag)
    _lib.call('wesup_sp_pool_mat_fwd', _p(Wm), _p(WmT), _p(s), _p(sp), ld, off, B, Kmax, hw, C, _p(ws), nbytes, _stream())
    return sp


def sp_pool_mat_bwd(Wm, WmT, gsp, off, ds, ws_tag='default'):
    """ds = Wm^T . gsp[:, :, off:off + C] per image: gsp (B,Kmax,ld), ds (B,hw,C).  The two routes of sp_pool_mat_fwd."""
    B, Kmax, hw, C, ld = _pool_mat_args(Wm, WmT, ds, gsp, off)
    ws, nbytes = None, 0
    if not sp_pool_mat_sparse(Kmax, hw):
        nbytes = _lib.load().wesup_gemm_tn_batched_workspace_bytes(B, hw, C, Kmax)
        ws = workspace(nbytes, Wm.device, ws_tag)
    _lib.call('wesup_sp_pool_mat_bwd', _p(Wm), _p(WmT), _p(gsp), ld, off, _p(ds), B, Kmax, hw, C, _p(ws), nbytes, _stream())
    return ds


def sp_pool_bwd(g, meta, out=None):
    _chk(g, name='g')
    B, Kmax, C = g.shape
    assert B == meta.B and Kmax == meta.Kmax
    if out is None:
        out = torch.empty(B, meta.H, meta.W, C, dtype=torch.float32, device=g.device)
    assert out.shape == (B, meta.H, meta.W, C) and out.is_contiguous()
    _lib.call('wesup_sp_pool_bwd', _p(g), _p(meta.new_row), _p(meta.area_new), _p(out), B, meta.H * meta.W, C, C, Kmax,
              _stream())
    return out


def paint_fwd(sp_pred, meta, cls=1, out=None):
    _chk(sp_pred, name='sp_pred')
    B, Kmax, C = sp_pred.shape
    assert B == meta.B and Kmax == meta.Kmax
    if out is None:
        out = torch.empty(B, meta.H, meta.W, dtype=torch.float32, device=sp_pred.device)
    tok = _tbegin('paint')
    _lib.call('wesup_paint_fwd', _p(sp_pred), _p(meta.new_row), _p(out), B, meta.H * meta.W, Kmax, C, cls, _stream())
    _tend(tok, 8.0 * B * meta.H * meta.W + 4.0 * B * Kmax * C)
    return out


def paint_argmax(sp_pred, meta, out=None):
    """Class-map paint-back for more than two classes: out (B,H,W) f32 = the index of each pixel's superpixel's largest probability
    (first maximum), wesup_paint_argmax."""
    _chk(sp_pred, name='sp_pred')
    B, Kmax, C = sp_pred.shape
    assert B == meta.B and Kmax == meta.Kmax
    if out is None:
        out = torch.empty(B, meta.H, meta.W, dtype=torch.float32, device=sp_pred.device)
    nb = _lib.load().wesup_paint_argmax_workspace_bytes(B, Kmax)
    ws = workspace(nb, sp_pred.device, 'argmax')
    tok = _tbegin('paint')
    _lib.call('wesup_paint_argmax', _p(sp_pred), _p(meta.new_row), _p(out), B, meta.H * meta.W, Kmax, C, _p(ws), nb, _stream())
    _tend(tok, 8.0 * B * meta.H * meta.W + 4.0 * B * Kmax * (C + 2))
    return out


def paint(sp_pred, meta, out=None):
    """What the model's forward returns per pixel: the class-1 probability for two classes, the class map (as floats) for more."""
    return paint_fwd(sp_pred, meta, 1, out=out) if sp_pred.shape[2] == 2 else paint_argmax(sp_pred, meta, out=out)


# ---------------------------------------------------------------- SLIC
def slic(img, n_segments, compactness=40.0, max_iter=10, enforce_connectivity=True, min_size_factor=0.5):
    """GPU SLIC: img (B,3,H,W) RGB in [0,1] -> (labels (B,H,W) int32 with contiguous ids, n_labels (B,) int32)."""
    _chk(img, name='img')
    B, C, H, W = img.shape
    assert C == 3
    labels = torch.empty(B, H, W, dtype=torch.int32, device=img.device)
    n_labels = torch.empty(B, dtype=torch.int32, device=img.device)
    nb = _lib.load().wesup_slic_workspace_bytes(B, H, W, int(n_segments))
    ws = workspace(nb, img.device, 'slic')
    _lib.call('wesup_slic', _p(img), _p(labels), _p(n_labels), B, H, W, int(n_segments), float(compactness), int(max_iter),
              int(enforce_connectivity), float(min_size_factor), _p(ws), nb, _stream())
    return labels, n_labels


# ---------------------------------------------------------------- head / loss / optimiser
MAX_CLASSES = _lib.MAX_CLASSES       # WESUP_MAX_CLASSES: the *_c entries take 2 <= C <= MAX_CLASSES
HEAD_MAX_D = _lib.HEAD_MAX_D         # WESUP_HEAD_MAX_D: propagate / head_fwd take 1 <= D <= HEAD_MAX_D


def classifier_fwd(feat, Wc, bc, out=None):
    """softmax(feat . Wc^T + bc): (R, D) -> (R, C), C = Wc.shape[0] (wesup_classifier_fwd_c: D <= 512)."""
    _chk(feat, name='feat'); _chk(Wc, name='Wc'); _chk(bc, name='bc')
    R, D = feat.shape
    C = Wc.shape[0]
    assert Wc.shape == (C, D) and bc.numel() == C
    if out is None:
        out = torch.empty(R, C, dtype=torch.float32, device=feat.device)
    assert out.numel() == R * C
    _lib.call('wesup_classifier_fwd_c', _p(feat), _p(Wc), _p(bc), _p(out), R, D, C, _stream())
    return out


def classifier_bwd_bytes(R, D, C=2):
    """Bytes of the classifier's per-64-row partial sums of dWc / dbc."""
    return _lib.load().wesup_classifier_bwd_c_workspace_bytes(R, D, C)


def classifier_bwd(feat, Wc, pred, dpred, dfeat_extra=None, dfeat=None, dWc=None, dbc=None):
    """Backward of classifier_fwd; C = Wc.shape[0] (wesup_classifier_bwd_c)."""
    _chk(feat, name='feat'); _chk(pred, name='pred'); _chk(dpred, name='dpred')
    R, D = feat.shape
    C = Wc.shape[0]
    assert pred.shape == (R, C) and dpred.shape == (R, C)
    if dfeat_extra is not None:
        _chk(dfeat_extra, name='dfeat_extra'); assert dfeat_extra.shape == (R, D)
    dev = feat.device
    dfeat = torch.empty(R, D, dtype=torch.float32, device=dev) if dfeat is None else dfeat
    dWc = torch.empty(C, D, dtype=torch.float32, device=dev) if dWc is None else dWc
    dbc = torch.empty(C, dtype=torch.float32, device=dev) if dbc is None else dbc
    nb = classifier_bwd_bytes(R, D, C)
    ws = workspace(nb, dev, 'cls')
    _lib.call('wesup_classifier_bwd_c', _p(feat), _p(Wc), _p(pred), _p(dpred), _p(dfeat_extra), _p(dfeat), _p(dWc), _p(dbc),
              R, D, C, _p(ws), nb, _stream())
    return dfeat, dWc, dbc


def propagate(feat, meta, threshold, enable=True, out=None):
    """feat (B,Kmax,D).  Returns y_all (B,Kmax,C), src_idx (B,Kmax) int32, max_sim (B,Kmax) (``out``: the three, reused)."""
    _chk(feat, name='feat')
    B, Kmax, D = feat.shape
    assert B == meta.B and Kmax == meta.Kmax
    dev = feat.device
    if out is not None:
        y_all, src, sim = out
        assert y_all.shape == (B, Kmax, meta.C) and src.shape == (B, Kmax) == sim.shape and src.dtype == torch.int32
    else:
        y_all = torch.empty(B, Kmax, meta.C, dtype=torch.float32, device=dev)
        src = torch.empty(B, Kmax, dtype=torch.int32, device=dev)
        sim = torch.empty(B, Kmax, dtype=torch.float32, device=dev)
    tok = _tbegin('propagate')
    _lib.call('wesup_propagate', _p(feat), _p(meta.sp_labels), _p(meta.n_sp), _p(meta.n_l), float(threshold), int(enable),
              _p(y_all), _p(src), _p(sim), B, Kmax, D, meta.C, _stream())
    _tend(tok, 4.0 * B * Kmax * (D + 2 * meta.C + 2))
    return y_all, src, sim


def loss_fwd(pred, y_all, meta, eps, prop_weight, out=None):
    _chk(pred, name='pred'); _chk(y_all, name='y_all')
    B, Kmax, C = pred.shape
    assert y_all.shape == (B, Kmax, C) and B == meta.B and Kmax == meta.Kmax
    if out is not None:
        loss, terms = out                  # (loss None: only the per-image terms; the caller forms their mean)
        assert (loss is None or loss.numel() == 1) and terms.shape == (B, 8) and terms.is_contiguous()
    else:
        terms = torch.empty(B, 8, dtype=torch.float32, device=pred.device)
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    _lib.call('wesup_loss_fwd', _p(pred), _p(y_all), _p(meta.n_sp), _p(meta.n_l), float(eps), float(prop_weight),
              _p(terms), _p(loss), B, Kmax, C, _stream())
    return loss, terms


def loss_bwd(pred, y_all, meta, terms, dloss, eps, prop_weight, out=None):
    _chk(dloss, name='dloss')
    B, Kmax, C = pred.shape
    if out is None:
        out = torch.empty_like(pred)
    _lib.call('wesup_loss_bwd', _p(pred), _p(y_all), _p(meta.n_sp), _p(meta.n_l), _p(terms), _p(dloss), float(eps),
              float(prop_weight), _p(out), B, Kmax, C, _stream())
    return out


def head_fwd(feat, Wc, bc, pred, meta, threshold, enable=True, out=None):
    """classifier_fwd + propagate in one launch (wesup_head_fwd_c): feat (B,Kmax,D) ->
    pred (B*Kmax,C) and (y_all, src_idx, max_sim)."""
    _chk(feat, name='feat'); _chk(Wc, name='Wc'); _chk(bc, name='bc'); _chk(pred, name='pred')
    B, Kmax, D = feat.shape
    C = Wc.shape[0]
    assert B == meta.B and Kmax == meta.Kmax and Wc.shape == (C, D) and bc.numel() == C and pred.numel() == B * Kmax * C
    assert C == meta.C, 'the classifier and the label masks disagree about the number of classes'
    y_all, src, sim = out
    assert y_all.shape == (B, Kmax, meta.C) and src.shape == (B, Kmax) == sim.shape and src.dtype == torch.int32
    tok = _tbegin('propagate')
    _lib.call('wesup_head_fwd_c', _p(feat), _p(Wc), _p(bc), _p(pred), _p(meta.sp_labels), _p(meta.n_sp), _p(meta.n_l),
              float(threshold), int(enable), _p(y_all), _p(src), _p(sim), B, Kmax, D, meta.C, _stream())
    _tend(tok, 4.0 * B * Kmax * (D + 2 * meta.C + 2))
    return y_all, src, sim


def head_supported(Kmax, C):
    """The fused head launches (wesup_head_fwd_c / wesup_head_bwd_c)."""
    return Kmax % 64 == 0 and 2 <= C <= MAX_CLASSES


def head_bwd_partials(R, D, device, C=2):
    """The buffer wesup_head_bwd_c leaves the partial sums of dWc / dbc in and wesup_classifier_bwd_c_finish reads (on another stream,
    launches later): owned by the caller -- the engine keeps one per buffer set -- never a shared grow-only workspace, which another
    tag's growth may replace between the two calls."""
    return torch.empty(max(int(classifier_bwd_bytes(R, D, C)), 256), dtype=torch.uint8, device=device)


def head_bwd(feat, Wc, pred, y_all, meta, dloss, eps, prop_weight, terms, dpred, dfeat, partials):
    """loss_fwd (terms) + loss_bwd (dpred) + the first kernel of classifier_bwd (dfeat, partial sums of dWc / dbc into ``partials``,
    see head_bwd_partials) in one launch (wesup_head_bwd_c); classifier_bwd_finish adds the partial sums up."""
    _chk(feat, name='feat'); _chk(pred, name='pred'); _chk(y_all, name='y_all'); _chk(dloss, name='dloss')
    _chk(partials, torch.uint8, 'partials')
    B, Kmax, C = y_all.shape
    R, D = feat.shape
    assert R == B * Kmax and pred.numel() == R * C and dpred.numel() == R * C and dfeat.shape == (R, D) and terms.shape == (B, 8)
    assert Wc.shape == (C, D) and head_supported(Kmax, C) and B == meta.B and Kmax == meta.Kmax
    nb = classifier_bwd_bytes(R, D, C)
    assert partials.numel() >= nb
    _lib.call('wesup_head_bwd_c', _p(feat), _p(Wc), _p(pred), _p(y_all), _p(meta.n_sp), _p(meta.n_l), _p(dloss), float(eps),
              float(prop_weight), _p(terms), _p(dpred), _p(dfeat), B, Kmax, D, C, _p(partials), nb, _stream())


def classifier_bwd_finish(partials, R, D, dWc, dbc):
    _chk(partials, torch.uint8, 'partials')
    C = dWc.shape[0]
    nb = classifier_bwd_bytes(R, D, C)
    assert partials.numel() >= nb and dWc.shape == (C, D) and dbc.numel() == C
    _lib.call('wesup_classifier_bwd_c_finish', _p(partials), nb, _p(dWc), _p(dbc), R, D, C, _stream())


def cross_entropy_fwd(y_hat, y_true, eps, class_weights=None):
    _chk(y_hat, name='y_hat'); _chk(y_true, name='y_true')
    n, C = y_hat.shape
    assert y_true.shape == (n, C)
    if class_weights is not None:
        _chk(class_weights, name='class_weights'); assert class_weights.numel() == C
    out2 = torch.empty(4, dtype=torch.float32, device=y_hat.device)
    _lib.call('wesup_cross_entropy_fwd', _p(y_hat), _p(y_true), _p(class_weights), float(eps), _p(out2), n, C, _stream())
    return out2


def cross_entropy_bwd(y_hat, y_true, out2, dloss, eps, class_weights=None):
    n, C = y_hat.shape
    dy = torch.empty_like(y_hat)
    if n > 0:
        _lib.call('wesup_cross_entropy_bwd', _p(y_hat), _p(y_true), _p(class_weights), _p(out2), _p(dloss), float(eps),
                  _p(dy), n, C, _stream())
    return dy


def sgd_step(p, g, v, lr, momentum, weight_decay, grad_scale, first_step):
    for t, n in ((p, 'p'), (g, 'g'), (v, 'v')):
        _chk(t, name=n)
    assert p.numel() == g.numel() == v.numel()
    tok = _tbegin('sgd')
    _lib.call('wesup_sgd_step', _p(p), _p(g), _p(v), p.numel(), float(lr), float(momentum), float(weight_decay),
              float(grad_scale), int(first_step), _stream())
    _tend(tok, 20.0 * p.numel())                     # read p, g, v; write p, v


ADAM_STATE_BYTES = 32        # AdamState of csrc/optim.hip: { double lr; int32 t; float step_size, inv_sqrt_bc2, decay; 8 unused }


def adam_state(lr, device, t=0):
    """A schedule block for adam_tick / adam_step on ``device``: lr as the double it is, the count t, the factors unset (the first
    tick forms them)."""
    raw = struct.pack('<di', float(lr), int(t)) + bytes(ADAM_STATE_BYTES - 12)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device, copy=True)


def adam_state_read(state):
    """The block's fields on the host (waits for the device)."""
    lr, t, step_size, inv_sqrt_bc2, decay = struct.unpack('<di3f', state.cpu().numpy().tobytes()[:24])
    return {'lr': lr, 't': t, 'step_size': step_size, 'inv_sqrt_bc2': inv_sqrt_bc2, 'decay': decay}


def _chk_adam_state(state):
    _chk(state, torch.uint8, 'state')
    if state.numel() != ADAM_STATE_BYTES:
        raise _lib.WesupHipError(f'state: expected {ADAM_STATE_BYTES} bytes, got {state.numel()}')


def adam_tick(state, betas, weight_decay):
    """t += 1 in the optimiser's device block and the three factors of that step from t and the block's lr.  ``betas`` are the
    host's doubles: their complements are formed here, in double, and rounded to float once."""
    _chk_adam_state(state)
    tok = _tbegin('sgd')
    _lib.call('wesup_adam_tick', _p(state), 1.0 - float(betas[0]), 1.0 - float(betas[1]), float(weight_decay), _stream())
    _tend(tok, 2.0 * ADAM_STATE_BYTES)


def adam_step(p, g, m, v, state, betas, eps, weight_decay, grad_scale, decoupled):
    """One Adam (decoupled: AdamW) update of p, m, v from g with the factors the last adam_tick left in ``state``."""
    for t, n in ((p, 'p'), (g, 'g'), (m, 'm'), (v, 'v')):
        _chk(t, name=n)
    _chk_adam_state(state)
    assert p.numel() == g.numel() == m.numel() == v.numel()
    b1, b2 = float(betas[0]), float(betas[1])
    tok = _tbegin('sgd')
    _lib.call('wesup_adam_step', _p(p), _p(g), _p(m), _p(v), p.numel(), _p(state), b1, 1.0 - b1, b2, 1.0 - b2, float(eps),
              float(weight_decay), float(grad_scale), int(bool(decoupled)), _stream())
    _tend(tok, 28.0 * p.numel())                     # read p, g, m, v; write p, m, v


def seg_metrics(pred, mask, out=None):
    """pred (B,H,W) f32, mask (B,C,H,W) uint8 -> (B,4) sums {#(P==G), sum(P*G), sum(P), sum(G)}."""
    _chk(pred, name='pred'); _chk(mask, torch.uint8, 'mask')
    B, H, W = pred.shape
    C = mask.shape[1]
    if out is None:
        out = torch.empty(B, 4, dtype=torch.float32, device=pred.device)
    assert out.shape == (B, 4) and out.is_contiguous()
    nb = _lib.load().wesup_seg_metrics_workspace_bytes(B)
    ws = workspace(nb, pred.device, 'seg')
    _lib.call('wesup_seg_metrics', _p(pred), _p(mask), _p(out), B, H * W, C, _p(ws), nb, _stream())
    return out


def seg_confusion(pred, mask, out=None, status=None):
    """pred (B,H,W) f32 class indices, mask (B,C,H,W) uint8 -> (conf (B,C,C) int32, status (1,) int32): conf[b][g][p] = pixels of
    ground-truth class g (first maximum over the mask's planes) predicted as p; status != 0: a predicted value outside [0, C).
    Both are zeroed by the entry."""
    _chk(pred, name='pred'); _chk(mask, torch.uint8, 'mask')
    B, H, W = pred.shape
    C = mask.shape[1]
    assert mask.shape == (B, C, H, W)
    if out is None:
        out = torch.empty(B, C, C, dtype=torch.int32, device=pred.device)
    if status is None:
        status = torch.empty(1, dtype=torch.int32, device=pred.device)
    _chk(out, torch.int32, 'conf'); _chk(status, torch.int32, 'status')
    assert out.numel() == B * C * C and status.numel() == 1
    _lib.call('wesup_seg_confusion', _p(pred), _p(mask), _p(out), _p(status), B, H * W, C, _stream())
    return out, status


# ---------------------------------------------------------------- mask post-processing and challenge scoring (csrc/regions.hip)
MORPH_ERODE, MORPH_DILATE, MORPH_OPEN = 0, 1, 2
CONTINGENCY_MAX_CELLS = 1 << 26      # above this a table is not allocated: the caller scores that image on the host
LABEL_SORT_MAX_LABELS = 16384        # labels 0 .. L with L below this (the placement kernel's cursor table in LDS)


def _mask3(mask, name='mask'):
    """(H,W) or (B,H,W) uint8 -> (B,H,W), and whether a batch axis was added."""
    _chk(mask, torch.uint8, name)
    if mask.dim() not in (2, 3):
        raise _lib.WesupHipError(f'{name}: expected (H,W) or (B,H,W), got {tuple(mask.shape)}')
    return (mask.unsqueeze(0), True) if mask.dim() == 2 else (mask, False)


def cc_label(mask, connectivity=8, value=1):
    """Connected components of the pixels where ``(mask != 0) == value``: mask (H,W) / (B,H,W) uint8 -> (labels int32 of the
    same shape, 0 elsewhere and 1..n in raster order of the first pixel like scipy.ndimage.label; n_labels (B,) int32)."""
    m, squeeze = _mask3(mask)
    B, H, W = m.shape
    if connectivity not in (4, 8):
        raise _lib.WesupHipError(f'cc_label: connectivity {connectivity} (4 or 8)')
    labels = torch.empty(B, H, W, dtype=torch.int32, device=m.device)
    n_labels = torch.empty(B, dtype=torch.int32, device=m.device)
    nb = _lib.load().wesup_cc_label_workspace_bytes(B, H, W)
    ws = workspace(nb, m.device, 'regions')
    _lib.call('wesup_cc_label', _p(m), _p(labels), _p(n_labels), B, H, W, int(connectivity), int(bool(value)), _p(ws), nb,
              _stream())
    return (labels[0] if squeeze else labels), n_labels


def remove_small_regions(mask, min_size=2000):
    """Both passes of evaluate.remove_small_regions on the device: mask (H,W) / (B,H,W) uint8 -> {0,1} uint8 of the same shape."""
    m, squeeze = _mask3(mask)
    B, H, W = m.shape
    out = torch.empty_like(m)
    nb = _lib.load().wesup_remove_small_regions_workspace_bytes(B, H, W)
    ws = workspace(nb, m.device, 'regions')
    _lib.call('wesup_remove_small_regions', _p(m), _p(out), B, H, W, int(min_size), _p(ws), nb, _stream())
    return out[0] if squeeze else out


def binary_morph(mask, footprint, op=MORPH_OPEN):
    """Erosion / dilation / opening of a {0,1} uint8 map (H,W) / (B,H,W) with scipy.ndimage's conventions (footprint origin at
    size // 2, dilation with the mirrored footprint, border mode 'reflect'); footprint: a 2-D array or tensor, non-zero = set."""
    m, squeeze = _mask3(mask)
    B, H, W = m.shape
    fp = torch.as_tensor(footprint)
    if fp.dim() != 2 or fp.numel() == 0 or fp.numel() > 1024 or max(fp.shape) > 255:
        raise _lib.WesupHipError(f'binary_morph: footprint {tuple(fp.shape)} (2-D, 1 .. 1024 cells)')
    if op not in (MORPH_ERODE, MORPH_DILATE, MORPH_OPEN):
        raise _lib.WesupHipError(f'binary_morph: op {op}')
    fp = (fp != 0).to(torch.uint8).to(m.device).contiguous()
    out = torch.empty_like(m)
    nb = _lib.load().wesup_binary_morph_workspace_bytes(B, H, W, int(op))
    ws = workspace(nb, m.device, 'regions')
    _lib.call('wesup_binary_morph', _p(m), _p(out), _p(fp), B, H, W, fp.shape[0], fp.shape[1], int(op), _p(ws), nb, _stream())
    return out[0] if squeeze else out


def binary_opening(mask, footprint):
    return binary_morph(mask, footprint, MORPH_OPEN)


# ---------------------------------------------------------------- splitting touching objects (csrc/split.hip)
GROW_ROUNDS = _lib.SPLIT_HALO     # rounds of one growth launch: the kernel's halo
GROW_CADENCE = 4                  # growth launches per read-back of the changed word (measured: profiles/split_micro.txt)


def edt_sq(mask, cap):
    """Capped squared distance map: mask (H,W) / (B,H,W) uint8 -> int32 of the same shape, 0 on the background and elsewhere
    min(cap, squared distance to the nearest background pixel of the same image); 1 <= cap <= 65025 (split.edt_sq_host)."""
    m, squeeze = _mask3(mask)
    B, H, W = m.shape
    if not 1 <= int(cap) <= 255 * 255:
        raise _lib.WesupHipError(f'edt_sq: cap {cap} (1 .. 65025)')
    d2 = torch.empty(B, H, W, dtype=torch.int32, device=m.device)
    nb = _lib.load().wesup_edt_sq_workspace_bytes(B, H, W)
    ws = workspace(nb, m.device, 'regions')
    _lib.call('wesup_edt_sq', _p(m), _p(d2), B, H, W, int(cap), _p(ws), nb, _stream())
    return d2[0] if squeeze else d2


def label_grow(mask, seeds, cadence=None, rounds=None, return_launches=False):
    """Grow the positive labels of ``seeds`` (int32, any positive values) over the foreground of ``mask`` to the fixed point of
    split.label_grow_host: mask, seeds (H,W) / (B,H,W) -> int32 labels of the same shape.  ``rounds`` synchronous rounds per
    launch (even, at most GROW_ROUNDS), ``cadence`` launches between two read-backs of the changed word, which reports the last
    launch of the group; growth stops after the first read-back of a launch that changed nothing.  Launches past the fixed point
    change nothing, so neither knob changes the map."""
    m, squeeze = _mask3(mask)
    _chk(seeds, torch.int32, 'seeds')
    if seeds.shape != mask.shape:
        raise _lib.WesupHipError(f'label_grow: seeds {tuple(seeds.shape)} for a mask {tuple(mask.shape)}')
    cadence = GROW_CADENCE if cadence is None else int(cadence)
    rounds = GROW_ROUNDS if rounds is None else int(rounds)
    if cadence < 1 or rounds < 2 or rounds > GROW_ROUNDS or rounds % 2:
        raise _lib.WesupHipError(f'label_grow: cadence {cadence} (>= 1), rounds {rounds} (even, 2 .. {GROW_ROUNDS})')
    B, H, W = m.shape
    src = seeds.reshape(B, H, W)
    bufs = [torch.empty(B, H, W, dtype=torch.int32, device=m.device) for _ in range(2)]
    changed = torch.empty(1, dtype=torch.int32, device=m.device)
    nb = _lib.load().wesup_label_grow_workspace_bytes(B, H, W)
    ws = workspace(nb, m.device, 'regions')
    launches = 0
    while True:
        dst = bufs[0] if src is not bufs[0] else bufs[1]
        _lib.call('wesup_label_grow', _p(m), _p(src), _p(dst), _p(changed), B, H, W, 1 + launches * rounds, cadence, rounds,
                  _p(ws), nb, _stream())
        launches += cadence
        src = dst
        if int(changed.item()) == 0:
            break
    out = src[0] if squeeze else src
    return (out, launches) if return_launches else out


def label_cut(mask, labels):
    """mask uint8, labels int32 (H,W) / (B,H,W) -> uint8 {0,1}: 0 on the background and where a pixel's label a > 0 has an
    8-neighbour with a label 0 < b < a (split.label_cut_host)."""
    m, squeeze = _mask3(mask)
    _chk(labels, torch.int32, 'labels')
    if labels.shape != mask.shape:
        raise _lib.WesupHipError(f'label_cut: labels {tuple(labels.shape)} for a mask {tuple(mask.shape)}')
    B, H, W = m.shape
    out = torch.empty_like(m)
    _lib.call('wesup_label_cut', _p(m), _p(labels), _p(out), B, H, W, _stream())
    return out[0] if squeeze else out


def split_objects(mask, radius, return_labels=False):
    """Separate touching objects of a binary mask (H,W) / (B,H,W) uint8 -> uint8 {0,1}: the components of {edt_sq >= radius^2}
    are the seeds (cc_label), their labels grow over the mask (label_grow) and a one-pixel cut is taken where two labels meet
    (label_cut); 1 <= radius <= 255, radius 1 is the identity.  Equal to split.split_objects bit for bit.  A seed pixel is never
    cut while different seeds lie more than 3 pixels apart; two cores closer than that lose a pixel of the larger label (the cut
    still separates them)."""
    radius = int(radius)
    if not 1 <= radius <= 255:
        raise _lib.WesupHipError(f'split_objects: radius {radius} (1 .. 255)')
    _mask3(mask)
    r2 = radius * radius
    core = (edt_sq(mask, r2) >= r2).to(torch.uint8)
    seeds, _ = cc_label(core)
    labels = label_grow(mask, seeds)
    out = label_cut(mask, labels)
    return (out, labels) if return_labels else out


# ---------------------------------------------------------------- surface-distance metrics (csrc/surface.hip)
EDT_NONE = _lib.EDT_NONE
SURFACE_STAT_KEYS = ('n_p', 'n_g', 'max_pg', 'max_gp', 'within_p', 'within_g', 'lo', 'hi', 'sum_pg', 'sum_gp')


def _edt_shape(B, H, W, name):
    if (H - 1) ** 2 + (W - 1) ** 2 >= EDT_NONE:
        raise _lib.WesupHipError(f'{name}: squared distances of a {H} x {W} image reach {EDT_NONE}')
    if not _lib.load().wesup_edt_full_workspace_bytes(B, H, W):
        raise _lib.WesupHipError(f'{name}: shape ({B}, {H}, {W}) is outside the entry\'s range')


def edt_sq_full(mask, invert=False):
    """Exact squared distance map without a cap: mask (H,W) / (B,H,W) uint8 -> int32 of the same shape, 0 where the mask is 0 and
    elsewhere the squared distance to the nearest zero pixel of the same image, EDT_NONE in an image without one
    (surface.edt_sq_full_host).  ``invert`` transforms ``mask == 0`` instead."""
    m, squeeze = _mask3(mask)
    B, H, W = m.shape
    _edt_shape(B, H, W, 'edt_sq_full')
    d2 = torch.empty(B, H, W, dtype=torch.int32, device=m.device)
    nb = _lib.load().wesup_edt_full_workspace_bytes(B, H, W)
    ws = workspace(nb, m.device, 'regions')
    _lib.call('wesup_edt_full', _p(m), _p(d2), B, H, W, int(bool(invert)), _p(ws), nb, _stream())
    return d2[0] if squeeze else d2


def mask_border(mask):
    """The 4-neighbour border of a mask: (H,W) / (B,H,W) uint8 -> {0,1} uint8 of the same shape, 1 on the foreground pixels with
    a neighbour on the background or outside the image (surface.border_host)."""
    m, squeeze = _mask3(mask)
    B, H, W = m.shape
    if min(B, H, W) < 1:
        raise _lib.WesupHipError(f'mask_border: empty shape {tuple(m.shape)}')
    out = torch.empty_like(m)
    _lib.call('wesup_mask_border', _p(m), _p(out), B, H, W, _stream())
    return out[0] if squeeze else out


def select_i32(keys, ranks, out=None):
    """keys (n,) int32, all >= 0 (not checked: that would be a read-back), ranks (r,) int64 ON THE DEVICE, r <= 4 -> (r,) int32:
    np.sort(keys)[ranks], exact, without a read-back.  A rank outside [0, n) is taken to the nearest end."""
    _chk(keys, torch.int32, 'keys'); _chk(ranks, torch.int64, 'ranks')
    n, r = keys.numel(), ranks.numel()
    if keys.dim() != 1 or ranks.dim() != 1 or n < 1 or not 1 <= r <= _lib.SELECT_MAX_RANKS or ranks.device != keys.device:
        raise _lib.WesupHipError(f'select_i32: keys {tuple(keys.shape)}, ranks {tuple(ranks.shape)} (1 .. {_lib.SELECT_MAX_RANKS} ranks)')
    out = torch.empty(r, dtype=torch.int32, device=keys.device) if out is None else _chk(out, torch.int32, 'out')
    if out.numel() != r or out.device != keys.device:
        raise _lib.WesupHipError(f'select_i32: out {tuple(out.shape)} for {r} ranks')
    nb = _lib.load().wesup_select_i32_workspace_bytes(n)
    ws = workspace(nb, keys.device, 'regions')
    _lib.call('wesup_select_i32', _p(keys), n, _p(ranks), r, _p(out), _p(ws), nb, _stream())
    return out


def surface_stats_blocks(pred, gt, tolerance, q=95.0):
    """The launch chain of ``surface_stats`` without its read-back: (B,H,W) masks -> the (B, 10) int64 tensor of the pairs'
    blocks on the device (slots 8 and 9 hold the bits of the two float64 sums).  Borders of both masks in one launch, both
    distance maps in one transform of 2 B images, the reductions and the selection."""
    p, _ = _mask3(pred, 'pred')
    g, _ = _mask3(gt, 'gt')
    if p.shape != g.shape or p.device != g.device:
        raise _lib.WesupHipError(f'surface_stats: pred {tuple(p.shape)} and gt {tuple(g.shape)} differ')
    tolerance, q = float(tolerance), float(q)
    if not 0.0 <= tolerance < float('inf') or not 0.0 <= q <= 100.0:
        raise _lib.WesupHipError(f'surface_stats: tolerance {tolerance} (finite, >= 0), q {q} (0 .. 100)')
    B, H, W = p.shape
    if 2 * B > 65535:
        raise _lib.WesupHipError(f'surface_stats: {B} pairs (at most 32767)')
    _edt_shape(2 * B, H, W, 'surface_stats')
    t2 = int(min(tolerance * tolerance, float(EDT_NONE)))            # floor of the float64 square, as the host takes it (no d2 is above EDT_NONE)
    q_bits = struct.unpack('<q', struct.pack('<d', q / 100.0))[0]
    borders = mask_border(torch.cat((p, g)))                         # S_P of every pair, then S_G
    d2 = edt_sq_full(borders, invert=True)                           # the distances to S_P, then to S_G
    stats = torch.empty(B, _lib.SURFACE_STATS, dtype=torch.int64, device=p.device)
    nb = _lib.load().wesup_surface_stats_workspace_bytes(B, H, W)
    ws = workspace(nb, p.device, 'surface')                          # (the distance maps' scratch is 'regions': another buffer)
    _lib.call('wesup_surface_stats', _p(borders[:B]), _p(borders[B:]), _p(d2[B:]), _p(d2[:B]), _p(stats), B, H, W, t2, q_bits,
              _p(ws), nb, _stream())
    return stats


def surface_stats(pred, gt, tolerance, q=95.0):
    """The raw quantities of the surface metrics (surface.surface_stats_host) as Python numbers: pred, gt (H,W) uint8 -> a dict
    of SURFACE_STAT_KEYS, (B,H,W) -> a list of B dicts.  One read-back of 80 bytes per pair, after the whole chain."""
    blocks = surface_stats_blocks(pred, gt, tolerance, q).cpu()
    sums = blocks[:, 8:].contiguous().view(torch.float64)
    rows = [dict(zip(SURFACE_STAT_KEYS, [int(v) for v in blocks[b, :8]] + [float(v) for v in sums[b]]))
            for b in range(blocks.shape[0])]
    return rows[0] if pred.dim() == 2 else rows


# ---------------------------------------------------------------- object outlines (csrc/contour.hip)
CONTOUR_RING = _lib.CONTOUR_RING


def _labels_bhw(labels, name):
    """(H,W) or (B,H,W) int32 -> (B,H,W) inside the entries' range (4 B H W < 2^31)."""
    _chk(labels, torch.int32, name)
    if labels.dim() not in (2, 3):
        raise _lib.WesupHipError(f'{name}: expected (H,W) or (B,H,W), got {tuple(labels.shape)}')
    l3 = labels.unsqueeze(0) if labels.dim() == 2 else labels
    if not _lib.load().wesup_contour_trace_workspace_bytes(*l3.shape, 0):
        raise _lib.WesupHipError(f'{name}: shape {tuple(l3.shape)} is outside the entry\'s range (B <= 65535, 4 B H W < 2^31)')
    return l3


def contour_count(labels):
    """labels (H,W) / (B,H,W) int32 -> (B, 2) int32 on the device: the cracks and the corners of every image
    (contour.count_host).  No read-back."""
    l3 = _labels_bhw(labels, 'contour_count')
    B, H, W = l3.shape
    counts = torch.empty(B, 2, dtype=torch.int32, device=l3.device)
    nb = _lib.load().wesup_contour_trace_workspace_bytes(B, H, W, 0)
    ws = workspace(nb, l3.device, 'contour')
    _lib.call('wesup_contour_count', _p(l3), _p(counts), B, H, W, _p(ws), nb, _stream())
    return counts


def contour_trace(labels):
    """The boundary rings of a label map, labels (H,W) / (B,H,W) int32 -> (rings (R, 12) int32, verts (V, 2) int32, n_rings (B,)
    int32) on the device, equal to contour.trace_host.  One read-back of the counts sizes the buffers before the trace; the
    status word and the ring counts come back together after it (rings is cut to R from them)."""
    l3 = _labels_bhw(labels, 'contour_trace')
    B, H, W = l3.shape
    dev = l3.device
    tot = contour_count(l3).sum(0, dtype=torch.int64).tolist()               # the read-back
    n_cracks, n_corners = int(tot[0]), int(tot[1])
    ring_cap = n_corners // 4
    rings = torch.empty(max(ring_cap, 1), CONTOUR_RING, dtype=torch.int32, device=dev)
    verts = torch.empty(max(n_corners, 1), 2, dtype=torch.int32, device=dev)
    tail = torch.zeros(B + 1, dtype=torch.int32, device=dev)                 # n_rings, then the status word
    nb = _lib.load().wesup_contour_trace_workspace_bytes(B, H, W, n_cracks)
    ws = workspace(nb, dev, 'contour')
    _lib.call('wesup_contour_trace', _p(l3), _p(rings), _p(verts), _p(tail), ctypes.c_void_p(tail.data_ptr() + 4 * B), B, H, W,
              n_cracks, n_corners, ring_cap, _p(ws), nb, _stream())
    t = tail.tolist()
    if t[B] != 0:
        raise _lib.WesupHipError(f'contour_trace: status {t[B]}: the map changed between the count and the trace')
    return rings[:sum(t[:B])], verts[:n_corners], tail[:B]


def contour_simplify(rings, verts, tol_q4):
    """Exact Douglas-Peucker of traced rings: rings (R, 12) and verts (V, 2) int32 as ``contour_trace`` leaves
    them, ``tol_q4`` the tolerance in sixteenths of a pixel (0 .. 4096) -> (rings2 (R, 12), verts2 (V2, 2), flags (R,), counts
    (4,): kept vertices, rings flagged 1, rings flagged 2, status) int32 on the device, equal to contour.simplify_host.  One
    read-back behind the call, of ``counts``: verts2 is cut to its length from it."""
    name = 'contour_simplify'
    _chk(rings, torch.int32, f'{name}: rings')
    _chk(verts, torch.int32, f'{name}: verts')
    if rings.dim() != 2 or rings.shape[1] != CONTOUR_RING or verts.dim() != 2 or verts.shape[1] != 2 or verts.device != rings.device:
        raise _lib.WesupHipError(f'{name}: expected rings (R, {CONTOUR_RING}) and verts (V, 2) on one device, got '
                                 f'{tuple(rings.shape)} and {tuple(verts.shape)}')
    tol = int(tol_q4)
    if tol != tol_q4 or not 0 <= tol <= _lib.SIMPLIFY_TOL_MAX:
        raise _lib.WesupHipError(f'{name}: tol_q4 {tol_q4}: an integer in 0 .. {_lib.SIMPLIFY_TOL_MAX}')
    dev = rings.device
    R, V = rings.shape[0], verts.shape[0]
    if R == 0 and V != 0:
        raise _lib.WesupHipError(f'{name}: {V} vertices without a ring')
    if R == 0:
        return (torch.empty(0, CONTOUR_RING, dtype=torch.int32, device=dev), torch.empty(0, 2, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev), torch.zeros(_lib.SIMPLIFY_COUNTS, dtype=torch.int32, device=dev))
    nb = _lib.load().wesup_contour_simplify_workspace_bytes(R, V)
    if not nb:
        raise _lib.WesupHipError(f'{name}: {R} rings of {V} vertices are outside the entry\'s range (R <= V <= 2^28)')
    rings2 = torch.empty(max(R, 1), CONTOUR_RING, dtype=torch.int32, device=dev)
    verts2 = torch.empty(max(V, 1), 2, dtype=torch.int32, device=dev)
    flags = torch.empty(max(R, 1), dtype=torch.int32, device=dev)
    counts = torch.empty(_lib.SIMPLIFY_COUNTS, dtype=torch.int32, device=dev)
    ws = workspace(nb, dev, 'simplify')
    _lib.call('wesup_contour_simplify', _p(rings), R, _p(verts), V, tol, _p(rings2), _p(verts2), _p(flags), _p(counts), _p(ws), nb,
              _stream())
    c = counts.tolist()                                                      # the read-back
    if c[3] != 0:
        raise _lib.WesupHipError(f'{name}: status {c[3]}: the records\' vertex ranges are not consecutive from 0 to {V}')
    return rings2[:R], verts2[:c[0]], flags[:R], counts


# ---------------------------------------------------------------- polygon fill (csrc/raster.hip)
def polygon_fill(verts, ring_first, feature_first_ring, feature_image, shape, values=None):
    """Polygons in CSR form, fixed point with 8 fractional bits (raster.pack) -> (labels int32, out8 uint8 or None, status (1,)
    int32) on the device, equal to raster.fill_host: verts (V, 2), ring_first (R + 1,), feature_first_ring (F + 1,),
    feature_image (F,) int32 device tensors, ``shape`` (H, W) or (B, H, W), ``values`` (F,) uint8 for the class map.  No
    read-back: bit 0 of status says that a feature was refused (it paints nothing)."""
    name = 'polygon_fill'
    for t, what in ((verts, 'verts'), (ring_first, 'ring_first'), (feature_first_ring, 'feature_first_ring'),
                    (feature_image, 'feature_image')):
        _chk(t, torch.int32, f'{name}: {what}')
    dev = verts.device
    s = tuple(int(v) for v in shape)
    if len(s) not in (2, 3):
        raise _lib.WesupHipError(f'{name}: shape (H, W) or (B, H, W), got {shape}')
    B, H, W = (1,) + s if len(s) == 2 else s
    F, R, V = feature_image.numel(), ring_first.numel() - 1, verts.shape[0] if verts.dim() == 2 else -1
    if V < 0 or verts.shape[1] != 2 or ring_first.dim() != 1 or R < 0 or feature_first_ring.dim() != 1 or \
            feature_first_ring.numel() != F + 1 or feature_image.dim() != 1:
        raise _lib.WesupHipError(f'{name}: expected verts (V, 2), ring_first (R + 1,), feature_first_ring (F + 1,), feature_image '
                                 f'(F,), got {tuple(verts.shape)}, {tuple(ring_first.shape)}, {tuple(feature_first_ring.shape)}, '
                                 f'{tuple(feature_image.shape)}')
    if any(t.device != dev for t in (ring_first, feature_first_ring, feature_image)):
        raise _lib.WesupHipError(f'{name}: the operands lie on different devices')
    nb = _lib.load().wesup_polygon_fill_workspace_bytes(B, H, W, F)
    if not nb:
        raise _lib.WesupHipError(f'{name}: shape {(B, H, W)} is outside the entry\'s range (B H W < 2^31, H, W <= 2^21)')
    out8 = None
    if values is not None:
        _chk(values, torch.uint8, f'{name}: values')
        if values.shape != (F,) or values.device != dev:
            raise _lib.WesupHipError(f'{name}: values {tuple(values.shape)} on {values.device}, expected ({F},) on {dev}')
        out8 = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = workspace(nb, dev, 'raster')
    _lib.call('wesup_polygon_fill', _p(verts), _p(ring_first), _p(feature_first_ring), _p(feature_image), _p(values), _p(labels),
              _p(out8), _p(status), B, H, W, F, R, V, _p(ws), nb, _stream())
    if len(s) == 2:
        labels, out8 = labels[0], (None if out8 is None else out8[0])
    return labels, out8, status


# ---------------------------------------------------------------- object measurements (csrc/measure.hip)
MEASURE_WORDS = _lib.MEASURE_WORDS


def measure_limits():
    """(labels L + 1 up to which a block keeps its moment table in LDS, candidates per block of the hull test)."""
    lib = _lib.load()
    return lib.wesup_measure_limit(0), lib.wesup_measure_limit(1)


def _measure_args(labels, L, name):
    _chk(labels, torch.int32, name)
    if labels.dim() not in (2, 3) or labels.numel() < 1:
        raise _lib.WesupHipError(f'{name}: expected (H,W) or (B,H,W), got {tuple(labels.shape)}')
    l3 = labels.unsqueeze(0) if labels.dim() == 2 else labels
    L = int(L)
    if not _lib.load().wesup_measure_workspace_bytes(*l3.shape, L, 0):
        raise _lib.WesupHipError(f'{name}: shape {tuple(l3.shape)} with L = {L} is outside the entry\'s range (B <= 65535, sides '
                                 'up to 32768, L + 1 <= 2^20, B (L + 1) <= 2^26)')
    return l3, L


def measure_profile_count(labels, L):
    """labels (H,W) / (B,H,W) int32 -> ((1,) int64 on the device: the lines of pixel corners all labels in 1 .. L span together,
    the profile capacity of ``object_measure``; status (B,) int32).  No read-back."""
    l3, L = _measure_args(labels, L, 'measure_profile_count')
    B, H, W = l3.shape
    count = torch.empty(1, dtype=torch.int64, device=l3.device)
    status = torch.empty(B, dtype=torch.int32, device=l3.device)
    nb = _lib.load().wesup_measure_workspace_bytes(B, H, W, L, 0)
    ws = workspace(nb, l3.device, 'measure')
    _lib.call('wesup_measure_profile_count', _p(l3), _p(count), _p(status), B, H, W, L, _p(ws), nb, _stream())
    return count, status


def object_measure(labels, L, d2=None):
    """Per-label measurements of a label map, labels (H,W) / (B,H,W) int32 with labels 0 .. L, d2 None or an int32 map of the same
    shape (``edt_sq_full(labels > 0)``) -> (table (B, L+1, 24) int64, hull_verts (V, 2) int32, status (B,) int32) on the device,
    equal to measure.measure_host.  The call's one read-back, 8 bytes, comes in front: the profile count sizes the workspace, the
    capacity of hull_verts (twice the count) and the grid.  The status words and the number of vertices (the sum of the table's
    word 17, to which hull_verts is cut) come back together after the call."""
    l3, L = _measure_args(labels, L, 'object_measure')
    B, H, W = l3.shape
    dev = l3.device
    if d2 is not None:
        _chk(d2, torch.int32, 'd2')
        if d2.numel() != l3.numel() or d2.device != dev:
            raise _lib.WesupHipError(f'object_measure: d2 {tuple(d2.shape)} for labels {tuple(labels.shape)}')
    n_prof = int(measure_profile_count(l3, L)[0].item())                      # the read-back
    if n_prof > _lib.load().wesup_measure_limit(5):
        raise _lib.WesupHipError(f'object_measure: {n_prof} profile lines')
    vert_cap = 2 * n_prof
    table = torch.empty(B, L + 1, MEASURE_WORDS, dtype=torch.int64, device=dev)
    verts = torch.empty(max(vert_cap, 1), 2, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    nb = _lib.load().wesup_measure_workspace_bytes(B, H, W, L, n_prof)
    ws = workspace(nb, dev, 'measure')
    _lib.call('wesup_object_measure', _p(l3), _p(d2), _p(table), _p(verts), _p(status), B, H, W, L, n_prof, vert_cap, _p(ws), nb,
              _stream())
    short = (status & 2).any()                                                 # (the table is unwritten then: not summed)
    tail = torch.stack((short.to(torch.int64), torch.where(short, 0, table[:, :, 17].sum()))).tolist()
    if tail[0]:
        raise _lib.WesupHipError('object_measure: status 2: the map changed between the count and the measurement')
    return table, verts[:tail[1]], status


def contingency(S, G, nS, nG):
    """Label maps S, G (H,W) / (B,H,W) int32 with labels in [0, nS] / [0, nG] -> (B, nS+1, nG+1) int32 pixel counts (the batch
    axis only for batched input).  Raises when a label lies outside the table or the table would exceed
    ``CONTINGENCY_MAX_CELLS`` (nothing is allocated then)."""
    _chk(S, torch.int32, 'S'); _chk(G, torch.int32, 'G')
    if S.shape != G.shape or S.dim() not in (2, 3):
        raise _lib.WesupHipError(f'contingency: shapes {tuple(S.shape)} and {tuple(G.shape)}')
    nS, nG = int(nS), int(nG)
    if nS < 0 or nG < 0 or (nS + 1) * (nG + 1) > CONTINGENCY_MAX_CELLS:
        raise _lib.WesupHipError(f'contingency: a table of {nS + 1} x {nG + 1} cells is not built on the device')
    B = 1 if S.dim() == 2 else S.shape[0]
    HW = S.shape[-1] * S.shape[-2]
    table = torch.empty(B, nS + 1, nG + 1, dtype=torch.int32, device=S.device)
    status = torch.empty(B, dtype=torch.int32, device=S.device)
    _lib.call('wesup_contingency', _p(S), _p(G), _p(table), _p(status), B, HW, nS, nG, _stream())
    return (table[0] if S.dim() == 2 else table), status


class LabelLists:
    """Per-label pixel lists of a label map (label_sort): ``pix[start[l]:start[l+1]]`` are the pixels of label l in ascending
    order, ``bpix`` / ``bstart`` the boundary pixels of the labels >= 1."""
    __slots__ = ('labels', 'L', 'start', 'pix', 'bstart', 'bpix', 'status')


def label_sort(labels, L):
    """labels (H,W) / (B,H,W) int32 in [0, L] -> LabelLists (tensors carry a batch axis only for batched input)."""
    _chk(labels, torch.int32, 'labels')
    if labels.dim() not in (2, 3):
        raise _lib.WesupHipError(f'label_sort: expected (H,W) or (B,H,W), got {tuple(labels.shape)}')
    L = int(L)
    if L < 0 or L >= LABEL_SORT_MAX_LABELS:
        raise _lib.WesupHipError(f'label_sort: {L} labels (below {LABEL_SORT_MAX_LABELS})')
    single = labels.dim() == 2
    B = 1 if single else labels.shape[0]
    H, W = labels.shape[-2:]
    dev = labels.device
    out = LabelLists()
    out.labels, out.L = labels, L
    out.start = torch.empty(B, L + 2, dtype=torch.int32, device=dev)
    out.bstart = torch.empty(B, L + 2, dtype=torch.int32, device=dev)
    out.pix = torch.empty(B, H * W, dtype=torch.int32, device=dev)
    out.bpix = torch.empty(B, H * W, dtype=torch.int32, device=dev)
    out.status = torch.empty(B, dtype=torch.int32, device=dev)
    nb = _lib.load().wesup_label_sort_workspace_bytes(B, H, W, L)
    ws = workspace(nb, dev, 'regions')
    _lib.call('wesup_label_sort', _p(labels), _p(out.start), _p(out.pix), _p(out.bstart), _p(out.bpix), _p(out.status), B, H, W,
              L, _p(ws), nb, _stream())
    if single:
        for k in ('start', 'pix', 'bstart', 'bpix'):
            setattr(out, k, getattr(out, k)[0])
    return out


def directed_hausdorff_sq(pairs, X, Y):
    """pairs (P,2) int32 of (object of X, object of Y); X, Y: LabelLists of two (H,W) label maps -> (P,) int32 squared directed
    Hausdorff distances max_{p in a} min_{q in b} |p - q|^2."""
    _chk(pairs, torch.int32, 'pairs')
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise _lib.WesupHipError(f'directed_hausdorff_sq: pairs {tuple(pairs.shape)}')
    if X.labels.dim() != 2 or X.labels.shape != Y.labels.shape:
        raise _lib.WesupHipError('directed_hausdorff_sq: two (H,W) label maps of one shape')
    H, W = X.labels.shape
    P = pairs.shape[0]
    d2 = torch.empty(P, dtype=torch.int32, device=pairs.device)
    if P:
        _lib.call('wesup_directed_hausdorff_sq', _p(pairs), _p(X.start), _p(X.pix), _p(Y.labels), _p(Y.bstart), _p(Y.bpix),
                  _p(d2), P, H, W, X.L, Y.L, _stream())
    return d2


# ---------------------------------------------------------------- painted object comparisons (csrc/paint.hip)
LABEL_PAINT_MAX_LUT = 1 << 26        # entries of a colour table


def object_match(table, nS_dev, nG_dev):
    """table (nS+1, nG+1) / (B, nS+1, nG+1) int32 as ``contingency`` writes it, nS_dev / nG_dev (B,) int32 device tensors with
    each image's own object counts (``cc_label``'s n_labels; cells outside them are not read) -> (B, nS+1) int32: the
    ground-truth object every predicted object takes its colour from (paint.match_objects_from_table), 0 for row 0 and the rows
    past an image's own count.  The batch axis only for batched input."""
    _chk(table, torch.int32, 'table'); _chk(nS_dev, torch.int32, 'nS_dev'); _chk(nG_dev, torch.int32, 'nG_dev')
    if table.dim() not in (2, 3) or table.shape[-1] < 1 or table.shape[-2] < 1:
        raise _lib.WesupHipError(f'object_match: table {tuple(table.shape)}')
    B = 1 if table.dim() == 2 else table.shape[0]
    nS, nG = table.shape[-2] - 1, table.shape[-1] - 1
    if B < 1 or (nS + 1) * (nG + 1) > CONTINGENCY_MAX_CELLS:
        raise _lib.WesupHipError(f'object_match: {B} tables of {nS + 1} x {nG + 1} cells')
    if tuple(nS_dev.shape) != (B,) or tuple(nG_dev.shape) != (B,) or nS_dev.device != table.device or nG_dev.device != table.device:
        raise _lib.WesupHipError(f'object_match: counts {tuple(nS_dev.shape)} and {tuple(nG_dev.shape)} for {B} tables (one device)')
    match = torch.empty(B, nS + 1, dtype=torch.int32, device=table.device)
    nb = _lib.load().wesup_object_match_workspace_bytes(B, nG)
    ws = workspace(nb, table.device, 'regions')
    _lib.call('wesup_object_match', _p(table), _p(nS_dev), _p(nG_dev), _p(match), B, nS, nG, _p(ws), nb, _stream())
    return match[0] if table.dim() == 2 else match


def label_paint(labels, lut):
    """labels (H,W) / (B,H,W) int32, lut (n_lut,) / (B, n_lut) int32 with one colour per label packed R | G << 8 | B << 16 ->
    ((..., H, W, 3) uint8 interleaved RGB, status (B,) int32).  A label outside [0, n_lut) paints black and sets bit 0 of its
    image's status; it is never used as an index."""
    _chk(labels, torch.int32, 'labels'); _chk(lut, torch.int32, 'lut')
    if labels.dim() not in (2, 3) or lut.dim() != labels.dim() - 1:
        raise _lib.WesupHipError(f'label_paint: labels {tuple(labels.shape)}, lut {tuple(lut.shape)}')
    single = labels.dim() == 2
    B = 1 if single else labels.shape[0]
    H, W = labels.shape[-2:]
    n_lut = lut.shape[-1]
    if B < 1 or H * W < 1 or n_lut < 1 or n_lut > LABEL_PAINT_MAX_LUT or (not single and lut.shape[0] != B):
        raise _lib.WesupHipError(f'label_paint: labels {tuple(labels.shape)}, lut {tuple(lut.shape)}')
    if lut.device != labels.device:
        raise _lib.WesupHipError('label_paint: labels and lut on different devices')
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=labels.device)
    status = torch.empty(B, dtype=torch.int32, device=labels.device)
    _lib.call('wesup_label_paint', _p(labels), _p(lut), _p(out), _p(status), B, H * W, n_lut, _stream())
    return (out[0] if single else out), status


# ---------------------------------------------------------------- exact t-SNE of superpixel features (csrc/tsne.hip)
TSNE_MAX_N = _lib.TSNE_MAX_N
TSNE_MAX_D = _lib.TSNE_MAX_D
TSNE_STATS = _lib.TSNE_STATS


def tsne_check_shape(n, d=1, perplexity=None):
    """The limits of the t-SNE entries, as ValueErrors before any tensor is looked at."""
    if not 2 <= int(n) <= TSNE_MAX_N:
        raise ValueError(f't-SNE: {n} rows, expected 2 .. {TSNE_MAX_N} (the joint probabilities are a dense fp32 matrix)')
    if not 1 <= int(d) <= TSNE_MAX_D:
        raise ValueError(f't-SNE: {d} features, expected 1 .. {TSNE_MAX_D}')
    if perplexity is not None and not 0 < float(perplexity) < int(n):
        raise ValueError(f't-SNE: perplexity {perplexity} for {n} rows, expected 0 < perplexity < rows')


def tsne_sqdist(x, out=None):
    """x (N, D) -> (N, N) squared Euclidean distances from differences: bit-symmetric, the diagonal exactly 0."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError('tsne_sqdist: expected an (N, D) tensor')
    n, d = x.shape
    tsne_check_shape(n, d)
    _chk(x, name='x')
    if out is None:
        out = torch.empty(n, n, dtype=torch.float32, device=x.device)
    _chk(out, name='out')
    if tuple(out.shape) != (n, n) or out.device != x.device:
        raise _lib.WesupHipError(f'tsne_sqdist: out {tuple(out.shape)} for {n} rows')
    _lib.call('wesup_tsne_sqdist', _p(x), n, d, _p(out), _stream())
    return out


def tsne_affinities(d2, perplexity, p=None, beta=None):
    """d2 (N, N) squared distances -> (P (N, N) joint probabilities, beta (N,)): scikit-learn's per-row perplexity search on the
    row minus its smallest off-diagonal entry, then max((C + C^T) / sum, eps) with the diagonal 0."""
    if not isinstance(d2, torch.Tensor) or d2.dim() != 2 or d2.shape[0] != d2.shape[1]:
        raise ValueError('tsne_affinities: expected an (N, N) tensor')
    n = d2.shape[0]
    tsne_check_shape(n, 1, perplexity)
    _chk(d2, name='d2')
    dev = d2.device
    p = torch.empty(n, n, dtype=torch.float32, device=dev) if p is None else _chk(p, name='p')
    beta = torch.empty(n, dtype=torch.float32, device=dev) if beta is None else _chk(beta, name='beta')
    if tuple(p.shape) != (n, n) or tuple(beta.shape) != (n,) or p.device != dev or beta.device != dev or p.data_ptr() == d2.data_ptr():
        raise _lib.WesupHipError(f'tsne_affinities: p {tuple(p.shape)}, beta {tuple(beta.shape)} for {n} rows (p apart from d2)')
    nb = _lib.load().wesup_tsne_affinities_workspace_bytes(n)
    ws = workspace(nb, dev, 'tsne')
    _lib.call('wesup_tsne_affinities', _p(d2), n, float(perplexity), _p(p), _p(beta), _p(ws), nb, _stream())
    return p, beta


def tsne_iterate(p, y, upd, gains, stats, iters, exaggeration=1.0, momentum=0.8, lr=200.0, min_gain=0.01):
    """Enqueues ``iters`` gradient iterations on y (N, 2) in place (upd, gains (N, 2) with it); the last one writes stats
    (TSNE_STATS,) = KL of the unexaggerated p, |g|, Z, sum p log p at the y it started from.  ``iters`` 0 only writes the stats.
    Nothing is synchronised."""
    if not isinstance(p, torch.Tensor) or p.dim() != 2 or p.shape[0] != p.shape[1]:
        raise ValueError('tsne_iterate: expected an (N, N) tensor p')
    n = p.shape[0]
    tsne_check_shape(n)
    for t, name in ((p, 'p'), (y, 'y'), (upd, 'upd'), (gains, 'gains'), (stats, 'stats')):
        _chk(t, name=name)
        if t.device != p.device:
            raise _lib.WesupHipError('tsne_iterate: tensors on different devices')
    if any(tuple(t.shape) != (n, 2) for t in (y, upd, gains)) or stats.numel() < TSNE_STATS:
        raise _lib.WesupHipError(f'tsne_iterate: y, upd, gains must be ({n}, 2) and stats hold {TSNE_STATS} floats')
    nb = _lib.load().wesup_tsne_iterate_workspace_bytes(n)
    ws = workspace(nb, p.device, 'tsne')
    _lib.call('wesup_tsne_iterate', _p(p), _p(y), _p(upd), _p(gains), _p(stats), n, int(iters), float(exaggeration),
              float(momentum), float(lr), float(min_gain), _p(ws), nb, _stream())
    return y


# ---------------------------------------------------------------- stain normalisation and stain jitter (csrc/stain.hip)
STAIN_BLOCK = _lib.STAIN_BLOCK
STAIN_IO, STAIN_ALPHA, STAIN_BETA, STAIN_MIN_TISSUE = 240.0, 1.0, 0.15, 16
STAIN_MAX_SAMPLES = 1 << 24        # samples of one fit: n_tissue travels as a float
_stain_ws = {}                     # (device, stream) -> grow-only byte buffer


def _stain_workspace(nbytes, device):
    """The stain entries' scratch, one per stream (the prefetcher's copy stream runs beside the step).  Apart from ``workspace()``
    on purpose: no recorded step plan holds one of these addresses, so a growth -- every new largest shape under multi-scale
    training -- must not bump ``ws_generation`` and drop the plans.  A replaced buffer goes back to torch's allocator, which
    orders its reuse behind the kernels queued on the stream it was allocated on: this one."""
    key = (str(device), torch.cuda.current_stream().cuda_stream)
    buf = _stain_ws.get(key)
    if buf is None or buf.numel() < nbytes:
        _stain_ws.pop(key, None)
        buf = _stain_ws[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    return buf


def select_f32(keys, ranks, out=None):
    """keys (n,) fp32, ranks (r,) int64 ON THE DEVICE, r <= 4 -> (r,) fp32: np.sort(keys)[ranks], bit for bit, without a
    read-back.  A rank outside [0, n) is taken to the nearest end."""
    _chk(keys, name='keys'); _chk(ranks, torch.int64, 'ranks')
    n, r = keys.numel(), ranks.numel()
    if keys.dim() != 1 or ranks.dim() != 1 or n < 1 or not 1 <= r <= _lib.SELECT_MAX_RANKS or ranks.device != keys.device:
        raise _lib.WesupHipError(f'select_f32: keys {tuple(keys.shape)}, ranks {tuple(ranks.shape)} (1 .. {_lib.SELECT_MAX_RANKS} ranks)')
    out = torch.empty(r, dtype=torch.float32, device=keys.device) if out is None else _chk(out, name='out')
    if out.numel() != r or out.device != keys.device:
        raise _lib.WesupHipError(f'select_f32: out {tuple(out.shape)} for {r} ranks')
    nb = _lib.load().wesup_select_f32_workspace_bytes(n)
    ws = _stain_workspace(nb, keys.device)
    _lib.call('wesup_select_f32', _p(keys), n, _p(ranks), r, _p(out), _p(ws), nb, _stream())
    return out


def stain_stride(H, W):
    """The smallest sampling stride that keeps a fit at or below 2^24 samples."""
    s = 1
    while -(-H // s) * -(-W // s) > STAIN_MAX_SAMPLES:
        s += 1
    return s


def _stain_images(img, name):
    _chk(img, torch.uint8, name)
    if img.dim() == 3:
        img = img[None]
    if img.dim() != 4 or img.shape[-1] != 3 or img.numel() == 0:
        raise _lib.WesupHipError(f'{name}: expected (H, W, 3) or (B, H, W, 3) uint8, got {tuple(img.shape)}')
    return img


def stain_fit(img, stride=None, io=STAIN_IO, alpha=STAIN_ALPHA, beta=STAIN_BETA, min_tissue=STAIN_MIN_TISSUE, blocks=None,
              return_stages=False):
    """img (B, H, W, 3) or (H, W, 3) uint8 -> (B, 16) fp32 fit blocks {HE[3][2], pinv[2][3], maxC[2], n_tissue, valid}: one chain of
    launches, nothing read back.  ``stride`` None picks stain_stride(H, W).  ``return_stages`` also returns views of the
    workspace, valid until the next stain call on this stream: moments (B, 10) fp64, eig (B, 3, 2) fp64, phi (B, n) fp32 (+inf where
    a sample is not tissue), conc (B, 2, n) fp32."""
    img = _stain_images(img, 'stain_fit: img')
    B, H, W, _ = img.shape
    stride = stain_stride(H, W) if stride is None else int(stride)
    if stride < 1 or -(-H // stride) * -(-W // stride) > STAIN_MAX_SAMPLES:
        raise _lib.WesupHipError(f'stain_fit: stride {stride} for {H} x {W} (at most 2^24 samples)')
    blocks = torch.empty(B, STAIN_BLOCK, dtype=torch.float32, device=img.device) if blocks is None else _chk(blocks, name='blocks')
    if tuple(blocks.shape) != (B, STAIN_BLOCK) or blocks.device != img.device:
        raise _lib.WesupHipError(f'stain_fit: blocks {tuple(blocks.shape)} for {B} images')
    lib = _lib.load()
    nb = lib.wesup_stain_fit_workspace_bytes(B, H, W, stride)
    ws = _stain_workspace(nb, img.device)
    _lib.call('wesup_stain_fit', _p(img), _p(blocks), B, H, W, stride, float(io), float(alpha), float(beta), int(min_tissue),
              _p(ws), nb, _stream())
    if not return_stages:
        return blocks
    n = -(-H // stride) * -(-W // stride)
    off = [lib.wesup_stain_fit_stage_offset(B, H, W, stride, s) for s in range(4)]
    stages = {
        'moments': ws[off[0]:off[0] + B * 80].view(torch.float64).view(B, 10),
        'eig': ws[off[1]:off[1] + B * 256].view(torch.float64).view(B, 32)[:, :6].reshape(B, 3, 2),
        'phi': ws[off[2]:off[2] + B * n * 4].view(torch.float32).view(B, n),
        'conc': ws[off[3]:off[3] + B * 2 * n * 4].view(torch.float32).view(B, 2, n),
    }
    return blocks, stages


def stain_apply(img, src_blocks, dst_blocks, jitter=None, keep_residual=0.0, io=STAIN_IO, out=None):
    """c = pinv_s OD;  c' = c (maxC_d / maxC_s) a + b;  OD' = HE_d c' + keep_residual (OD - HE_s c);  uint8 again.  src_blocks
    (B, 16); dst_blocks (16,) or (1, 16) for one target, (B, 16) for one each; jitter (B, 4) fp32 {a_H, b_H, a_E, b_E} or None;
    ``out`` may be ``img`` (in place).  An invalid fit on either side makes that image a copy."""
    squeeze = isinstance(img, torch.Tensor) and img.dim() == 3
    img = _stain_images(img, 'stain_apply: img')
    B, H, W, _ = img.shape
    dev = img.device
    _chk(src_blocks, name='src_blocks'); _chk(dst_blocks, name='dst_blocks')
    dst_rows = dst_blocks.numel() // STAIN_BLOCK
    if src_blocks.numel() != B * STAIN_BLOCK or dst_blocks.numel() != dst_rows * STAIN_BLOCK or dst_rows not in (1, B) \
            or src_blocks.device != dev or dst_blocks.device != dev:
        raise _lib.WesupHipError(f'stain_apply: src_blocks {tuple(src_blocks.shape)}, dst_blocks {tuple(dst_blocks.shape)} for {B} images')
    dst_stride = STAIN_BLOCK if dst_rows > 1 else 0
    if jitter is not None:
        _chk(jitter, name='jitter')
        if tuple(jitter.shape) != (B, 4) or jitter.device != dev:
            raise _lib.WesupHipError(f'stain_apply: jitter {tuple(jitter.shape)} for {B} images')
    if out is None:
        out = torch.empty_like(img)
    else:
        o4 = _stain_images(out, 'stain_apply: out')
        if o4.shape != img.shape or o4.device != dev:
            raise _lib.WesupHipError(f'stain_apply: out {tuple(out.shape)} for img {tuple(img.shape)}')
        out = o4
    _lib.call('wesup_stain_apply', _p(img), _p(out), _p(src_blocks), _p(dst_blocks), dst_stride, _p(jitter), float(keep_residual),
              B, H, W, float(io), _stream())
    return out[0] if squeeze else out


# ---------------------------------------------------------------- the inference tools' wrappers below: shared argument checks
def _out(out, shape, dtype, device, name):
    """The output of a wrapper: a new ``shape`` tensor of ``dtype`` on ``device``, or the caller's buffer, checked to be one."""
    shape = tuple(shape)
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _chk(out, dtype, 'out')
    if tuple(out.shape) != shape or out.device != device:
        raise _lib.WesupHipError(f'{name}: out {tuple(out.shape)} on {out.device}, expected {shape}')
    return out


def _image_u8(img, name):
    """(H, W) of an (H,W,3) image tensor (its dtype and device are the caller's ``_chk``: a lattice is checked first)."""
    if not isinstance(img, torch.Tensor) or img.dim() != 3 or img.shape[-1] != 3:
        raise _lib.WesupHipError(f'{name}: expected an (H,W,3) uint8 image')
    return img.shape[0], img.shape[1]


def _plane_stride(t, name):
    """The element stride of a view that is dense but for one constant step between its elements, such as ``pred[..., 1]`` of a
    (..., C) prediction, read in place by the kernels (a size-1 dimension's stride means nothing)."""
    dims = [(n, s) for n, s in zip(t.shape, t.stride()) if n > 1]
    stride = expect = dims[-1][1] if dims else 1
    for n, s in reversed(dims):
        if s != expect or stride < 1:
            raise _lib.WesupHipError(f'{name} strides {t.stride()} for shape {tuple(t.shape)}')
        expect *= n
    return stride


def _classes_of(pred, n_classes, indexed, name):
    """C of a class-map entry.  ``indexed``: pred holds class indices and ``n_classes`` says how many there are; otherwise C is
    pred's last dimension, and an ``n_classes`` given besides must agree with it."""
    if indexed and n_classes is None:
        raise _lib.WesupHipError(f'{name}: class indices need n_classes')
    C = _chk_classes(n_classes if indexed else pred.shape[-1], name)
    if n_classes is not None and int(n_classes) != C:
        raise _lib.WesupHipError(f'{name}: pred {tuple(pred.shape)} for {n_classes} classes')
    return C


# ---------------------------------------------------------------- window inference on large images (csrc/tiles.hip)
_lattice_cache = {}    # (device, axis positions) -> int32 device tensor: an image size meets the same few lattices again and again


def _lattice_axis(pos, size, p, name, device):
    """One axis of a window lattice (infer_tile.window_grid), checked on the HOST -- the kernels read it from device memory and
    cannot be asked -- and uploaded once per (device, contents): sorted, first window at 0, last one flush at ``size - p``, no
    pixel between two windows left uncovered."""
    pos = [int(v) for v in pos]
    if not pos:
        raise _lib.WesupHipError(f'window lattice: {name} is empty')
    if any(b < a for a, b in zip(pos, pos[1:])):
        raise _lib.WesupHipError(f'window lattice: {name} {pos} is not sorted')
    if pos[0] != 0 or pos[-1] != size - p:
        raise _lib.WesupHipError(f'window lattice: {name} {pos} does not run from 0 to size - p = {size - p}')
    if any(b - a > p for a, b in zip(pos, pos[1:])):
        raise _lib.WesupHipError(f'window lattice: {name} {pos} leaves pixels between windows of {p} uncovered')
    key = (str(device), tuple(pos))
    t = _lattice_cache.get(key)
    if t is None:
        if len(_lattice_cache) >= 256:
            _lattice_cache.clear()
        t = _lattice_cache[key] = torch.tensor(pos, dtype=torch.int32, device=device)
    return t


def _lattice(tops, lefts, H, W, p, device):
    p = int(p)
    if p < 1 or p > H or p > W:
        raise _lib.WesupHipError(f'window lattice: patch size {p} for an image of {H} x {W}')
    return _lattice_axis(tops, H, p, 'tops', device), _lattice_axis(lefts, W, p, 'lefts', device)


def _view_word(views, name):
    """A view list (infer_tile.VIEW_SETS: 1 .. 8 distinct indices in [0, 8), any order) -> (V, the word the entries take: four
    bits per view, the first view in the lowest bits)."""
    try:
        views = [int(v) for v in views]
    except (TypeError, ValueError):
        raise _lib.WesupHipError(f'{name}: views {views!r}') from None
    if not 1 <= len(views) <= 8 or len(set(views)) != len(views) or any(not 0 <= v < 8 for v in views):
        raise _lib.WesupHipError(f'{name}: views {views}, expected 1 .. 8 distinct indices in [0, 8)')
    return len(views), sum(v << (4 * t) for t, v in enumerate(views))


def _views_tail(views, name):
    """``views=`` of the window entries -> (V, the ``n_views, views`` arguments of the ``_views`` entry).  ``None``
    is (1, ()): the plain entry, the same kernel under the one upright view, whose buffers have no V axis."""
    if views is None:
        return 1, ()
    V, word = _view_word(views, name)
    return V, (V, word)


def window_gather(img_u8_hwc, tops, lefts, p, first, count, out=None, views=None):
    """Network input windows of an image on the device: img (H,W,3) uint8, the lattice ``tops`` x ``lefts`` of
    infer_tile.window_grid (host integer sequences; checked here, their device copies are cached) -> (count,3,p,p) fp32 in
    [0, 1], the row-major windows ``first .. first + count - 1``, bit-equal to infer_tile._to_tensor.  Indices past the last
    window repeat it (the padding of a ragged final batch).

    ``views`` (a view list, V of them): the slots of windows x views instead -- slot ``s`` is window ``s // V`` under view
    ``views[s % V]`` (infer_tile.apply_view), each bit-equal to ``_to_tensor(apply_view(window, v))``; slots past the last one
    repeat it."""
    H, W = _image_u8(img_u8_hwc, 'window_gather')
    first, count, p = int(first), int(count), int(p)
    if first < 0 or count < 1:
        raise _lib.WesupHipError(f'window_gather: {"windows" if views is None else "slots"} [{first}, {first} + {count})')
    V, tail = _views_tail(views, 'window_gather')
    tops_d, lefts_d = _lattice(tops, lefts, H, W, p, img_u8_hwc.device)
    _chk(img_u8_hwc, torch.uint8, 'img')
    out = _out(out, (count, 3, p, p), torch.float32, img_u8_hwc.device, 'window_gather')
    if out.data_ptr() % 16:
        raise _lib.WesupHipError('window_gather: out is not 16-byte aligned')
    tok = _tbegin('window_gather')
    _lib.call('wesup_window_gather_views' if tail else 'wesup_window_gather', _p(img_u8_hwc), _p(tops_d), _p(lefts_d), _p(out), H, W,
              tops_d.numel(), lefts_d.numel(), p, *tail, first, count, _stream())
    _tend(tok, 15.0 * count * p * p)                  # 3 bytes in, 3 floats out per window pixel
    return out


def _window_preds(pred, views, tops, lefts, H, W, tail_dims, name, classes=None):
    """What the window merges share, in the order the checks have always had: pred (N,p,p,...) -- (N,V,p,p,...) under ``views`` --
    with ``tail_dims`` allowed numbers of dimensions behind p x p, for ALL N = len(tops) * len(lefts) windows of the lattice ->
    (N, V, p, C, the entry's view arguments, the lattice on the device).  C is pred's last dimension (1 without one), or with
    ``classes = (n_classes, indexed)`` what ``_classes_of`` makes of it.  ``pred``'s own dtype, device and layout are the caller's
    ``_chk``: the lattice is checked first."""
    lead = 1 if views is None else 2
    if not isinstance(pred, torch.Tensor) or pred.dim() - lead - 2 not in tail_dims:
        shapes = ' or '.join('(N,p,p' + ',C' * d + ')' for d in tail_dims)
        raise _lib.WesupHipError(f'{name}: expected {shapes} predictions, with V behind N under views')
    C = 1 if pred.dim() == lead + 2 else pred.shape[-1]
    if classes is not None:
        C = _classes_of(pred, *classes, name)
    V, tail = _views_tail(views, name)
    N, (p, p2) = pred.shape[0], pred.shape[lead:lead + 2]
    if p != p2 or C < 1 or (tail and pred.shape[1] != V):
        raise _lib.WesupHipError(f'{name}: pred {tuple(pred.shape)}' + (f' for {V} views' if tail else ''))
    tops_d, lefts_d = _lattice(tops, lefts, int(H), int(W), p, pred.device)
    if N != tops_d.numel() * lefts_d.numel():
        raise _lib.WesupHipError(f'{name}: {N} windows for a lattice of {tops_d.numel()} x {lefts_d.numel()}')
    return N, V, p, C, tail, tops_d, lefts_d


def window_merge(pred, tops, lefts, H, W, round_first=False, out=None, views=None):
    """Mean over the covering windows: pred (N,p,p,C) or (N,p,p) fp32 for ALL N = len(tops) * len(lefts) windows of one image
    (row-major) -> (H,W,C) / (H,W) fp64, equal to infer_tile.combine_patches_to_image bit for bit; ``round_first`` rounds
    every value half to even before it is added (torch.round / np.round of the per-window path).

    ``views`` (a view list, V of them): the mean over the covering windows and their views -- pred (N,V,p,p,C) or (N,V,p,p), every
    prediction in the space of its view -- equal to infer_tile.combine_views_to_image bit for bit."""
    N, V, p, C, tail, tops_d, lefts_d = _window_preds(pred, views, tops, lefts, H, W, (0, 1), 'window_merge')
    flat = pred.dim() == (4 if tail else 3)
    H, W = int(H), int(W)
    _chk(pred, name='pred')
    out = _out(out, (H, W) if flat else (H, W, C), torch.float64, pred.device, 'window_merge')
    tok = _tbegin('window_merge')
    _lib.call('wesup_window_merge_views' if tail else 'wesup_window_merge', _p(pred), _p(tops_d), _p(lefts_d), _p(out), H, W, C,
              tops_d.numel(), lefts_d.numel(), p, *tail, int(bool(round_first)), _stream())
    _tend(tok, 4.0 * N * V * p * p * C + 8.0 * H * W * C)
    return out


# ``views=`` as a positional argument, the spelling before the keyword: forwarded, nothing of their own.
def window_gather_views(img_u8_hwc, tops, lefts, p, views, first, count, out=None):
    return window_gather(img_u8_hwc, tops, lefts, p, first, count, out=out, views=views)


def window_merge_views(pred, views, tops, lefts, H, W, round_first=False, out=None):
    return window_merge(pred, tops, lefts, H, W, round_first=round_first, out=out, views=views)


def window_merge_classes_views(pred, views, tops, lefts, H, W, n_classes=None, votes=False, out=None, status=None):
    return window_merge_classes(pred, tops, lefts, H, W, n_classes=n_classes, votes=votes, out=out, status=status, views=views)


# ---------------------------------------------------------------- whole-image multi-scale pixel inference (csrc/pixel.hip)
def image_resize_u8(img_u8_hwc, h, w, out=None):
    """to_tensor + F.interpolate(mode='bilinear', align_corners=True) of pixel_infer.py:40,46 in one pass: img (H,W,3) uint8 on
    the device -> (1,3,h,w) fp32, ``img / 255.f`` resampled (at the image's own size: ``img / 255.f`` bit for bit)."""
    H, W = _image_u8(img_u8_hwc, 'image_resize_u8')
    _chk(img_u8_hwc, torch.uint8, 'img')
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise _lib.WesupHipError(f'image_resize_u8: target size {h} x {w}')
    out = _out(out, (1, 3, h, w), torch.float32, img_u8_hwc.device, 'image_resize_u8')
    _lib.call('wesup_image_resize_u8', _p(img_u8_hwc), _p(out), H, W, h, w, _stream())
    return out


def plane_resize_acc(src, out, alpha=1.0, accumulate=False):
    """out (H,W) = (accumulate ? out : 0) + alpha * bilinear_ac(src); src is an (h,w) fp32 plane, contiguous or a view with an
    element stride such as ``pred[..., 1]`` of an (h,w,C) prediction (read in place)."""
    _chk(out, name='out')
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != torch.float32 or src.dim() != 2 or out.dim() != 2:
        raise _lib.WesupHipError('plane_resize_acc: expected 2-D float32 CUDA/HIP planes')
    h, w = src.shape
    stride = _plane_stride(src, 'plane_resize_acc: src')
    if src.device != out.device:
        raise _lib.WesupHipError(f'plane_resize_acc: src on {src.device}, out on {out.device}')
    H, W = out.shape
    _lib.call('wesup_plane_resize_acc', _p(src), _p(out), h, w, H, W, stride, float(alpha), int(bool(accumulate)), _stream())
    return out


def pixel_gather_fwd(p0, bias, coarse=(), out=None):
    """out (B,H,W,N) = ReLU(bias + p0 + sum_r bilinear_ac(coarse[r])): the first fc layer of the pixel head from its
    per-resolution products p0 (B,H,W,N) and up to four coarse maps (B,h_r,w_r,N), each interpolated straight to (H,W).
    out=None works in place on p0."""
    _chk(p0, name='p0'); _chk(bias, name='bias')
    B, H, W, N = p0.shape
    if out is None:
        out = p0
    _chk(out, name='out')
    if out.shape != p0.shape or bias.numel() != N or N % 4 or len(coarse) > 4:
        raise _lib.WesupHipError(f'pixel_gather_fwd: p0 {tuple(p0.shape)}, out {tuple(out.shape)}, bias {bias.numel()}, {len(coarse)} levels')
    levels = (_lib.CoarseMap * max(len(coarse), 1))()
    for r, c in enumerate(coarse):
        _chk(c, name=f'coarse[{r}]')
        if c.dim() != 4 or c.shape[0] != B or c.shape[3] != N or c.device != p0.device:
            raise _lib.WesupHipError(f'pixel_gather_fwd: coarse[{r}] {tuple(c.shape)} under p0 {tuple(p0.shape)}')
        levels[r].p, levels[r].h, levels[r].w = c.data_ptr(), c.shape[1], c.shape[2]
    _lib.call('wesup_pixel_gather_fwd', _p(p0), _p(bias), _p(out), levels, len(coarse), B, H, W, N, _stream())
    return out


# ---------------------------------------------------------------- whole-slide evaluation: the DP2019 patch pipeline (csrc/slide.hip)
def _patch_lattice(H, W, p, first, count, name):
    H, W, p, first, count = int(H), int(W), int(p), int(first), int(count)
    if H < 1 or W < 1 or p < 1 or max(H, W, p) > 1 << 30:
        raise _lib.WesupHipError(f'{name}: patch size {p} for a slide of {H} x {W}')
    if first < 0 or count < 1:
        raise _lib.WesupHipError(f'{name}: patches [{first}, {first} + {count})')
    return H, W, p, first, count


def _patch_list(patch_list, device, name):
    """The ``(pointer, length)`` tail of a ``*_list`` entry: a non-empty 1-d int32 tensor of patch indices on ``device``
    (``tissue_select``'s list, cut to its ``n_keep``).  Its values are the kernels' to check: they never become addresses."""
    _chk(patch_list, torch.int32, 'patch_list')
    if patch_list.dim() != 1 or patch_list.numel() < 1 or patch_list.device != device:
        raise _lib.WesupHipError(f'{name}: patch_list {tuple(patch_list.shape)} on {patch_list.device}, expected a non-empty 1-d '
                                 f'int32 tensor on {device}')
    return _p(patch_list), patch_list.numel()


def patch_gather_resize(img_u8_hwc, p, h, w, first, count, align_corners=False, out=None, patch_list=None):
    """Network inputs for the patches of a slide on the device: img (H,W,3) uint8 -> (count,3,h,w) fp32, the zero-padded
    ``p`` x ``p`` patches ``first .. first + count - 1`` of the ``ceil(H / p)`` x ``ceil(W / p)`` lattice (row-major), each
    ``patch / 255.f`` resized bilinearly to (h, w): ``F.interpolate(mode='bilinear')`` of infer.py, or with ``align_corners`` the
    resize of pixel_infer.py (ops.image_resize_u8 of the patch, bit for bit, where the patch lies inside the slide).  Indices
    past the last patch repeat it (the padding of a ragged final batch).  ``out``: a buffer reused across passes.

    ``patch_list`` (int32 device tensor): slot ``i`` is patch ``patch_list[min(first + i, len - 1)]`` -- a ragged
    last pass repeats the last listed patch; a listed patch gets the bits it gets without a list."""
    H, W = _image_u8(img_u8_hwc, 'patch_gather_resize')
    _chk(img_u8_hwc, torch.uint8, 'img')
    H, W, p, first, count = _patch_lattice(H, W, p, first, count, 'patch_gather_resize')
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise _lib.WesupHipError(f'patch_gather_resize: target size {h} x {w}')
    out = _out(out, (count, 3, h, w), torch.float32, img_u8_hwc.device, 'patch_gather_resize')
    tail = () if patch_list is None else _patch_list(patch_list, img_u8_hwc.device, 'patch_gather_resize')
    tok = _tbegin('patch_gather_resize')
    _lib.call('wesup_patch_gather_resize_list' if tail else 'wesup_patch_gather_resize', _p(img_u8_hwc), _p(out), H, W, p, h, w,
              int(bool(align_corners)), first, count, *tail, _stream())
    _tend(tok, 12.0 * count * h * w)
    return out


def patch_scatter_u8(pred, out, p, first, mode=0, patch_list=None):
    """Paste patch predictions into the slide-size map: pred (count,h,w) fp32 -- contiguous, or a view with an element stride
    such as ``probs[..., 1]`` of a (count,h,w,C) prediction, read in place -- for the patches ``first .. first + count - 1``;
    out (H,W) uint8.  Every slide pixel inside those patches becomes ``255 * round(v)`` (half to even), ``v`` the prediction
    resized to ``p`` x ``p``: ``mode`` 0 nearest (infer.py), 1 bilinear with align_corners (pixel_infer.py at one scale).  The
    rest of ``out`` is left as it is; the lattice's padding beyond the slide is never written.

    ``patch_list``: slot ``i`` pastes patch ``patch_list[first + i]``; a slot at or beyond the list's end, or a value outside the
    lattice, pastes nothing."""
    _chk(out, torch.uint8, 'out')
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda or pred.dtype != torch.float32 or pred.dim() != 3 or out.dim() != 2:
        raise _lib.WesupHipError('patch_scatter_u8: expected (count,h,w) float32 CUDA/HIP predictions and an (H,W) uint8 map')
    if mode not in (0, 1):
        raise _lib.WesupHipError(f'patch_scatter_u8: mode {mode}')
    count, h, w = pred.shape
    H, W, p, first, count = _patch_lattice(out.shape[0], out.shape[1], p, first, count, 'patch_scatter_u8')
    if h < 1 or w < 1:
        raise _lib.WesupHipError(f'patch_scatter_u8: pred {tuple(pred.shape)}')
    stride = _plane_stride(pred, 'patch_scatter_u8: pred')
    if pred.device != out.device:
        raise _lib.WesupHipError(f'patch_scatter_u8: pred on {pred.device}, out on {out.device}')
    tail = () if patch_list is None else _patch_list(patch_list, out.device, 'patch_scatter_u8')
    tok = _tbegin('patch_scatter_u8')
    _lib.call('wesup_patch_scatter_u8_list' if tail else 'wesup_patch_scatter_u8', _p(pred), _p(out), H, W, p, h, w, stride,
              int(mode), first, count, *tail, _stream())
    _tend(tok, 4.0 * count * h * w + 1.0 * count * p * p)
    return out


# ---------------------------------------------------------------- tissue selection for whole-slide evaluation (csrc/tissue.hip)
TISSUE_CHANNELS = ('luma', 'chroma')


def _tissue_channel(channel, name):
    if channel not in TISSUE_CHANNELS:
        raise _lib.WesupHipError(f'{name}: channel {channel!r}, expected one of {TISSUE_CHANNELS}')
    return TISSUE_CHANNELS.index(channel)


def _tissue_lattice(H, W, p, name):
    """(H, W, p, n) of the tissue entries: the patch lattice with p <= 65535 (a cell of a histogram is a uint32) and at most
    2^32 pixels (Otsu's integers stay below 2^64)."""
    H, W, p, _, _ = _patch_lattice(H, W, p, 0, 1, name)
    if p > 65535 or H * W > 1 << 32:
        raise _lib.WesupHipError(f'{name}: patch size {p} for a slide of {H} x {W} (p <= 65535, H * W <= 2^32)')
    return H, W, p, -(-H // p) * -(-W // p)


def patch_value_hist(img_u8_hwc, p, channel='luma', out=None):
    """Per-patch histograms of a pixel value in one read of the resident slide: img (H,W,3) uint8 -> (n,256) int32 holding
    uint32 counts (torch has no arithmetic on uint32: read them as ``.cpu().numpy().view(numpy.uint32)``; below 2^31 for
    p <= 46340), ``hist[k][v]`` = the slide pixels of patch ``k`` of the ``ceil(H / p)`` x ``ceil(W / p)`` lattice whose value is
    ``v``: ``luma`` (77 R + 150 G + 29 B + 128) >> 8, ``chroma`` max - min (slide.pixel_value).  The zero padding is never
    counted.  Equal to ``slide.patch_histograms`` exactly."""
    H, W = _image_u8(img_u8_hwc, 'patch_value_hist')
    _chk(img_u8_hwc, torch.uint8, 'img')
    ch = _tissue_channel(channel, 'patch_value_hist')
    H, W, p, n = _tissue_lattice(H, W, p, 'patch_value_hist')
    out = _out(out, (n, 256), torch.int32, img_u8_hwc.device, 'patch_value_hist')
    tok = _tbegin('patch_value_hist')
    _lib.call('wesup_patch_value_hist', _p(img_u8_hwc), _p(out), H, W, p, ch, _stream())
    _tend(tok, 3.0 * H * W + 1024.0 * n)
    return out


def tissue_select(hist, H, W, p, channel='luma', threshold=-1, min_ppm=10000):
    """The rest of the selection from ``patch_value_hist``'s histograms, without a read-back: returns the device tensors
    ``(info, total, counts, list)``.  ``total`` (256,) int64 the summed histogram; ``t`` = ``threshold`` (0 .. 254), or Otsu's
    over ``total`` with ``threshold=-1`` (slide.otsu_threshold: -1 for a one-level slide); ``counts`` (n,) int32 (uint32 bits)
    the tissue pixels per patch; ``list`` (n,) int32 with the kept patches in ascending order in its first ``n_keep`` places
    (slide.select_patches; the rest is not written); ``info`` (8,) int32 = ``{t, n_keep, n, flat, 0, 0, 0, 0}``."""
    _chk(hist, torch.int32, 'hist')
    ch = _tissue_channel(channel, 'tissue_select')
    H, W, p, n = _tissue_lattice(H, W, p, 'tissue_select')
    threshold, min_ppm = int(threshold), int(min_ppm)
    if tuple(hist.shape) != (n, 256):
        raise _lib.WesupHipError(f'tissue_select: hist {tuple(hist.shape)}, expected {(n, 256)}')
    if not -1 <= threshold <= 254 or not 0 <= min_ppm <= 1000000:
        raise _lib.WesupHipError(f'tissue_select: threshold {threshold} (-1 .. 254), min_ppm {min_ppm} (0 .. 10^6)')
    dev = hist.device
    info = torch.empty(8, dtype=torch.int32, device=dev)
    total = torch.empty(256, dtype=torch.int64, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    plist = torch.empty(n, dtype=torch.int32, device=dev)
    tok = _tbegin('tissue_select')
    _lib.call('wesup_tissue_select', _p(hist), H, W, p, ch, threshold, min_ppm, _p(info), _p(total), _p(counts), _p(plist), _stream())
    _tend(tok, 2.0 * 1024.0 * n + 12.0 * n)
    return info, total, counts, plist


def tissue_mask(img_u8_hwc, info, channel='luma', out=None):
    """The tissue mask of a slide under ``tissue_select``'s threshold, read from ``info`` on the device: (H,W) uint8, 255 where
    the pixel is tissue (``luma`` v <= t, ``chroma`` v > t, t = -1 everywhere), 0 elsewhere."""
    H, W = _image_u8(img_u8_hwc, 'tissue_mask')
    _chk(img_u8_hwc, torch.uint8, 'img'); _chk(info, torch.int32, 'info')
    ch = _tissue_channel(channel, 'tissue_mask')
    if info.numel() != 8 or info.device != img_u8_hwc.device or H < 1 or W < 1 or max(H, W) > 1 << 30:
        raise _lib.WesupHipError(f'tissue_mask: info {tuple(info.shape)} on {info.device} for a slide of {H} x {W}')
    out = _out(out, (H, W), torch.uint8, img_u8_hwc.device, 'tissue_mask')
    tok = _tbegin('tissue_mask')
    _lib.call('wesup_tissue_mask_u8', _p(img_u8_hwc), _p(info), _p(out), H, W, ch, _stream())
    _tend(tok, 4.0 * H * W)
    return out


def mask_scores(S, G, negative=False, out=None):
    """The pixel counts behind overall accuracy and Dice of two uint8 maps of one shape: (4,) int64 on the device,
    ``{#(s == g), #(s > 0 and g > 0), #(s > 0), #(g > 0)}``, after ``x -> 255 - x`` on both with ``negative``
    (compute_metrics(negative=True) of the reference).  ``out``: a (4,) int64 buffer to reuse."""
    _chk(S, torch.uint8, 'S'); _chk(G, torch.uint8, 'G')
    if S.shape != G.shape or S.numel() < 1 or S.device != G.device:
        raise _lib.WesupHipError(f'mask_scores: maps {tuple(S.shape)} and {tuple(G.shape)}')
    out = _out(out, (4,), torch.int64, S.device, 'mask_scores')
    tok = _tbegin('mask_scores')
    _lib.call('wesup_mask_scores', _p(S), _p(G), _p(out), S.numel(), int(bool(negative)), _stream())
    _tend(tok, 2.0 * S.numel())
    return out


# ---------------------------------------------------------------- class maps for more than two classes (csrc/classmap.hip)
def _chk_classes(C, name):
    C = int(C)
    if not 2 <= C <= _lib.MAX_CLASSES:
        raise _lib.WesupHipError(f'{name}: {C} classes, expected 2 .. {_lib.MAX_CLASSES}')
    return C


def _status(status, device, name):
    """The (1,) int32 status word of an entry: the caller's, or a new zeroed one."""
    if status is None:
        return torch.zeros(1, dtype=torch.int32, device=device)
    _chk(status, torch.int32, 'status')
    if status.numel() != 1 or status.device != device:
        raise _lib.WesupHipError(f'{name}: status {tuple(status.shape)} on {status.device}, expected one int32 on {device}')
    return status


def window_merge_classes(pred, tops, lefts, H, W, n_classes=None, votes=False, out=None, status=None, views=None):
    """The class map of a window-merged prediction for ALL N = len(tops) * len(lefts) windows of one image (row-major) ->
    (out (H,W) uint8 class indices, status (1,) int32), equal to infer_tile.combine_patches_to_classes bit for bit.
    ``votes=False``: pred (N,p,p,C) fp32 probabilities; per class the fp64 mean over the covering windows of ``window_merge``,
    then the first maximum.  ``votes=True``: pred (N,p,p) fp32 class indices (what the superpixel model paints for C > 2) and
    ``n_classes``; every covering window votes and the first maximum of the counts wins.  A vote outside [0, C) is not counted
    and sets ``status`` (zeroed by the entry).

    ``views`` (a view list, V of them): over windows x views -- pred (N,V,p,p,C) or, with votes, (N,V,p,p), every prediction in the
    space of its view; every (window, view) votes -- equal to infer_tile.combine_views_to_classes bit for bit."""
    votes = bool(votes)
    N, V, p, C, tail, tops_d, lefts_d = _window_preds(pred, views, tops, lefts, H, W, (0,) if votes else (1,), 'window_merge_classes',
                                                      classes=(n_classes, votes))
    H, W = int(H), int(W)
    _chk(pred, name='pred')
    out = _out(out, (H, W), torch.uint8, pred.device, 'window_merge_classes')
    status = _status(status, pred.device, 'window_merge_classes')
    tok = _tbegin('window_merge_classes')
    _lib.call('wesup_window_merge_classes_views' if tail else 'wesup_window_merge_classes', _p(pred), _p(tops_d), _p(lefts_d), _p(out),
              _p(status), H, W, C, tops_d.numel(), lefts_d.numel(), p, *tail, int(votes), _stream())
    _tend(tok, 4.0 * N * V * p * p * (1 if votes else C) + 1.0 * H * W)
    return out, status


def planes_resize_acc(src, out, alpha=1.0, accumulate=False):
    """out (H,W,C) = (accumulate ? out : 0) + alpha * bilinear_ac(src) for an (h,w,C) fp32 prediction, all C planes in one pass:
    every plane equals ``plane_resize_acc(src[..., c], out[..., c])`` bit for bit."""
    _chk(src, name='src'); _chk(out, name='out')
    if src.dim() != 3 or out.dim() != 3 or src.shape[2] != out.shape[2] or src.device != out.device:
        raise _lib.WesupHipError(f'planes_resize_acc: src {tuple(src.shape)}, out {tuple(out.shape)}: expected (h,w,C) and (H,W,C)')
    h, w, C = src.shape
    C = _chk_classes(C, 'planes_resize_acc')
    H, W = out.shape[:2]
    if min(h, w, H, W) < 1:
        raise _lib.WesupHipError(f'planes_resize_acc: src {tuple(src.shape)}, out {tuple(out.shape)}')
    tok = _tbegin('planes_resize_acc')
    _lib.call('wesup_planes_resize_acc', _p(src), _p(out), h, w, H, W, C, float(alpha), int(bool(accumulate)), _stream())
    _tend(tok, 4.0 * C * (h * w + (2 if accumulate else 1) * H * W))
    return out


def class_argmax_u8(src, out=None):
    """src (..., C) fp32 -> (...) uint8: the first maximum of every row of C values (np.argmax on data without NaNs)."""
    _chk(src, name='src')
    if src.dim() < 2 or src.numel() < 1:
        raise _lib.WesupHipError(f'class_argmax_u8: src {tuple(src.shape)}: expected (..., C)')
    C = _chk_classes(src.shape[-1], 'class_argmax_u8')
    out = _out(out, src.shape[:-1], torch.uint8, src.device, 'class_argmax_u8')
    n = src.numel() // C
    tok = _tbegin('class_argmax_u8')
    _lib.call('wesup_class_argmax_u8', _p(src), _p(out), n, C, _stream())
    _tend(tok, (4.0 * C + 1.0) * n)
    return out


def patch_scatter_classes_u8(pred, out, p, first, n_classes=None, mode=0, status=None, patch_list=None):
    """``patch_scatter_u8`` for class maps: pastes a class index per slide pixel of the patches ``first .. first + count - 1`` into
    out (H,W) uint8 -- the same lattice, the same crop, the rest of ``out`` left as it is.  ``mode`` 0: pred (count,h,w) fp32
    class indices (the superpixel model's painted map) and ``n_classes``, nearest resize; an index outside [0, C) pastes 0 and
    sets ``status``.  ``mode`` 1: pred (count,h,w,C) fp32 probabilities; per class the bilinear align_corners value of
    ``planes_resize_acc(alpha=1)``, then the first maximum.  ``status`` (1,) int32 is OR-ed into, so that one word serves all the
    passes of a slide; a new zeroed one is made when none is given.  Returns (out, status).  ``patch_list``: as in
    ``patch_scatter_u8``; a list value outside the lattice sets ``status`` too."""
    _chk(out, torch.uint8, 'out'); _chk(pred, name='pred')
    if mode not in (0, 1):
        raise _lib.WesupHipError(f'patch_scatter_classes_u8: mode {mode}')
    if pred.dim() != (3 if mode == 0 else 4) or out.dim() != 2 or pred.device != out.device:
        raise _lib.WesupHipError('patch_scatter_classes_u8: expected (count,h,w) class indices (mode 0) or (count,h,w,C) '
                                 'probabilities (mode 1) and an (H,W) uint8 map on one device')
    C = _classes_of(pred, n_classes, mode == 0, 'patch_scatter_classes_u8')
    count, h, w = pred.shape[:3]
    H, W, p, first, count = _patch_lattice(out.shape[0], out.shape[1], p, first, count, 'patch_scatter_classes_u8')
    if h < 1 or w < 1:
        raise _lib.WesupHipError(f'patch_scatter_classes_u8: pred {tuple(pred.shape)}')
    status = _status(status, out.device, 'patch_scatter_classes_u8')
    tail = () if patch_list is None else _patch_list(patch_list, out.device, 'patch_scatter_classes_u8')
    tok = _tbegin('patch_scatter_classes_u8')
    _lib.call('wesup_patch_scatter_classes_u8_list' if tail else 'wesup_patch_scatter_classes_u8', _p(pred), _p(out), _p(status),
              H, W, p, h, w, C, int(mode), first, count, *tail, _stream())
    _tend(tok, 4.0 * count * h * w * (C if mode else 1) + 1.0 * count * p * p)
    return out, status


def label_confusion(S, G, n_classes, out=None, status=None):
    """The confusion table of two uint8 class-index maps of one shape: (conf (C,C) int64, status (1,) int32) on the device,
    ``conf[g][s]`` = pixels of ground-truth class g predicted as s (utils.metrics.confusion); a byte >= C is not counted and sets
    ``status``.  Both are zeroed by the entry."""
    _chk(S, torch.uint8, 'S'); _chk(G, torch.uint8, 'G')
    C = _chk_classes(n_classes, 'label_confusion')
    if S.shape != G.shape or S.numel() < 1 or S.device != G.device:
        raise _lib.WesupHipError(f'label_confusion: maps {tuple(S.shape)} and {tuple(G.shape)}')
    out = _out(out, (C, C), torch.int64, S.device, 'label_confusion')
    status = _status(status, S.device, 'label_confusion')
    tok = _tbegin('label_confusion')
    _lib.call('wesup_label_confusion', _p(S), _p(G), _p(out), _p(status), S.numel(), C, _stream())
    _tend(tok, 2.0 * S.numel())
    return out, status


# ---------------------------------------------------------------- weak-label preparation (csrc/prepare.hip)
LABEL_STATS_MAX_LABELS = 1 << 26     # labels 0 .. L with L below this
SP_VOTE_MAX_PIXELS = ((1 << 32) - 1) // 255      # 32-bit sums of uint8 values


def prepare_lds_entries():
    """(labels of label_stats, ids of sp_vote) up to which a block keeps its table in LDS; above, the adds go to global memory."""
    lib = _lib.load()
    return lib.wesup_prepare_lds_entries(0), lib.wesup_prepare_lds_entries(1)


def _labels3(labels, name):
    _chk(labels, torch.int32, 'labels')
    if labels.dim() not in (2, 3) or labels.numel() < 1:
        raise _lib.WesupHipError(f'{name}: expected (H,W) or (B,H,W), got {tuple(labels.shape)}')
    return (labels.unsqueeze(0), True) if labels.dim() == 2 else (labels, False)


def label_stats(labels, L):
    """labels (H,W) / (B,H,W) int32 in [0, L] -> (stats (B, L+1, 3) int64 = pixels, sum of row indexes, sum of column indexes per
    label (the batch axis only for batched input); status (B,) int32, bit 0 set for a label outside [0, L])."""
    lab, squeeze = _labels3(labels, 'label_stats')
    B, H, W = lab.shape
    L = int(L)
    if L < 0 or L >= LABEL_STATS_MAX_LABELS:
        raise _lib.WesupHipError(f'label_stats: {L} labels (below {LABEL_STATS_MAX_LABELS})')
    stats = torch.empty(B, L + 1, 3, dtype=torch.int64, device=lab.device)
    status = torch.empty(B, dtype=torch.int32, device=lab.device)
    tok = _tbegin('label_stats')
    _lib.call('wesup_label_stats', _p(lab), _p(stats), _p(status), B, H, W, L, _stream())
    _tend(tok, 4.0 * lab.numel())
    return (stats[0] if squeeze else stats), status


def sp_vote(labels, values, K, paint=True):
    """Every superpixel of labels (H,W) / (B,H,W) int32 in [0, K) votes the rounded mean (half to even) of its pixels of values
    (uint8, same shape) -> (painted uint8 of the same shape or None without ``paint``; agree (B,) int64, the pixels whose painted
    value equals their own; status (B,) int32, bit 0 set for a label outside [0, K))."""
    lab, squeeze = _labels3(labels, 'sp_vote')
    _chk(values, torch.uint8, 'values')
    if values.shape != labels.shape or values.device != labels.device:
        raise _lib.WesupHipError(f'sp_vote: labels {tuple(labels.shape)} and values {tuple(values.shape)}')
    B, H, W = lab.shape
    K = int(K)
    if K < 1 or K > LABEL_STATS_MAX_LABELS or H * W > SP_VOTE_MAX_PIXELS:
        raise _lib.WesupHipError(f'sp_vote: K = {K}, {H} x {W} pixels (K in [1, 2^26], at most {SP_VOTE_MAX_PIXELS} pixels)')
    painted = torch.empty(B, H, W, dtype=torch.uint8, device=lab.device) if paint else None
    agree = torch.empty(B, dtype=torch.int64, device=lab.device)
    status = torch.empty(B, dtype=torch.int32, device=lab.device)
    nb = _lib.load().wesup_sp_vote_workspace_bytes(B, H, W, K)
    ws = workspace(nb, lab.device, 'prepare')
    tok = _tbegin('sp_vote')
    _lib.call('wesup_sp_vote', _p(lab), _p(values), _p(painted), _p(agree), _p(status), B, H, W, K, _p(ws), nb, _stream())
    _tend(tok, 11.0 * lab.numel())
    if paint and squeeze:
        painted = painted[0]
    return painted, agree, status


def spl_paint(labels, points, K, n_classes=2):
    """labels (H,W) int32 in [0, K), points (P,3) int32 rows of (row, col, class) inside the image and the classes -> (out (H,W,C)
    uint8, 1 where a point of class c lies in the pixel's superpixel; status (1,) int32: bit 0 a label outside [0, K), bit 1 a
    point outside the image or the classes)."""
    _chk(labels, torch.int32, 'labels')
    _chk(points, torch.int32, 'points')
    if labels.dim() != 2 or labels.numel() < 1 or points.dim() != 2 or points.shape[1] != 3 or points.device != labels.device:
        raise _lib.WesupHipError(f'spl_paint: labels {tuple(labels.shape)}, points {tuple(points.shape)}')
    H, W = labels.shape
    K, C, P = int(K), int(n_classes), points.shape[0]
    if K < 1 or C < 1 or C > 256 or K * C > LABEL_STATS_MAX_LABELS:
        raise _lib.WesupHipError(f'spl_paint: K = {K}, {C} classes')
    out = torch.empty(H, W, C, dtype=torch.uint8, device=labels.device)
    status = torch.empty(1, dtype=torch.int32, device=labels.device)
    nb = _lib.load().wesup_spl_paint_workspace_bytes(K, C)
    ws = workspace(nb, labels.device, 'prepare')
    _lib.call('wesup_spl_paint', _p(labels), _p(points) if P else None, _p(out), _p(status), H, W, K, C, P, _p(ws), nb, _stream())
    return out, status
