"""Every route of the direct 3x3 convolutions of csrc/gemm.hip (gemm_nt_kernel<MODE 1/2> through conv_common, gemm_tn_kernel<MODE 1/2>
through wesup_conv3x3_wgrad) at its borders, tiles and splits: the rows of tests/_convcases.py (what route a row reaches is
tests/test_conv_routes_cpu.py's business), through the C ABI, each row in the two passes of tests/test_gemm_routes_gpu.py:

  int    x, w, bias, dy, mask, the old output, side weights and side bias are integers of {-3 .. 3}: every partial sum is an
         integer below 2^24 (asserted per row), so every fp32 sum is exact whatever the tiling, the split or the stream-K cut, and
         the output has to EQUAL the float64 reference.  A lost border pixel, tap or K-step is a count and a box of wrong elements.
  gauss  Gaussian data, |got - ref64| <= gamma(n) (|x| * |w| + |bias| + |old|) per element, the absolute-value convolution
         computed in float64: n = 9 Cin + 2 forward / dgrad, n = B H W + 2 for the weight gradient (_gemmcases' TN family).

References: F.conv2d, F.conv_transpose2d and autograd of F.conv2d in float64 on the CPU.
Epilogue order (include/wesup_hip.h): ReLU on load, bias, mask > 0, + old content (accumulate); y_relu = max(y, 0).

In both passes every operand and output is a view inside a NaN-filled allocation of the test's own, with at least (W + 2) C NaN
floats in front of and behind x, dy and mask_src: the conv descriptor starts (W + 1) Cin floats early, so a border tap that is
wrongly live poisons the result instead of reading outside the allocation.  The outputs' surroundings are a NaN sentinel whose
bits must survive, and a second call must give the same bits."""
import pytest
import torch
import torch.nn.functional as F

import _convcases as c
import _gemmcases as g
from test_gemm_routes_gpu import ERR_INVALID, ERR_WORKSPACE, PASSES, Pad, check, data, gamma, where_wrong
from test_kernels_gpu import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope='module')
def stream():
    from wesup_amd import ops
    return ops._stream


def dense(n, halo=8):
    """n contiguous floats (n % 4 == 0) as a Pad view with at least `halo` NaN floats on either side."""
    halo = g.align_up(halo, 4)
    assert n % 4 == 0
    return Pad(1, 1, n, n + 2 * halo, col_off=halo, extra=0)


def nhwc(t):
    """(B, C, H, W) -> (1, B H W, C)"""
    return t.permute(0, 2, 3, 1).reshape(1, -1, t.shape[1])


def relu_bits(t):
    """max(t, 0) as the kernels' epilogue takes it (x < 0 ? 0 : x), as bits"""
    return torch.where(t < 0, torch.zeros((), device=t.device), t).contiguous().view(torch.int32)


# ---------------------------------------------------------------- the layouts of include/wesup_hip.h, by their index formulas
def pack_fwd_host(w):
    """w_fwd [Co][Kf]: k = ((ci / 32) * 9 + kh * 3 + kw) * 32 + ci % 32 for Ci >= 32; image layer: k = (kh * 3 + kw) * 4 + ci"""
    Co, Ci = w.shape[:2]
    out = torch.zeros(Co, c.conv_kpad(Ci), dtype=w.dtype)
    ci, t = torch.arange(Ci)[:, None], torch.arange(9)[None, :]
    k = ((ci // 32) * 9 + t) * 32 + ci % 32 if Ci >= 32 else t * 4 + ci
    out[:, k.reshape(-1)] = w.reshape(Co, Ci * 9)
    return out


def pack_dgrad_host(w):
    """w_dgrad [Ci][9 Co]: k = ((co / 32) * 9 + (2 - kh) * 3 + (2 - kw)) * 32 + co % 32"""
    Co, Ci = w.shape[:2]
    out = torch.zeros(Ci, 9 * Co, dtype=w.dtype)
    co, kh, kw = torch.arange(Co)[:, None, None], torch.arange(3)[None, :, None], torch.arange(3)[None, None, :]
    k = ((co // 32) * 9 + (2 - kh) * 3 + (2 - kw)) * 32 + co % 32
    out[:, k.reshape(-1)] = w.permute(1, 0, 2, 3).reshape(Ci, Co * 9)
    return out


@pytest.mark.parametrize('Co,Ci', [(64, 3), (36, 3), (36, 32), (96, 32), (64, 64), (32, 128)])
def test_pack_conv3x3_weight_is_the_header_permutation(lib, stream, Co, Ci):
    w = torch.arange(1, Co * Ci * 9 + 1, dtype=torch.float32).reshape(Co, Ci, 3, 3)         # any data: a permutation
    wsrc = dense(w.numel()).load(w)
    wf, wd = dense(Co * c.conv_kpad(Ci)), (dense(Ci * 9 * Co) if Co % 32 == 0 else None)
    lib.call('wesup_pack_conv3x3_weight', wsrc.ptr, wf.ptr, None if wd is None else wd.ptr, Co, Ci, stream())
    assert torch.equal(wf.view().cpu().reshape(Co, -1), pack_fwd_host(w)) and wf.surroundings_untouched()
    if wd is not None:                             # (the dgrad panel is laid out in whole 32-channel chunks of Co)
        assert torch.equal(wd.view().cpu().reshape(Ci, -1), pack_dgrad_host(w)) and wd.surroundings_untouched()
        only = dense(Ci * 9 * Co)                  # either panel may be NULL
        lib.call('wesup_pack_conv3x3_weight', wsrc.ptr, None, only.ptr, Co, Ci, stream())
        assert torch.equal(only.bits(), wd.bits())


def pack_image(lib, stream, x, halo):
    """The image tensor as the kernels read it: wesup_pack_input's NCHW -> NHWC4 with zeros in channel 3, checked exactly."""
    B, _, H, W = x.shape
    src = dense(x.numel() + (-x.numel()) % 4).load(torch.cat([x.reshape(-1), torch.zeros((-x.numel()) % 4)]))
    out = dense(B * H * W * 4, halo)
    lib.call('wesup_pack_input', src.ptr, out.ptr, B, H, W, stream())
    want = torch.cat([x.permute(0, 2, 3, 1), torch.zeros(B, H, W, 1)], 3)
    assert torch.equal(out.view().cpu().reshape(B, H, W, 4), want), 'wesup_pack_input: NCHW -> NHWC4, zeros in channel 3'
    assert out.surroundings_untouched(), 'wesup_pack_input: a store outside the tensor'
    return out


def conv_check(got, ref, bound, kind, tile, what, H, W):
    """check() of an (1, B H W, C) tensor, with (image, row, column, channel) of the first wrong element added."""
    try:
        check(got, ref, bound, kind, tile, what)
    except AssertionError as e:
        got = got.detach().cpu().double().reshape(ref.shape)
        bad = ~(got == ref) if kind == 'int' else ~((got - ref).abs() <= bound)
        _, m, ch = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f'{e}; (image, row, column, channel) = {(m // (H * W), m % (H * W) // W, m % W, ch)}') from None


# ---------------------------------------------------------------- forward / dgrad
_cache = {}


def operands(lib, stream, r, kind, op):
    """Host data, device operands and float64 products of one row's shape, computed once and shared by the row's flag combinations
    (and by the rows that differ in their workspace only).  op: 'fwd' (the layer Cin -> Cout) or 'dgrad' (the layer Cout -> Cin)."""
    key = (op, r.B, r.H, r.W, r.Cin, r.Cout, kind)
    if _cache.get('key') != key:
        _cache.clear()
        B, H, W, Ci, Co = r.B, r.H, r.W, r.Cin, r.Cout
        M = B * H * W
        o = dict(key=key, P={}, E={})
        o['x'] = data((B, Ci, H, W), kind, 1)                        # the tensor the kernel reads: x forward, dy for dgrad
        if op == 'fwd':
            o['w'] = data((Co, Ci, 3, 3), kind, 2, (9 * Ci) ** -0.5)
            o['wdev'] = dense(Co * c.conv_kpad(Ci)).load(pack_fwd_host(o['w']))
        else:
            o['w'] = data((Ci, Co, 3, 3), kind, 2, (9 * Ci) ** -0.5)    # layer Co -> Ci: torch's (out, in, 3, 3)
            o['wdev'] = dense(Co * 9 * Ci).load(pack_dgrad_host(o['w']))
            o['mask'] = data((B, Co, H, W), kind, 5)
            o['maskdev'] = dense(M * Co, (W + 2) * Co).load(nhwc(o['mask']))
        o['bias'] = data((Co,), kind, 3)
        o['old'] = data((1, M, Co), kind, 4)
        Ct = 4 if c.is_image(Ci) else Ci                             # channels of the tensor in memory
        o['xdev'] = pack_image(lib, stream, o['x'], (W + 2) * 4) if c.is_image(Ci) else dense(M * Ci, (W + 2) * Ci).load(nhwc(o['x']))
        assert 9 * (9 * Ct) + 3 < 2 ** 24                            # int pass: the largest possible |partial sum|, exact in fp32
        _cache.update(o)
    return _cache


def products(o, op, relu_in):
    """-> (x * w, |x| * |w|) in float64 as (1, B H W, Cout)"""
    if relu_in not in o['P']:
        x, w = o['x'].double(), o['w'].double()
        x = x.clamp_min(0) if relu_in else x
        conv = (lambda a, b: F.conv2d(a, b, padding=1)) if op == 'fwd' else (lambda a, b: F.conv_transpose2d(a, b, padding=1))
        o['P'][relu_in] = nhwc(conv(x, w))
        o['E'][relu_in] = nhwc(conv(x.abs(), w.abs())) if o['key'][-1] == 'gauss' else None
    return o['P'][relu_in], o['E'][relu_in]


def workspace(lib, r):
    full = lib.load().wesup_conv3x3_workspace_bytes(r.B, r.H, r.W, r.Cin, r.Cout)
    assert full == c.conv_workspace_bytes(r.B, r.H, r.W, r.Cin, r.Cout) and (r.ws is None or full > 0)
    ws = torch.full((max(full, 16),), 0xFF, dtype=torch.uint8, device=dev()) if r.ws else None
    return ws, {None: 0, 'full': full, 'short': full - 1}[r.ws]


FWD_COMBOS = ('plain', 'relu_in', 'y_relu', 'nobias')


@pytest.mark.parametrize('combo', FWD_COMBOS)
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('r', c.CONV_CASES, ids=lambda r: r.id)
def test_conv3x3_fwd_route(lib, stream, r, kind, combo):
    B, H, W, Ci, Co = r.B, r.H, r.W, r.Cin, r.Cout
    M, Ct = B * H * W, (4 if c.is_image(Ci) else Ci)
    o = operands(lib, stream, r, kind, 'fwd')
    relu_in = combo == 'relu_in'
    bias = None if combo == 'nobias' else dense(Co).load(o['bias'])
    y, y2 = dense(M * Co), (dense(M * Co) if combo == 'y_relu' else None)
    ws, ws_bytes = workspace(lib, r)

    def run():
        y.reset()
        if y2 is not None:
            y2.reset()
        if ws is not None:
            ws.fill_(0xFF)                                           # NaN: a partial tile read but never written shows
        lib.call('wesup_conv3x3_fwd', o['xdev'].ptr, o['wdev'].ptr, None if bias is None else bias.ptr, y.ptr,
                 None if y2 is None else y2.ptr, B, H, W, Ct, Co, int(relu_in), None if ws is None else ws.data_ptr(), ws_bytes, stream())
        return y.bits(), (None if y2 is None else y2.bits())
    first = run()
    P, E = products(o, 'fwd', relu_in)
    ref, bound = P, E
    if bias is not None:
        ref = ref + o['bias'].double()
        bound = None if E is None else E + o['bias'].double().abs()
    what = f'{r.id} [{r.route}, {r.tiles[0]} x {r.tiles[1]} tiles] {combo}'
    conv_check(y.view(), ref, None if bound is None else gamma(9 * Ct + 2) * bound, kind, c.CONV_TILE[r.route], what, H, W)
    assert y.surroundings_untouched(), 'a store outside y'
    if y2 is not None:
        assert torch.equal(y2.view().contiguous().view(torch.int32), relu_bits(y.view())), 'y_relu is not max(y, 0) bit for bit'
        assert y2.surroundings_untouched(), 'a store outside y_relu'
    second = run()
    assert torch.equal(first[0], second[0]) and (y2 is None or torch.equal(first[1], second[1])), 'a second call gave other bits'


DGRAD_COMBOS = ('plain', 'mask', 'accum', 'mask-accum')
DGRAD_CASES = [r for r in c.CONV_CASES if not c.is_image(r.Cin)]


@pytest.mark.parametrize('combo', DGRAD_COMBOS)
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('r', DGRAD_CASES, ids=lambda r: r.id)
def test_conv3x3_dgrad_route(lib, stream, r, kind, combo):
    """The row's implicit GEMM as an input gradient: dy has r.Cin channels, dx r.Cout (the layer r.Cout -> r.Cin)."""
    B, H, W, Cdy, Cdx = r.B, r.H, r.W, r.Cin, r.Cout
    M = B * H * W
    o = operands(lib, stream, r, kind, 'dgrad')
    use_mask, accum = 'mask' in combo, 'accum' in combo
    dx = dense(M * Cdx)
    ws, ws_bytes = workspace(lib, r)

    def run():
        dx.reset(o['old'])
        if ws is not None:
            ws.fill_(0xFF)
        lib.call('wesup_conv3x3_dgrad', o['xdev'].ptr, o['wdev'].ptr, o['maskdev'].ptr if use_mask else None, dx.ptr, B, H, W, Cdx, Cdy,
                 int(accum), None if ws is None else ws.data_ptr(), ws_bytes, stream())
        return dx.bits()
    first = run()
    ref, bound = products(o, 'dgrad', False)
    if use_mask:
        ref = torch.where(nhwc(o['mask']) > 0, ref, torch.zeros((), dtype=torch.float64))
    if accum:
        ref = ref + o['old'].double()
        bound = None if bound is None else bound + o['old'].double().abs()
    what = f'{r.id} [{r.route}, {r.tiles[0]} x {r.tiles[1]} tiles] dgrad {combo}'
    conv_check(dx.view(), ref, None if bound is None else gamma(9 * Cdy + 2) * bound, kind, c.CONV_TILE[r.route], what, H, W)
    assert dx.surroundings_untouched(), 'a store outside dx'
    assert torch.equal(first, run()), 'a second call gave other bits'


# ---------------------------------------------------------------- forward with the fused side conv
SIDE_COMBOS = [(b, sb, ri) for b in (1, 0) for sb in (1, 0) for ri in (0, 1)]


@pytest.mark.parametrize('combo', SIDE_COMBOS, ids=lambda v: '-'.join(n for n, on in zip(('bias', 'sidebias', 'relu_in'), v) if on) or 'bare')
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('r', c.SIDE_CASES, ids=lambda r: r.id)
def test_conv3x3_fwd_side_route(lib, stream, r, kind, combo):
    """side = y . sw^T + sb from the fp32 conv output y^ = y + e1, |e1| <= g1 E1 with g1 = gamma(9 Cin + 2), E1 = |x| * |w| + |b|
    (the forward bound).  The second product is an fp32 dot product of length Cout plus a bias over y^:
        |side^ - side| <= g2 (|y^| . |sw| + |sb|) + |e1| . |sw|,   g2 = gamma(Cout + 2),   |y^| <= |y| + g1 E1,
    so the bound is  g2 (|y| . |sw| + |sb|) + (1 + g2) g1 (E1 . |sw|),  every term computed in float64.
    y and y_relu equal the unfused launch's: bit for bit in the int pass, within 2e-6 of the maximum otherwise (the bias is added
    before instead of after the LDS image)."""
    has_bias, has_sb, relu_in = combo
    B, H, W, Ci, Co = r.B, r.H, r.W, r.Cin, r.Cout
    M, Ct, Cs = B * H * W, (4 if c.is_image(Ci) else Ci), r.Cout // 2
    assert Co * 3 * (9 * (9 * Ct) + 3) + 3 < 2 ** 24                 # int pass: the side output's largest |partial sum|
    o = operands(lib, stream, r, kind, 'fwd')
    if 'sw' not in o:
        o['sw'], o['sb'] = data((Cs, Co), kind, 6, Co ** -0.5), data((Cs,), kind, 7)
    bias = dense(Co).load(o['bias']) if has_bias else None
    sw, sb = dense(Cs * Co).load(o['sw']), (dense(Cs).load(o['sb']) if has_sb else None)
    y, y2, y0, y02 = dense(M * Co), dense(M * Co), dense(M * Co), dense(M * Co)
    side = Pad(1, M, Cs, Cs + 8)                                     # ld_side wider than Cout / 2
    bp = None if bias is None else bias.ptr

    def run():
        for t in (y, y2, side):
            t.reset()
        lib.call('wesup_conv3x3_fwd_side', o['xdev'].ptr, o['wdev'].ptr, bp, y.ptr, y2.ptr, sw.ptr, None if sb is None else sb.ptr,
                 side.ptr, side.ld, B, H, W, Ct, Co, relu_in, stream())
        return y.bits(), y2.bits(), side.bits()
    first = run()
    lib.call('wesup_conv3x3_fwd', o['xdev'].ptr, o['wdev'].ptr, bp, y0.ptr, y02.ptr, B, H, W, Ct, Co, relu_in, None, 0, stream())
    P, E = products(o, 'fwd', bool(relu_in))
    b64 = o['bias'].double() if has_bias else torch.zeros(Co, dtype=torch.float64)
    yref = P + b64
    g1, g2 = gamma(9 * Ct + 2), gamma(Co + 2)
    what = f'{r.id} [{r.route}] {combo}'
    conv_check(y.view(), yref, None if E is None else g1 * (E + b64.abs()), kind, c.CONV_TILE[r.route], what + ' y', H, W)
    sw64 = o['sw'].double().t()
    sb64 = o['sb'].double() if has_sb else torch.zeros(Cs, dtype=torch.float64)
    sbound = None if E is None else g2 * (yref.abs() @ sw64.abs() + sb64.abs()) + (1 + g2) * g1 * ((E + b64.abs()) @ sw64.abs())
    conv_check(side.view(), yref @ sw64 + sb64, sbound, kind, (c.CONV_TILE[r.route][0], 32), what + ' side output', H, W)
    if kind == 'int':
        assert torch.equal(y.bits(), y0.bits()) and torch.equal(y2.bits(), y02.bits()), 'y / y_relu differ from the unfused launch'
    else:
        top = float(y0.view().abs().max())
        assert float((y.view() - y0.view()).abs().max()) <= 2e-6 * top and float((y2.view() - y02.view()).abs().max()) <= 2e-6 * top
    assert torch.equal(y2.view().contiguous().view(torch.int32), relu_bits(y.view())), 'y_relu is not max(y, 0) bit for bit'
    assert y.surroundings_untouched() and y2.surroundings_untouched() and side.surroundings_untouched(), 'a store outside an output'
    assert all(torch.equal(a, b) for a, b in zip(first, run())), 'a second call gave other bits'


# ---------------------------------------------------------------- weight gradient
_wcache = {}


def wgrad_operands(lib, stream, r, kind):
    key = (r.id, kind)
    if _wcache.get('key') != key:
        _wcache.clear()
        B, H, W, Ci, Co = r.B, r.H, r.W, r.Ci, r.Cout
        K = B * H * W
        assert 9 * K < 2 ** 24                                       # int pass: the largest possible |partial sum|
        o = dict(key=key, R={})
        o['x'], o['dy'] = data((B, Ci, H, W), kind, 1), data((B, Co, H, W), kind, 4, K ** -0.5)
        o['xdev'] = pack_image(lib, stream, o['x'], (W + 2) * 4) if c.is_image(Ci) else dense(K * Ci, (W + 2) * Ci).load(nhwc(o['x']))
        o['dydev'] = dense(K * Co, (W + 2) * Co).load(nhwc(o['dy']))
        _wcache.update(o)
    return _wcache


def wgrad_reference(o, relu_in, Ci, Co):
    """autograd of F.conv2d in float64 -> (dw, db, |dy| x |x|, sum |dy|); dw as (1, Co, 9 Ci) with columns tap * Ci + ci, the
    order of the kernel's slab, so that the box of wrong elements can be read in tiles"""
    if relu_in not in o['R']:
        def grads(x, dy):
            w = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
            b = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
            F.conv2d(x, w, b, padding=1).backward(dy)
            return w.grad.reshape(Co, Ci, 9).permute(0, 2, 1).reshape(1, Co, 9 * Ci), b.grad.reshape(1, 1, Co)
        x, dy = o['x'].double(), o['dy'].double()
        x = x.clamp_min(0) if relu_in else x
        o['R'][relu_in] = grads(x, dy) + (grads(x.abs(), dy.abs()) if o['key'][1] == 'gauss' else (None, None))
    return o['R'][relu_in]


WGRAD_COMBOS = [(ri, db) for ri in (0, 1) for db in (1, 0)]


@pytest.mark.parametrize('combo', WGRAD_COMBOS, ids=lambda v: ('relu_in-' if v[0] else '') + ('db' if v[1] else 'nodb'))
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('r', c.WGRAD_CASES, ids=lambda r: r.id)
def test_conv3x3_wgrad_route(lib, stream, r, kind, combo):
    relu_in, want_db = combo
    B, H, W, Ci, Co = r.B, r.H, r.W, r.Ci, r.Cout
    K = B * H * W
    o = wgrad_operands(lib, stream, r, kind)
    dw, db = dense(Co * Ci * 9 + (-Co * Ci * 9) % 4), (dense(Co) if want_db else None)
    nbytes = lib.load().wesup_conv3x3_wgrad_workspace_bytes(B, H, W, Ci, Co)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())

    def run():
        dw.reset()
        if db is not None:
            db.reset()
        ws.fill_(0xFF)                                               # NaN: a slab element read but never written shows
        lib.call('wesup_conv3x3_wgrad', o['xdev'].ptr, o['dydev'].ptr, dw.ptr, None if db is None else db.ptr, B, H, W, Ci, Co, relu_in,
                 ws.data_ptr(), nbytes, stream())
        return dw.bits(), (None if db is None else db.bits())
    first = run()
    rdw, rdb, edw, edb = wgrad_reference(o, relu_in, Ci, Co)
    what = f'{r.id} [{r.route}, S = {r.S}{", weighted" if r.weighted else ""}] {"relu_in" if relu_in else "plain"}'
    got = dw.view().reshape(-1)[:Co * Ci * 9].reshape(Co, Ci, 9).permute(0, 2, 1).reshape(1, Co, 9 * Ci)
    tile = int(r.route.split('-')[0])
    try:
        check(got, rdw, None if edw is None else gamma(K + 2) * edw, kind, (tile, tile), what + ' dw (columns: tap * Ci + ci)')
    except AssertionError as e:
        g64 = got.cpu().double()
        bad = ~(g64 == rdw) if kind == 'int' else ~((g64 - rdw).abs() <= gamma(K + 2) * edw)
        _, co, col = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f'{e}; (co, ci, kh, kw) = {(co, col % Ci, col // Ci // 3, col // Ci % 3)}') from None
    tail = dw.view().reshape(-1)[Co * Ci * 9:]                       # (the image layer's 27 Co: rounded up to whole quads)
    assert bool(torch.isnan(tail).all()) and dw.surroundings_untouched(), 'a store outside dw'
    if db is not None:
        check(db.view(), rdb, None if edb is None else gamma(K + 2) * edb, kind, (1, tile), what + ' db')
        assert db.surroundings_untouched(), 'a store outside db'
    second = run()
    assert torch.equal(first[0], second[0]) and (db is None or torch.equal(first[1], second[1])), 'a second call gave other bits'


# ---------------------------------------------------------------- argument checks: an error code and no launch
def test_conv_argument_checks_leave_the_output_alone(lib, stream):
    h = lib.load()
    B, H, W, Ci, Co = 2, 5, 6, 32, 64
    M = B * H * W
    x = dense(M * Ci, (W + 2) * Ci).load(data((M * Ci,), 'int', 1))
    w = dense(Co * 9 * Ci).load(data((Co * 9 * Ci,), 'int', 2))
    bias = dense(Co).load(data((Co,), 'int', 3))
    mask = dense(M * Co, (W + 2) * Co).load(data((M * Co,), 'int', 5))
    sw = dense(32 * 64).load(data((32 * 64,), 'int', 6))
    y, y2, side = dense(M * 68), dense(M * 68), dense(M * 64)
    dw = dense(Co * Ci * 9)
    before = [t.bits() for t in (y, y2, side, dw)]

    def fwd(x_=x.ptr, w_=w.ptr, b_=bias.ptr, y_=y.ptr, y2_=y2.ptr, shape=(B, H, W, Ci, Co)):
        return h.wesup_conv3x3_fwd(x_, w_, b_, y_, y2_, *shape, 0, None, 0, stream())
    assert fwd(shape=(B, H, W, Ci, 66)) == ERR_INVALID               # Cout % 4 != 0: the epilogue stores whole quads
    assert fwd(shape=(B, H, W, 48, Co)) == ERR_INVALID               # Cin neither 4 nor a power of two >= 32
    assert fwd(x_=x.ptr + 4) == ERR_INVALID                          # each pointer misaligned in turn
    assert fwd(w_=w.ptr + 8) == ERR_INVALID
    assert fwd(b_=bias.ptr + 4) == ERR_INVALID
    assert fwd(y_=y.ptr + 4) == ERR_INVALID
    assert fwd(y2_=y2.ptr + 12) == ERR_INVALID
    # outside FastDiv's exact range (csrc/common.hpp): (B H W - 1) ceil(2^40 / W) reaches 2^64; B H W * W above 2^40 -- both with
    # fewer than 2^31 elements, so nothing else refuses them.  One image less is inside the range (not run: only its query)
    wrap, wide = (2 ** 24 + 1, 1, 1, 32, 32), (1, 1025, 32768, 32, 32)
    for shape in (wrap, wide):
        assert shape[0] * shape[1] * shape[2] * 32 < 2 ** 31
        assert fwd(shape=shape) == ERR_INVALID

    def dgrad(dy_=x.ptr, m_=mask.ptr, dx_=y.ptr, shape=(B, H, W, Co, Ci)):
        return h.wesup_conv3x3_dgrad(dy_, w.ptr, m_, dx_, *shape, 0, None, 0, stream())
    assert dgrad(m_=mask.ptr + 4) == ERR_INVALID                     # (WESUP_MASK without a mask cannot be asked for through this ABI:
    assert dgrad(dx_=y.ptr + 8) == ERR_INVALID                       #  the flag is set from the pointer)
    assert dgrad(shape=(B, H, W, 66, Ci)) == ERR_INVALID             # the output's channel count here is Cin
    assert dgrad(shape=wrap) == ERR_INVALID and dgrad(shape=wide) == ERR_INVALID

    def fwd_side(Co_, sw_=sw.ptr, so_=side.ptr, ld=64):
        return h.wesup_conv3x3_fwd_side(x.ptr, w.ptr, bias.ptr, y.ptr, y2.ptr, sw_, None, so_, ld, B, H, W, Ci, Co_, 0, stream())
    for Co_ in (32, 96, 256):                                        # the fused side conv: Cout in {64, 128}
        assert fwd_side(Co_) == ERR_INVALID
    assert fwd_side(64, sw_=sw.ptr + 4) == ERR_INVALID and fwd_side(64, so_=side.ptr + 4) == ERR_INVALID
    assert fwd_side(64, ld=28) == ERR_INVALID                        # ld_side below Cout / 2
    assert h.wesup_conv3x3_fwd_side(x.ptr, w.ptr, bias.ptr, y.ptr, y2.ptr, sw.ptr, None, side.ptr, 64, B, H, W, 4, 128, 0,
                                    stream()) == ERR_INVALID         # the image layer has no 128-channel form

    nbytes = h.wesup_conv3x3_wgrad_workspace_bytes(B, H, W, Ci, Co)
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev())

    def wgrad(x_=x.ptr, dy_=mask.ptr, dw_=dw.ptr, ws_=ws.data_ptr(), nb=nbytes, shape=(B, H, W, Ci, Co)):
        return h.wesup_conv3x3_wgrad(x_, dy_, dw_, None, *shape, 0, ws_, nb, stream())
    assert wgrad(nb=nbytes - 1) == ERR_WORKSPACE                     # a short workspace
    assert wgrad(x_=x.ptr + 4) == ERR_INVALID and wgrad(dy_=mask.ptr + 8) == ERR_INVALID
    assert wgrad(ws_=ws.data_ptr() + 4) == ERR_INVALID and wgrad(dw_=dw.ptr + 2) == ERR_INVALID
    assert wgrad(shape=(B, H, W, Ci, 48)) == ERR_INVALID and wgrad(shape=(B, H, W, Ci, 0)) == ERR_INVALID
    assert wgrad(shape=wrap, nb=2 ** 40) == ERR_INVALID and wgrad(shape=wide, nb=2 ** 40) == ERR_INVALID
    torch.cuda.synchronize()
    assert all(torch.equal(a, t.bits()) for a, t in zip(before, (y, y2, side, dw))), 'a rejected call wrote to an output'
    # ... and the same arguments without the fault go through
    assert fwd() == 0 and wgrad() == 0
