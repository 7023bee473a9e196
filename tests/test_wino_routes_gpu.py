"""Every pass of the Winograd family (csrc/winograd.hip, csrc/wino_fused.hip, the Winograd composites of csrc/gemm.hip) at its
tile, plane and epilogue edges: the rows of tests/_winocases.py (what a row reaches is tests/test_wino_routes_cpu.py's business),
through the C ABI, each row in the two passes of tests/test_gemm_routes_gpu.py:

  int    small integers.  B^T and A^T of both point sets are dyadic, so the activation transforms, the output transform and the
         one-kernel route on given V, U are EXACT in fp32 whatever the order of operations (premise asserted on the rows' data by
         the CPU test): the result has to EQUAL the float64 reference.  A lost tap, tile, plane or mask bit is a count and a box of
         wrong elements.  Anything through G of F(4x4) (thirds) cannot be exact and is held to the bound below in both passes.
  gauss  Gaussian data, |got - ref64| <= gamma(n) * absref per element: absref the same pipeline in float64 with the absolute
         value of every matrix and operand (+ |bias| + |old|), n the roundings on the longest path (_winocases.ROUNDINGS).

References: oracle/winograd_oracle.py in float64; F.conv2d and its autograd in float64 for the composites.
Epilogue order (include/wesup_hip.h): bias, mask > 0, + old content (accumulate) or a gathered row; y_relu = max(y, 0); the pool
is floor mode.  Unpooling: the first positive maximum of a 2x2 window in row-major order gets the value; dead windows get nothing.

Every operand and output is a view inside a NaN-filled allocation of the test's own, with at least (W + 2) C NaN floats around x,
dy, mask_src, unpool_src and the old content; compact operands (sign bits, pool codes, new_row, area_new) sit in sentinel-filled
integer buffers.  After each call the surroundings (the gaps between strided position planes included) must hold their bits, and a
second call must give the same bits."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _winocases as w
from oracle import winograd_oracle as wo
from test_gemm_routes_gpu import ERR_INVALID, ERR_WORKSPACE, PASSES, Pad, check, gamma
from test_kernels_gpu import dev

pytestmark = pytest.mark.gpu
RN = w.ROUNDINGS


@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope='module')
def stream():
    from wesup_amd import ops
    return ops._stream


# ---------------------------------------------------------------- operands
def flat(n, halo=8):
    """n contiguous floats as a Pad view with at least `halo` NaN floats on either side, 16-byte aligned"""
    halo = w.align_up(halo, 4)
    return Pad(1, 1, n, w.align_up(n, 4) + 2 * halo, col_off=halo, extra=0)


def pixels(shape, data=None):
    """a (B, H, W, C) tensor with (W + 2) C NaN floats around it"""
    B, H, W, C = shape
    p = flat(B * H * W * C, (W + 2) * C)
    return p if data is None else p.load(torch.from_numpy(np.ascontiguousarray(data)))


def planes(P, T, C, padded, data=None):
    """a transformed tensor [P][T][C]; padded: plane_elems = T C + 12, with NaN between the planes -> (Pad, plane_elems)"""
    p = Pad(P, T, C, C, col_off=0, extra=0, batch_pad=12 if padded else 0)
    if data is not None:
        p.load(torch.from_numpy(data))
    return p, (T * C + 12 if padded else 0)


class IntPad:
    """n integers inside a buffer filled with `sentinel`"""

    def __init__(self, n, dtype, sentinel, data=None, halo=64):
        self.n, self.halo, self.sentinel = n, halo, sentinel
        self.buf = torch.full((n + 2 * halo,), sentinel, dtype=dtype, device=dev())
        if data is not None:
            self.view().copy_(torch.from_numpy(np.ascontiguousarray(data)).reshape(-1).to(dtype))

    def view(self):
        return self.buf[self.halo:self.halo + self.n]

    def reset(self):
        self.buf.fill_(self.sentinel)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.halo * self.buf.element_size()

    def surroundings_untouched(self):
        return bool((self.buf[:self.halo] == self.sentinel).all() and (self.buf[self.halo + self.n:] == self.sentinel).all())

    def bits(self):
        return self.buf.clone()


def t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def wcheck(got, ref, bound, kind, what, names, decode=None, box=(1, 4)):
    """check() of a device tensor against a float64 numpy reference of the same shape (flattened to three axes: the first, the
    middle ones, the last), with the named coordinates of the first wrong element added."""
    ref = np.asarray(ref, dtype=np.float64)
    shape = ref.shape
    r3 = t64(ref).reshape(shape[0], -1, shape[-1])
    b3 = None if kind == 'int' or bound is None else t64(np.broadcast_to(bound, shape)).reshape(r3.shape)
    g3 = got.detach().cpu().double().reshape(r3.shape)
    try:
        check(g3, r3, b3, 'int' if b3 is None else 'gauss', box, what)
    except AssertionError as e:
        bad = ~(g3 == r3) if b3 is None else ~((g3 - r3).abs() <= b3)
        i = np.unravel_index(int(bad.reshape(-1).nonzero()[0]), shape)
        where = tuple(int(v) for v in (decode(i) if decode else i))
        raise AssertionError(f'{e}; {names} = {where}') from None


def tile_decode(B, H, W, m):
    Th, Tw = w.cdiv(H, m), w.cdiv(W, m)
    return lambda i: (i[1] // (Th * Tw), i[1] // Tw % Th, i[1] % Tw, i[0], i[2])


TILE_NAMES = '(image, tile row, tile column, position, channel)'
PIXEL_NAMES = '(image, row, column, channel)'


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def relu_bits(t):
    return torch.where(t < 0, torch.zeros((), device=t.device), t).contiguous().view(torch.int32)


def pack4(b):
    """(..., C) of 0 / 1 or codes -> (..., C / 4) with bit (or 3-bit field) j of an entry = channel 4 q + j"""
    return b.reshape(*b.shape[:-1], b.shape[-1] // 4, 4)


def first_max(src, H, W):
    """(B, >= 2H, >= 2W, C) -> (B, H, W, C) codes of the 2x2 windows: 0 = the maximum is not positive, k + 1 = the first maximum is
    at window position k (row-major)"""
    win = np.stack([src[:, 0:2 * H:2, 0:2 * W:2], src[:, 0:2 * H:2, 1:2 * W:2], src[:, 1:2 * H:2, 0:2 * W:2], src[:, 1:2 * H:2, 1:2 * W:2]], 0)
    return np.where(win.max(0) > 0, win.argmax(0) + 1, 0)                    # (numpy's argmax returns the first occurrence)


def code12(c):
    q = pack4(c).astype(np.int64)
    return (q[..., 0] | (q[..., 1] << 3) | (q[..., 2] << 6) | (q[..., 3] << 9)).astype(np.int16)


def scatter(dst, code, v, H, W):
    """dst (B, Hu, Wu, C) += v (B, H, W, C) at the window positions the codes pick"""
    for k in range(4):
        dst[:, (k >> 1):2 * H:2, (k & 1):2 * W:2] += np.where(code == k + 1, v, 0.0)
    return dst


def unpool_source(B, Hu, Wu, H, W, C, kind):
    """pre-pool activations with a seeded four-way tie (channels 0 .. 7 of the first window: the first position takes it) and a dead
    window (channels 8 .. 15 of the last one: exact zeros, a negative zero and a negative value)"""
    src = w._data((B, Hu, Wu, C), kind, 6)
    src[0, 0:2, 0:2, :8] = 2.0
    src[B - 1, 2 * H - 2:2 * H, 2 * W - 2:2 * W, 8:16] = np.array([0.0, -0.0, -1.0, 0.0], dtype=np.float32).reshape(2, 2, 1)
    return src


def pool(y, relu):
    B, H, W, C = y.shape
    p = y[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))
    return np.maximum(p, 0) if relu else p


# ---------------------------------------------------------------- 1. activation transforms
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('r', w.ACT_CASES, ids=lambda r: r.id)
def test_activation_transforms(lib, stream, r, kind):
    h = lib.load()
    B, H, W, C = r.B, r.H, r.W, r.C
    x = w.act_data(r, kind)
    xd = pixels(x.shape, x)
    refs = {}

    def ref(name, m, relu=False):
        """-> (reference, absref) of a transform, computed once per row"""
        key = (name, m, relu)
        if key not in refs:
            f = (lambda o, a: o.input_transform(a, relu, m=m)) if name == 'in' else (lambda o, a: o.outgrad_transform(a, m=m))
            with w.absolute() as ab:
                E = None if kind == 'int' else f(ab, np.abs(x))
            refs[key] = (f(wo, x), E)
        return refs[key]

    def vcheck(pad, name, m, relu, what):
        V, E = ref(name, m, relu)
        n = RN[('in' if name == 'in' else 'og') + str(m)]
        wcheck(pad.view(), V, None if E is None else gamma(n) * E, kind, what, TILE_NAMES, tile_decode(B, H, W, m))
        assert pad.surroundings_untouched(), f'{what}: a store outside the tensor or between its planes'

    for entry in w.act_entries(r):
        m = 2 if '2' in entry else 4
        P, T = w.wino_positions(m), w.wino_tiles(B, H, W, m)
        relu = entry.endswith('-relu')
        for padded in ((0, 1) if entry.startswith(('in', 'bits')) else (0,)):
            what = f'{r.id} {entry} plane_elems = {"T C + 12" if padded else 0} [{kind}]'
            if entry.startswith(('in', 'bits')):
                V, pe = planes(P, T, C, padded)
                bits = IntPad(B * H * W * C // 4, torch.uint8, 0xFF) if entry.startswith('bits') else None

                def run():
                    V.reset()
                    if bits is None:
                        lib.call('wesup_winograd_input_transform', xd.ptr, V.ptr, pe, B, H, W, C, int(relu), m, stream())
                        return (V.bits(),)
                    bits.reset()
                    lib.call('wesup_winograd_input_transform_bits', xd.ptr, V.ptr, pe, bits.ptr, B, H, W, C, int(relu), stream())
                    return V.bits(), bits.bits()
                first = run()
                vcheck(V, 'in', m, relu, what)
                if bits is not None:
                    q = pack4((x > 0).astype(np.uint8))
                    want = torch.from_numpy(q[..., 0] | (q[..., 1] << 1) | (q[..., 2] << 2) | (q[..., 3] << 3)).reshape(-1)
                    bad = (bits.view().cpu() != want).nonzero()
                    assert bad.numel() == 0, (f'{what}: {bad.shape[0]} of {want.numel()} sign-bit bytes wrong, first at (pixel, quad) = '
                                              f'{divmod(int(bad[0]), C // 4)}')
                    assert bits.surroundings_untouched(), f'{what}: a store outside relu_bits'
                assert same(first, run()), f'{what}: a second call gave other bits'
                continue
            dM, _ = planes(P, T, C, 0)
            if entry in ('og2', 'og4', 'og4-db'):
                db = flat(C) if entry == 'og4-db' else None
                nbytes = h.wesup_winograd_outgrad_workspace_bytes(B, H, W, C, m)
                assert nbytes == w.outgrad_workspace_bytes(B, H, W, C, m)
                ws = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=dev()) if db is not None else None

                def run():
                    dM.reset()
                    if db is not None:
                        db.reset()
                        ws.fill_(0xFF)
                    lib.call('wesup_winograd_outgrad_transform', xd.ptr, dM.ptr, None if db is None else db.ptr, B, H, W, C, m,
                             None if ws is None else ws.data_ptr(), nbytes if ws is not None else 0, stream())
                    return dM.bits(), (None if db is None else db.bits())
                first = run()
                vcheck(dM, 'og', m, False, what)
                if db is not None:
                    dM.reset()                                                  # a workspace one byte short is refused before any launch
                    assert h.wesup_winograd_outgrad_transform(xd.ptr, dM.ptr, db.ptr, B, H, W, C, m, ws.data_ptr(), nbytes - 1,
                                                              stream()) == ERR_WORKSPACE
                    torch.cuda.synchronize()
                    assert bool(torch.isnan(dM.buf).all()), f'{what}: a refused call wrote to dM'
                    first = run()
                    wcheck(db.view(), x.astype(np.float64).sum((0, 1, 2)).reshape(1, 1, C),
                           gamma(16 * T) * np.abs(x).astype(np.float64).sum((0, 1, 2)).reshape(1, 1, C), kind,
                           what + (' db (block column sums)' if w.block_colsum_ok(C) else ' db (wesup_colsum on dy)'), '(-, -, channel)')
                    assert db.surroundings_untouched(), f'{what}: a store outside db'
                assert same(first, run()), f'{what}: a second call gave other bits'
                continue
            # the dual transform
            V, _ = planes(P, T, C, 0)
            rows = w.bias_rows(B, H, W, C) if entry == 'dual-bias' else 0
            assert rows == h.wesup_winograd_bias_rows(B, H, W, C) or entry != 'dual-bias'
            part = Pad(1, rows, C, C, col_off=0, extra=0) if rows else None

            def run():
                V.reset()
                dM.reset()
                if part is not None:
                    part.reset()
                lib.call('wesup_winograd_dual_transform', xd.ptr, V.ptr, dM.ptr, None if part is None else part.ptr, B, H, W, C, stream())
                return V.bits(), dM.bits(), (None if part is None else part.bits())
            first = run()
            vcheck(V, 'in', 4, False, what + ' V')
            vcheck(dM, 'og', 4, False, what + ' dM')
            if part is not None:
                # row L = the column sum of dy over the tiles of logical block L: 256 / (C/4) tiles each
                Th, Tw, tpb = w.cdiv(H, 4), w.cdiv(W, 4), 256 // (C // 4)
                xp = np.zeros((B, 4 * Th, 4 * Tw, C))
                xp[:, :H, :W] = x
                per_tile = xp.reshape(B, Th, 4, Tw, 4, C)
                full = np.zeros((rows * tpb, C))
                absfull = np.zeros((rows * tpb, C))
                full[:T] = per_tile.sum((2, 4)).reshape(T, C)
                absfull[:T] = np.abs(per_tile).sum((2, 4)).reshape(T, C)
                want, bound = full.reshape(rows, tpb, C).sum(1), gamma(16 * tpb) * absfull.reshape(rows, tpb, C).sum(1)
                wcheck(part.view(), want[None], bound[None], kind, what + ' bias_part', '(-, block, channel)')
                assert part.surroundings_untouched(), f'{what}: a store outside bias_part'
                if kind == 'int':
                    assert np.array_equal(part.view().cpu().double().numpy().sum((0, 1)), x.astype(np.float64).sum((0, 1, 2)))
            assert same(first, run()), f'{what}: a second call gave other bits'


# ---------------------------------------------------------------- 2. output transform
def epilogue(res, absres, d, bias, mask, accum):
    """-> (y, absref) of bias, mask > 0, + old content, float64"""
    y, E = res.copy(), (None if absres is None else absres.copy())
    if bias:
        y += d['bias'].astype(np.float64)
        E = None if E is None else E + np.abs(d['bias']).astype(np.float64)
    if mask:
        y = np.where(d['mask'] > 0, y, 0.0)
    if accum:
        y = y + d['old'].astype(np.float64)
        E = None if E is None else E + np.abs(d['old']).astype(np.float64)
    return y, E


@pytest.mark.parametrize('padded', (0, 1), ids=('dense', 'planes'))
@pytest.mark.parametrize('m', (2, 4))
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('r', w.OUT_CASES, ids=lambda r: r.id)
def test_output_transform(lib, stream, r, kind, m, padded):
    B, H, W, C = r.B, r.H, r.W, r.C
    P, T, Hp, Wp = w.wino_positions(m), w.wino_tiles(B, H, W, m), H // 2, W // 2
    d = w.out_data(r, kind, m)
    Mt, pe = planes(P, T, C, padded, d['Mt'])
    res = wo.output_transform(d['Mt'], B, H, W, None, np.float64, m)
    with w.absolute() as ab:
        absres = None if kind == 'int' else ab.output_transform(np.abs(d['Mt']), B, H, W, None, np.float64, m)
    bias_d, mask_d = flat(C).load(torch.from_numpy(d['bias'])), pixels(d['mask'].shape, d['mask'])
    n = RN[f'out{m}']
    for bias, mask, accum, yrelu, pl in w.OUT_COMBOS:
        if pl is not None and Hp * Wp == 0:
            continue
        what = (f'{r.id} m = {m} plane_elems = {pe}: ' + ('+'.join(k for k, on in (('bias', bias), ('mask', mask), ('accum', accum),
                ('y_relu', yrelu), ('y_pool', pl is not None), ('pool_relu', pl)) if on) or 'bare') + f' [{kind}]')
        y, y2 = pixels(d['old'].shape), (pixels(d['old'].shape) if yrelu else None)
        yp = pixels((B, Hp, Wp, C)) if pl is not None else None

        def run():
            y.reset(torch.from_numpy(d['old']))
            for t in (y2, yp):
                if t is not None:
                    t.reset()
            lib.call('wesup_winograd_output_transform', Mt.ptr, pe, bias_d.ptr if bias else None, mask_d.ptr if mask else None, y.ptr,
                     None if y2 is None else y2.ptr, None if yp is None else yp.ptr, int(bool(pl)), B, H, W, C, accum, m, stream())
            return y.bits(), (None if y2 is None else y2.bits()), (None if yp is None else yp.bits())
        first = run()
        want, E = epilogue(res, absres, d, bias, mask, accum)
        wcheck(y.view(), want, None if E is None else gamma(n) * E, kind, what, PIXEL_NAMES)
        got = y.view().reshape(B, H, W, C)
        assert y.surroundings_untouched(), f'{what}: a store outside y'
        if y2 is not None:
            assert torch.equal(y2.view().reshape(-1).view(torch.int32), relu_bits(got).reshape(-1)), f'{what}: y_relu is not max(y, 0) bit for bit'
            assert y2.surroundings_untouched(), f'{what}: a store outside y_relu'
        if yp is not None:
            # the pooled output is the maximum of the stored values themselves (floor mode), in both passes
            wcheck(yp.view(), pool(got.cpu().double().numpy(), pl), None, 'int', what + ' y_pool against the stored y', PIXEL_NAMES)
            if kind == 'int':
                wcheck(yp.view(), pool(want, pl), None, 'int', what + ' y_pool', PIXEL_NAMES)
            assert yp.surroundings_untouched(), f'{what}: a store outside y_pool'
        assert same(first, run()), f'{what}: a second call gave other bits'


@pytest.mark.parametrize('padded', (0, 1), ids=('dense', 'planes'))
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('r', w.OUT_CASES, ids=lambda r: r.id)
def test_output_transform_unpool(lib, stream, r, kind, padded):
    B, H, W, C = r.B, r.H, r.W, r.C
    T = w.wino_tiles(B, H, W, 4)
    d = w.out_data(r, kind, 4)
    Mt, pe = planes(36, T, C, padded, d['Mt'])
    res = wo.output_transform(d['Mt'], B, H, W, None, np.float64, 4)
    with w.absolute() as ab:
        absres = None if kind == 'int' else ab.output_transform(np.abs(d['Mt']), B, H, W, None, np.float64, 4)
    bias_d, mask_d = flat(C).load(torch.from_numpy(d['bias'])), pixels(d['mask'].shape, d['mask'])
    for bias, mask, odd in w.UNPOOL_COMBOS:
        Hu, Wu = 2 * H + odd, 2 * W + odd
        src, old = unpool_source(B, Hu, Wu, H, W, C, kind), w._data((B, Hu, Wu, C), kind, 7)
        what = (f'{r.id} unpool Hu x Wu = {Hu} x {Wu} plane_elems = {pe}: ' + ('+'.join(k for k, on in (('bias', bias), ('mask', mask)) if on) or 'bare')
                + f' [{kind}]')
        src_d, dst = pixels(src.shape, src), pixels(old.shape)

        def run():
            dst.reset(torch.from_numpy(old))
            lib.call('wesup_winograd_output_transform_unpool', Mt.ptr, pe, bias_d.ptr if bias else None, mask_d.ptr if mask else None,
                     src_d.ptr, dst.ptr, B, H, W, Hu, Wu, C, 4, stream())
            return (dst.bits(),)
        first = run()
        v, E = epilogue(res, absres, d, bias, mask, 0)
        code = first_max(src, H, W)
        assert (code[0, 0, 0, :8] == 1).all() and (code[B - 1, H - 1, W - 1, 8:16] == 0).all()
        want = scatter(old.astype(np.float64), code, v, H, W)
        bound = None if E is None else gamma(RN['out4']) * scatter(np.abs(old).astype(np.float64), code, E, H, W)
        wcheck(dst.view(), want, bound, kind, what, PIXEL_NAMES)
        assert dst.surroundings_untouched(), f'{what}: a store outside unpool_dst'
        assert same(first, run()), f'{what}: a second call gave other bits'


# ---------------------------------------------------------------- 3. the one-kernel route
KMAX = 6


def gather_operands(B, pix, N, kind):
    """side [B][KMAX][N] with the last row of every image NaN (what a label read outside new_row -- the sentinel -- would gather),
    new_row [B][pix] below KMAX - 1, area_new [B][KMAX] of {1, 2, 4} (the reciprocal and the product are exact on integers)
    -> (side, new_row, area_new, value(pixel) = side[new_row] / area_new[new_row] in float64, the same without the division)"""
    side = w._data((B, KMAX, N), kind, 8)
    side[:, KMAX - 1] = np.nan
    gen = torch.Generator().manual_seed(9)
    rows = torch.randint(0, KMAX - 1, (B, pix), generator=gen).numpy().astype(np.int32)
    area = (1 << torch.randint(0, 3, (B, KMAX), generator=gen).numpy()).astype(np.int32)
    b = np.arange(B)[:, None]
    raw = side.astype(np.float64)[b, rows]
    return side, rows, area, raw / area[b, rows][..., None], raw


@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('r', w.FUSED_CASES, ids=lambda r: r.id)
def test_one_kernel_route(lib, stream, r, kind):
    B, H, W, K, N = r.B, r.H, r.W, r.K, r.N
    T, Hp, Wp = w.wino_tiles(B, H, W, 4), H // 2, W // 2
    d = w.fused_data(r, kind)
    V64, U64 = d['V'].astype(np.float64), d['U'].astype(np.float64).transpose(0, 2, 1)
    res = wo.output_transform(np.matmul(V64, U64), B, H, W, None, np.float64, 4)
    with w.absolute() as ab:
        absres = None if kind == 'int' else ab.output_transform(np.matmul(np.abs(V64), np.abs(U64)), B, H, W, None, np.float64, 4)
    n = K + 2 + RN['fused']
    U = flat(36 * N * K).load(torch.from_numpy(d['U']))
    bias_d, mask_d = flat(N).load(torch.from_numpy(d['bias'])), pixels(d['mask'].shape, d['mask'])
    q = pack4((d['mask'] > 0).astype(np.uint8))
    bits_d = IntPad(B * H * W * N // 4, torch.uint8, 0xFF, q[..., 0] | (q[..., 1] << 1) | (q[..., 2] << 2) | (q[..., 3] << 3))
    for padded in (0, 1):
        V, pe = planes(36, T, K, padded, d['V'])
        for form, opts in w.fused_options(r):
            o = set(opts)
            unpool, gather, accum = bool(o & {'unpool_src', 'unpool_code'}), 'side' in o, int('accum' in o)
            Hu, Wu = ((2 * H, 2 * W) if gather else (2 * H + 1, 2 * W + 1)) if unpool else (0, 0)
            what = f'{r.id} [{form}] {"+".join(opts) or "bare"} plane_elems = {pe} [{kind}]'
            v, E = epilogue(res, absres, d, 'bias' in o, bool(o & {'mask', 'bits'}), 0)
            shape = (B, Hu, Wu, N) if unpool else (B, H, W, N)
            side_d = row_d = area_d = None
            if gather:
                side, rows, area, value, raw = gather_operands(B, shape[1] * shape[2], N, kind)
                side_d = flat(side.size).load(torch.from_numpy(side))
                row_d = IntPad(rows.size, torch.int32, KMAX - 1, rows)
                area_d = IntPad(area.size, torch.int32, 0, area) if 'area' in o else None
                base, old = (value if 'area' in o else raw).reshape(shape), None
            elif unpool or accum:
                old = w._data(shape, kind, 7) if unpool else d['old']
                base = old.astype(np.float64)
            else:
                base, old = np.zeros(shape), None
            src_d = code_d = yp = code_out = None
            if unpool:
                src = unpool_source(B, Hu, Wu, H, W, N, kind)
                code = first_max(src, H, W)
                src_d = pixels(src.shape, src) if 'unpool_src' in o else None
                code_d = IntPad(code.size // 4, torch.int16, -1, code12(code)) if 'unpool_code' in o else None
                want = scatter(base.copy(), code, v, H, W)
                bound = None if E is None else gamma(n) * scatter(np.abs(base), code, E, H, W)
            else:
                want, bound = base + v, (None if E is None else gamma(n) * (np.abs(base) + E))
                if 'pool' in o:
                    yp = pixels((B, Hp, Wp, N))
                    code_out = IntPad(B * Hp * Wp * N // 4, torch.int16, -1) if 'code' in o else None
            dst = pixels(shape)
            P = lambda t: None if t is None else t.ptr                                   # noqa: E731
            bias_p, mask_p = (bias_d.ptr if 'bias' in o else None), (mask_d.ptr if 'mask' in o else None)

            def run():
                dst.reset(None if old is None else torch.from_numpy(old))                # (NaN where the destination is written, never read)
                for t in (yp, code_out):
                    if t is not None:
                        t.reset()
                if o & {'bits', 'code', 'unpool_code'}:
                    lib.call('wesup_winograd_gemm_output_transform_ex', V.ptr, pe, U.ptr, bias_p, mask_p, bits_d.ptr if 'bits' in o else None,
                             None if unpool else dst.ptr, P(yp), int('pool_relu' in o), P(code_out), P(src_d), P(code_d),
                             dst.ptr if unpool else None, Hu, Wu, P(side_d), P(row_d), P(area_d), KMAX if gather else 0, B, H, W, K, N, accum,
                             stream())
                elif gather:
                    lib.call('wesup_winograd_gemm_output_transform_gather', V.ptr, pe, U.ptr, mask_p, dst.ptr, P(src_d), Hu, Wu, side_d.ptr,
                             row_d.ptr, P(area_d), KMAX, B, H, W, K, N, stream())
                else:
                    lib.call('wesup_winograd_gemm_output_transform', V.ptr, pe, U.ptr, bias_p, mask_p, None if unpool else dst.ptr, P(yp),
                             int('pool_relu' in o), P(src_d), dst.ptr if unpool else None, Hu, Wu, B, H, W, K, N, accum, stream())
                return dst.bits(), (None if yp is None else yp.bits()), (None if code_out is None else code_out.bits())
            first = run()
            wcheck(dst.view(), want, bound, kind, what, PIXEL_NAMES)
            assert dst.surroundings_untouched(), f'{what}: a store outside the destination'
            if yp is not None:
                got = dst.view().reshape(shape).cpu().double().numpy()
                wcheck(yp.view(), pool(got, 'pool_relu' in o), None, 'int', what + ' y_pool against the stored y', PIXEL_NAMES)
                if kind == 'int':
                    wcheck(yp.view(), pool(want, 'pool_relu' in o), None, 'int', what + ' y_pool', PIXEL_NAMES)
                assert yp.surroundings_untouched(), f'{what}: a store outside y_pool'
                if code_out is not None:
                    # the decisions are taken on the stored values themselves: exact in both passes, ties included
                    for name, yy in (('the stored y', got),) + ((('the reference', want),) if kind == 'int' else ()):
                        c = torch.from_numpy(code12(first_max(yy, Hp, Wp))).reshape(-1)
                        bad = (code_out.view().cpu() != c).nonzero()
                        assert bad.numel() == 0, (f'{what}: {bad.shape[0]} of {c.numel()} pool codes differ from the decisions on {name}, '
                                                  f'first at (window, quad) = {divmod(int(bad[0]), N // 4)}')
                    assert code_out.surroundings_untouched(), f'{what}: a store outside pool_code'
            assert same(first, run()), f'{what}: a second call gave other bits'


# ---------------------------------------------------------------- 4. filter transforms
# (wesup_winograd_pack_weights leaves the bits of the single calls: tests/test_batched_gpu.py asserts exactly that)
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('m', (2, 4))
@pytest.mark.parametrize('Co,Ci', w.PACK_CASES)
def test_filter_transform(lib, stream, Co, Ci, m, kind):
    P = w.wino_positions(m)
    wt = w._data((Co, Ci, 3, 3), kind, 2)
    wd = flat(wt.size).load(torch.from_numpy(wt))
    uf, ud = flat(P * Co * Ci), flat(P * Co * Ci)
    lib.call('wesup_winograd_pack_weight', wd.ptr, uf.ptr, ud.ptr, Co, Ci, m, stream())
    refs = wo.pack_weight(wt, np.float64, m)
    with w.absolute() as ab:
        absrefs = ab.pack_weight(np.abs(wt), np.float64, m)
    exact = m == 2 and kind == 'int'
    for name, got, ref, E in (('u_fwd [p][co][ci]', uf, refs[0], absrefs[0]), ('u_dgrad [p][ci][co]', ud, refs[1], absrefs[1])):
        wcheck(got.view(), ref, gamma(RN[f'pack{m}']) * E, 'int' if exact else 'gauss', f'pack_weight {Co} x {Ci} m = {m} {name} [{kind}]',
               '(position, row, column)')
        assert got.surroundings_untouched(), f'a store outside {name}'
    for f, dg in ((1, 0), (0, 1)):                                            # either panel may be NULL: the other's bits stay
        one = flat(P * Co * Ci)
        lib.call('wesup_winograd_pack_weight', wd.ptr, one.ptr if f else None, one.ptr if dg else None, Co, Ci, m, stream())
        assert torch.equal(one.bits(), (uf if f else ud).bits())


# ---------------------------------------------------------------- 5. filter-gradient reduce
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('r', w.REDUCE_CASES, ids=lambda r: r.id)
def test_filter_grad_reduce(lib, stream, r, kind):
    Co, Ci, m = r.Cout, r.Cin, r.m
    P, tot = w.wino_positions(m), Co * Ci
    for S in r.S:
        s = w.reduce_data(r, kind, S)
        slabs = Pad(P, S, tot + Co, tot + Co + r.pad, col_off=0, extra=0, batch_pad=r.gap).load(torch.from_numpy(s))
        assert w.reduce_variant(Co, Ci, m, slabs.ld, slabs.stride, slabs.ptr) == r.variant
        dw, db = flat(tot * 9), (flat(Co) if r.db else None)
        what = f'{r.id} [{r.variant}] S = {S} [{kind}]'

        def run():
            dw.reset()
            if db is not None:
                db.reset()
            lib.call('wesup_winograd_filter_grad', slabs.ptr, slabs.ld, slabs.stride, S, dw.ptr, None if db is None else db.ptr, Co, Ci, m,
                     stream())
            return dw.bits(), (None if db is None else db.bits())
        first = run()
        s64 = s.astype(np.float64)
        ref = wo.filter_grad(s64[:, :, :tot].sum(1).reshape(P, Co, Ci), np.float64, m)
        with w.absolute() as ab:
            E = ab.filter_grad(np.abs(s64[:, :, :tot]).sum(1).reshape(P, Co, Ci), np.float64, m)
        exact = m == 2 and kind == 'int'
        wcheck(dw.view(), ref.reshape(Co, Ci, 9), gamma(S + RN[f'reduce{m}']) * E.reshape(Co, Ci, 9), 'int' if exact else 'gauss', what + ' dw',
               '(co, ci, tap)')
        assert dw.surroundings_untouched(), f'{what}: a store outside dw'
        if db is not None:
            wcheck(db.view(), s64[5, :, tot:].sum(0).reshape(1, 1, Co), gamma(S) * np.abs(s64[5, :, tot:]).sum(0).reshape(1, 1, Co), kind,
                   what + ' db', '(-, -, co)')
            assert db.surroundings_untouched(), f'{what}: a store outside db'
        assert same(first, run()), f'{what}: a second call gave other bits'
        # the vector and the scalar kernels add the slabs in the same order: rows that differ in their strides only give the same bits
        twin = _reduce_bits.setdefault((Co, Ci, m, S, kind), (r.variant, dw.view().cpu().clone()))
        assert torch.equal(twin[1].view(torch.int32), dw.view().cpu().view(torch.int32)), f'{what}: other bits than {twin[0]}'


_reduce_bits = {}


@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('B,H,W,Ci,Co,rows,edge', w.BIASROW_CASES)
def test_bias_rows_fold_through_the_pre_entry(lib, stream, B, H, W, Ci, Co, rows, edge, kind):
    """wesup_conv3x3_wgrad_winograd_pre with a synthetic bias_part: db is its column sum (exact on integers, the rows in a fixed
    order otherwise); the operands are zeros, so dw has to be zero."""
    h = lib.load()
    T = w.wino_tiles(B, H, W, 4)
    assert h.wesup_winograd_bias_rows(B, H, W, Co) == rows
    part = w._data((rows, Co), kind, 3)
    part_d = Pad(1, rows, Co, Co, col_off=0, extra=0).load(torch.from_numpy(part))
    v = torch.zeros(36 * T * Ci, device=dev())
    dm = torch.zeros(36 * T * Co, device=dev())
    nbytes = h.wesup_conv3x3_wgrad_winograd_workspace_bytes(B, H, W, Ci, Co, 4)
    assert nbytes == w.wgrad_workspace_bytes(B, H, W, Ci, Co, 4)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev())
    dw, db = flat(Co * Ci * 9), flat(Co)

    def run():
        dw.reset()
        db.reset()
        lib.call('wesup_conv3x3_wgrad_winograd_pre', v.data_ptr(), dm.data_ptr(), part_d.ptr, rows, dw.ptr, db.ptr, B, H, W, Ci, Co,
                 ws.data_ptr(), nbytes, stream())
        return dw.bits(), db.bits()
    first = run()
    what = f'bias rows {rows} x {Co} [{kind}]'
    p64 = part.astype(np.float64)
    wcheck(db.view(), p64.sum(0).reshape(1, 1, Co), gamma(rows) * np.abs(p64).sum(0).reshape(1, 1, Co), kind, what + ' db', '(-, -, co)')
    assert bool((dw.view() == 0).all()) and dw.surroundings_untouched() and db.surroundings_untouched(), what
    assert same(first, run()), f'{what}: a second call gave other bits'
    assert h.wesup_conv3x3_wgrad_winograd_pre(v.data_ptr(), dm.data_ptr(), part_d.ptr, rows + 1, dw.ptr, db.ptr, B, H, W, Ci, Co,
                                              ws.data_ptr(), nbytes, stream()) == ERR_INVALID
    assert h.wesup_conv3x3_wgrad_winograd_pre(v.data_ptr(), dm.data_ptr(), part_d.ptr, rows, dw.ptr, db.ptr, B, H, W, Ci, Co,
                                              ws.data_ptr(), nbytes - 1, stream()) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert same(first, (dw.bits(), db.bits())), f'{what}: a refused call wrote to an output'


# ---------------------------------------------------------------- 6. composites
# Roundings of a whole chain (the stages' counts added up, _winocases.ROUNDINGS): forward / input gradient over K channels
#   F(2x2)            in2 + pack2 + (K + 2) + out2             = K + 14      (exact on integers)
#   F(4x4) two kernels in4 + pack4 + (K + 2) + out4            = K + 24
#   F(4x4) one kernel  in4 + pack4 + (K + 2) + fused           = K + 26
# weight gradient over T tiles in S splits:  in + og + (T + 2) + S + reduce = T + S + 10 (F(2x2), exact on integers), T + S + 20;
# its db: F(2x2) the column sums of dM at (1,1): og2 + T + S; F(4x4) any-order sum of 16 T values.
# absref: the Winograd pipeline itself on absolute values (oracle conv_fwd / conv_dgrad / conv_wgrad under _winocases.absolute()).
COMP_ROUTES = (('f2', 2, None), ('two', 4, None), ('one', 4, 0))            # (route, m, fused_min_blocks or None: the default)


class min_blocks:
    """wesup_winograd_set_fused_min_blocks(v) for a block, restored afterwards (None: the default rule stays)"""

    def __init__(self, h, v):
        self.h, self.v = h, v

    def __enter__(self):
        self.was = None if self.v is None else self.h.wesup_winograd_set_fused_min_blocks(self.v)

    def __exit__(self, *exc):
        if self.was is not None:
            self.h.wesup_winograd_set_fused_min_blocks(self.was)


def chain_n(route, K):
    return K + {'f2': 14, 'two': 24, 'one': 26}[route]


def to_nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).permute(0, 3, 1, 2)


def to_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


_comp = {}


def comp_data(lib, stream, B, H, W, Cin, Cout, kind):
    """Host data and float64 references of a composite row (F.conv2d and its autograd), the same for every route"""
    key = (B, H, W, Cin, Cout, kind)
    if _comp.get('key') != key:
        _comp.clear()
        x, dy = w.seed_zeros(w._data((B, H, W, Cin), kind, 1)), w._data((B, H, W, Cout), kind, 4)
        wt, bias = w._data((Cout, Cin, 3, 3), kind, 2, 1.0 if kind == 'int' else (9 * Cin) ** -0.5), w._data((Cout,), kind, 3)
        o = dict(key=key, x=x, dy=dy, wt=wt, bias=bias, old=w._data((B, H, W, Cin), kind, 5), mask=w.mask_data((B, H, W, Cin), kind, 6))
        w64 = torch.from_numpy(wt).double()
        for relu in (0, 1):
            xx = to_nchw(x).clamp_min(0) if relu else to_nchw(x)
            o['fwd', relu] = to_nhwc(F.conv2d(xx, w64, torch.from_numpy(bias).double(), padding=1))
            wv, bv = w64.clone().requires_grad_(True), torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
            F.conv2d(xx, wv, bv, padding=1).backward(to_nchw(dy))
            o['dw', relu], o['db'] = wv.grad.numpy(), bv.grad.numpy()
        o['dx'] = to_nhwc(F.conv_transpose2d(to_nchw(dy), w64, padding=1))
        for m in (2, 4):
            with w.absolute() as ab:
                o['Efwd', m] = ab.conv_fwd(np.abs(x), np.abs(wt), np.abs(bias), m=m)
                o['Edx', m] = ab.conv_dgrad(np.abs(dy), np.abs(wt), m=m)
                o['Edw', m], _ = ab.conv_wgrad(np.abs(x), np.abs(dy), m=m)
        o['Edb'] = np.abs(dy).astype(np.float64).sum((0, 1, 2))
        _comp.update(o)
    return _comp


def packed_filters(lib, stream, o, m):
    Cout, Cin = o['wt'].shape[:2]
    wd = flat(o['wt'].size).load(torch.from_numpy(o['wt']))
    uf, ud = flat(w.wino_positions(m) * Cout * Cin), flat(w.wino_positions(m) * Cout * Cin)
    lib.call('wesup_winograd_pack_weight', wd.ptr, uf.ptr, ud.ptr, Cout, Cin, m, stream())
    return uf, ud


def workspace(h, B, H, W, K, N, m):
    nbytes = h.wesup_conv3x3_winograd_workspace_bytes(B, H, W, K, N, m)
    assert nbytes == w.conv_workspace_bytes(B, H, W, K, N, m) and nbytes > 0
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev()), nbytes


@pytest.mark.parametrize('route,m,minb', COMP_ROUTES, ids=[r[0] for r in COMP_ROUTES])
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('B,H,W,Cin,Cout', w.COMP_CASES)
def test_composite_forward(lib, stream, B, H, W, Cin, Cout, kind, route, m, minb):
    h = lib.load()
    o = comp_data(lib, stream, B, H, W, Cin, Cout, kind)
    takes = w.composite_route(B, H, W, Cin, Cout, m, w.FUSED_MIN_BLOCKS if minb is None else minb)
    uf, _ = packed_filters(lib, stream, o, m)
    xd, bias_d = pixels(o['x'].shape, o['x']), flat(Cout).load(torch.from_numpy(o['bias']))
    ws, nbytes = workspace(h, B, H, W, Cin, Cout, m)
    P, T, Hp, Wp = w.wino_positions(m), w.wino_tiles(B, H, W, m), H // 2, W // 2
    exact = m == 2 and kind == 'int'
    for opts in ((), ('bias',), ('bias', 'relu_in', 'y_relu'), ('bias', 'pool'), ('bias', 'relu_in', 'pool', 'pool_relu', 'v_keep')):
        relu = int('relu_in' in opts)
        now = 'two' if takes == 'one' and 'y_relu' in opts else takes           # a second output takes two kernels
        what = f'fwd {B}x{H}x{W} {Cin} -> {Cout} [{now}] {"+".join(opts) or "bare"} [{kind}]'
        y, y2 = pixels((B, H, W, Cout)), (pixels((B, H, W, Cout)) if 'y_relu' in opts else None)
        yp = pixels((B, Hp, Wp, Cout)) if 'pool' in opts else None
        vk = planes(P, T, Cin, 0)[0] if 'v_keep' in opts else None
        args = lambda nb: (xd.ptr, uf.ptr, bias_d.ptr if 'bias' in opts else None, y.ptr, None if y2 is None else y2.ptr,      # noqa: E731
                           None if yp is None else yp.ptr, int('pool_relu' in opts), None if vk is None else vk.ptr, B, H, W, Cin, Cout, relu, m,
                           ws.data_ptr(), nb, stream())

        def run():
            for t in (y, y2, yp, vk):
                if t is not None:
                    t.reset()
            ws.fill_(0xFF)
            with min_blocks(h, minb):
                lib.call('wesup_conv3x3_fwd_winograd', *args(nbytes))
            return tuple(None if t is None else t.bits() for t in (y, y2, yp, vk))
        first = run()
        want = o['fwd', relu] - (0 if 'bias' in opts else o['bias'].astype(np.float64))
        E = o['Efwd', m] - (0 if 'bias' in opts else np.abs(o['bias']).astype(np.float64))
        wcheck(y.view(), want, gamma(chain_n(now, Cin)) * E, 'int' if exact else 'gauss', what, PIXEL_NAMES)
        got = y.view().reshape(B, H, W, Cout)
        if y2 is not None:
            assert torch.equal(y2.view().reshape(-1).view(torch.int32), relu_bits(got).reshape(-1)), f'{what}: y_relu is not max(y, 0) bit for bit'
        if yp is not None:
            wcheck(yp.view(), pool(got.cpu().double().numpy(), 'pool_relu' in opts), None, 'int', what + ' y_pool against the stored y', PIXEL_NAMES)
        if vk is not None:
            V = wo.input_transform(o['x'], bool(relu), np.float64, m)
            with w.absolute() as ab:
                EV = ab.input_transform(np.abs(o['x']), bool(relu), np.float64, m)
            wcheck(vk.view(), V, gamma(RN[f'in{m}']) * EV, kind, what + ' v_keep', TILE_NAMES, tile_decode(B, H, W, m))
        assert all(t is None or t.surroundings_untouched() for t in (y, y2, yp, vk)), f'{what}: a store outside an output'
        assert same(first, run()), f'{what}: a second call gave other bits'
        for t in (y, y2, yp, vk):
            if t is not None:
                t.reset()
        assert h.wesup_conv3x3_fwd_winograd(*args(nbytes - 1)) == ERR_WORKSPACE
        torch.cuda.synchronize()
        assert all(t is None or bool(torch.isnan(t.buf).all()) for t in (y, y2, yp, vk)), f'{what}: a refused call wrote to an output'


@pytest.mark.parametrize('route,m,minb', COMP_ROUTES, ids=[r[0] for r in COMP_ROUTES])
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('B,H,W,Cin,Cout', w.COMP_CASES)
def test_composite_input_gradient(lib, stream, B, H, W, Cin, Cout, kind, route, m, minb):
    """wesup_conv3x3_dgrad_winograd, _unpool and _gather of the layer Cin -> Cout: the product runs over K = Cout channels."""
    h = lib.load()
    o = comp_data(lib, stream, B, H, W, Cin, Cout, kind)
    takes = w.composite_route(B, H, W, Cout, Cin, m, w.FUSED_MIN_BLOCKS if minb is None else minb)
    _, ud = packed_filters(lib, stream, o, m)
    dyd, mask_d = pixels(o['dy'].shape, o['dy']), pixels(o['mask'].shape, o['mask'])
    ws, nbytes = workspace(h, B, H, W, Cout, Cin, m)
    exact = m == 2 and kind == 'int'
    n = chain_n(takes, Cout)
    for mask, accum in ((0, 0), (1, 0), (0, 1), (1, 1)):
        what = f'dgrad {B}x{H}x{W} {Cin} <- {Cout} [{takes}] {"mask " if mask else ""}{"accum " if accum else ""}[{kind}]'
        dx = pixels((B, H, W, Cin))
        args = lambda nb: (dyd.ptr, ud.ptr, mask_d.ptr if mask else None, dx.ptr, B, H, W, Cin, Cout, accum, m, ws.data_ptr(), nb, stream())      # noqa: E731

        def run():
            dx.reset(torch.from_numpy(o['old']))
            ws.fill_(0xFF)
            with min_blocks(h, minb):
                lib.call('wesup_conv3x3_dgrad_winograd', *args(nbytes))
            return (dx.bits(),)
        first = run()
        want = np.where(o['mask'] > 0, o['dx'], 0.0) if mask else o['dx']
        want, E = (want + o['old'], o['Edx', m] + np.abs(o['old'])) if accum else (want, o['Edx', m])
        wcheck(dx.view(), want, gamma(n) * E, 'int' if exact else 'gauss', what, PIXEL_NAMES)
        assert dx.surroundings_untouched(), f'{what}: a store outside dx'
        assert same(first, run()), f'{what}: a second call gave other bits'
        before = dx.bits()
        assert h.wesup_conv3x3_dgrad_winograd(*args(nbytes - 1)) == ERR_WORKSPACE
        torch.cuda.synchronize()
        assert torch.equal(before, dx.bits()), f'{what}: a refused call wrote to dx'
    if m != 4:
        return
    # through the max-pool backward: the destination holds old content at (2H + 1) x (2W + 1), its trailing row and column stay
    Hu, Wu = 2 * H + 1, 2 * W + 1
    src, old = unpool_source(B, Hu, Wu, H, W, Cin, kind), w._data((B, Hu, Wu, Cin), kind, 7)
    code = first_max(src, H, W)
    src_d, dst = pixels(src.shape, src), pixels(old.shape)
    what = f'dgrad_unpool {B}x{H}x{W} {Cin} <- {Cout} [{takes}] [{kind}]'
    uargs = lambda nb: (dyd.ptr, ud.ptr, src_d.ptr, dst.ptr, B, H, W, Hu, Wu, Cin, Cout, 4, ws.data_ptr(), nb, stream())      # noqa: E731

    def run_unpool():
        dst.reset(torch.from_numpy(old))
        ws.fill_(0xFF)
        with min_blocks(h, minb):
            lib.call('wesup_conv3x3_dgrad_winograd_unpool', *uargs(nbytes))
        return (dst.bits(),)
    first = run_unpool()
    wcheck(dst.view(), scatter(old.astype(np.float64), code, o['dx'], H, W),
           gamma(n) * scatter(np.abs(old).astype(np.float64), code, o['Edx', 4], H, W), 'gauss', what, PIXEL_NAMES)
    assert dst.surroundings_untouched() and same(first, run_unpool()), what
    assert h.wesup_conv3x3_dgrad_winograd_unpool(*uargs(nbytes - 1)) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(first[0], dst.bits()), f'{what}: a refused call wrote to the destination'
    # with the side gradient gathered in the epilogue: one kernel always, for the product shapes it covers
    for unpool in (0, 1):
        shape = (B, 2 * H, 2 * W, Cin) if unpool else (B, H, W, Cin)
        side, rows, area, value, raw = gather_operands(B, shape[1] * shape[2], Cin, kind)
        side_d, row_d = flat(side.size).load(torch.from_numpy(side)), IntPad(rows.size, torch.int32, KMAX - 1, rows)
        area_d = IntPad(area.size, torch.int32, 0, area) if not unpool else None          # (the unpool form: rows divided already)
        base = (raw if unpool else value).reshape(shape)
        src2 = unpool_source(B, 2 * H, 2 * W, H, W, Cin, kind) if unpool else None
        src2_d, dx = (None if src2 is None else pixels(src2.shape, src2)), pixels(shape)
        what = f'dgrad_gather {B}x{H}x{W} {Cin} <- {Cout} {"unpool " if unpool else "mask "}[{kind}]'
        gargs = lambda nb: (dyd.ptr, ud.ptr, None if unpool else mask_d.ptr, None if src2_d is None else src2_d.ptr, dx.ptr, side_d.ptr,      # noqa: E731
                            row_d.ptr, None if area_d is None else area_d.ptr, KMAX, B, H, W, 2 * H * unpool, 2 * W * unpool, Cin, Cout,
                            ws.data_ptr(), nb, stream())
        if w.fused_supported(Cout, Cin, 4) != 2:
            assert h.wesup_conv3x3_dgrad_winograd_gather(*gargs(nbytes)) == ERR_INVALID
            torch.cuda.synchronize()
            assert bool(torch.isnan(dx.buf).all())
            continue

        def run_gather():
            dx.reset()
            ws.fill_(0xFF)
            lib.call('wesup_conv3x3_dgrad_winograd_gather', *gargs(nbytes))
            return (dx.bits(),)
        first = run_gather()
        if unpool:
            c2 = first_max(src2, H, W)
            want, E = scatter(base.copy(), c2, o['dx'], H, W), scatter(np.abs(base), c2, o['Edx', 4], H, W)
        else:
            want, E = base + np.where(o['mask'] > 0, o['dx'], 0.0), np.abs(base) + o['Edx', 4]
        wcheck(dx.view(), want, gamma(chain_n('one', Cout)) * E, 'gauss', what, PIXEL_NAMES)
        assert dx.surroundings_untouched() and row_d.surroundings_untouched() and same(first, run_gather()), what
        dx.reset()
        assert h.wesup_conv3x3_dgrad_winograd_gather(*gargs(nbytes - 1)) == ERR_WORKSPACE
        torch.cuda.synchronize()
        assert bool(torch.isnan(dx.buf).all()), f'{what}: a refused call wrote to dx'


WGRAD_ROWS = sorted({s[:5] for s in w.WGRAD_SPLITS} | set(w.COMP_CASES))


@pytest.mark.parametrize('m', (2, 4))
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('B,H,W,Ci,Cout', WGRAD_ROWS)
def test_composite_weight_gradient(lib, stream, B, H, W, Ci, Cout, kind, m):
    """wesup_conv3x3_wgrad_winograd from x and from the forward's kept V, and (m = 4) wesup_conv3x3_wgrad_winograd_pre from the dual
    transform's operands: the same dw / db as autograd of F.conv2d."""
    h = lib.load()
    o = comp_data(lib, stream, B, H, W, Ci, Cout, kind)
    P, T = w.wino_positions(m), w.wino_tiles(B, H, W, m)
    S = w.wgrad_plan(B, H, W, Ci, Cout, m).S
    nbytes = h.wesup_conv3x3_wgrad_winograd_workspace_bytes(B, H, W, Ci, Cout, m)
    assert nbytes == w.wgrad_workspace_bytes(B, H, W, Ci, Cout, m)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev())
    xd, dyd = pixels(o['x'].shape, o['x']), pixels(o['dy'].shape, o['dy'])
    exact = m == 2 and kind == 'int'
    n_dw = T + S + (10 if m == 2 else 20)
    n_db = (2 + T + S) if m == 2 else 16 * T
    dw, db = flat(Cout * Ci * 9), flat(Cout)

    def verify(what, relu, with_db=True):
        wcheck(dw.view(), o['dw', relu].reshape(Cout, Ci, 9), gamma(n_dw) * o['Edw', m].reshape(Cout, Ci, 9), 'int' if exact else 'gauss',
               what + ' dw', '(co, ci, tap)')
        if with_db:
            wcheck(db.view(), o['db'].reshape(1, 1, Cout), gamma(n_db) * o['Edb'].reshape(1, 1, Cout), kind, what + ' db', '(-, -, co)')
        assert dw.surroundings_untouched() and db.surroundings_untouched(), f'{what}: a store outside an output'

    for relu, want_db in ((0, 1), (1, 1), (0, 0)):
        what = f'wgrad {B}x{H}x{W} {Ci} -> {Cout} m = {m} S = {S}{" relu_in" if relu else ""}{"" if want_db else " no db"} [{kind}]'
        args = lambda nb: (xd.ptr, None, dyd.ptr, dw.ptr, db.ptr if want_db else None, B, H, W, Ci, Cout, relu, m, ws.data_ptr(), nb, stream())      # noqa: E731

        def run():
            dw.reset()
            db.reset()
            ws.fill_(0xFF)
            lib.call('wesup_conv3x3_wgrad_winograd', *args(nbytes))
            return dw.bits(), db.bits()
        first = run()
        verify(what, relu, want_db)
        assert want_db or bool(torch.isnan(db.buf).all())
        assert same(first, run()), f'{what}: a second call gave other bits'
        assert h.wesup_conv3x3_wgrad_winograd(*args(nbytes - 1)) == ERR_WORKSPACE
        torch.cuda.synchronize()
        assert same(first, (dw.bits(), db.bits())), f'{what}: a refused call wrote to an output'
    # from the transformed input the forward kept (x = NULL)
    V = planes(P, T, Ci, 0)[0]
    lib.call('wesup_winograd_input_transform', xd.ptr, V.ptr, 0, B, H, W, Ci, 0, m, stream())
    dw.reset()
    db.reset()
    lib.call('wesup_conv3x3_wgrad_winograd', None, V.ptr, dyd.ptr, dw.ptr, db.ptr, B, H, W, Ci, Cout, 0, m, ws.data_ptr(), nbytes, stream())
    verify(f'wgrad from v_pre {B}x{H}x{W} {Ci} -> {Cout} m = {m} [{kind}]', 0)
    if m != 4:
        return
    # ... and from the dual transform's dM and bias rows
    Vdy, dM = planes(36, T, Cout, 0)[0], planes(36, T, Cout, 0)[0]
    rows = w.bias_rows(B, H, W, Cout)
    part = Pad(1, rows, Cout, Cout, col_off=0, extra=0)
    lib.call('wesup_winograd_dual_transform', dyd.ptr, Vdy.ptr, dM.ptr, part.ptr, B, H, W, Cout, stream())
    dw.reset()
    db.reset()
    lib.call('wesup_conv3x3_wgrad_winograd_pre', V.ptr, dM.ptr, part.ptr, rows, dw.ptr, db.ptr, B, H, W, Ci, Cout, ws.data_ptr(), nbytes,
             stream())
    verify(f'wgrad_pre {B}x{H}x{W} {Ci} -> {Cout} [{kind}]', 0)


# ---------------------------------------------------------------- 7. argument checks: an error code and no launch
def test_argument_checks_leave_every_output_alone(lib, stream):
    h = lib.load()
    B, H, W, C, K, N = 2, 5, 6, 32, 64, 64
    T = w.wino_tiles(B, H, W, 4)
    x = pixels((B, H, W, C), w._data((B, H, W, C), 'int', 1))
    bias, mask = flat(N).load(torch.from_numpy(w._data((N,), 'int', 3))), pixels((B, H, W, N), w._data((B, H, W, N), 'int', 5))
    Vpad = T * C + 12
    V = Pad(36, T, K, K, col_off=0, extra=0, batch_pad=12).load(torch.from_numpy(w._data((36, T, K), 'int', 1)))      # (as [36][T][32]: a prefix)
    U = flat(36 * N * K).load(torch.from_numpy(w._data((36 * N * K,), 'int', 2)))
    y, yp, dst = pixels((B, H, W, N)), pixels((B, H // 2, W // 2, N)), pixels((B, 2 * H, 2 * W, N))
    src = pixels((B, 2 * H, 2 * W, N), w._data((B, 2 * H, 2 * W, N), 'int', 6))
    bits = IntPad(B * H * W * N // 4, torch.uint8, 0xFF)
    code = IntPad(B * (H // 2) * (W // 2) * N // 4, torch.int16, -1)
    side = flat(B * KMAX * N).load(torch.from_numpy(w._data((B * KMAX * N,), 'int', 8)))
    row = IntPad(B * 4 * H * W, torch.int32, 0, np.zeros(B * 4 * H * W, dtype=np.int32))
    dw, db = flat(64 * 32 * 9), flat(64)
    slabs = flat(36 * (64 * 32 + 64)).load(torch.from_numpy(w._data((36 * (64 * 32 + 64),), 'int', 9)))
    outs = (V, y, yp, dst, bits, code, dw, db)
    st = stream()

    def it(x_=x.ptr, V_=V.ptr, pe=Vpad, C_=C, m=4):
        return h.wesup_winograd_input_transform(x_, V_, pe, B, H, W, C_, 0, m, st)

    def itb(V_=V.ptr, pe=Vpad, b_=bits.ptr):
        return h.wesup_winograd_input_transform_bits(x.ptr, V_, pe, b_, B, H, W, C, 0, st)

    def ot(M_=V.ptr, pe=T * K + 12, b_=bias.ptr, mk=mask.ptr, y_=y.ptr, yp_=yp.ptr, C_=N, m=4):
        return h.wesup_winograd_output_transform(M_, pe, b_, mk, y_, None, yp_, 0, B, H, W, C_, 0, m, st)

    def otu(Hu=2 * H, Wu=2 * W, pe=T * K + 12, s_=src.ptr, d_=dst.ptr, m=4):
        return h.wesup_winograd_output_transform_unpool(V.ptr, pe, bias.ptr, None, s_, d_, B, H, W, Hu, Wu, N, m, st)

    def fu(V_=V.ptr, pe=T * K + 12, U_=U.ptr, y_=y.ptr, yp_=None, s_=None, d_=None, Hu=0, Wu=0, K_=K, N_=N, accum=0):
        return h.wesup_winograd_gemm_output_transform(V_, pe, U_, bias.ptr, None, y_, yp_, 0, s_, d_, Hu, Wu, B, H, W, K_, N_, accum, st)

    def ex(bias_=None, yp_=None, code_=None, side_=None, accum=0, s_=None, d_=None, Hu=0, Wu=0):
        return h.wesup_winograd_gemm_output_transform_ex(V.ptr, T * K + 12, U.ptr, bias_, None, None, y.ptr, yp_, 0, code_, s_, None, d_, Hu, Wu,
                                                         side_, row.ptr if side_ else None, None, KMAX if side_ else 0, B, H, W, K, N, accum, st)

    def ga(s_=None, Hu=0, Wu=0, side_=side.ptr, Kmax=KMAX):
        return h.wesup_winograd_gemm_output_transform_gather(V.ptr, T * K + 12, U.ptr, None, dst.ptr if s_ else y.ptr, s_, Hu, Wu, side_, row.ptr,
                                                             None, Kmax, B, H, W, K, N, st)
    before = [t.bits() for t in outs]
    bad = {
        'a pointer off 16 bytes': [it(x_=x.ptr + 4), it(V_=V.ptr + 8), itb(V_=V.ptr + 4), ot(M_=V.ptr + 4), ot(y_=y.ptr + 4), ot(b_=bias.ptr + 4),
                                   ot(mk=mask.ptr + 8), ot(yp_=yp.ptr + 4), otu(s_=src.ptr + 4), otu(d_=dst.ptr + 4), fu(V_=V.ptr + 4),
                                   fu(U_=U.ptr + 4), ga(side_=side.ptr + 4)],
        'plane_elems % 4': [it(pe=T * C + 2), itb(pe=T * C + 6), ot(pe=T * N + 2), otu(pe=T * N + 2), fu(pe=T * K + 2)],
        '0 < plane_elems < T C': [it(pe=T * C - 4), itb(pe=4), ot(pe=T * N - 4), otu(pe=T * N - 4), fu(pe=T * K - 4)],
        'C % 4, C < 32, m = 3': [it(C_=34), it(C_=28), it(m=3), ot(C_=34), ot(C_=28), ot(m=3), otu(m=2), fu(K_=32), fu(K_=96), fu(N_=32), fu(N_=96)],
        'unpool with Hu/2 != H, y_pool or accumulate': [otu(Hu=2 * H + 2), otu(Wu=2 * W - 1), otu(d_=None),
                                                        fu(y_=None, s_=src.ptr, d_=dst.ptr, Hu=2 * H + 2, Wu=2 * W),
                                                        fu(y_=None, yp_=yp.ptr, s_=src.ptr, d_=dst.ptr, Hu=2 * H, Wu=2 * W),
                                                        fu(y_=None, s_=src.ptr, d_=dst.ptr, Hu=2 * H, Wu=2 * W, accum=1),
                                                        fu(y_=None, s_=src.ptr, d_=None, Hu=2 * H, Wu=2 * W)],
        'pool_code without y_pool': [ex(code_=code.ptr), itb(b_=None)],
        'gather with bias, accumulate, y_pool or odd Hu': [ex(bias_=bias.ptr, side_=side.ptr), ex(side_=side.ptr, accum=1),
                                                           ex(side_=side.ptr, yp_=yp.ptr), ga(s_=src.ptr, Hu=2 * H + 1, Wu=2 * W),
                                                           ex(side_=side.ptr, s_=src.ptr, d_=dst.ptr, Hu=2 * H, Wu=2 * W + 1), ga(Kmax=0)],
        'filter_grad': [h.wesup_winograd_filter_grad(slabs.ptr, 64 * 32 + 64, 64 * 32 + 64, 1, dw.ptr, db.ptr, 64, 32, 4, st),
                        h.wesup_winograd_filter_grad(slabs.ptr, 64 * 32 + 63, 64 * 32 + 64, 1, dw.ptr, None, 64, 32, 4, st),
                        h.wesup_winograd_filter_grad(slabs.ptr, 64 * 32 + 64, 64 * 32 + 63, 1, dw.ptr, None, 64, 32, 4, st),
                        h.wesup_winograd_filter_grad(slabs.ptr, 64 * 32 + 64, 64 * 32 + 64, 0, dw.ptr, None, 64, 32, 4, st),
                        h.wesup_winograd_filter_grad(slabs.ptr, 64 * 32 + 64, 64 * 32 + 64, 1, dw.ptr, None, 64, 32, 3, st)],
        'dual transform': [h.wesup_winograd_dual_transform(x.ptr + 4, V.ptr, V.ptr, None, B, H, W, C, st),
                           h.wesup_winograd_dual_transform(x.ptr, V.ptr, V.ptr, db.ptr, B, H, W, 36, st),       # bias rows need C/4 | 256
                           h.wesup_winograd_outgrad_transform(x.ptr, V.ptr, db.ptr, B, H, W, C, 2, None, 0, st)],
    }
    for name, codes in bad.items():
        assert all(c == ERR_INVALID for c in codes), (name, codes)
    torch.cuda.synchronize()
    assert all(torch.equal(a, t.bits()) for a, t in zip(before, outs)), 'a rejected call wrote to an output'
    # ... and the same arguments without the fault go through
    assert it() == 0 and itb() == 0 and fu() == 0 and fu(y_=None, s_=src.ptr, d_=dst.ptr, Hu=2 * H, Wu=2 * W) == 0 and ga() == 0
    assert ex(yp_=yp.ptr, code_=code.ptr) == 0 and ex(side_=side.ptr) == 0
    assert h.wesup_winograd_filter_grad(slabs.ptr, 64 * 32 + 64, 64 * 32 + 64, 1, dw.ptr, None, 64, 32, 4, st) == 0
    torch.cuda.synchronize()
