"""Every GEMM route of csrc/gemm.hip at its tile, K and split edges (the rows of tests/_gemmcases.py; what route a row reaches
is tests/test_gemm_routes_cpu.py's business), each row twice:

  int    A, B, bias, mask and the old output are integers of {-3 .. 3}: every product and partial sum is an integer below
         9 K <= 540 000 < 2^24, so every fp32 sum is exact whatever the tiling, the split or the stream-K cut, and the output has
         to EQUAL the float64 reference.  A lost K-step, bias, row or column shows as a count and a box of wrong elements.
  gauss  Gaussian data, |got - ref64| <= gamma (|A| |B| + |bias| + |old|) per element with gamma = n u / (1 - n u), u = 2^-24,
         n = K + 2: the textbook bound of an fp32 dot product summed in any order (Higham, Accuracy and Stability of Numerical
         Algorithms, 2nd ed., section 3.1) -- derived, loose for a correct kernel, far below a lost term or reduced precision.

In both: operands and outputs are views inside larger allocations of the test's own.  The padding columns and the rows above
and below the operands are NaN (a read outside the operand poisons the result), the output's surroundings are a NaN sentinel
whose bits must survive, and a second call must give the same bits.
Epilogue order (include/wesup_hip.h): ReLU on load, bias, mask > 0, + old content (ACCUM), RELU_OUT."""
import ctypes

import pytest
import torch

import _gemmcases as g
from test_kernels_gpu import dev, rnd

pytestmark = pytest.mark.gpu

RELU_IN, RELU_OUT, ACCUM, MASK = 1, 2, 4, 8
COMBOS = [('none', 0), ('relu_in', RELU_IN), ('relu_out', RELU_OUT), ('mask', MASK), ('accum', ACCUM),
          ('all', RELU_IN | RELU_OUT | ACCUM | MASK)]
PASSES = ('int', 'gauss')
NAN_BITS = 0x7fc00000
U = 2.0 ** -24
ERR_INVALID, ERR_WORKSPACE = -1, -3


def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope='module')
def stream():
    from wesup_amd import ops
    return ops._stream


class Pad:
    """A (nb, rows, cols) tensor as a view inside one allocation filled with NaN: `ld` floats per row with the columns starting
    at col_off, a spare row above, `extra` rows below each item, `batch_pad` more floats between the items."""

    def __init__(self, nb, rows, cols, ld, col_off=4, extra=2, batch_pad=0):
        assert cols + col_off <= ld
        self.sizes = (nb, rows, cols)
        self.strides = ((rows + extra) * ld + batch_pad, ld, 1)
        self.offset = ld + col_off
        self.ld, self.stride = ld, self.strides[0]
        self.buf = torch.full((self.offset + nb * self.strides[0] + ld,), float('nan'), dtype=torch.float32, device=dev())

    def view(self, buf=None):
        return (self.buf if buf is None else buf).as_strided(self.sizes, self.strides, self.offset)

    def load(self, t):
        self.view().copy_(t.reshape(self.sizes).to(self.buf.device))
        return self

    def reset(self, t=None):
        self.buf.fill_(float('nan'))
        return self if t is None else self.load(t)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.offset

    def surroundings_untouched(self):
        a = self.buf.clone()
        self.view(a).fill_(float('nan'))
        return bool((a.view(torch.int32) == NAN_BITS).all())

    def bits(self):
        return self.buf.view(torch.int32).clone()


def data(shape, kind, seed, scale=1.0):
    if kind == 'int':
        return torch.randint(-3, 4, shape, generator=torch.Generator().manual_seed(seed)).float()
    return rnd(*shape, seed=seed, scale=scale)


def where_wrong(bad, tile, what):
    """Count and bounding box of the wrong elements of an (nb, M, N) result, in element and tile coordinates."""
    idx = bad.nonzero()
    b, r, c = idx[:, 0], idx[:, 1], idx[:, 2]
    bm, bn = tile
    return (f'{what}: {idx.shape[0]} of {bad.numel()} elements wrong; products {int(b.min())}..{int(b.max())}, '
            f'rows {int(r.min())}..{int(r.max())} of {bad.shape[1]}, columns {int(c.min())}..{int(c.max())} of {bad.shape[2]}; '
            f'{bm} x {bn} tiles: rows of tiles {int(r.min()) // bm}..{int(r.max()) // bm}, columns of tiles '
            f'{int(c.min()) // bn}..{int(c.max()) // bn}; first at (product, row, column) = {tuple(int(v) for v in idx[0])}')


def check(got, ref, bound, kind, tile, what):
    """got (nb, M, N) fp32 from the device against ref float64: equal (int), or within the per-element bound (gauss)."""
    got = got.detach().cpu().double().reshape(ref.shape)
    if kind == 'int':
        bad = ~(got == ref)
    else:
        bad = ~((got - ref).abs() <= bound)              # (a NaN fails either)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(where_wrong(bad, tile, what) + f': got {float(got[i])!r}, want {float(ref[i])!r}'
                             + ('' if kind == 'int' else f', bound {float(bound[i])!r}'))


# ---------------------------------------------------------------- NT family
_nt_cache = {}


def nt_operands(key, kind, nb, M, N, K):
    """Host data of one row and its float64 products, computed once and shared by the row's flag combinations."""
    if _nt_cache.get('key') != (key, kind):
        _nt_cache.clear()
        A = data((nb, M, K), kind, 1)
        B = data((nb, N, K), kind, 2, K ** -0.5)
        _nt_cache.update(key=(key, kind), A=A, B=B, bias=data((nb, N), kind, 3), mask=data((nb, M, N), kind, 5),
                         old=data((nb, M, N), kind, 4), P={}, E={})
    return _nt_cache


def nt_products(c, relu_in):
    if relu_in not in c['P']:
        A = c['A'].double().clamp_min(0) if relu_in else c['A'].double()
        Bt = c['B'].double().transpose(1, 2)
        c['P'][relu_in] = A @ Bt
        c['E'][relu_in] = A.abs() @ Bt.abs()
    return c['P'][relu_in], c['E'][relu_in]


def nt_reference(c, flags, bias, K):
    """bias: (nb, N) float64 or None -> (reference, bound), float64"""
    P, E = nt_products(c, bool(flags & RELU_IN))
    ref, bound = P, E
    if bias is not None:
        ref = ref + bias[:, None, :]
        bound = bound + bias.abs()[:, None, :]
    if flags & MASK:
        ref = torch.where(c['mask'] > 0, ref, torch.zeros((), dtype=torch.float64))
    if flags & ACCUM:
        ref = ref + c['old'].double()
        bound = bound + c['old'].double().abs()
    if flags & RELU_OUT:
        ref = ref.clamp_min(0)
    return ref, gamma(K + 2) * bound


@pytest.mark.parametrize('combo', COMBOS, ids=[n for n, _ in COMBOS])
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('case', g.NT_CASES, ids=lambda c: c.id)
def test_gemm_nt_route(lib, stream, case, kind, combo):
    name, flags = combo
    M, N, K = case.M, case.N, case.K
    c = nt_operands(case.id, kind, 1, M, N, K)
    A = Pad(1, M, K, K + 8).load(c['A'])
    B = Pad(1, N, K, K + 8).load(c['B'])
    C = Pad(1, M, N, N + 8)
    mask = Pad(1, M, N, N + 12).load(c['mask']) if flags & MASK else None           # ldmask != N, != ldc
    bias = None if name == 'mask' else c['bias'][0].to(dev())                          # ('mask' also runs the NULL bias)
    full = lib.load().wesup_gemm_nt_workspace_bytes(M, N, K)
    ws_bytes = {None: 0, 'full': full, 'short': full - 1}[case.ws]
    ws = torch.full((max(full, 16),), 0xFF, dtype=torch.uint8, device=dev()) if case.ws else None
    assert (full > 0) == (case.ws is not None)

    def run():
        C.reset(c['old'])
        lib.call('wesup_gemm_nt', A.ptr, A.ld, B.ptr, B.ld, None if bias is None else bias.data_ptr(), C.ptr, C.ld,
                 None if mask is None else mask.ptr, 0 if mask is None else mask.ld, M, N, K, flags,
                 None if ws is None else ws.data_ptr(), ws_bytes, stream())
        return C.bits()
    first = run()
    ref, bound = nt_reference(c, flags, None if bias is None else c['bias'].double(), K)
    check(C.view(), ref, bound, kind, g.NT_TILE[case.route], f'{case.id} [{case.route}] {name}')
    assert C.surroundings_untouched(), 'a store outside the M x N slice'
    assert torch.equal(first, run()), 'a second call gave other bits'


def _batched(lib, stream, case, kind, entry, bias_mode):
    nb, M, N, K = case.nbatch, case.M, case.N, case.K
    c = nt_operands(case.id, kind, nb, M, N, K)
    A = Pad(nb, M, K, K + 8).load(c['A'])                                             # lda > K, strideA > M lda
    B = Pad(nb, N, K, K + 8).load(c['B'])
    C = Pad(nb, M, N, N + 8, extra=3)                                                  # strideC > M ldc
    bias = bias_ref = None
    if bias_mode == 'strided':
        bias = Pad(nb, 1, N, N + 8).load(c['bias'])
        bias_ref = c['bias'].double()
    elif bias_mode == 'shared':
        bias = Pad(1, 1, N, N + 8).load(c['bias'][:1])
        bias_ref = c['bias'][:1].double().expand(nb, N)

    def run():
        C.reset(c['old'])
        if entry == 'wesup_gemm_nt_batched':
            lib.call(entry, A.ptr, A.ld, A.stride, B.ptr, B.ld, B.stride, C.ptr, C.ld, C.stride, nb, M, N, K, stream())
        else:
            lib.call(entry, A.ptr, A.ld, A.stride, B.ptr, B.ld, B.stride, None if bias is None else bias.ptr,
                     bias.stride if bias_mode == 'strided' else 0, C.ptr, C.ld, C.stride, nb, M, N, K, stream())
        return C.bits()
    first = run()
    ref, bound = nt_reference(c, 0, bias_ref, K)
    check(C.view(), ref, bound, kind, g.NT_TILE[case.route], f'{case.id} [{case.route}] bias {bias_mode}')
    assert C.surroundings_untouched(), 'a store outside the M x N slices'
    assert torch.equal(first, run()), 'a second call gave other bits'


@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('case', g.NTB_CASES, ids=lambda c: c.id)
def test_gemm_nt_batched_route(lib, stream, case, kind):
    _batched(lib, stream, case, kind, 'wesup_gemm_nt_batched', None)


@pytest.mark.parametrize('bias_mode', g.BIAS_MODES)
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('case', g.NTBB_CASES, ids=lambda c: c.id)
def test_gemm_nt_batched_bias_route(lib, stream, case, kind, bias_mode):
    _batched(lib, stream, case, kind, 'wesup_gemm_nt_batched_bias', bias_mode)


# ---------------------------------------------------------------- TN family
_tn_cache = {}


def tn_operands(key, kind, nb, M, N, K):
    if _tn_cache.get('key') != (key, kind):
        _tn_cache.clear()
        _tn_cache.update(key=(key, kind), A=data((nb, K, M), kind, 1), B=data((nb, K, N), kind, 2, K ** -0.5), P={}, E={})
    return _tn_cache


def tn_reference(c, relu_b, K):
    if relu_b not in c['P']:
        At = c['A'].double().transpose(1, 2)
        B = c['B'].double().clamp_min(0) if relu_b else c['B'].double()
        c['P'][relu_b] = At @ B
        c['E'][relu_b] = At.abs() @ B.abs()
    return c['P'][relu_b], gamma(K + 2) * c['E'][relu_b]


def _variant_id(v):
    return '-'.join(n for n, on in zip(('relu_b', 'colsum', 'oddld'), v) if on) or 'plain'


TN_RUNS = [(c, v) for c in g.TN_CASES for v in c.variants]


@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('case,variant', TN_RUNS, ids=[f'{c.id}-{_variant_id(v[:3])}' for c, v in TN_RUNS])
def test_gemm_tn_route(lib, stream, case, variant, kind):
    relu_b, colsum, odd, store = variant
    M, N, K = case.M, case.N, case.K
    c = tn_operands(case.id, kind, 1, M, N, K)
    A = Pad(1, K, M, M + 8).load(c['A'])                                               # lda > M
    B = Pad(1, K, N, N + 8).load(c['B'])
    C = Pad(1, M, N, N + (5 if odd else 8))
    cs = Pad(1, 1, M, M + 8) if colsum else None
    nbytes = lib.load().wesup_gemm_tn_workspace_bytes(M, N, K)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev())

    def run():
        C.reset()
        ws.fill_(0xFF)                                                                 # NaN: a slab element read but never written shows
        if cs is not None:
            cs.reset()
        lib.call('wesup_gemm_tn', A.ptr, A.ld, B.ptr, B.ld, C.ptr, C.ld, None if cs is None else cs.ptr, M, N, K, relu_b,
                 ws.data_ptr(), nbytes, stream())
        return C.bits(), (None if cs is None else cs.bits())
    first = run()
    ref, bound = tn_reference(c, relu_b, K)
    what = f'{case.id} [{case.tile} x {case.tile}, S = {case.S}, {store}{", weighted" if case.weighted else ""}] {_variant_id(variant[:3])}'
    check(C.view(), ref, bound, kind, (case.tile, case.tile), what)
    assert C.surroundings_untouched(), 'a store outside the M x N slice'
    if cs is not None:
        a64 = c['A'].double()
        check(cs.view(), a64.sum(1, keepdim=True), gamma(K + 2) * a64.abs().sum(1, keepdim=True), kind, (1, case.tile),
              what + ' column sums')
        assert cs.surroundings_untouched(), 'a store outside the M column sums'
    second = run()
    assert torch.equal(first[0], second[0]), 'a second call gave other bits'
    assert cs is None or torch.equal(first[1], second[1]), 'a second call gave other column sums'


TNB_RUNS = [(c, v) for c in g.TNB_CASES for v in c.variants]


@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('case,variant', TNB_RUNS,
                         ids=[f'{c.id}-' + ('-'.join(n for n, on in zip(('relu_b', 'oddstride'), v) if on) or 'plain') for c, v in TNB_RUNS])
def test_gemm_tn_batched_route(lib, stream, case, variant, kind):
    relu_b, odd, store = variant
    nb, M, N, K = case.nbatch, case.M, case.N, case.K
    c = tn_operands(case.id, kind, nb, M, N, K)
    A = Pad(nb, K, M, M + 8).load(c['A'])
    B = Pad(nb, K, N, N + 8).load(c['B'])                                              # row-strided B and C
    C = Pad(nb, M, N, N + 8, extra=1, batch_pad=1 if odd else 0)
    assert C.stride % 2 == (1 if odd else 0)
    nbytes = lib.load().wesup_gemm_tn_batched_workspace_bytes(nb, M, N, K)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev())

    def run():
        C.reset()
        ws.fill_(0xFF)
        lib.call('wesup_gemm_tn_batched', A.ptr, A.ld, A.stride, B.ptr, B.ld, B.stride, C.ptr, C.ld, C.stride, nb, M, N, K,
                 relu_b, ws.data_ptr(), nbytes, stream())
        return C.bits()
    first = run()
    ref, bound = tn_reference(c, relu_b, K)
    check(C.view(), ref, bound, kind, (case.tile, case.tile), f'{case.id} [{case.tile} x {case.tile}, S = {case.S}, {store}]')
    assert C.surroundings_untouched(), 'a store outside the M x N slices'
    assert torch.equal(first, run()), 'a second call gave other bits'


# ---------------------------------------------------------------- column sums, transposes
@pytest.mark.parametrize('kind', PASSES)
@pytest.mark.parametrize('M,N,pad', g.COLSUM_CASES)
def test_colsum_chunks_and_strides(lib, stream, M, N, pad, kind):
    a = data((1, M, N), kind, 7)
    A = Pad(1, M, N, N + pad, col_off=4 if pad else 0).load(a)
    out = Pad(1, 1, N, N + 8)
    nbytes = lib.load().wesup_colsum_workspace_bytes(M, N)
    assert nbytes == g.colsum_workspace_bytes(M, N)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev())

    def run():
        out.reset()
        ws.fill_(0xFF)
        lib.call('wesup_colsum', A.ptr, A.ld, out.ptr, M, N, ws.data_ptr(), nbytes, stream())
        return out.bits()
    first = run()
    a64 = a.double()
    check(out.view(), a64.sum(1, keepdim=True), gamma(M + 2) * a64.abs().sum(1, keepdim=True), kind, (1, 64),
          f'colsum {M} x {N}, lda {A.ld}, {g.colsum_chunks(M, N)} chunks')
    assert out.surroundings_untouched() and torch.equal(first, run())


@pytest.mark.parametrize('rows,cols', g.TRANSPOSE_CASES)
def test_transpose_tiles(lib, stream, rows, cols):
    a = rnd(1, rows, cols, seed=8)
    src = Pad(1, rows, cols, cols, col_off=0).load(a)
    dst = Pad(1, cols, rows, rows, col_off=0)
    lib.call('wesup_transpose', src.ptr, dst.ptr, rows, cols, stream())
    assert torch.equal(dst.view().cpu(), a.transpose(1, 2)) and dst.surroundings_untouched()


def _transpose_items(lib, shapes):
    srcs = [Pad(1, r, c, c, col_off=0).load(rnd(1, r, c, seed=20 + i)) for i, (r, c) in enumerate(shapes)]
    dsts = [Pad(1, c, r, r, col_off=0) for r, c in shapes]
    arr = (lib.TransposeItem * len(shapes))()
    for i, (r, c) in enumerate(shapes):
        arr[i].src, arr[i].dst, arr[i].rows, arr[i].cols = srcs[i].ptr, dsts[i].ptr, r, c
    return srcs, dsts, arr


@pytest.mark.parametrize('n', [1, 3, g.TRANSPOSE_MAX])
def test_transpose_batched_unequal_items(lib, stream, n):
    kinds = [(1, 1), (33, 65), (32, 32), (5, 100), (64, 31), (97, 2), (1, 40)]
    shapes = [kinds[i % len(kinds)] for i in range(n)]
    srcs, dsts, arr = _transpose_items(lib, shapes)
    lib.call('wesup_transpose_batched', ctypes.cast(arr, ctypes.c_void_p), n, stream())
    for i, (s, d) in enumerate(zip(srcs, dsts)):
        assert torch.equal(d.view(), s.view().transpose(1, 2)), f'item {i} of {n}: {shapes[i]}'
        assert d.surroundings_untouched(), f'item {i} of {n}: a store outside the output'


# ---------------------------------------------------------------- argument checks: an error code and no launch
def test_argument_checks_leave_the_output_alone(lib, stream):
    h = lib.load()
    M, N, K = 70, 68, 96
    A = Pad(1, M, K, K + 8).load(data((1, M, K), 'int', 1))
    B = Pad(1, N, K, K + 8).load(data((1, N, K), 'int', 2))
    mask = Pad(1, M, N, N + 12).load(data((1, M, N), 'int', 5))
    C = Pad(1, 96, N, N + 8)                                # (room for the TN shape below as well)
    before = C.bits()

    def nt(a=A.ptr, c=C.ptr, m=mask.ptr, N_=N, K_=K, flags=0):
        return h.wesup_gemm_nt(a, A.ld, B.ptr, B.ld, None, c, C.ld, m, mask.ld, M, N_, K_, flags, None, 0, stream())
    assert nt(K_=48) == ERR_INVALID                         # K % 32 != 0
    assert nt(N_=66) == ERR_INVALID                         # N % 4 != 0
    assert nt(a=A.ptr + 4) == ERR_INVALID                   # a misaligned operand ...
    assert nt(c=C.ptr + 8) == ERR_INVALID                   # ... and output
    assert nt(m=None, flags=MASK) == ERR_INVALID            # MASK without a mask
    assert h.wesup_gemm_nt_batched(A.ptr, A.ld, A.stride, B.ptr, B.ld, B.stride, C.ptr, C.ld, C.stride, 1, M, N, 48, stream()) == ERR_INVALID
    assert h.wesup_gemm_nt_batched_bias(A.ptr, A.ld, A.stride, B.ptr, B.ld, B.stride, None, 0, C.ptr, C.ld, C.stride, 1, M, 66, K,
                                        stream()) == ERR_INVALID
    # TN: A is K x M there; N % 4, a misaligned operand, a workspace one byte short
    Kt, Mt, Nt = 70, 96, 68
    nbytes = h.wesup_gemm_tn_workspace_bytes(Mt, Nt, Kt)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())

    def tn(a=A.ptr, N_=Nt, nb=nbytes):
        return h.wesup_gemm_tn(a, A.ld, mask.ptr, mask.ld, C.ptr, C.ld, None, Mt, N_, Kt, 0, ws.data_ptr(), nb, stream())
    assert tn(N_=66) == ERR_INVALID
    assert tn(a=A.ptr + 4) == ERR_INVALID
    assert tn(nb=nbytes - 1) == ERR_WORKSPACE
    nbb = h.wesup_gemm_tn_batched_workspace_bytes(1, Mt, Nt, Kt)
    assert h.wesup_gemm_tn_batched(A.ptr, A.ld, A.stride, mask.ptr, mask.ld, mask.stride, C.ptr, C.ld, C.stride, 1, Mt, Nt, Kt, 0,
                                   ws.data_ptr(), nbb - 1, stream()) == ERR_WORKSPACE
    assert h.wesup_colsum(A.ptr, A.ld, C.ptr, M, 66, ws.data_ptr(), nbytes, stream()) == ERR_INVALID
    assert h.wesup_colsum(A.ptr, A.ld, C.ptr, M, 64, ws.data_ptr(), h.wesup_colsum_workspace_bytes(M, 64) - 1, stream()) == ERR_WORKSPACE
    _, _, arr = _transpose_items(lib, [(2, 3)] * (g.TRANSPOSE_MAX + 1))
    assert h.wesup_transpose_batched(ctypes.cast(arr, ctypes.c_void_p), g.TRANSPOSE_MAX + 1, stream()) == ERR_INVALID
    assert h.wesup_transpose(A.ptr, C.ptr, 0, 4, stream()) == ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(before, C.bits()), 'a rejected call wrote to the output'
