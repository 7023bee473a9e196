"""The Winograd case tables (tests/_winocases.py) reach the kernels, sizes and edges they claim, the restated host decisions agree
with the library wherever the C ABI shows them (tile counts, weight floats, fused_supported / fused_route, bias rows and the three
workspace queries are host code), and the premise of the GPU test's integer pass holds on the rows' own data: the absolute-value
pipeline times 2^f stays below 2^24 (f fractional bits), and the oracle in fp32 equals the oracle in float64.  No GPU.

What checks the values is tests/test_wino_routes_gpu.py."""
import os

import numpy as np
import pytest

import _gemmcases as g
import _winocases as w
from oracle import winograd_oracle as wo


@pytest.fixture(scope='module')
def h():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


BAR = w.NT_STREAM_BYTES


# ---------------------------------------------------------------- the tables
def test_activation_rows_carry_the_edges_they_name():
    by = {r.id: r for r in w.ACT_CASES}
    assert all(w.wino_shape_ok(r.B, r.H, r.W, r.C, r.C, m) for r in w.ACT_CASES for m in (2, 4))
    r = by['act-1x1x1x32']
    assert w.wino_tiles(r.B, r.H, r.W, 4) == 1 and w.wino_tiles(r.B, r.H, r.W, 2) == 1
    r = by['act-2x5x7x32']
    assert (r.H % 4, r.W % 4) == (1, 3) and r.H % 2 and r.W % 2
    r = by['act-2x6x10x64']
    assert w.wino_tiles(r.B, r.H, r.W, 4) * (r.C // 4) == 192 and w.transform_blocks(r.B, r.H, r.W, r.C, 4) == 1
    r = by['act-3x13x9x128']
    T = w.wino_tiles(r.B, r.H, r.W, 4)
    assert T * (r.C // 4) == 4 * 256 + 128 and w.transform_blocks(r.B, r.H, r.W, r.C, 4) == 5 and w.bias_rows(r.B, r.H, r.W, r.C) == 5
    assert [w.xcd_remap(b, 5) for b in range(5)] == [0, 1, 2, 3, 4]         # (up to 8 blocks the remap is the identity ...)
    r = by['act-5x13x18x128']                                                # ... beyond, it is not: the row that shows the order of the bias rows
    assert w.wino_tiles(r.B, r.H, r.W, 4) * (r.C // 4) == 12 * 256 + 128 and w.bias_rows(r.B, r.H, r.W, r.C) == 13 and 'dual-bias' in w.act_entries(r)
    assert sorted(w.xcd_remap(b, 13) for b in range(13)) == list(range(13)) and [w.xcd_remap(b, 13) for b in range(4)] == [0, 2, 4, 6]
    r = by['act-3x9x8x36']
    assert r.C // 4 == 9 and not w.block_colsum_ok(r.C) and w.bias_rows(r.B, r.H, r.W, r.C) == 0 and 'dual-bias' not in w.act_entries(r)
    assert 'og4-db' in w.act_entries(r)
    # C/4 | 256 from both sides
    a, b = by['act-1x4x4x1024'], by['act-1x4x4x1028']
    assert (a.C // 4, b.C // 4) == (256, 257) and w.block_colsum_ok(a.C) and not w.block_colsum_ok(b.C)
    assert w.bias_rows(a.B, a.H, a.W, a.C) == 1 and w.bias_rows(b.B, b.H, b.W, b.C) == 0
    assert 'dual-bias' in w.act_entries(a) and 'dual-bias' not in w.act_entries(b) and 'og4-db' in w.act_entries(b)
    # the 16 MiB bar of the single and of the dual transforms from both sides
    lo, hi = by['act-1x120x120x128'], by['act-1x121x121x128']
    assert 4 * 36 * 900 * 128 == 16588800 < BAR < 4 * 36 * 961 * 128 == 17713152
    assert not w.nt_single(lo.B, lo.H, lo.W, lo.C) and w.nt_single(hi.B, hi.H, hi.W, hi.C) and not w.nt_single(hi.B, hi.H, hi.W, hi.C, 2)
    lo, hi = by['act-1x84x84x128'], by['act-1x88x88x128']
    assert 2 * 4 * 36 * 441 * 128 == 16257024 < BAR < 2 * 4 * 36 * 484 * 128 == 17842176
    assert not w.nt_dual(lo.B, lo.H, lo.W, lo.C) and w.nt_dual(hi.B, hi.H, hi.W, hi.C)
    assert not w.nt_single(hi.B, hi.H, hi.W, hi.C)                           # (only the dual launch streams there)
    # every entry runs on some row, and every small row runs them all
    assert {e for r in w.ACT_CASES for e in w.act_entries(r)} == set(w.ACT_ENTRIES)
    small = ('act-1x1x1x32', 'act-2x5x7x32', 'act-2x6x10x64', 'act-3x13x9x128', 'act-3x9x8x36')
    assert all(by[i].entries is None for i in small)
    # NT of every row, by launch kind: only the rows named for it stream
    single = [r.id for r in w.ACT_CASES if w.nt_single(r.B, r.H, r.W, r.C) and set(w.act_entries(r)) & {'in4', 'bits', 'og4', 'og4-db'}]
    dual = [r.id for r in w.ACT_CASES if w.nt_dual(r.B, r.H, r.W, r.C) and set(w.act_entries(r)) & {'dual', 'dual-bias'}]
    assert single == ['act-1x121x121x128'] and dual == ['act-1x88x88x128']


def test_output_rows_carry_the_edges_they_name():
    by = {r.id: r for r in w.OUT_CASES}
    assert all(w.wino_shape_ok(r.B, r.H, r.W, r.C, r.C, m) for r in w.OUT_CASES for m in (2, 4))
    assert by['out-1x1x1x32'].H // 2 == 0 and by['out-1x2x2x32'].H // 2 == 1
    r = by['out-2x5x7x32']
    assert r.H % 2 and r.W % 2 and r.W % 4 == 3 and r.H % 4 == 1             # clamped columns at both m; a row and a column outside every window
    assert by['out-3x9x8x36'].C // 4 == 9 and w.transform_blocks(3, 13, 9, 128, 4) == 5
    assert len(w.OUT_COMBOS) == 48 and len(set(w.OUT_COMBOS)) == 48 and len(w.UNPOOL_COMBOS) == 8


def test_fused_rows_carry_the_edges_they_name():
    assert {f for f, _ in w.FUSED_OPTIONS} == set(w.FUSED_FORMS)
    for form, o in w.FUSED_OPTIONS:
        assert w.fused_form(o) == form, (form, o)
        assert not ('side' in o and ({'bias', 'accum', 'pool'} & set(o)))        # what the gather forms refuse
        assert 'code' not in o or 'pool' in o
    opts = {o for _, o in w.FUSED_OPTIONS}
    # the table of the issue, form by form
    assert {('bias',), ('bias', 'pool'), ('pool', 'pool_relu', 'code')} <= opts
    assert {('bias', 'bits'), ('bias', 'accum'), ('bias', 'bits', 'accum'), ('side',)} <= opts
    assert {('bias', 'unpool_code'), ('unpool_code', 'side')} <= opts
    assert {('bias', 'mask'), ('bias', 'mask', 'accum'), ('bias', 'unpool_src'), ('side', 'area'), ('unpool_src', 'side', 'area')} <= opts
    assert all(w.fused_supported(r.K, r.N, 4) == 2 and w.wino_shape_ok(r.B, r.H, r.W, r.K, r.N, 4) for r in w.FUSED_CASES)
    assert {r.K for r in w.FUSED_CASES} == {64, 128, 256} and {r.N for r in w.FUSED_CASES} >= {64, 128, 192}
    tiles = {(r.B, r.H, r.W): w.wino_tiles(r.B, r.H, r.W, 4) for r in w.FUSED_CASES}
    assert tiles[(1, 2, 2)] == 1 and tiles[(3, 9, 8)] == 18 and tiles[(2, 13, 21)] == 48 and tiles[(4, 13, 21)] == 96
    assert 13 % 4 == 1 and 21 % 4 == 1 and 24 < 32 < 48                      # 24 tiles an image: the boundary sits inside the first block
    assert w.fused_grid(48, 64) == (2, 1) and 48 - 32 == 16
    assert w.fused_grid(96, 192) == (3, 3) and any((r.B, r.H, r.W, r.N) == (4, 13, 21, 192) for r in w.FUSED_CASES)
    # the streaming-store bar of the plain and of the unpooling launch
    assert not w.nt_fused(1, 128, 128, 256) and w.nt_fused(1, 129, 128, 256) and 4 * 129 * 128 * 256 == 16908288
    assert not w.nt_fused(1, 64, 64, 256, True) and w.nt_fused(1, 65, 64, 256, True) and w.nt_fused(1, 66, 64, 256, True)
    nt = [r.id for r in w.FUSED_CASES for _, o in w.fused_options(r) if w.nt_fused(r.B, r.H, r.W, r.N, bool({'unpool_src', 'unpool_code'} & set(o)))]
    assert set(nt) == {'fu-1x129x128-64x256', 'fu-1x66x64-64x256'}
    big = [r for r in w.FUSED_CASES if r.only]
    assert {(r.H, w.nt_fused(r.B, r.H, r.W, r.N, 'side' in r.only[0])) for r in big} == {(128, False), (129, True), (64, False), (66, True)}
    # the 200-block rule from both sides, and what lifts it
    assert w.fused_route(64, 64, 4, 200 * 32) == 2 and w.fused_route(64, 64, 4, 199 * 32) == 0 and w.fused_route(64, 64, 4, 199 * 32 + 1) == 2
    assert w.fused_route(64, 128, 4, 100 * 32) == 2 and w.fused_route(64, 128, 4, 99 * 32 + 32) == 2 and w.fused_route(64, 128, 4, 99 * 32) == 0
    assert w.fused_route(64, 64, 4, 1, min_blocks=0) == 2 and w.fused_route(512, 64, 4, 10 ** 6) == 0


def test_reduce_rows_reach_their_kernels():
    assert {r.variant for r in w.REDUCE_CASES} == set(w.REDUCE_VARIANTS)
    for r in w.REDUCE_CASES:
        elems = r.Cout * r.Cin + r.Cout
        for S in r.S:
            stride, batch = elems + r.pad, S * (elems + r.pad) + r.gap
            # (the GPU test's slabs begin `stride` floats into a 16-byte aligned allocation)
            assert w.reduce_variant(r.Cout, r.Cin, r.m, stride, batch, 4 * stride) == r.variant, (r.id, S)
        assert not r.db or r.m == 2
    by = {r.id: r for r in w.REDUCE_CASES}
    assert 128 * 252 // 64 == 504 < 512 == 128 * 256 // 64
    assert by['red-128x252-f4'].variant == 'f4-16v' and by['red-128x256-f4'].variant == 'f4-64v'
    assert (5 * 7) % 4 and w.reduce_grid(5, 7, 4, 'f4-16') == (3, 0) and w.reduce_grid(260, 32, 2, 'f2', db=True) == (130, 2)
    tails = {(S % 4, S // 4 > 0) for r in w.REDUCE_CASES if r.variant.endswith('v') for S in r.S}
    assert {s for s, _ in tails} == {0, 1, 2, 3} and {(S // 2 > 0, S % 2) for S in by['red-36x32-f4-odd'].S} == {(False, 1), (True, 0), (True, 1)}
    assert set(by['red-36x32-f4'].S) == {1, 2, 3, 4, 5, 7}
    for B, H, W, Ci, Cout, rows, _ in w.BIASROW_CASES:
        assert w.bias_rows(B, H, W, Cout) == rows
    rows = [c[5] for c in w.BIASROW_CASES]
    assert 545 in rows and 545 > 512 and (545 - 512) // 64 == 0 and min(rows) == 1 and any(1 < n < 64 for n in rows)


def test_composite_rows_reach_their_routes():
    routes = set()
    for B, H, W, Cin, Cout in w.COMP_CASES:
        for K, N in ((Cin, Cout), (Cout, Cin)):
            assert K % 32 == 0 and w.conv_workspace_bytes(B, H, W, K, N, 4) > 0
            routes |= {w.composite_route(B, H, W, K, N, 2), w.composite_route(B, H, W, K, N, 4), w.composite_route(B, H, W, K, N, 4, 0)}
            assert w.composite_route(B, H, W, K, N, 4) == 'two'              # small grids: the 200-block rule sends them to two kernels
            assert w.composite_route(B, H, W, K, N, 4, 0) == ('one' if w.fused_supported(K, N, 4) else 'two')
    assert routes == set(w.COMP_ROUTES)
    assert w.composite_route(2, 5, 7, 32, 64, 4, 0) == 'two'                 # K = 32: never one kernel
    for B, H, W, Ci, Cout, m, S in w.WGRAD_SPLITS:
        p = w.wgrad_plan(B, H, W, Ci, Cout, m)
        assert p.S == S, (B, H, W, Ci, Cout, m, p)
    assert w.wino_tiles(2, 64, 64, 4) == 512 and w.wino_tiles(2, 64, 64, 2) == 2048
    ragged = [(w.wino_tiles(B, H, W, m), w.wgrad_plan(B, H, W, Ci, Cout, m)) for B, H, W, Ci, Cout, m, S in w.WGRAD_SPLITS if S > 1]
    assert any(T % p.k_per_split for T, p in ragged) and any(T % p.k_per_split == 0 for T, p in ragged)
    assert all((p.S - 1) * p.k_per_split < T <= p.S * p.k_per_split for T, p in ragged)
    assert {S for *_, S in w.WGRAD_SPLITS} >= {1, 2}


# ---------------------------------------------------------------- the restatement against the library
def _shapes():
    act = [(r.B, r.H, r.W, r.C, r.C) for r in w.ACT_CASES + w.OUT_CASES]
    fused = [(r.B, r.H, r.W, r.K, r.N) for r in w.FUSED_CASES]
    comp = [s for s in w.COMP_CASES] + [(B, H, W, Ci, Co) for B, H, W, Ci, Co, _, _ in w.WGRAD_SPLITS]
    rows = [(B, H, W, Ci, Co) for B, H, W, Ci, Co, _, _ in w.BIASROW_CASES]
    odd = [(1, 7, 9, 256, 512), (4, 60, 60, 512, 512), (1, 8, 8, 28, 64), (1, 8, 8, 64, 66), (0, 8, 8, 64, 64), (1, 8, 8, 48, 64)]
    return act + fused + comp + rows + odd


def test_restated_queries_agree_with_the_library(h):
    for B, H, W, Ci, Co in _shapes():
        for m in (2, 3, 4):
            ok = m in (2, 4)
            assert h.wesup_winograd_tiles(B, H, W, m) == (w.wino_tiles(B, H, W, m) if ok else 0)
            assert h.wesup_winograd_weight_floats(Ci, Co, m) == (w.wino_positions(m) * Ci * Co if ok else 0)
            assert h.wesup_winograd_fused_supported(Ci, Co, m) == w.fused_supported(Ci, Co, m)
            for s in ((B, H, W, Ci, Co), (B, H, W, Co, Ci)):
                assert h.wesup_conv3x3_winograd_workspace_bytes(*s, m) == w.conv_workspace_bytes(*s, m), (s, m)
                assert h.wesup_conv3x3_wgrad_winograd_workspace_bytes(*s, m) == w.wgrad_workspace_bytes(*s, m), (s, m)
            for C in (Ci, Co):
                assert h.wesup_winograd_outgrad_workspace_bytes(B, H, W, C, m) == w.outgrad_workspace_bytes(B, H, W, C, m), (B, H, W, C, m)
        for C in (Ci, Co):
            assert h.wesup_winograd_bias_rows(B, H, W, C) == w.bias_rows(B, H, W, C), (B, H, W, C)


def test_the_200_block_rule_and_its_knob(h):
    assert h.wesup_winograd_set_fused_min_blocks(-1) == w.FUSED_MIN_BLOCKS              # (a negative value only reads it)
    for K, N in ((64, 64), (64, 128), (128, 192), (256, 64), (512, 64), (64, 96), (32, 64)):
        per = N // 64 or 1
        for blocks in (199, 200, 201):
            for tiles in ((blocks // per) * 32, (blocks // per) * 32 + 1, (blocks // per - 1) * 32 + 1):
                assert h.wesup_winograd_fused_route(K, N, 4, tiles) == w.fused_route(K, N, 4, tiles), (K, N, tiles)
        assert h.wesup_winograd_fused_route(K, N, 2, 10 ** 5) == 0 and h.wesup_winograd_fused_route(K, N, 4, 0) == w.fused_supported(K, N, 4)
    was = h.wesup_winograd_set_fused_min_blocks(0)
    try:
        assert h.wesup_winograd_fused_route(64, 64, 4, 1) == 2 == w.fused_route(64, 64, 4, 1, 0)
    finally:
        assert h.wesup_winograd_set_fused_min_blocks(was) == 0
    assert h.wesup_winograd_fused_route(64, 64, 4, 1) == 0


def test_split_counts_show_in_the_wgrad_workspace_query(h):
    for B, H, W, Ci, Cout, m, S in w.WGRAD_SPLITS:
        P, T = w.wino_positions(m), w.wino_tiles(B, H, W, m)
        fixed = g.align_up(P * T * Ci * 4, 256) + g.align_up(P * T * Cout * 4, 256) + w.outgrad_workspace_bytes(B, H, W, Cout, m)
        got = h.wesup_conv3x3_wgrad_winograd_workspace_bytes(B, H, W, Ci, Cout, m)
        size = lambda s: fixed + g.align_up(P * s * (Cout * Ci + Cout) * 4, 256)      # noqa: E731
        assert size(S) == got and size(S + 1) != got and (S == 1 or size(S - 1) != got)


SOURCE_PINS = [          # thresholds no query shows: each line stands in the named file this many times, blanks aside
    ('winograd.hip', 'static bool wino4_block_colsum_ok(int C) { const int Q = C / 4; return Q <= 256 && 256 % Q == 0; }', 1),
    ('winograd.hip', 'const bool narrow = m == 4 && tot / 64 < 512;', 1),
    ('winograd.hip', 'const bool vec = m == 4 && tot % 4 == 0 && slab_stride % 4 == 0 && batch_stride % 4 == 0 && !((uintptr_t)slabs & 15);', 1),
    ('winograd.hip', 'g2.nt = wino_nt_stores(4.0 * 36 * g.T * C);', 1),
    ('winograd.hip', 'g.nt = m == 4 ? wino_nt_stores(4.0 * 36 * g.T * C) : 0;', 1),
    ('winograd.hip', 'g.nt = wino_nt_stores(2 * 4.0 * 36 * g.T * C);', 2),
    ('winograd.hip', 'for (; r + 7 * 64 < bias_rows; r += 8 * 64) {', 1),
    ('wino_fused.hip', 'p.nt = wino_nt_stores(4.0 * B * (unpool ? 4.0 : 1.0) * H * W * N);', 1),
    ('wino_fused.hip', 'static int g_fused_min_blocks = 200;', 1),
    ('wino_fused.hip', 'static FusedShape fused_shape(long, int) { return FusedShape{2, 3}; }', 1),
    ('wino_fused.hip', 'const bool batched = !up.dst && !p.mask && !(p.gat.src && p.gat.area) && (p.mask_bits || p.accum || p.gat.src);', 1),
    ('wino_fused.hip', 'const bool ubatched = up.dst && p.up_code && !p.mask && !p.mask_bits && !(p.gat.src && p.gat.area);', 1),
    ('wino_fused.hip', 'const bool plain = !batched && !ubatched && !p.mask && !up.dst && !p.gat.src && !p.accum;', 1),
    ('common.hpp', 'return (e ? atof(e) : 16.0) * 1048576.0; }();', 1),
    ('gemm.hip', 'const TnPlan pl = plan_tn(Cout, Ci, (int)T, 1, P);', 3),
    ('gemm.hip', 'const int fused = out_relu ? 0 : wino_fused_route(Cin, Cout, m, T);', 1),
]


def test_thresholds_no_query_shows_stand_in_the_source_as_restated():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'wesup_amd', 'csrc')
    src = {}
    for name, line, count in SOURCE_PINS:
        if name not in src:
            src[name] = ''.join(open(os.path.join(root, name)).read().split())
        assert src[name].count(''.join(line.split())) == count, f'csrc/{name} no longer says `{line}`: update tests/_winocases.py with it'


# ---------------------------------------------------------------- the premise of the integer pass, on the rows' own data
def _exact(bound, f):
    return float(bound) * 2 ** f < 2 ** 24


def test_the_absolute_pipeline_is_the_pipeline_on_absolute_matrices():
    x = np.arange(-8, 8, dtype=np.float64).reshape(1, 4, 4, 1)
    with w.absolute() as a:
        assert (a._BT[4] >= 0).all() and (a._AT[2] >= 0).all() and (a._G[4] >= 0).all()
        big = a.input_transform(np.abs(x), m=4)
    assert (wo._BT[4] < 0).any() and (wo._G[2] < 0).any()                    # restored
    assert (big >= np.abs(wo.input_transform(x, m=4)) - 1e-12).all()


@pytest.mark.parametrize('r', [r for r in w.ACT_CASES if r.H <= 13], ids=lambda r: r.id)
def test_activation_int_pass_is_exact(r):
    x = w.act_data(r, 'int')
    assert set(np.unique(x)) <= set(range(-3, 4)) and (x == 0).any() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    for m in (2, 4):
        f = 12 if m == 4 else 0
        for relu in (False, True):
            v64 = wo.input_transform(x, relu, np.float64, m)
            assert np.array_equal(wo.input_transform(x, relu, np.float32, m).astype(np.float64), v64)
            with w.absolute() as a:
                assert _exact(a.input_transform(np.abs(x), relu, m=m).max(), f)
        assert np.array_equal(wo.outgrad_transform(x, np.float32, m).astype(np.float64), wo.outgrad_transform(x, np.float64, m))
        with w.absolute() as a:
            assert _exact(a.outgrad_transform(np.abs(x), m=m).max(), f)
    assert _exact(np.abs(x).sum((0, 1, 2)).max(), 0)                         # db and the bias rows: integer sums


def test_activation_int_pass_is_exact_at_the_large_rows():
    """(the data of a large row are the same draws at a larger shape: the bound is a per-patch one)"""
    for r in w.ACT_CASES:
        assert _exact(3 * np.abs(wo._BT[4]).sum(1).max() ** 2, 12) and _exact(3 * np.abs(wo._AT[4]).sum(0).max() ** 2, 12)
        assert _exact(3 * r.B * r.H * r.W, 0)


@pytest.mark.parametrize('r', w.OUT_CASES, ids=lambda r: r.id)
def test_output_int_pass_is_exact(r):
    for m in (2, 4):
        d = w.out_data(r, 'int', m)
        assert set(np.unique(d['mask'])) <= {-1.0, 0.0, 1.0} and np.signbit(d['mask'][d['mask'] == 0]).any()
        y64 = wo.output_transform(d['Mt'], r.B, r.H, r.W, d['bias'], np.float64, m)
        assert np.array_equal(wo.output_transform(d['Mt'], r.B, r.H, r.W, d['bias'], np.float32, m).astype(np.float64), y64)
        with w.absolute() as a:
            bound = a.output_transform(np.abs(d['Mt']), r.B, r.H, r.W, np.abs(d['bias']), m=m) + np.abs(d['old'])
        assert _exact(bound.max() + 3, 12 if m == 4 else 0)                  # (+ 3: the unpooling destination's old content)


@pytest.mark.parametrize('r', w.FUSED_CASES, ids=lambda r: r.id)
def test_fused_int_pass_is_exact(r):
    """The products are sums of K terms of {-1, 0, 1}: integers, exact in any order.  The transform then adds multiples of 2^-12
    (A^T has six fractional bits, twice): every partial sum of its fma chains is a sub-sum of A^T M A's terms, so it is bounded by
    |A^T| |M| |A| with M = V U^T the integer products themselves, and exact while that bound (+ |bias| + |old| + the unpooling
    destination's 3) stays below 2^24 / 2^12 = 4096."""
    d = w.fused_data(r, 'int')
    assert set(np.unique(d['V'])) == {-1.0, 0.0, 1.0} and abs((d['V'] == 0).mean() - 0.5) < 0.1
    M = np.abs(np.matmul(d['V'].astype(np.float64), d['U'].astype(np.float64).transpose(0, 2, 1)))
    assert M.max() <= r.K
    with w.absolute() as a:
        bound = a.output_transform(M, r.B, r.H, r.W, np.abs(d['bias']), m=4) + np.abs(d['old'])
    assert bound.max() + 3 < 4096 and _exact(bound.max() + 3, 12), bound.max()


def test_filter_int_passes():
    for Co, Ci in w.PACK_CASES:
        assert Co != Ci
        wt = w._data((Co, Ci, 3, 3), 'int', 2)
        for u32, u64 in zip(wo.pack_weight(wt, np.float32, 2), wo.pack_weight(wt, np.float64, 2)):
            assert np.array_equal(u32.astype(np.float64), u64) and np.array_equal(u64 * 4, np.round(u64 * 4))      # quarters
    for r in w.REDUCE_CASES:
        if r.m != 2:
            continue
        for S in r.S:
            s = w.reduce_data(r, 'int', S)
            dU = s[:, :, :r.Cout * r.Cin].sum(1).reshape(16, r.Cout, r.Cin)
            assert np.array_equal(wo.filter_grad(dU, np.float32, 2).astype(np.float64), wo.filter_grad(dU, np.float64, 2))
            with w.absolute() as a:
                assert _exact(a.filter_grad(np.abs(s[:, :, :r.Cout * r.Cin]).sum(1).reshape(16, r.Cout, r.Cin), m=2).max(), 2)


def test_f2_chain_int_pass_is_exact():
    """F(2x2) composites on integers: V integers, U quarters, so every product and partial sum is a multiple of 1/4 below the
    absolute-value chain's bound; the weight gradient's dU are integers and G^T dU G quarters again."""
    for B, H, W, Cin, Cout in w.COMP_CASES + [s[:5] for s in w.WGRAD_SPLITS if s[5] == 2]:
        x, wt, dy = w._data((B, H, W, Cin), 'int', 1), w._data((Cout, Cin, 3, 3), 'int', 2), w._data((B, H, W, Cout), 'int', 4)
        with w.absolute() as a:
            fwd = a.conv_fwd(np.abs(x), np.abs(wt), np.full(Cout, 3.0), m=2) + 3
            dg = a.conv_dgrad(np.abs(dy), np.abs(wt), m=2) + 3
            dw, db = a.conv_wgrad(np.abs(x), np.abs(dy), m=2)
        assert _exact(max(fwd.max(), dg.max(), dw.max(), db.max()), 2), (B, H, W, Cin, Cout)
