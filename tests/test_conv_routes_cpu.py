"""The conv case table (tests/_convcases.py) reaches the routes it claims, and the restated conv dispatch agrees with the
library wherever the C ABI lets it be seen: wesup_conv3x3_kpad and the two workspace queries, which are host code.  No GPU.

A change that moves a threshold of csrc/gemm.hip without the restatement fails the workspace checks where the threshold shows
in a query and the source pins where it does not; one that updates the restatement without the table fails the route checks."""
import os

import pytest

import _convcases as c
import _gemmcases as g


@pytest.fixture(scope='module')
def h():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _ws(r):
    full = c.conv_workspace_bytes(r.B, r.H, r.W, r.Cin, r.Cout)
    return {None: 0, 'full': full, 'short': full - 1}[r.ws]


@pytest.mark.parametrize('r', c.CONV_CASES + c.SIDE_CASES, ids=lambda r: r.id)
def test_conv_row_reaches_its_route(r):
    side = r in c.SIDE_CASES
    assert r.Cout % 4 == 0 and (c.is_image(r.Cin) and r.Cin == 3 or r.Cin >= 32 and r.Cin & (r.Cin - 1) == 0)
    if r.ws == 'short':
        assert c.conv_workspace_bytes(r.B, r.H, r.W, r.Cin, r.Cout) > 0, 'a short workspace needs a stream-K shape'
    route, sk = c.conv_route(r.B, r.H, r.W, r.Cin, r.Cout, _ws(r), side)
    assert route == r.route, (r.id, route)
    bm, bn = c.CONV_TILE[route]
    assert (g.cdiv(r.B * r.H * r.W, bm), g.cdiv(r.Cout, bn)) == r.tiles, r.id
    if route == 'cv128sk':
        assert (sk.full, sk.parts, sk.steps) == r.sk
        assert sk.full % 8 == 0                                      # the kernel's XCD remap of the whole tiles counts on it
        assert sk.steps // sk.parts < c.conv_kpad(r.Cin) // 32       # a part is shorter than a tile: at most two tiles, two slots
    else:
        assert sk.parts == 0 and r.sk is None
    if side:
        assert r.tiles[1] == 1 and r.Cout in (64, 128)
    # the int pass of the GPU test: every partial sum is an integer below 2^24
    cin = 4 if c.is_image(r.Cin) else r.Cin
    assert 9 * (9 * cin) + 3 < 2 ** 24
    if side:
        assert r.Cout * 3 * (9 * 9 * cin + 3) + 3 < 2 ** 24


def test_conv_rows_carry_the_edges_they_name():
    by = {r.id: r for r in c.CONV_CASES + c.SIDE_CASES}
    rows = c.CONV_CASES
    assert any(r.H == 1 and r.W == 1 for r in rows) and any(r.W == 1 and r.H > 1 for r in rows) and any(r.H == 1 and r.W > 64 for r in rows)
    assert any(r.W == 2 for r in rows) and any(r.Cout < 64 and r.Cout % 32 for r in rows) and any(64 < r.Cout < 128 for r in rows)
    r = by['cv-3x7x9x64x68']
    assert r.H * r.W == 63 and r.B * r.H * r.W > 128 and r.Cin == 64          # every tile of 64 rows holds an image boundary
    # both sides of the two 384-tile thresholds
    assert g.cdiv(223 * 220, 128) == 384 and g.cdiv(222 * 220, 128) == 382
    assert by['cv-1x223x220x32x64'].route == 'cv128x64' and by['cv-1x222x220x32x64'].route == 'cv64'
    assert g.cdiv(112 * 109, 128) * 4 == 384 and g.cdiv(112 * 108, 128) * 4 == 380
    assert by['cv-1x112x109x32x512'].route == 'cv128' and by['cv-1x112x108x32x512'].route == 'cv64'
    assert (112 * 109) % 128 and by['cv-1x130x126x32x260'].Cout % 128
    # streaming stores: rows on both sides of the 16 MiB bar, under either number of outputs
    st = {(c.conv_streams(r.B * r.H * r.W, r.Cout), c.conv_streams(r.B * r.H * r.W, r.Cout, outputs=2)) for r in rows}
    assert st == {(False, False), (False, True), (True, True)}
    assert c.conv_streams(112 * 109, 512) and not c.conv_streams(112 * 109, 512, accum=True)
    # a stream-K row whose parts end one tile and begin the next, with images that straddle the tiles
    r = by['cv-2x20x19x128x128-sk']
    nk, per = c.conv_kpad(r.Cin) // 32, r.sk[2] // r.sk[1]
    assert r.sk[2] % r.sk[1] == 0 and nk % per != 0 and r.sk[0] == 0 and (r.H * r.W) % 128
    r = by['cv-1x149x147x64x260-sk']
    assert r.sk[0] == 512 and r.tiles[0] * r.tiles[1] - r.sk[0] == 4
    assert by['cv-1x149x147x64x260-shortws'].ws == 'short' and by['cv-2x20x19x128x128'].ws is None
    for r in c.SIDE_CASES:                                                     # 130-pixel images under a 128-row tile
        assert r.H * r.W == 130 and (r.B * r.H * r.W) % 128


@pytest.mark.parametrize('r', c.WGRAD_CASES, ids=lambda r: r.id)
def test_wgrad_row_reaches_its_route(r):
    assert r.Cout % 32 == 0 and (r.Ci == 3 or r.Ci >= 32 and r.Ci & (r.Ci - 1) == 0)
    p = c.wgrad_plan(r.B, r.H, r.W, r.Ci, r.Cout)
    assert c.wgrad_route(r.B, r.H, r.W, r.Ci, r.Cout) == r.route, (r.id, p)
    assert ((p.tiles_m, p.tiles_n), p.S, p.weighted) == (r.tiles, r.S, r.weighted), (r.id, p)
    tile, kind, path, store = r.route.split('-')
    assert (int(tile), kind == 'image', path == 'tiny', store) == (p.tile, c.is_image(r.Ci), p.tiny, p.store)
    assert p.taps == (1 if c.is_image(r.Ci) else 9)
    K = r.B * r.H * r.W
    if p.S > 1:
        assert (p.S - 1) * p.k_per_split < K <= p.S * p.k_per_split           # every split has rows
    assert 9 * K < 2 ** 24                                                     # the int pass of the GPU test is exact


def test_wgrad_rows_carry_the_edges_they_name():
    by = {r.id: r for r in c.WGRAD_CASES}
    fast = [r for r in c.WGRAD_CASES if '-fast-' in r.route]
    assert all(r.W >= 16 and r.H >= 2 for r in fast)
    assert any(r.W == 16 and r.H == 2 for r in fast)                           # the fast path at its minimum
    assert {r.W for r in fast if r.Ci >= 32} >= {16, 17, 31, 32, 33}           # the widths around the carry classes of the conv mode
    # the second carry: some K-step of the row begins at a column w0 = 32 j mod W with w0 + 31 >= 2 W, inside K -- for exactly the
    # rows the table names, in every instantiation that has the carry: 64 and 128 tiles, equal and weighted splits, image layer
    for r in fast:
        steps = c.second_carry_steps(r.B, r.H, r.W)
        assert bool(steps) == (r.id in c.WGRAD_SECOND_CARRY), (r.id, steps)
        assert all((32 * j) % r.W + 31 >= 2 * r.W for j in steps) and (not steps or 17 <= r.W <= 30)
        assert ('second carry' in r.edge) == bool(steps), r.id
    two = [r for r in fast if r.id in c.WGRAD_SECOND_CARRY]
    assert len(two) == len(c.WGRAD_SECOND_CARRY)
    assert {(int(r.route.split('-')[0]), c.is_image(r.Ci)) for r in two} == {(64, False), (128, False), (64, True)}
    assert {r.weighted for r in two if r.route.startswith('128')} == {True, False}
    assert any(r.S > 1 for r in two if r.Ci == 3)
    # ... and by both pieces of code that compute it, in each conv instantiation
    for r in two:
        who = c.second_carry_code(r.B, r.H, r.W, r.Ci, r.Cout)
        assert who == ({'mask_b'} if r.Ci == 3 else {'mask_b', 'step_mask'}), (r.id, who)
    assert not c.second_carry_steps(1, 9, 16) and not c.second_carry_steps(1, 37, 31) and not c.second_carry_steps(1, 2, 16)
    tiny = [r for r in c.WGRAD_CASES if '-tiny-' in r.route]
    assert any(r.H == 1 and r.W >= 16 for r in tiny) and any(r.W < 16 and r.H >= 2 for r in tiny)
    r = by['wg-3x5x17x32x32']
    assert (r.B * r.H * r.W) % 32 and (r.H * r.W) % 32                         # ragged K; K-steps cross image boundaries
    r = by['wg-2x33x17x64x64']
    assert c.wgrad_plan(r.B, r.H, r.W, r.Ci, r.Cout).k_per_split % r.W         # splits begin in mid-row
    w = [r for r in c.WGRAD_CASES if r.weighted]
    assert {('-tiny-' in r.route) for r in w} == {True, False}
    for r in w:            # how many splits of a tile sit among the first 256 blocks differs between the tiles of one grid
        gx = r.tiles[0] * r.tiles[1] * 9
        assert len({min(r.S, (255 - bx) // gx + 1) for bx in range(gx)}) == 2 and gx * r.S > 256
    assert any(r.Cout % 64 for r in c.WGRAD_CASES)                             # a ragged M-tile
    assert {r.S for r in c.WGRAD_CASES} >= {1, 2, 4, 16, 32, 36}


def test_every_named_route_has_a_row():
    assert {r.route for r in c.CONV_CASES} == set(c.CONV_ROUTES)
    assert {r.route for r in c.SIDE_CASES} == set(c.SIDE_ROUTES)
    assert {r.route for r in c.WGRAD_CASES} == set(c.WGRAD_ROUTES)
    assert any(r.weighted for r in c.WGRAD_CASES)
    assert set(c.CONV_TILE) == set(c.CONV_ROUTES) | set(c.SIDE_ROUTES)


def test_what_the_plan_cannot_produce():
    """The routes WGRAD_ROUTES leaves out do not exist, by plan_tn's own text: the image layer calls it with N = 64, and `big` asks
    for N >= 128, so its tile is 64 x 64; a conv calls it with nine taps, so it has at least nine tiles, 9 * 32 >= 192, and more
    than 32 splits are cut back to 32 (ceil(K / k_per_split) never raises the count): nothing to fold.  The sweep restates that
    on the plan over every channel count a layer can have up to 2048 and K from one pixel to 2^24 / 9."""
    Ks = [1, 31, 255, 256, 300, 1000, 5000, 8448, 33 * 8 * 32, 34 * 8 * 32, 100000, 1000000, 2 ** 24 // 9]
    for Cout in range(32, 2049, 32):
        for K in Ks:
            assert g.plan_tn(Cout, 64, K, taps=1).tile == 64
            for Ci in (32, 64, 128, 256, 512, 1024, 2048):
                assert g.plan_tn(Cout, Ci, K, taps=9).S <= 32


def test_restated_queries_agree_with_the_library(h):
    for Ci in (1, 3, 4, 32, 64, 100, 128, 512):
        assert h.wesup_conv3x3_kpad(Ci) == c.conv_kpad(Ci), Ci
    conv = [(r.B, r.H, r.W, r.Cin, r.Cout) for r in c.CONV_CASES + c.SIDE_CASES] + c.EXISTING_CONV
    for s in conv + [(b, hh, w, co, ci) for b, hh, w, ci, co in conv]:          # (and as the dgrad asks: channel counts swapped)
        assert h.wesup_conv3x3_workspace_bytes(*s) == c.conv_workspace_bytes(*s), s
    for s in [(r.B, r.H, r.W, r.Ci, r.Cout) for r in c.WGRAD_CASES] + c.EXISTING_WGRAD:
        assert h.wesup_conv3x3_wgrad_workspace_bytes(*s) == c.wgrad_workspace_bytes(*s), (s, c.wgrad_plan(*s))


def test_split_counts_show_in_the_wgrad_workspace_query(h):
    """S is the one number of plan_wgrad the ABI shows: S and S + 1 ask for different sizes on every row."""
    for r in c.WGRAD_CASES:
        p = c.wgrad_plan(r.B, r.H, r.W, r.Ci, r.Cout)
        elems = (r.Cout * p.Nslab + r.Cout) * 4
        got = h.wesup_conv3x3_wgrad_workspace_bytes(r.B, r.H, r.W, r.Ci, r.Cout)

        def size(S):
            return g.align_up(S * elems, 256) + g.align_up((16 if S > 32 else 0) * elems, 256)
        assert size(r.S) == got and size(r.S + 1) != got and (r.S == 1 or size(r.S - 1) != got), r.id


def test_thresholds_are_pinned_from_both_sides(h):
    for B, H, W, Cin, Cout, streamk in c.CONV_PINS:
        want = c.conv_workspace_bytes(B, H, W, Cin, Cout)
        assert (want > 0) == streamk, (B, H, W, Cin, Cout)
        assert h.wesup_conv3x3_workspace_bytes(B, H, W, Cin, Cout) == want, (B, H, W, Cin, Cout)
    for B, H, W, Ci, Cout, tile, S in c.WGRAD_PINS:
        p = c.wgrad_plan(B, H, W, Ci, Cout)
        assert (p.tile, p.S) == (tile, S), (B, H, W, Ci, Cout, p)
        assert h.wesup_conv3x3_wgrad_workspace_bytes(B, H, W, Ci, Cout) == c.wgrad_workspace_bytes(B, H, W, Ci, Cout), (B, H, W, Ci, Cout)


def test_thresholds_no_query_shows_stand_in_the_source_as_restated():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, pins in (('gemm.hip', c.SOURCE_PINS), ('common.hpp', c.COMMON_PINS)):
        src = ''.join(open(os.path.join(root, 'wesup_amd', 'csrc', name)).read().split())
        for line, count in pins:
            assert src.count(''.join(line.split())) == count, f'csrc/{name} no longer says `{line}`: update tests/_convcases.py with it'
    assert c.NT_STREAM_BYTES == 16 * 1048576
