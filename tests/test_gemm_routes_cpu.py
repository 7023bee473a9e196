"""The GEMM case table (tests/_gemmcases.py) reaches the routes it claims, and the restated dispatch agrees with the library
wherever the C ABI lets it be seen: the workspace queries, which are host code.  No GPU.

A change that moves a threshold of csrc/gemm.hip without the restatement fails the workspace checks where the threshold shows
in a query, and one that updates the restatement without the table fails the route checks: both are meant to."""
import os

import pytest

import _gemmcases as g


@pytest.fixture(scope='module')
def h():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _nt_ws(c):
    full = g.nt_workspace_bytes(c.M, c.N, c.K)
    return {None: 0, 'full': full, 'short': full - 1}[c.ws]


@pytest.mark.parametrize('c', g.NT_CASES, ids=lambda c: c.id)
def test_nt_row_reaches_its_route(c):
    assert c.K % 32 == 0 and c.N % 4 == 0
    if c.ws == 'short':
        assert g.nt_workspace_bytes(c.M, c.N, c.K) > 0, 'a short workspace needs a stream-K shape'
    route, sk = g.nt_route(c.M, c.N, c.K, _nt_ws(c))
    assert route == c.route, (c.id, route)
    if c.route == 'nt128sk':
        assert (sk.full, sk.parts, sk.steps) == c.sk
        assert sk.full % 8 == 0                       # the kernel's XCD remap of the whole tiles counts on it
        assert sk.steps // sk.parts < c.K // 32       # a part is shorter than a tile: at most two tiles, two slots
    else:
        assert sk.parts == 0


def test_nt_rows_carry_the_edges_they_name():
    by = {c.id: c for c in g.NT_CASES}
    two = [c for c in g.NT_CASES if c.route == 'nt64x2']
    assert {c.N <= 64 for c in two} == {True, False}
    assert all(512 < g.cdiv(c.M, 64) * g.cdiv(c.N, 64) for c in two)
    assert any(c.K == 32 and c.route == 'nt64x3' for c in g.NT_CASES) and any(c.K == 32 and c.route == 'nt64x2' for c in g.NT_CASES)
    assert any(c.N > 64 and c.N % 64 for c in g.NT_CASES) and any(c.N == 4 for c in g.NT_CASES) and any(c.M < 64 for c in g.NT_CASES)
    c = by['nt-130x132x1088-sk']                      # a part that ends one tile and begins the next
    nk, per = c.K // 32, c.sk[2] // c.sk[1]
    assert c.sk[2] % c.sk[1] == 0 and nk % per != 0
    c = by['nt-130x132x1024-sk']
    assert (c.K // 32) % (c.sk[2] // c.sk[1]) == 0    # ... and one whose parts never do


@pytest.mark.parametrize('c', g.NTB_CASES + g.NTBB_CASES, ids=lambda c: c.id)
def test_batched_nt_row_reaches_its_route(c):
    assert c.K in (32, 64) and c.N % 4 == 0
    route = (g.ntbb_route if c.id.startswith('ntbb') else g.ntb_route)(c.nbatch, c.M, c.N, c.K)
    assert route == c.route, (c.id, route)


@pytest.mark.parametrize('c', g.TN_CASES, ids=lambda c: c.id)
def test_tn_row_reaches_its_route(c):
    pl = g.plan_tn(c.M, c.N, c.K)
    assert (pl.tile, pl.S, g.tn_weighted(pl)) == (c.tile, c.S, c.weighted), (c.id, pl)
    assert c.M % 4 == 0 and c.N % 4 == 0
    for relu_b, colsum, odd, store in c.variants:
        ldc = c.N + (5 if odd else 8)
        assert g.tn_store(pl, bool(colsum), ldc) == store, (c.id, relu_b, colsum, odd)
    if c.S > 1:
        assert (c.S - 1) * pl.k_per_split < c.K <= c.S * pl.k_per_split          # every split has rows


@pytest.mark.parametrize('c', g.TNB_CASES, ids=lambda c: c.id)
def test_batched_tn_row_reaches_its_route(c):
    pl = g.plan_tn(c.M, c.N, c.K, c.nbatch)
    assert (pl.tile, pl.S) == (c.tile, c.S), (c.id, pl)
    assert not g.tn_weighted(pl, c.nbatch)
    for relu_b, odd, store in c.variants:
        strideC = (c.M + 1) * (c.N + 8) + (1 if odd else 0)
        assert g.tn_store(pl, False, c.N + 8, strideC) == store, (c.id, odd)


def test_every_named_route_has_a_row():
    assert {c.route for c in g.NT_CASES} == set(g.NT_ROUTES)
    assert {c.route for c in g.NTB_CASES} == set(g.NTB_ROUTES)
    assert {c.route for c in g.NTBB_CASES} == set(g.NTBB_ROUTES)
    assert any(c.nbatch == 1 for c in g.NTB_CASES)
    tn = {(c.tile, v[-1]) for c in g.TN_CASES for v in c.variants}
    assert tn == set(g.TN_ROUTES)                      # (128 x 128 tiles never fold: S > 32 needs fewer than six tiles)
    assert any(c.weighted for c in g.TN_CASES) and any(c.tile == 128 and c.S >= 2 for c in g.TNB_CASES)
    assert any(c.S == 32 for c in g.TN_CASES) and any(c.K < 32 for c in g.TN_CASES)
    for c in g.TN_CASES:
        if c.tile == 128:                              # relu_b off and on, with and without colsum
            assert {(v[0], v[1]) for v in c.variants} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert {(c.tile, v[-1]) for c in g.TNB_CASES for v in c.variants} >= {(128, 'reduce'), (64, 'reduce'), (128, 'direct'), (128, 'slab')}


def test_restated_plans_agree_with_the_library(h):
    nt = [(c.M, c.N, c.K) for c in g.NT_CASES] + g.EXISTING_NT
    nt += [(c.M, c.N, c.K) for c in g.NTB_CASES + g.NTBB_CASES]
    for M, N, K in nt:
        _, sk = g.choose_nt(M, N, K, True)
        want = sk.parts * 2 * 128 * 128 * 4
        assert want == g.nt_workspace_bytes(M, N, K)
        assert h.wesup_gemm_nt_workspace_bytes(M, N, K) == want, (M, N, K)
    for M, N, K in [(c.M, c.N, c.K) for c in g.TN_CASES] + g.EXISTING_TN:
        pl = g.plan_tn(M, N, K)
        want = g.align_up(pl.S * (M * N + M) * 4, 256) + (16 * (M * N + M) * 4 if pl.S > 32 else 0)
        assert want == g.tn_workspace_bytes(M, N, K)
        assert h.wesup_gemm_tn_workspace_bytes(M, N, K) == want, (M, N, K, pl)
    for nb, M, N, K in [(c.nbatch, c.M, c.N, c.K) for c in g.TNB_CASES] + g.EXISTING_TNB:
        want = nb * g.plan_tn(M, N, K, nb).S * (M * N + M) * 4
        assert h.wesup_gemm_tn_batched_workspace_bytes(nb, M, N, K) == want, (nb, M, N, K)
    for M, N, _ in g.COLSUM_CASES:
        assert h.wesup_colsum_workspace_bytes(M, N) == g.colsum_workspace_bytes(M, N), (M, N)


def test_split_counts_show_in_the_workspace_queries(h):
    """S is the one number of plan_tn the ABI shows, and only while the slab term is not rounded away: the table's rows pin it
    from both sides (S and S + 1 ask for different sizes), so a moved threshold of plan_tn cannot hide behind the alignment."""
    for c in g.TN_CASES:
        elems = (c.M * c.N + c.M) * 4
        if elems < 256:
            continue
        got = h.wesup_gemm_tn_workspace_bytes(c.M, c.N, c.K)
        fold = 16 * elems if c.S > 32 else 0
        assert g.align_up(c.S * elems, 256) + fold == got
        assert g.align_up((c.S + 1) * elems, 256) + (16 * elems if c.S + 1 > 32 else 0) != got
    for c in g.TNB_CASES:
        assert h.wesup_gemm_tn_batched_workspace_bytes(c.nbatch, c.M, c.N, c.K) == c.nbatch * c.S * (c.M * c.N + c.M) * 4


def test_thresholds_are_pinned_from_both_sides(h):
    for M, N, K, streamk in g.NT_PINS:
        want = g.nt_workspace_bytes(M, N, K)
        assert (want > 0) == streamk, (M, N, K)
        assert h.wesup_gemm_nt_workspace_bytes(M, N, K) == want, (M, N, K)
    for nb, M, N, K, S in g.TN_PINS:
        assert g.plan_tn(M, N, K, nb).S == S, (nb, M, N, K, g.plan_tn(M, N, K, nb))
        assert h.wesup_gemm_tn_batched_workspace_bytes(nb, M, N, K) == nb * S * (M * N + M) * 4, (nb, M, N, K)
        if nb == 1:
            assert h.wesup_gemm_tn_workspace_bytes(M, N, K) == g.tn_workspace_bytes(M, N, K), (M, N, K)


def test_thresholds_no_query_shows_stand_in_the_source_as_restated():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ''.join(open(os.path.join(root, 'wesup_amd', 'csrc', 'gemm.hip')).read().split())
    for line, count in g.SOURCE_PINS:
        assert src.count(''.join(line.split())) == count, f'csrc/gemm.hip no longer says `{line}`: update tests/_gemmcases.py with it'


def test_colsum_and_transpose_rows_sit_at_their_boundaries():
    assert (1, 4, 0) in g.COLSUM_CASES
    assert any(M % 64 == 1 and N % 64 == 4 and N > 64 for M, N, _ in g.COLSUM_CASES)          # one row, one quad past a boundary
    assert any(pad for _, _, pad in g.COLSUM_CASES)
    assert any(g.cdiv(M, 64) > 2048 // g.cdiv(N, 64) for M, N, _ in g.COLSUM_CASES)            # the cap on the chunk count binds
    assert (1, 1) in g.TRANSPOSE_CASES and any(r % 32 == 1 and c % 32 == 1 and r > 32 for r, c in g.TRANSPOSE_CASES)
