"""The dispatch decisions of wesup_amd/csrc/gemm.hip restated in plain Python, and the table of GEMM cases that
tests/test_gemm_routes_cpu.py (does every row reach the route it names?) and tests/test_gemm_routes_gpu.py (is every row
exact?) share.

Only the default settings are restated: the routes behind WESUP_NT_SHAPE, WESUP_NTB_SHAPE, WESUP_TN_SMALL_RULE,
WESUP_TN_S1_MIN_TILES and WESUP_TN_WEIGHTS are read once per process by the library and are not covered here.

A change that moves a threshold in choose_nt, plan_streamk, nt_three_stages, the batched tile choices, plan_tn, tn_direct,
launch_tn's weighted-split condition or slab_fold_chunks has to update the restatement below AND the rows whose route it
moves, in the same change: that is what the CPU test is for.
"""
from collections import namedtuple

BK = 32


def cdiv(a, b):
    return -(-a // b)


def align_up(v, a):
    return cdiv(v, a) * a


# ---------------------------------------------------------------- NT family
SkPlan = namedtuple('SkPlan', 'full parts steps ws_bytes')
NO_SK = SkPlan(0, 0, 0, 0)


def plan_streamk(M, N, K, bm, bn, slots):
    tiles = cdiv(M, bm) * cdiv(N, bn)
    nk = K // BK
    R = tiles % slots
    if N <= 64 or nk < 16 or R == 0 or R * 10 > slots * 9:
        return NO_SK
    if tiles < slots and nk < 32:
        return NO_SK
    W = R * nk
    P = min(W // 8, slots)
    if P <= R:
        return NO_SK
    return SkPlan(tiles - R, P, W, P * 2 * bm * bn * 4)


def choose_nt(M, N, K, with_ws):
    """-> (shape, SkPlan); shape in 'std' (128 x 128), 'n64' (128 x 64), 'small' (64 x 64).  The 256 x 128 shape is only taken
    under WESUP_NT_SHAPE=big."""
    t128 = cdiv(M, 128) * cdiv(N, 128)
    if N > 64:
        if with_ws:
            sk = plan_streamk(M, N, K, 128, 128, 512)
            if sk.parts > 0:
                return 'std', sk
        if t128 >= 384:
            return 'std', NO_SK
    if N <= 64 and cdiv(M, 128) >= 384:
        return 'n64', NO_SK
    return 'small', NO_SK


def nt_three_stages(blocks):
    return blocks <= 512


def nt_workspace_bytes(M, N, K):
    if M <= 0 or N <= 0 or K <= 0 or K % BK:
        return 0
    return choose_nt(M, N, K, True)[1].ws_bytes


# route -> (tile rows, tile columns)
NT_TILE = {'nt64x3': (64, 64), 'nt64x2': (64, 64), 'nt128x64': (128, 64), 'nt128': (128, 128), 'nt128sk': (128, 128),
           'ntb64x128': (64, 128), 'ntb128x64': (128, 64), 'ntb64x3': (64, 64), 'ntb64x2': (64, 64),
           'ntbb128': (128, 128), 'ntbb64x3': (64, 64), 'ntbb64x2': (64, 64)}


def nt_route(M, N, K, ws_bytes=0):
    """Route of wesup_gemm_nt when the caller passes an aligned workspace of ws_bytes (0: none) -> (route, SkPlan)."""
    shape, sk = choose_nt(M, N, K, ws_bytes > 0)
    if sk.parts > 0 and ws_bytes < sk.ws_bytes:
        shape, sk = choose_nt(M, N, K, False)
    if shape == 'std':
        return ('nt128sk' if sk.parts > 0 else 'nt128'), sk
    if shape == 'n64':
        return 'nt128x64', sk
    return ('nt64x3' if nt_three_stages(cdiv(M, 64) * cdiv(N, 64)) else 'nt64x2'), sk


def ntb_route(nbatch, M, N, K):
    """wesup_gemm_nt_batched"""
    t128 = cdiv(M, 128) * cdiv(N, 128) * nbatch
    t64 = cdiv(M, 64) * cdiv(N, 64) * nbatch
    if N > 64 and t128 >= 384:
        if cdiv(M, 64) * 64 * cdiv(N, 128) * 128 < cdiv(M, 128) * 128 * cdiv(N, 64) * 64:
            return 'ntb64x128'
        return 'ntb128x64'
    return 'ntb64x3' if nt_three_stages(t64) else 'ntb64x2'


def ntbb_route(nbatch, M, N, K):
    """wesup_gemm_nt_batched_bias"""
    t128 = cdiv(M, 128) * cdiv(N, 128) * nbatch
    t64 = cdiv(M, 64) * cdiv(N, 64) * nbatch
    if N > 64 and t128 >= 384:
        return 'ntbb128'
    return 'ntbb64x3' if nt_three_stages(t64) else 'ntbb64x2'


# ---------------------------------------------------------------- TN family
TnPlan = namedtuple('TnPlan', 'tile tiles_m tiles_n S k_per_split taps', defaults=(1,))


def plan_tn(M, N, K, nbatch=1, taps=1):
    """taps: the nine taps of a direct conv3x3 weight gradient ride in grid.x and count as tiles, exactly where nbatch does."""
    big = M >= 128 and N >= 128
    ks = cdiv(K, BK)
    if big:
        t128 = cdiv(M, 128) * cdiv(N, 128) * taps * nbatch
        ms = 32 if ks // 8 > 32 else (ks // 8 if ks // 8 > 0 else 1)
        if t128 * ms < 384:
            big = False
    tile = 128 if big else 64
    tiles_m, tiles_n = cdiv(M, tile), cdiv(N, tile)
    tiles = tiles_m * tiles_n * taps * nbatch
    slots = 256 * (2 if big else 4)
    maxS = ks // 8 if ks // 8 > 0 else 1
    S, best = 1, -1.0
    for rounds in (1, 2, 3):
        cand = min(max((slots * rounds) // tiles, 1), maxS)
        blocks = tiles * cand
        fill = blocks / (cdiv(blocks, slots) * slots)
        if fill > best + 0.02:
            best, S = fill, cand
    if tiles >= 600:
        S = 1
    if S > 32 and tiles * 32 >= 192:
        S = 32
    k_per_split = cdiv(ks, S) * BK
    return TnPlan(tile, tiles_m, tiles_n, cdiv(K, k_per_split), k_per_split, taps)


def slab_fold_chunks(S):
    return 16 if S > 32 else 0


def tn_direct(pl, colsum, ldc, c_addr=0, strideC=0):
    return pl.S == 1 and not colsum and ldc % 2 == 0 and c_addr % 8 == 0 and strideC % 2 == 0


def tn_weighted(pl, nbatch=1):
    return pl.tile == 128 and nbatch == 1 and pl.S >= 2 and pl.tiles_m * pl.tiles_n * pl.taps * pl.S <= 512


def tn_store(pl, colsum=False, ldc=0, strideC=0):
    """How the product reaches C: 'direct' (the tiles are the result), 'slab' (one split through a slab and the reduce kernel),
    'reduce' (2 to 32 slabs), 'fold' (more: a fold launch in front of the reduce)."""
    if tn_direct(pl, colsum, ldc, 0, strideC):
        return 'direct'
    if pl.S == 1:
        return 'slab'
    return 'fold' if slab_fold_chunks(pl.S) else 'reduce'


def tn_workspace_bytes(M, N, K):
    pl = plan_tn(M, N, K)
    elems = M * N + M
    return align_up(pl.S * elems * 4, 256) + slab_fold_chunks(pl.S) * elems * 4


def tn_batched_workspace_bytes(nbatch, M, N, K):
    return nbatch * plan_tn(M, N, K, nbatch).S * (M * N + M) * 4


def colsum_chunks(M, N):
    return max(1, min(2048 // cdiv(N, 64), cdiv(M, 64)))


def colsum_workspace_bytes(M, N):
    return colsum_chunks(M, N) * N * 4


TRANSPOSE_MAX = 40

# ---------------------------------------------------------------- the cases
# ws: how wesup_gemm_nt gets its stream-K workspace: None (NULL, 0), 'full' (what the query asks for), 'short' (one byte less:
# the dispatch has to fall back to plain tiling)
NtCase = namedtuple('NtCase', 'id M N K route edge ws sk', defaults=(None, None))
NT_CASES = [
    NtCase('nt-5x4x32', 5, 4, 32, 'nt64x3', 'one K-step: the prologue is the last step; M = 5, N = 4'),
    NtCase('nt-100x36x32', 100, 36, 32, 'nt64x3', 'two M-tiles, ragged; one K-step'),
    NtCase('nt-70x68x96', 70, 68, 96, 'nt64x3', 'N tail above 64; three K-steps: every buffer of the ring once'),
    NtCase('nt-40004x36x32', 40004, 36, 32, 'nt64x2', '626 blocks, N <= 64, one K-step in two stages'),
    NtCase('nt-19204x132x64', 19204, 132, 64, 'nt64x2', '903 blocks, N > 64 below the 128-tile threshold'),
    NtCase('nt-49028x36x64', 49028, 36, 64, 'nt128x64', '384 M-tiles of 128: the threshold itself; ragged M'),
    NtCase('nt-24452x260x64', 24452, 260, 64, 'nt128', '576 tiles, ragged M and N'),
    NtCase('nt-130x132x1024-sk', 130, 132, 1024, 'nt128sk', 'no whole tiles, 16 parts of 8 steps', 'full', (0, 16, 128)),
    NtCase('nt-130x132x1088-sk', 130, 132, 1088, 'nt128sk', '34 steps per tile, 8 per part: parts end one tile and begin the next',
           'full', (0, 17, 136)),
    NtCase('nt-24452x260x512-sk', 24452, 260, 512, 'nt128sk', '512 whole tiles + 128 parts over the other 64', 'full', (512, 128, 1024)),
    NtCase('nt-130x132x1024-shortws', 130, 132, 1024, 'nt64x3', 'workspace one byte short: plain tiling', 'short'),
]

# wesup_gemm_nt_batched: K = 32 or 64, strided operands
NtbCase = namedtuple('NtbCase', 'id nbatch M N K route edge')
NTB_CASES = [
    NtbCase('ntb-36x900x256x64', 36, 900, 256, 64, 'ntb64x128', 'M pads less at 64: 960 rows instead of 1024'),
    NtbCase('ntb-36x1028x132x32', 36, 1028, 132, 32, 'ntb128x64', 'ragged M and N, one K-step'),
    NtbCase('ntb-5x100x68x32', 5, 100, 68, 32, 'ntb64x3', '20 blocks, N tail above 64'),
    NtbCase('ntb-20x1700x36x64', 20, 1700, 36, 64, 'ntb64x2', '540 blocks'),
    NtbCase('ntb-1x70x68x32', 1, 70, 68, 32, 'ntb64x3', 'nbatch = 1'),
]
NTBB_CASES = [
    NtbCase('ntbb-3x16388x132x32', 3, 16388, 132, 32, 'ntbb128', '774 tiles of 128 x 128, ragged M and N'),
    NtbCase('ntbb-3x100x68x64', 3, 100, 68, 64, 'ntbb64x3', '12 blocks'),
    NtbCase('ntbb-3x11524x36x32', 3, 11524, 36, 32, 'ntbb64x2', '543 blocks'),
]
BIAS_MODES = ('strided', 'shared', 'null')

# wesup_gemm_tn.  variants: (relu_b, colsum, odd ldc, how the product reaches C)
TnCase = namedtuple('TnCase', 'id M N K tile S weighted edge variants')
TN_CASES = [
    TnCase('tn-4x4x5', 4, 4, 5, 64, 1, False, 'K < 32', ((0, 0, 0, 'direct'), (1, 1, 0, 'slab'))),
    TnCase('tn-36x20x33', 36, 20, 33, 64, 1, False, 'ragged K: one row in the second step', ((0, 0, 0, 'direct'), (1, 1, 0, 'slab'))),
    TnCase('tn-260x132x290', 260, 132, 290, 64, 1, False, 'ragged tiles; colsum and an odd ldc force the slab',
           ((0, 0, 0, 'direct'), (0, 1, 0, 'slab'), (0, 0, 1, 'slab'))),
    TnCase('tn-132x132x3000', 132, 132, 3000, 64, 11, False, 'ragged last split', ((0, 0, 0, 'reduce'), (1, 1, 0, 'reduce'))),
    TnCase('tn-68x132x60000', 68, 132, 60000, 64, 32, False, 'S capped at 32', ((0, 0, 0, 'reduce'), (1, 1, 1, 'reduce'))),
    TnCase('tn-64x128x57600', 64, 128, 57600, 64, 225, False, 'fold launch in front of the reduce', ((0, 0, 0, 'fold'), (1, 1, 0, 'fold'))),
    TnCase('tn-2564x2564x36', 2564, 2564, 36, 128, 1, False, 'ragged tiles in both directions',
           ((0, 0, 0, 'direct'), (1, 0, 0, 'direct'), (0, 1, 0, 'slab'), (1, 1, 0, 'slab'))),
    TnCase('tn-516x516x4100', 516, 516, 4100, 128, 15, True, 'weighted split, ragged last K-step',
           ((0, 0, 0, 'reduce'), (1, 0, 0, 'reduce'), (0, 1, 0, 'reduce'), (1, 1, 0, 'reduce'))),
    TnCase('tn-1028x1028x2052', 1028, 1028, 2052, 128, 6, True, 'weighted split',
           ((0, 0, 0, 'reduce'), (1, 0, 0, 'reduce'), (0, 1, 0, 'reduce'), (1, 1, 0, 'reduce'))),
]

# wesup_gemm_tn_batched, row-strided B and C.  variants: (relu_b, odd strideC, how the product reaches C)
TnbCase = namedtuple('TnbCase', 'id nbatch M N K tile S edge variants')
TNB_CASES = [
    TnbCase('tnb-3x1028x1028x4100', 3, 1028, 1028, 4100, 128, 2, 'not weighted: nbatch > 1', ((0, 0, 'reduce'), (1, 0, 'reduce'))),
    TnbCase('tnb-2x132x132x900', 2, 132, 132, 900, 64, 3, 'ragged last split', ((0, 0, 'reduce'), (1, 1, 'reduce'))),
    TnbCase('tnb-7x1284x1284x40', 7, 1284, 1284, 40, 128, 1, '847 tiles; an odd strideC forces the slab',
            ((0, 0, 'direct'), (0, 1, 'slab'))),
]

# wesup_colsum (M, N, lda - N): 64 columns and colsum_chunks row ranges per pass
COLSUM_CASES = [(1, 4, 0), (65, 68, 0), (65, 68, 12), (131073, 4, 4), (1000, 260, 4)]
# wesup_transpose (rows, cols): 32 x 32 tiles; the entry takes no row stride, so the input is always contiguous
TRANSPOSE_CASES = [(1, 1), (33, 65), (32, 32), (5, 1000)]

# every route the issue names must have a row
NT_ROUTES = ('nt64x3', 'nt64x2', 'nt128x64', 'nt128', 'nt128sk')
NTB_ROUTES = ('ntb64x128', 'ntb128x64', 'ntb64x3', 'ntb64x2')
NTBB_ROUTES = ('ntbb128', 'ntbb64x3', 'ntbb64x2')
TN_ROUTES = ((64, 'direct'), (64, 'slab'), (64, 'reduce'), (64, 'fold'), (128, 'direct'), (128, 'slab'), (128, 'reduce'))

# Shapes that no kernel runs: they sit on either side of a threshold whose effect shows in a workspace query, so that the
# threshold cannot move in gemm.hip alone.  (M, N, K, does stream-K apply) and (nbatch, M, N, K, splits).
NT_PINS = [
    (24452, 260, 512, True), (24452, 260, 480, False),                # 16 K-steps and 15
    (324 * 128, 260, 512, True), (495 * 128, 260, 512, False),        # 460 and 461 tiles left over of 512 slots: the nine-tenths rule
    (130, 132, 1024, True), (130, 132, 992, False),                   # under one round: 32 K-steps and 31
    (24452, 64, 1024, False), (24452, 68, 1024, True),                # N <= 64 never
    (65536, 256, 512, False),                                         # whole rounds
]
TN_PINS = [
    (1, 4036, 2556, 600, 1), (1, 3328, 2944, 600, 2),                 # 640 tiles: one split; 598: the fullest of three rounds
    (1, 516, 516, 4100, 15), (1, 512, 768, 3900, 10),                 # 25 tiles x 16 splits >= 384: 128 x 128; 24 x 15 < 384: 64 x 64
    (1, 68, 132, 60000, 32), (1, 64, 128, 57600, 225),                # six 64 x 64 tiles: capped at 32 splits; two: not
    (1, 132, 132, 255, 1), (1, 132, 132, 512, 2),                     # every split keeps eight K-steps
    (3, 1028, 1028, 4100, 2), (7, 1284, 1284, 40, 1),
]
# The thresholds no query shows (which tile a product takes, two or three stages, the weighted split, the direct store) are
# held by their source text: each line below must stand in csrc/gemm.hip this many times, blanks aside.
SOURCE_PINS = [
    ('if (N <= 64 || nk < 16 || R == 0 || R * 10 > slots * 9) return pl;', 1),
    ('if (tiles < slots && nk < 32) return pl;', 1),
    ('const int P = (int)(W / 8 < slots ? W / 8 : slots);', 1),
    ('const SkPlan sk = plan_streamk(M, N, K, 128, 128, 512);', 1),
    ('if (t128 >= 384) { c.shape = NT_STD; return c; }', 1),
    ('if (N <= 64 && (long)ceil_div(M, 128) >= 384) { c.shape = NT_N64; return c; }', 1),
    ('static bool nt_three_stages(long blocks) { return blocks <= 512; }', 1),
    ('if (N > 64 && t128 >= 384)', 2),
    ('(alt == 2 && (long)ceil_div(M, 64) * 64 * ceil_div(N, 128) * 128 < (long)ceil_div(M, 128) * 128 * ceil_div(N, 64) * 64)', 1),
    ('bool big = (M >= 128 && N >= 128);', 1),
    ('if (t128 * ms < 384) big = false;', 1),
    ('const int slots = 256 * (big ? 2 : 4);', 1),
    ('if (fill > best + 0.02) { best = fill; S = cand; }', 1),
    ('return e ? atoi(e) : 600; }();', 1),
    ('if (small_rule && S > 32 && (long)tiles * 32 >= 192) S = 32;', 1),
    ('if (pl.bm == 128 && nbatch == 1 && pl.S >= 2 && (long)grid_blocks(pl) <= 512) {', 1),
    ('return pl.S == 1 && !colsum_a && (ldc % 2) == 0 && (((uintptr_t)C) & 7) == 0;', 1),
    ('if (tn_direct(pl, nullptr, C, ldc) && strideC % 2 == 0) {', 1),
    ('static int slab_fold_chunks(int S) { return S > 32 ? 16 : 0; }', 1),
    ('int chunks = 2048 / ceil_div(N, 64);', 1),
]

# the GEMM shapes tests/test_kernels_gpu.py runs ("GEMMs" and "stream-K" blocks): their workspace queries are held to the
# restatement as well
EXISTING_NT = [(100, 32, 64), (2400, 1024, 2112), (600, 2112, 1024), (57600, 64, 128), (50000, 256, 64), (37, 32, 1024),
               (49160, 32, 64), (2336, 1024, 2112), (3600, 512, 4608), (14400, 512, 2304), (57600, 256, 1152), (130, 128, 1024),
               (66000, 128, 512), (130, 128, 512), (14400, 256, 512), (3600, 256, 512), (900, 256, 512)]
EXISTING_TN = [(32, 1024, 2400), (1024, 2112, 600), (64, 128, 57600), (256, 512, 3601), (32, 64, 230400), (4036, 2556, 330),
               (584, 768, 900)]
EXISTING_TNB = [(3, 584, 768, 900), (4, 3600, 768, 640)]
