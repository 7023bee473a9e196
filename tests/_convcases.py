"""The dispatch of the direct 3x3 convolutions of wesup_amd/csrc/gemm.hip (conv_common -> gemm_nt_kernel<MODE 1/2>, wesup_conv3x3_wgrad
-> gemm_tn_kernel<MODE 1/2>) restated on top of tests/_gemmcases.py, and the table of conv cases that tests/test_conv_routes_cpu.py
(does every row reach the route it names?) and tests/test_conv_routes_gpu.py (is every row exact?) share.

Only the default settings are restated, as in _gemmcases.py: the routes behind WESUP_NT_SHAPE, WESUP_TN_SMALL_RULE,
WESUP_TN_S1_MIN_TILES, WESUP_TN_WEIGHTS, WESUP_TN_XCD and WESUP_NT_MB are read once per process and are not covered here.

A row of the forward table is the shape of the implicit GEMM: Cin channels in the tensor the kernel reads, Cout in the one it
writes.  The forward test runs it as the layer Cin -> Cout, the dgrad test as the layer Cout -> Cin (dy has Cin channels, dx
Cout): the same route, which is what "dgrad is the forward with the channel roles swapped" means in conv_common.

A change that moves a threshold of conv_common, dispatch_nt_r, dispatch_nt_side, plan_wgrad or launch_tn has to update the
restatement below AND the rows whose route it moves, in the same change.
"""
from collections import namedtuple

import _gemmcases as g
from _gemmcases import NO_SK, cdiv

NT_STREAM_BYTES = 16 * 1048576           # wino_nt_stores' default (WESUP_NT_MB)


def conv_kpad(Ci):
    return cdiv(9 * max(Ci, 4), g.BK) * g.BK


def is_image(Cin):
    """The image layer: 3 true channels in a 4-channel tensor (the entries take Cin = 4 forward, Ci = 3 in the weight gradient)."""
    return Cin < 32


# ---------------------------------------------------------------- forward / dgrad
# route -> (tile rows, tile columns)
CONV_TILE = {'cv64': (64, 64), 'cv128x64': (128, 64), 'cv128': (128, 128), 'cv128sk': (128, 128), 'im64': (64, 64),
             'im128x64': (128, 64), 'cvside64': (128, 64), 'cvside128': (128, 128), 'imside64': (128, 64)}


def conv_workspace_bytes(B, H, W, Cin, Cout):
    if B <= 0 or H <= 0 or W <= 0 or Cin < 32 or Cout <= 0:
        return 0
    return g.choose_nt(B * H * W, Cout, 9 * Cin, True)[1].ws_bytes


def conv_route(B, H, W, Cin, Cout, ws_bytes=0, side=False):
    """-> (route, SkPlan) of conv_common for an aligned workspace of ws_bytes (0: none); route None: WESUP_ERR_INVALID."""
    M, N, K = B * H * W, Cout, conv_kpad(Cin)
    pre = 'im' if is_image(Cin) else 'cv'
    if side:                                           # dispatch_nt_side: one N-tile holds all output channels, no stream-K
        if N == 64:
            return pre + 'side64', NO_SK
        if N == 128 and not is_image(Cin):
            return 'cvside128', NO_SK
        return None, NO_SK
    if is_image(Cin):                                  # dispatch_nt<2>(p, st, nullptr, 0)
        shape, sk = g.choose_nt(M, N, K, False)
    else:
        shape, sk = g.choose_nt(M, N, K, ws_bytes > 0)
        if sk.parts > 0 and ws_bytes < sk.ws_bytes:
            shape, sk = g.choose_nt(M, N, K, False)
    if shape == 'std':
        return pre + ('128sk' if sk.parts > 0 else '128'), sk
    if shape == 'n64':
        return pre + '128x64', sk
    return pre + '64', sk                              # never three stages: (MODE == 0 || MODE == 3) only


def conv_streams(M, Cout, accum=False, outputs=1):
    """NT_FLAG_STREAM: the output is written with streaming stores."""
    return not accum and 4.0 * M * Cout * outputs > NT_STREAM_BYTES


# ---------------------------------------------------------------- weight gradient
WgradPlan = namedtuple('WgradPlan', 'tile tiles_m tiles_n taps S k_per_split weighted tiny store Nslab')


def wgrad_plan(B, H, W, Ci, Cout):
    K = B * H * W
    if is_image(Ci):
        pl, ncol = g.plan_tn(Cout, 64, K, taps=1), 64
    else:
        pl, ncol = g.plan_tn(Cout, Ci, K, taps=9), Ci
    store = 'slab' if pl.S == 1 else ('fold' if g.slab_fold_chunks(pl.S) else 'reduce')
    return WgradPlan(pl.tile, pl.tiles_m, pl.tiles_n, pl.taps, pl.S, pl.k_per_split, g.tn_weighted(pl), W < 16 or H < 2, store,
                     ncol * pl.taps)


def wgrad_route(B, H, W, Ci, Cout):
    p = wgrad_plan(B, H, W, Ci, Cout)
    return f"{p.tile}-{'image' if is_image(Ci) else 'conv'}-{'tiny' if p.tiny else 'fast'}-{p.store}"


def wgrad_workspace_bytes(B, H, W, Ci, Cout):
    if B <= 0 or H <= 0 or W <= 0 or Ci <= 0 or Cout <= 0:
        return 0
    p = wgrad_plan(B, H, W, Ci, Cout)
    elems = Cout * p.Nslab + Cout
    return g.align_up(p.S * elems * 4, 256) + g.align_up(g.slab_fold_chunks(p.S) * elems * 4, 256)


# ---------------------------------------------------------------- the cases
# ws: None (NULL, 0), 'full' (what wesup_conv3x3_workspace_bytes asks for), 'short' (one byte less: plain tiling).
# tiles: (rows of tiles, columns of tiles) of the route's tile.  sk: (whole tiles, parts, K-steps shared).
ConvCase = namedtuple('ConvCase', 'id B H W Cin Cout route tiles edge ws sk', defaults=(None, None))
CONV_CASES = [
    ConvCase('cv-1x1x1x32x32', 1, 1, 1, 32, 32, 'cv64', (1, 1), 'one pixel: only the centre tap is live'),
    ConvCase('cv-1x40x1x32x36', 1, 40, 1, 32, 36, 'cv64', (1, 1), 'W = 1: no left or right tap; N tail below 64'),
    ConvCase('cv-1x1x70x32x32', 1, 1, 70, 32, 32, 'cv64', (2, 1), 'H = 1: no upper or lower tap; two M-tiles'),
    ConvCase('cv-2x5x2x32x32', 2, 5, 2, 32, 32, 'cv64', (1, 1), 'W = 2: every pixel on a border'),
    ConvCase('cv-3x7x9x64x68', 3, 7, 9, 64, 68, 'cv64', (3, 2),
             '63-pixel images: every 64-row tile straddles two; N tail above 64; two 32-channel chunks'),
    ConvCase('cv-1x223x220x32x64', 1, 223, 220, 32, 64, 'cv128x64', (384, 1), 'exactly 384 M-tiles of 128: the threshold itself'),
    ConvCase('cv-1x222x220x32x64', 1, 222, 220, 32, 64, 'cv64', (764, 1), 'the other side of that threshold'),
    ConvCase('cv-1x112x109x32x512', 1, 112, 109, 32, 512, 'cv128', (96, 4), '384 tiles: the threshold itself; ragged M; streaming stores'),
    ConvCase('cv-1x112x108x32x512', 1, 112, 108, 32, 512, 'cv64', (189, 8), 'the other side: 380 tiles of 128'),
    ConvCase('cv-1x130x126x32x260', 1, 130, 126, 32, 260, 'cv128', (128, 3), 'ragged N, three N-tiles; streaming stores'),
    ConvCase('cv-2x20x19x128x128-sk', 2, 20, 19, 128, 128, 'cv128sk', (6, 1),
             'no whole tiles, 27 parts over 6 tiles: parts end one tile and begin the next; images straddle tiles', 'full', (0, 27, 216)),
    ConvCase('cv-2x20x19x128x128', 2, 20, 19, 128, 128, 'cv64', (12, 2), 'the same shape without a workspace'),
    ConvCase('cv-1x149x147x64x260-sk', 1, 149, 147, 64, 260, 'cv128sk', (172, 3), '512 whole tiles + 9 parts over the other 4', 'full',
             (512, 9, 72)),
    ConvCase('cv-1x149x147x64x260-shortws', 1, 149, 147, 64, 260, 'cv128', (172, 3), 'workspace one byte short: plain tiling', 'short'),
    ConvCase('im-1x223x220x3x64', 1, 223, 220, 3, 64, 'im128x64', (384, 1), 'image layer at the 128 x 64 threshold'),
    ConvCase('im-2x9x11x3x64', 2, 9, 11, 3, 64, 'im64', (4, 1), 'image layer, 99-pixel images, ragged last tile'),
    ConvCase('im-1x1x1x3x64', 1, 1, 1, 3, 64, 'im64', (1, 1), 'image layer, one pixel'),
]
# wesup_conv3x3_fwd_side; ld_side is wider than Cout / 2 in the GPU test
SIDE_CASES = [
    ConvCase('side-2x13x10x32x64', 2, 13, 10, 32, 64, 'cvside64', (3, 1), '130-pixel images: the 128-row tile straddles two; ragged last tile'),
    ConvCase('side-2x13x10x64x128', 2, 13, 10, 64, 128, 'cvside128', (3, 1), 'the same under the 128 x 128 tile'),
    ConvCase('side-2x13x10x3x64', 2, 13, 10, 3, 64, 'imside64', (3, 1), 'image layer'),
]

WgradCase = namedtuple('WgradCase', 'id B H W Ci Cout route tiles S weighted edge')
WGRAD_CASES = [
    WgradCase('wg-3x5x7x32x32', 3, 5, 7, 32, 32, '64-conv-tiny-slab', (1, 1), 1, False, 'tiny by W = 7; K = 105'),
    WgradCase('wg-1x1x40x32x32', 1, 1, 40, 32, 32, '64-conv-tiny-slab', (1, 1), 1, False, 'tiny by H = 1'),
    WgradCase('wg-2x40x9x32x32', 2, 40, 9, 32, 32, '64-conv-tiny-reduce', (1, 1), 2, False, 'tiny, two splits'),
    WgradCase('wg-1x2x16x32x64', 1, 2, 16, 32, 64, '64-conv-fast-slab', (1, 1), 1, False, 'the fast path at its minimum: H = 2, W = 16 (steps begin at column 0: one carry)'),
    WgradCase('wg-3x5x17x32x32', 3, 5, 17, 32, 32, '64-conv-fast-slab', (1, 1), 1, False,
              'W = 17: second carry; K = 255 ragged; K-steps cross image boundaries'),
    WgradCase('wg-2x33x17x64x64', 2, 33, 17, 64, 64, '64-conv-fast-reduce', (1, 1), 4, False, 'W = 17: second carry; splits begin in mid-row'),
    WgradCase('wg-2x20x31x32x32', 2, 20, 31, 32, 32, '64-conv-fast-reduce', (1, 1), 4, False, 'W = 31: a step can end on a row end, one carry'),
    WgradCase('wg-2x20x32x32x32', 2, 20, 32, 32, 32, '64-conv-fast-reduce', (1, 1), 5, False, 'W = 32: a step is a row, one carry'),
    WgradCase('wg-2x20x33x32x32', 2, 20, 33, 32, 32, '64-conv-fast-reduce', (1, 1), 5, False, 'W = 33: at most one row end per step'),
    WgradCase('wg-1x64x64x32x32', 1, 64, 64, 32, 32, '64-conv-fast-reduce', (1, 1), 16, False, '16 splits'),
    WgradCase('wg-1x160x160x32x32', 1, 160, 160, 32, 32, '64-conv-fast-reduce', (1, 1), 32, False, '32 splits'),
    WgradCase('wg-1x30x30x128x256', 1, 30, 30, 128, 256, '64-conv-fast-reduce', (4, 2), 3, False, '4 x 2 tiles of 64'),
    WgradCase('wg-2x20x17x32x96', 2, 20, 17, 32, 96, '64-conv-fast-reduce', (2, 1), 2, False, 'Cout = 96: ragged M-tile; W = 17: second carry'),
    WgradCase('wg-1x56x56x256x256', 1, 56, 56, 256, 256, '128-conv-fast-reduce', (2, 2), 11, True, 'weighted split, 396 blocks'),
    WgradCase('wg-1x32x32x512x512', 1, 32, 32, 512, 512, '128-conv-fast-reduce', (4, 4), 3, True, 'weighted split, 4 x 4 tiles'),
    WgradCase('wg-1x46x17x512x512', 1, 46, 17, 512, 512, '128-conv-fast-reduce', (4, 4), 3, True,
              'weighted split under W = 17: second carry in the 128 x 128 instance'),
    WgradCase('wg-1x52x15x512x512', 1, 52, 15, 512, 512, '128-conv-tiny-reduce', (4, 4), 3, True, 'weighted split on the tiny path'),
    WgradCase('wg-1x5x7x1024x1024', 1, 5, 7, 1024, 1024, '128-conv-tiny-slab', (8, 8), 1, False, '576 blocks, one split, two K-steps'),
    WgradCase('wg-1x2x16x1024x1024', 1, 2, 16, 1024, 1024, '128-conv-fast-slab', (8, 8), 1, False, '576 blocks, one K-step'),
    WgradCase('wg-1x8x17x1024x1024', 1, 8, 17, 1024, 1024, '128-conv-fast-slab', (8, 8), 1, False,
              '576 blocks, five K-steps, W = 17: second carry, one split'),
    WgradCase('wg-1x20x15x3x64', 1, 20, 15, 3, 64, '64-image-tiny-slab', (1, 1), 1, False, 'image layer, tiny'),
    WgradCase('wg-1x60x15x3x64', 1, 60, 15, 3, 64, '64-image-tiny-reduce', (1, 1), 3, False, 'image layer, tiny, three splits'),
    WgradCase('wg-1x700x15x3x64', 1, 700, 15, 3, 64, '64-image-tiny-fold', (1, 1), 37, False, 'image layer, tiny, fold'),
    WgradCase('wg-1x9x16x3x64', 1, 9, 16, 3, 64, '64-image-fast-slab', (1, 1), 1, False, 'image layer, W = 16 (steps begin at column 0: one carry), one split'),
    WgradCase('wg-1x37x31x3x64', 1, 37, 31, 3, 64, '64-image-fast-reduce', (1, 1), 4, False, 'image layer, W = 31: one carry, S = 4'),
    WgradCase('wg-1x40x23x3x64', 1, 40, 23, 3, 64, '64-image-fast-reduce', (1, 1), 3, False, 'image layer, W = 23: second carry, S = 3'),
    WgradCase('wg-1x96x96x3x64', 1, 96, 96, 3, 64, '64-image-fast-fold', (1, 1), 36, False, 'image layer, S = 36: fold'),
]



def second_carry_steps(B, H, W):
    """The K-steps of the fast path (W >= 16, H >= 2) in which some pixel takes the SECOND carry of mask_b / step_mask.  Every
    split begins at a multiple of 32 pixels (k_per_split is one; so is a weighted range), so the steps begin at the pixels 32 j:
    column w0 = 32 j mod W, and lane r <= 31 wraps twice when w0 + r >= 2 W -- possible only for 17 <= W <= 30 (W = 16 always begins
    at column 0; W = 31 would need w0 = 31).  Only pixels inside K count: beyond it the lane is masked whatever its coordinates."""
    K = B * H * W
    return [j for j in range(cdiv(K, 32)) if (32 * j) % W + 31 >= 2 * W and 32 * j + 2 * W - (32 * j) % W < K]


def split_starts(B, H, W, Ci, Cout):
    """The first K-step of every split, as the kernel cuts K: equal ranges of k_per_split, or the weighted ranges (3 : 2) of
    gemm_tn_kernel, which differ between the tiles by how many of a tile's splits sit among the first 256 blocks.  -> a list of
    lists, one per kind of tile."""
    p, K = wgrad_plan(B, H, W, Ci, Cout), B * H * W
    if not p.weighted:
        return [[y * p.k_per_split // 32 for y in range(p.S)]]
    gx, T, out = p.tiles_m * p.tiles_n * p.taps, cdiv(K, 32), []
    for n_o in sorted({min(p.S, (255 - bx) // gx + 1) if bx < 256 else 0 for bx in range(gx)}):
        wtot = 3 * n_o + 2 * (p.S - n_o)
        out.append([T * (3 * min(y, n_o) + 2 * max(0, y - n_o)) // wtot for y in range(p.S)])
    return out


def second_carry_code(B, H, W, Ci, Cout):
    """Which code computes a second carry of the row: the conv mode takes the masks of a split's first two K-steps from mask_b and
    those of the later ones from the balloted step_mask; the image layer takes all from mask_b.  -> a set of their names."""
    who = set()
    for starts in split_starts(B, H, W, Ci, Cout):
        for j in second_carry_steps(B, H, W):
            rel = j - max(s0 for s0 in starts if s0 <= j)
            who.add('mask_b' if is_image(Ci) or rel < 2 else 'step_mask')
    return who


# the rows of the fast path that take the second carry (the CPU test proves it, and that no other fast row does)
WGRAD_SECOND_CARRY = ('wg-3x5x17x32x32', 'wg-2x33x17x64x64', 'wg-2x20x17x32x96', 'wg-1x46x17x512x512', 'wg-1x8x17x1024x1024',
                      'wg-1x40x23x3x64')

# every route must have a row
CONV_ROUTES = ('cv64', 'cv128x64', 'cv128', 'cv128sk', 'im64', 'im128x64')
SIDE_ROUTES = ('cvside64', 'cvside128', 'imside64')
# (64 | 128) x (conv | image) x (tiny | fast) x (slab | reduce | fold) where plan_tn can produce it: the image layer has N = 64
# and so never 128 x 128 tiles; with nine taps in the grid a conv has at least nine tiles, where more than 32 splits are capped
# at 32: only the image layer folds
WGRAD_ROUTES = tuple(f'{t}-conv-{p}-{s}' for t in (64, 128) for p in ('tiny', 'fast') for s in ('slab', 'reduce')) + \
    tuple(f'64-image-{p}-{s}' for p in ('tiny', 'fast') for s in ('slab', 'reduce', 'fold'))

# Shapes that no kernel runs, on either side of a threshold a workspace query shows.
# (B, H, W, Cin, Cout, does stream-K apply)
CONV_PINS = [
    (1, 149, 147, 64, 260, True), (1, 149, 147, 32, 260, False), (1, 149, 147, 64, 64, False),    # 18 K-steps, 9 (< 16); N <= 64 never
    (2, 20, 19, 128, 128, True), (2, 20, 19, 64, 128, False),                  # under one round: 36 K-steps and 18 (< 32)
    (1, 149, 147, 3, 260, False), (1, 149, 147, 16, 260, False),               # Cin < 32: the query answers 0
    (1, 128, 128, 64, 512, False),                                             # 512 tiles: whole rounds
    (1, 247, 256, 64, 260, True), (1, 252, 251, 64, 260, False),               # 458 and 461 tiles left over of 512 slots: the nine-tenths rule
]
# (B, H, W, Ci, Cout, tile, S)
WGRAD_PINS = [
    (1, 56, 56, 256, 256, 128, 11), (1, 40, 40, 256, 256, 64, 6),              # 36 tiles x 12 >= 384: 128 x 128; 36 x 6 < 384: 64 x 64
    (1, 32, 32, 512, 512, 128, 3), (1, 16, 30, 512, 512, 64, 1),
    (1, 64, 64, 32, 32, 64, 16), (1, 160, 160, 32, 32, 64, 32),                # nine tiles: capped at 32 splits
    (1, 96, 96, 3, 64, 64, 36), (1, 96, 96, 3, 128, 64, 36), (1, 96, 96, 3, 384, 64, 32),     # one and two tiles: not capped; six: capped
    (1, 5, 7, 1024, 1024, 128, 1), (1, 16, 16, 32, 32, 64, 1), (1, 16, 32, 32, 32, 64, 2),    # every split keeps eight K-steps
]
# The thresholds no query shows are held by their source text, as in _gemmcases.SOURCE_PINS: each line must stand in
# csrc/gemm.hip (csrc/common.hpp for the last) this many times, blanks aside.
SOURCE_PINS = [
    ('const bool tiny = (MODE == 1 || MODE == 2) && (p.W < 16 || p.H < 2);', 1),
    ('&& (MODE == 0 || MODE == 3)) return launch_nt<4, 64, 64, 1, 1, MODE, 3, RELU>(p, st);', 1),
    ('return launch_nt<4, 64, 64, 1, 1, MODE, 2, RELU>(p, st);', 1),
    ('if (p.N == 64) return launch_nt<4, 128, 64, 2, 1, MODE, 2, RELU, true>(p, st);', 1),
    ('if (p.N == 128) return launch_nt<4, 128, 128, 2, 2, MODE, 2, RELU, true>(p, st);', 1),
    ('TnPlan pl = plan_tn(Cout, 64, K, 1);', 1),
    ('return plan_tn(Cout, Ci, K, 9);', 1),
    ('return small ? dispatch_nt<2>(p, st, nullptr, 0) : dispatch_nt<1>(p, st, ws, ws_bytes);', 1),
    ('return choose_nt(B * H * W, Cout, 9 * Cin, true).sk.ws_bytes;', 1),
    ('p.flags = flags | ((!(flags & WESUP_ACCUM) && wino_nt_stores(4.0 * p.M * Cout * (y_relu ? 2 : 1))) ? NT_FLAG_STREAM : 0);', 1),
]
COMMON_PINS = [
    ('static const double limit = [] { const char* e = getenv("WESUP_NT_MB"); return (e ? atof(e) : 16.0) * 1048576.0; }();', 1),
    ('return bytes_written > limit ? 1 : 0;', 1),
]

# the conv shapes tests/test_kernels_gpu.py already runs (forward / dgrad / stream-K, fused side conv, wgrad): their workspace
# queries are held to the restatement as well
EXISTING_CONV = [(2, 12, 10, 64, 64), (1, 6, 6, 128, 256), (3, 5, 7, 256, 128), (1, 2, 2, 512, 512), (2, 16, 12, 3, 64),
                 (1, 224, 224, 64, 64), (1, 224, 224, 64, 128), (1, 230, 218, 3, 64), (1, 40, 36, 3, 64), (2, 33, 29, 64, 64),
                 (1, 37, 41, 64, 128), (2, 24, 24, 128, 128), (1, 11, 7, 32, 64), (4, 30, 30, 512, 512), (2, 60, 60, 256, 512),
                 (1, 120, 120, 128, 256)]
EXISTING_WGRAD = EXISTING_CONV[:5] + [(1, 120, 96, 64, 64), (2, 60, 60, 128, 128), (1, 100, 90, 3, 64), (3, 35, 17, 64, 64),
                                      (2, 33, 40, 32, 160), (1, 70, 50, 128, 64)]
