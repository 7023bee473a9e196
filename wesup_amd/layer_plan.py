"""What the engine launches for one shape, decided once: the per-layer forms of the forward and backward walk as data.

``groups_for`` says which resolutions take the interpolation-matrix form, ``build`` turns a shape, that grouping, the
routing and the switches into an immutable ``StepPlan`` (thirteen ``LayerPlan`` records + a few step-level facts).  The
engine (engine.py) launches what the plan says, on the buffers ``buffers`` lists for it (what a set of that shape holds, and
costs: ``nbytes``); nothing here imports torch or touches the GPU, so the whole decision table can be checked on the CPU
(tests/test_engine_plan_cpu.py).  The queries of the library a decision or a size depends on (ops.winograd_fused_supported,
ops.winograd_bias_rows, the classifier's partial-sum block) come in as callables.
"""
from collections import namedtuple

CONV_IDX = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
CONV_CH = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256),
           (256, 512), (512, 512), (512, 512), (512, 512), (512, 512), (512, 512)]
POOL_AFTER = [False, True, False, True, False, False, True, False, False, True, False, False, False]
SIDE_OFF = [0, 32, 64, 128, 192, 320, 448, 576, 832, 1088, 1344, 1600, 1856]
FM_CHANNELS = 2112
# (the 13th conv is followed by a MaxPool in VGG16 whose output the reference discards, models/wesup.py:279)

# Positions of the backward walk, measured in rounds 3 - 5 (every alternative within +-0.05 ms, HISTORY.md) and fixed: the deep
# layers' side-conv weight gradients are queued when the chain reaches conv2_1; the weight gradient of the layer above the lowest
# trainable one stays in front of its input gradient, every other one goes behind
DEEP_SIDE_WGRAD_AT = 2
WGRAD_EARLY_LAYERS = 1

# The engine's six boolean switches, its two class-level ones, the three class attributes of the weight-gradient routing, and
# its class-level int unpool_on_load.
Switches = namedtuple('Switches', 'fuse_pool_bwd fuse_pool_fwd two_streams wgrad_winograd conv_winograd plain matrix_pool '
                                  'fuse_side_fwd wgrad_min_ci wgrad_min_co wgrad_tile unpool_on_load',
                      defaults=(True, True, True, True, True, False, True, True, 128, 256, 4, 1))

Group = namedtuple('Group', 'layers h w off C')      # the layers of one coarse resolution: side outputs side by side, one matrix

LayerPlan = namedtuple('LayerPlan', [
    'ci', 'co', 'h', 'w',
    'm',              # 0: implicit GEMM, 2 / 4: Winograd F(m x m, 3x3) -- forward and input gradient
    'pool',           # a 2x2 max-pool follows
    'group',          # index of the layer's matrix-form group, or None (gather form)
    'commuted',       # side conv behind upsample + superpixel mean (one row per superpixel) instead of in front
    'side_in_conv',   # side conv in the epilogue of the direct-form conv
    'src', 'relu_in',  # what the conv reads: 'x0', or 'y' / 'yr' / 'yp' of layer l - 1; ReLU applied while loading
    'write_yr',       # the ReLU'd copy yr[l] is written
    'write_bits',     # this layer's input transform leaves the sign bits of y[l-1] (its input gradient reads them)
    'write_codes',    # this layer's pooling epilogue leaves the 3-bit pooling codes of y[l] (layer l + 1's input gradient reads them)
    'keep_v',         # the transformed input is kept for the weight gradient
    'defer_side',     # the side work is queued behind the next layer's input transform
    'trainable',
    'gather',         # the input gradient of layer l + 1 gathers this layer's side gradient in its epilogue
    'dual',           # both F(4x4) transforms of G[l] in one pass ...
    'bias_rows',      # ... which leaves this many rows of partial bias sums (0 without)
    'wgrad', 'wgrad_m',  # None | 'pre' (operands from the dual transform) | 'winograd_v' (kept V) | 'winograd' | 'direct'; its m
    'wgrad_late',     # queued behind the layer's input gradient instead of in front
    'dgrad',          # gradient handed to layer l - 1: None | 'gather' | 'unpool' | 'winograd' | 'direct'
    'pool_bwd',       # ... at pooled resolution, a maxpool2_bwd launch follows
])

StepPlan = namedtuple('StepPlan', [
    'shape', 'route', 'train', 'layers',
    'lowest',         # lowest trainable backbone layer (13: none)
    'relu_stored',    # pooled tensors are stored ReLU'd
    'runs',           # commuted layers whose G the input-gradient chain needs, deepest first, <= 3 layers of one resolution per run
    'late_at', 'late_side',   # the grouped layers' side-conv weight gradients are queued when the chain reaches late_at
    'shallow_first',  # the shallow layers' side gradients go to the head of the weight-gradient stream
    'fm', 'dfm',      # the (B,H,W,2112) feature map / its gradient are materialised (the unfused switches)
    # Per layer l, None or where its input gradient stays at pooled resolution (dP) for the dual transform of the pooled layer
    # l - 1 to unpool while loading (ops.winograd_dual_transform_unpool) instead of the 'gather' / 'unpool' epilogue scattering
    # it into G[l - 1]: ('G', 0) the head quarter of G[l - 1]'s own storage ('gather': nothing else writes that tensor), or
    # ('dV', first element) the tail of the shared dV buffer ('unpool': G[l - 1] holds the side gradient).  Storage the set
    # holds anyway: no row of the layer table and no buffer changes with it.
    'dp_on_load',
])

# One buffer of a set: b.<name> (layer None), b.<name>[layer], or b.groups[layer].<name[2:]> for the 'g.' names (layer = the group's
# index).  group: the side output (gradient) of a grouped layer is a channel slice of that group's 'g.s' ('g.ds'), no storage of its own
Buf = namedtuple('Buf', 'name layer shape dtype group')
ITEMSIZE = {'float32': 4, 'int16': 2, 'uint8': 1}


def tiles(B, H, W, m):
    """Tiles of the F(m x m, 3x3) domain of a (B,H,W) map (ops.winograd_tiles)."""
    return B * ((H + m - 1) // m) * ((W + m - 1) // m)


def dv_elems(B, dims):
    """Elements of the shared dV buffer: V' = B^T dY B of one layer at a time, the largest of them."""
    return max(36 * tiles(B, *dims[l], 4) * CONV_CH[l][1] for l in range(1, 13))


def layer_dims(H, W):
    dims, h, w = [], H, W
    for pool in POOL_AFTER:
        dims.append((h, w))
        if pool:
            h, w = h // 2, w // 2
    return dims


def route(route_fn, conv_winograd, B, H, W):
    """Per layer: m of the Winograd domain its forward / input gradient run in, or 0 for the implicit-GEMM kernel."""
    return tuple(int(route_fn(ci, co, h, w, B)) if (conv_winograd and ci >= 32) else 0
                 for (ci, co), (h, w) in zip(CONV_CH, layer_dims(H, W)))


def groups_for(B, H, W, Kmax, switches):
    """Coarse resolutions (deep layers): upsample + scatter-mean and its backward run as GEMMs with the interpolation-pooling
    matrix Wm of the resolution; the side outputs of the layers that share a resolution sit side by side in one buffer so that
    one GEMM per image serves all of them.  Returns (groups, group_of): Group records, and per layer its group's index or None."""
    dims = layer_dims(H, W)
    groups, group_of = [], [None] * 13
    if switches.fuse_pool_fwd and switches.fuse_pool_bwd and switches.matrix_pool and Kmax % 4 == 0:
        l = 0
        while l < 13:
            e = l
            while e + 1 < 13 and dims[e + 1] == dims[l]:
                e += 1
            gh, gw = dims[l]
            # ... up to 4096 cells and a matrix of at most 16 MB per image: beyond that (1024^2 with 3025 superpixels: conv5_x's
            # 64 x 64 map under 3072 rows = 50 MB per image, 19 GF per image and direction) the gather form with the side
            # conv commuted is faster (8 x 1024^2: 62.3 -> 61.2 ms, round 6); below it the matrix form is (batch 1: 7 - 9 %)
            if (gh, gw) != (H, W) and gh * gw <= 4096 and (gh * gw) % 4 == 0 and Kmax * gh * gw <= (4 << 20):
                layers = tuple(range(l, e + 1))
                for i in layers:
                    group_of[i] = len(groups)
                groups.append(Group(layers, gh, gw, SIDE_OFF[l], sum(CONV_CH[i][1] // 2 for i in layers)))
            l = e + 1
    return tuple(groups), tuple(group_of)


def build(shape, group_of, route, switches, diag_skip, frozen, train, fused_supported, bias_rows):
    """The plan of one walk.  shape = (B, H, W[, Kmax]); route: m per layer; frozen: names of the parameters that do not train;
    train=False: an evaluation forward (no backward: every backward field stays at its empty value);
    fused_supported(K, N, m, tiles) and bias_rows(B, h, w, C): ops.winograd_fused_supported / ops.winograd_bias_rows."""
    B, H, W = shape[:3]
    sw = switches
    fancy = not sw.plain      # commute_side, gather_side_grad, dual_transform, compact_masks, fuse_unpool: what ``plain`` switches off
    dims = layer_dims(H, W)
    commuted = [bool(fancy and sw.fuse_pool_fwd and sw.fuse_pool_bwd and group_of[l] is None) for l in range(13)]
    # the ReLU'd copy the next conv (forward and wgrad) reads: the pooled tensor where the layer is pooled (stored ReLU'd),
    # a second output of the conv kernel elsewhere; the last layer has no reader
    yr_wanted = [bool(not POOL_AFTER[l] and l < 12) for l in range(13)]
    relu_stored = all(yr_wanted[l] for l in range(12) if not POOL_AFTER[l])
    trainable = [not {f'backbone.{i}.weight', f'backbone.{i}.bias'} <= set(frozen) for i in CONV_IDX]
    lowest = min([l for l in range(13) if trainable[l]], default=13)

    fwd, src, relu_in = [], 'x0', False
    for l, (ci, co) in enumerate(CONV_CH):
        h, w = dims[l]
        m = route[l]
        # A Winograd-domain consumer reads its input once (input transform) and its weight gradient reads the kept V: then the
        # ReLU'd copy is not written at all and the transform applies the ReLU while loading y.
        write_yr = bool(yr_wanted[l] and not (l < 12 and route[l + 1] and (sw.wgrad_winograd or not train)))
        bits = codes = False
        if train and fancy and m == 4:
            t = tiles(B, h, w, 4)
            # sign bits of y_{l-1}: this layer's input transform reads it (pre-ReLU, not pooled) and this layer's input
            # gradient is the consumer (one-kernel route: product co -> ci)
            bits = bool(l >= 1 and src == 'y' and relu_in and fused_supported(co, ci, 4, t) == 2)
            # pooling codes of y_l: this layer's pooling epilogue writes them, the input gradient of layer l + 1 (through
            # the max-pool backward, one-kernel route) reads them
            codes = bool(POOL_AFTER[l] and l < 12 and not write_yr and fancy and route[l + 1] == 4
                         and fused_supported(ci, co, 4, t) >= 1
                         and fused_supported(CONV_CH[l + 1][1], CONV_CH[l + 1][0], 4, tiles(B, h // 2, w // 2, 4)) == 2)
        fwd.append(dict(
            ci=ci, co=co, h=h, w=w, m=m, pool=POOL_AFTER[l], group=group_of[l], commuted=commuted[l],
            side_in_conv=bool(sw.fuse_side_fwd and co <= 128 and not m and not commuted[l]),
            src=src, relu_in=relu_in, write_yr=write_yr, write_bits=bits, write_codes=codes, keep_v=bool(train and m),
            defer_side=bool(sw.two_streams and l < 12 and route[l + 1]), trainable=trainable[l]))
        if POOL_AFTER[l]:
            src, relu_in = 'yp', not relu_stored
        elif write_yr:
            src, relu_in = 'yr', False
        else:
            src, relu_in = 'y', True

    bwd = [dict(gather=False, dual=False, bias_rows=0, wgrad=None, wgrad_m=0, wgrad_late=False, dgrad=None, pool_bwd=False) for _ in range(13)]
    runs, late_at, late_side = [], None, ()
    if train:
        # native-resolution commuted layers whose G is written by the dgrad epilogue of the layer above (gather form)
        if fancy:
            for l in range(0, 12):
                ci1, co1 = CONV_CH[l + 1]
                bwd[l]['gather'] = bool(
                    group_of[l] is None and commuted[l] and dims[l] == (H, W) and l >= lowest and route[l + 1] == 4
                    and fused_supported(co1, ci1, 4, tiles(B, *dims[l + 1], 4)) == 2
                    and (not POOL_AFTER[l] or (fancy and H % 2 == 0 and W % 2 == 0)))
        for l in range(12, -1, -1):
            if group_of[l] is None and commuted[l] and l >= lowest:
                if runs and dims[runs[-1][0]] == dims[l] and len(runs[-1]) < 3:
                    runs[-1].append(l)
                else:
                    runs.append([l])
        # The side convs' own weight gradients are parameter gradients nobody waits for before the optimiser, while the
        # dgrad chain waits for every G_l: the grouped layers' ones are queued late, where the chain reaches late_at
        late_at = DEEP_SIDE_WGRAD_AT if sw.two_streams else None
        if late_at is not None and not (lowest < late_at <= 12):      # the main loop never reaches such a layer
            late_at = None
        late_side = tuple(l for l in range(12, -1, -1) if late_at is not None and group_of[l] is not None)
        for l in range(12, lowest - 1, -1):
            ci, co = CONV_CH[l]
            h, w = dims[l]
            m, r = route[l], bwd[l]
            # one pass over G_l for both consumers (F(4x4) input gradient and weight gradient)
            dual = r['dual'] = bool(fancy and m == 4 and l > lowest and trainable[l] and sw.wgrad_winograd
                                    and fwd[l]['keep_v'] and 'wgrad' not in diag_skip and bias_rows(B, h, w, co) > 0
                                    and not (POOL_AFTER[l - 1] and not fancy))
            r['bias_rows'] = bias_rows(B, h, w, co) if dual else 0
            if not trainable[l] or 'wgrad' in diag_skip:
                pass
            elif dual:
                r['wgrad'], r['wgrad_m'] = 'pre', 4
            # the forward's kept V decides; without one (direct forward) only the layers where a transform pass of its own still pays
            elif sw.wgrad_winograd and (m or (ci >= sw.wgrad_min_ci and co >= sw.wgrad_min_co)):
                r['wgrad'], r['wgrad_m'] = ('winograd_v' if m else 'winograd'), (m or sw.wgrad_tile)
            else:
                r['wgrad'] = 'direct'
            # With its operands ready (dual transform) a weight gradient can start any time.  Queued behind the layer's input
            # gradient instead of in front of it, its TN products run beside the NEXT layer's (memory-bound) transform rather
            # than beside this layer's products: 9.35 -> 9.20 ms.
            r['wgrad_late'] = bool(sw.two_streams and dual and l > lowest + WGRAD_EARLY_LAYERS)
            if l > lowest:
                unpooled = False
                if bwd[l - 1]['gather']:
                    r['dgrad'], unpooled = 'gather', True
                elif m:
                    if POOL_AFTER[l - 1] and fancy and m == 4:
                        r['dgrad'], unpooled = 'unpool', True
                    else:
                        r['dgrad'] = 'winograd'
                else:
                    r['dgrad'] = 'direct'
                r['pool_bwd'] = bool(POOL_AFTER[l - 1] and not unpooled)
    dp_on_load = [None] * 13
    if train and fancy and sw.unpool_on_load and 'dual' not in diag_skip:      # (--diag-skip dual takes the transform out, nothing else)
        dv = dv_elems(B, dims)
        for l in range(lowest + 1, 13):
            hu, wu = dims[l - 1]
            # the transform of G[l - 1] is the dual one, the forward left the pooling's codes, every pre-pool pixel sits in a window
            if not (POOL_AFTER[l - 1] and bwd[l - 1]['dual'] and fwd[l - 1]['write_codes'] and hu % 2 == 0 and wu % 2 == 0):
                continue
            if 4 * B * hu * wu * CONV_CH[l - 1][1] >= 1 << 32:       # (the kernel's 32-bit byte offsets)
                continue
            if bwd[l]['dgrad'] == 'gather':
                dp_on_load[l] = ('G', 0)
            elif bwd[l]['dgrad'] == 'unpool':
                # dP in the tail of dV: behind v_dy(l), which the input gradient reads while it writes dP, and behind
                # v_dy(l - 1), which the transform writes while it reads dP
                n = B * (hu // 2) * (wu // 2) * CONV_CH[l - 1][1]
                v_l = 36 * tiles(B, *dims[l], 4) * CONV_CH[l][1]
                v_below = 36 * tiles(B, hu, wu, 4) * CONV_CH[l - 1][1]
                if max(v_l, v_below) + n <= dv:
                    dp_on_load[l] = ('dV', dv - n)
    return StepPlan(shape=tuple(shape), route=tuple(route), train=bool(train),
                    layers=tuple(LayerPlan(**f, **r) for f, r in zip(fwd, bwd)),
                    lowest=lowest, relu_stored=relu_stored, runs=tuple(tuple(r) for r in runs), late_at=late_at,
                    late_side=late_side, shallow_first=bool(train and sw.two_streams and sw.fuse_pool_bwd),
                    fm=not sw.fuse_pool_fwd, dfm=bool(train and not sw.fuse_pool_bwd), dp_on_load=tuple(dp_on_load))


def buffers(plan, groups, Kmax, D, cls_part_bytes, C=2):
    """Every buffer the walk under ``plan`` reads or writes, as Buf records: what a set of that shape holds once it has been fitted
    to the plan (engine._fit), and so what it costs (``nbytes``).  groups: the set's Group records (groups_for); cls_part_bytes: the
    size of the classifier's partial-sum block, a number or a callable (rows, D) -> bytes (what ops.head_bwd_partials asks the
    library for).  C: classes of the classifier -- the width of sp_pred, and (through cls_part_bytes, which the engine forms for its
    C) of the partial-sum block; the loss gradient dpred (B, Kmax, C) is the step runner's, not the set's."""
    B, H, W = plan.shape[:3]
    R, Ls = B * Kmax, plan.layers
    out = []

    def add(name, layer, shape, dtype='float32', group=None):
        out.append(Buf(name, layer, tuple(int(n) for n in shape), dtype, group))

    def side(name, l, L, in_fm):
        # a side output / its gradient at native resolution: a slice of the group's buffer, a buffer of its own, or nothing at all
        # where the unfused path reads / writes the full-resolution layer's channel slice of fm / dfm itself
        if L.group is not None:
            add(name, l, (B, L.h, L.w, L.co // 2), group=L.group)
        elif not ((L.h, L.w) == (H, W) and in_fm):
            add(name, l, (B, L.h, L.w, L.co // 2))

    add('x0', None, (B, H, W, 4))
    for i, g in enumerate(groups):      # (in front of their layers' slices)
        add('g.s', i, (B, g.h, g.w, g.C))
        add('g.Wm', i, (B, Kmax, g.h * g.w))
        add('g.WmT', i, (B, g.h * g.w, Kmax))
    for l, L in enumerate(Ls):
        add('y', l, (B, L.h, L.w, L.co))
        if L.pool:
            add('yp', l, (B, L.h // 2, L.w // 2, L.co))
        if L.write_yr:
            add('yr', l, (B, L.h, L.w, L.co))
        if L.keep_v:
            add('V', l, ((L.m + 2) ** 2, tiles(B, L.h, L.w, L.m), L.ci))
        if L.write_bits:
            add('mbits', l - 1, (B, L.h, L.w, L.ci // 4), 'uint8')
        if L.write_codes:
            add('pcode', l, (B, L.h // 2, L.w // 2, L.co // 4), 'int16')
        if L.commuted:
            add('ybar', l, (B, Kmax, L.co))
        else:
            side('s', l, L, plan.fm)
    if plan.fm:
        add('fm', None, (B, H, W, FM_CHANNELS))
    add('sp_in', None, (B, Kmax, FM_CHANNELS))
    add('h1', None, (R, 1024))
    add('h2', None, (R, 1024))
    add('feats', None, (R, D))
    add('sp_pred', None, (R, C))
    add('pred', None, (B, H, W))
    if not plan.train:
        return tuple(out)
    for i, g in enumerate(groups):
        add('g.ds', i, (B, g.h, g.w, g.C))
    for l, L in enumerate(Ls):
        add('G', l, (B, L.h, L.w, L.co))
        # layer l + 1's input gradient at pooled resolution, in front of the max-pool backward launch: the 'gather' / 'unpool' forms
        # write G[l] themselves, and at or below the lowest trainable layer there is no input gradient
        if L.pool and Ls[l + 1].pool_bwd:
            add('dxp', l, (B, L.h // 2, L.w // 2, Ls[l + 1].ci))
        if not L.commuted:
            side('ds', l, L, plan.dfm)
        if L.dual:
            add('dM', l, (36, tiles(B, L.h, L.w, 4), L.co))
            add('bpart', l, (L.bias_rows, L.co))
    for l in (l for run in plan.runs for l in run):
        add('dybar', l, (B, Kmax, Ls[l].co))
    if any(L.dual for L in Ls):       # one V' = B^T dY B for all layers, the largest of them
        add('dV', None, (dv_elems(B, [(L.h, L.w) for L in Ls]),))
    if plan.dfm:
        add('dfm', None, (B, H, W, FM_CHANNELS))
    add('dfeat', None, (R, D))
    add('dh2', None, (R, 1024))
    add('dh1', None, (R, 1024))
    add('gsp', None, (B, Kmax, FM_CHANNELS))
    # (partial sums of the classifier's weight gradient between ops.head_bwd and ops.classifier_bwd_finish: the set's own block)
    add('cls_part', None, (max(int(cls_part_bytes(R, D) if callable(cls_part_bytes) else cls_part_bytes), 256),), 'uint8')
    return tuple(out)


def nbytes(bufs):
    """Device bytes of a buffer table; a slice of a group's buffer has no storage of its own."""
    total = 0
    for b in bufs:
        if b.group is None:
            n = ITEMSIZE[b.dtype]
            for d in b.shape:
                n *= d
            total += n
    return total
