"""wesup_amd.layer_plan on the CPU: the engine's whole decision table -- which layers are Winograd, commuted, grouped, gathered,
bit-masked, code-unpooled, dual-transformed, which weight- and input-gradient form each takes and what is queued late -- as data.

The expected tables below were NOT produced by layer_plan: they were recorded on an MI355X from the commit before the plan
existed, by walking one training step and one evaluation forward per configuration with every ops.* call of the walk logged (which
call, which buffers by name, which keyword arguments) and the buffer set's own decision state read afterwards (x_in, x_relu,
mbits_ok, pcode_ok, wino_fwd, s_valid, group_of), the two agreeing.  One row per layer:

    m<tile> g<group|-> <C: side conv commuted><S: side conv in the conv epilogue> <input>[+relu] <y: ReLU'd copy written><b: sign
    bits written><c: pooling codes written><v: V kept><d: side work deferred>
    | <T: trainable><G: side gradient gathered by the layer above><D: dual transform>:<bias rows> w=<weight-gradient form><m><L:
    queued late> d=<input-gradient form>[+pool: a max-pool backward launch follows]

The library's two queries (one-kernel route, bias rows) are host functions: the built library answers them without a GPU."""
import os
import subprocess
import sys

import pytest

from wesup_amd import layer_plan as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKBONE = lambda upto: {f'backbone.{i}.{t}' for i in lp.CONV_IDX[:upto] for t in ('weight', 'bias')}
# name: (B, H, W, Kmax, switches, (WINOGRAD_TILE, WINOGRAD_CONV_MIN_CI) of the default routing rule, frozen parameters)
CONFIGS = {
    'c01_default': (4, 480, 480, 576, {}, (4, 64), set()),
    'c02_plain': (4, 480, 480, 576, dict(plain=True), (4, 64), set()),
    'c03_plain_unfused': (4, 480, 480, 576, dict(plain=True, fuse_pool_fwd=False, fuse_pool_bwd=False), (4, 64), set()),
    'c04_direct': (4, 480, 480, 576, dict(conv_winograd=False, wgrad_winograd=False), (4, 64), set()),
    'c05_one_stream': (4, 480, 480, 576, dict(two_streams=False), (4, 64), set()),
    'c07a_frozen_to_conv3_3': (4, 480, 480, 576, {}, (4, 64), BACKBONE(7)),
    'c07b_frozen_all': (4, 480, 480, 576, {}, (4, 64), BACKBONE(13)),
    'c08_odd_96x80': (1, 96, 80, 52, {}, (4, 64), set()),
    'c09_8x1024': (8, 1024, 1024, 3072, {}, (4, 64), set()),
    'c09b_1x1024': (1, 1024, 1024, 3072, {}, (4, 64), set()),
    'c10_f2_min128': (4, 480, 480, 576, dict(wgrad_tile=2), (2, 128), set()),
}

# ---- recorded from the commit before layer_plan existed (see the module docstring); 'shallow_evidence': side-gradient work was
# seen at the head of the weight-gradient stream
PARENT = {'c01_default': {'groups': [((7, 8, 9), 60, 60, 576, 768), ((10, 11, 12), 30, 30, 1344, 768)],
                 'group_of': [None, None, None, None, None, None, None, 0, 0, 0, 1, 1, 1],
                 'train': ['m0 g- C. x0 ....d | TG.:0 w=direct0. d=-',
                           'm4 g- C. y+relu .bcvd | TGD:3600 w=pre4. d=gather',
                           'm4 g- C. yp ...vd | T.D:1800 w=pre4L d=gather',
                           'm4 g- C. y+relu .bcvd | T.D:1800 w=pre4L d=winograd',
                           'm4 g- C. yp ...vd | T.D:900 w=pre4L d=unpool',
                           'm4 g- C. y+relu .b.vd | T.D:900 w=pre4L d=winograd',
                           'm4 g- C. y+relu .b.vd | T.D:900 w=pre4L d=winograd',
                           'm4 g0 .. yp ...vd | T.D:450 w=pre4L d=unpool',
                           'm4 g0 .. y+relu ...vd | T.D:450 w=pre4L d=winograd',
                           'm4 g0 .. y+relu ...vd | T.D:450 w=pre4L d=winograd',
                           'm4 g1 .. yp ...vd | T.D:128 w=pre4L d=unpool',
                           'm4 g1 .. y+relu ...vd | T.D:128 w=pre4L d=winograd',
                           'm4 g1 .. y+relu ...v. | T.D:128 w=pre4L d=winograd'],
                 'step': {'lowest': 0,
                          'runs': ((6, 5, 4), (3, 2), (1, 0)),
                          'late_at': 2,
                          'late_side': (12, 11, 10, 9, 8, 7),
                          'shallow_evidence': True,
                          'relu_stored': True},
                 'eval': ['m0 g- C. x0 ....d',
                          'm4 g- C. y+relu ....d',
                          'm4 g- C. yp ....d',
                          'm4 g- C. y+relu ....d',
                          'm4 g- C. yp ....d',
                          'm4 g- C. y+relu ....d',
                          'm4 g- C. y+relu ....d',
                          'm4 g0 .. yp ....d',
                          'm4 g0 .. y+relu ....d',
                          'm4 g0 .. y+relu ....d',
                          'm4 g1 .. yp ....d',
                          'm4 g1 .. y+relu ....d',
                          'm4 g1 .. y+relu .....']},
 'c02_plain': {'groups': [((7, 8, 9), 60, 60, 576, 768), ((10, 11, 12), 30, 30, 1344, 768)],
               'group_of': [None, None, None, None, None, None, None, 0, 0, 0, 1, 1, 1],
               'train': ['m0 g- .S x0 ....d | T..:0 w=direct0. d=-',
                         'm4 g- .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                         'm4 g- .. yp ...vd | T..:0 w=winograd_v4. d=winograd+pool',
                         'm4 g- .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                         'm4 g- .. yp ...vd | T..:0 w=winograd_v4. d=winograd+pool',
                         'm4 g- .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                         'm4 g- .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                         'm4 g0 .. yp ...vd | T..:0 w=winograd_v4. d=winograd+pool',
                         'm4 g0 .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                         'm4 g0 .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                         'm4 g1 .. yp ...vd | T..:0 w=winograd_v4. d=winograd+pool',
                         'm4 g1 .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                         'm4 g1 .. y+relu ...v. | T..:0 w=winograd_v4. d=winograd'],
               'step': {'lowest': 0, 'runs': (), 'late_at': 2, 'late_side': (12, 11, 10, 9, 8, 7), 'shallow_evidence': True, 'relu_stored': True},
               'eval': ['m0 g- .S x0 ....d',
                        'm4 g- .. y+relu ....d',
                        'm4 g- .. yp ....d',
                        'm4 g- .. y+relu ....d',
                        'm4 g- .. yp ....d',
                        'm4 g- .. y+relu ....d',
                        'm4 g- .. y+relu ....d',
                        'm4 g0 .. yp ....d',
                        'm4 g0 .. y+relu ....d',
                        'm4 g0 .. y+relu ....d',
                        'm4 g1 .. yp ....d',
                        'm4 g1 .. y+relu ....d',
                        'm4 g1 .. y+relu .....']},
 'c03_plain_unfused': {'groups': [],
                       'group_of': [None, None, None, None, None, None, None, None, None, None, None, None, None],
                       'train': ['m0 g- .S x0 ....d | T..:0 w=direct0. d=-',
                                 'm4 g- .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                                 'm4 g- .. yp ...vd | T..:0 w=winograd_v4. d=winograd+pool',
                                 'm4 g- .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                                 'm4 g- .. yp ...vd | T..:0 w=winograd_v4. d=winograd+pool',
                                 'm4 g- .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                                 'm4 g- .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                                 'm4 g- .. yp ...vd | T..:0 w=winograd_v4. d=winograd+pool',
                                 'm4 g- .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                                 'm4 g- .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                                 'm4 g- .. yp ...vd | T..:0 w=winograd_v4. d=winograd+pool',
                                 'm4 g- .. y+relu ...vd | T..:0 w=winograd_v4. d=winograd',
                                 'm4 g- .. y+relu ...v. | T..:0 w=winograd_v4. d=winograd'],
                       'step': {'lowest': 0, 'runs': (), 'late_at': None, 'late_side': (), 'shallow_evidence': False, 'relu_stored': True},
                       'eval': ['m0 g- .S x0 ....d',
                                'm4 g- .. y+relu ....d',
                                'm4 g- .. yp ....d',
                                'm4 g- .. y+relu ....d',
                                'm4 g- .. yp ....d',
                                'm4 g- .. y+relu ....d',
                                'm4 g- .. y+relu ....d',
                                'm4 g- .. yp ....d',
                                'm4 g- .. y+relu ....d',
                                'm4 g- .. y+relu ....d',
                                'm4 g- .. yp ....d',
                                'm4 g- .. y+relu ....d',
                                'm4 g- .. y+relu .....']},
 'c04_direct': {'groups': [((7, 8, 9), 60, 60, 576, 768), ((10, 11, 12), 30, 30, 1344, 768)],
                'group_of': [None, None, None, None, None, None, None, 0, 0, 0, 1, 1, 1],
                'train': ['m0 g- C. x0 y.... | T..:0 w=direct0. d=-',
                          'm0 g- C. yr ..... | T..:0 w=direct0. d=direct',
                          'm0 g- C. yp y.... | T..:0 w=direct0. d=direct+pool',
                          'm0 g- C. yr ..... | T..:0 w=direct0. d=direct',
                          'm0 g- C. yp y.... | T..:0 w=direct0. d=direct+pool',
                          'm0 g- C. yr y.... | T..:0 w=direct0. d=direct',
                          'm0 g- C. yr ..... | T..:0 w=direct0. d=direct',
                          'm0 g0 .. yp y.... | T..:0 w=direct0. d=direct+pool',
                          'm0 g0 .. yr y.... | T..:0 w=direct0. d=direct',
                          'm0 g0 .. yr ..... | T..:0 w=direct0. d=direct',
                          'm0 g1 .. yp y.... | T..:0 w=direct0. d=direct+pool',
                          'm0 g1 .. yr y.... | T..:0 w=direct0. d=direct',
                          'm0 g1 .. yr ..... | T..:0 w=direct0. d=direct'],
                'step': {'lowest': 0,
                         'runs': ((6, 5, 4), (3, 2), (1, 0)),
                         'late_at': 2,
                         'late_side': (12, 11, 10, 9, 8, 7),
                         'shallow_evidence': True,
                         'relu_stored': True},
                'eval': ['m0 g- C. x0 y....',
                         'm0 g- C. yr .....',
                         'm0 g- C. yp y....',
                         'm0 g- C. yr .....',
                         'm0 g- C. yp y....',
                         'm0 g- C. yr y....',
                         'm0 g- C. yr .....',
                         'm0 g0 .. yp y....',
                         'm0 g0 .. yr y....',
                         'm0 g0 .. yr .....',
                         'm0 g1 .. yp y....',
                         'm0 g1 .. yr y....',
                         'm0 g1 .. yr .....']},
 'c05_one_stream': {'groups': [((7, 8, 9), 60, 60, 576, 768), ((10, 11, 12), 30, 30, 1344, 768)],
                    'group_of': [None, None, None, None, None, None, None, 0, 0, 0, 1, 1, 1],
                    'train': ['m0 g- C. x0 ..... | TG.:0 w=direct0. d=-',
                              'm4 g- C. y+relu .bcv. | TGD:3600 w=pre4. d=gather',
                              'm4 g- C. yp ...v. | T.D:1800 w=pre4. d=gather',
                              'm4 g- C. y+relu .bcv. | T.D:1800 w=pre4. d=winograd',
                              'm4 g- C. yp ...v. | T.D:900 w=pre4. d=unpool',
                              'm4 g- C. y+relu .b.v. | T.D:900 w=pre4. d=winograd',
                              'm4 g- C. y+relu .b.v. | T.D:900 w=pre4. d=winograd',
                              'm4 g0 .. yp ...v. | T.D:450 w=pre4. d=unpool',
                              'm4 g0 .. y+relu ...v. | T.D:450 w=pre4. d=winograd',
                              'm4 g0 .. y+relu ...v. | T.D:450 w=pre4. d=winograd',
                              'm4 g1 .. yp ...v. | T.D:128 w=pre4. d=unpool',
                              'm4 g1 .. y+relu ...v. | T.D:128 w=pre4. d=winograd',
                              'm4 g1 .. y+relu ...v. | T.D:128 w=pre4. d=winograd'],
                    'step': {'lowest': 0,
                             'runs': ((6, 5, 4), (3, 2), (1, 0)),
                             'late_at': None,
                             'late_side': (),
                             'shallow_evidence': False,
                             'relu_stored': True},
                    'eval': ['m0 g- C. x0 .....',
                             'm4 g- C. y+relu .....',
                             'm4 g- C. yp .....',
                             'm4 g- C. y+relu .....',
                             'm4 g- C. yp .....',
                             'm4 g- C. y+relu .....',
                             'm4 g- C. y+relu .....',
                             'm4 g0 .. yp .....',
                             'm4 g0 .. y+relu .....',
                             'm4 g0 .. y+relu .....',
                             'm4 g1 .. yp .....',
                             'm4 g1 .. y+relu .....',
                             'm4 g1 .. y+relu .....']},
 'c07a_frozen_to_conv3_3': {'groups': [((7, 8, 9), 60, 60, 576, 768), ((10, 11, 12), 30, 30, 1344, 768)],
                            'group_of': [None, None, None, None, None, None, None, 0, 0, 0, 1, 1, 1],
                            'train': ['m0 g- C. x0 ....d | ...:0 w=-0. d=-',
                                      'm4 g- C. y+relu .bcvd | ...:0 w=-0. d=-',
                                      'm4 g- C. yp ...vd | ...:0 w=-0. d=-',
                                      'm4 g- C. y+relu .bcvd | ...:0 w=-0. d=-',
                                      'm4 g- C. yp ...vd | ...:0 w=-0. d=-',
                                      'm4 g- C. y+relu .b.vd | ...:0 w=-0. d=-',
                                      'm4 g- C. y+relu .b.vd | ...:0 w=-0. d=-',
                                      'm4 g0 .. yp ...vd | T..:0 w=winograd_v4. d=-',
                                      'm4 g0 .. y+relu ...vd | T.D:450 w=pre4. d=winograd',
                                      'm4 g0 .. y+relu ...vd | T.D:450 w=pre4L d=winograd',
                                      'm4 g1 .. yp ...vd | T.D:128 w=pre4L d=unpool',
                                      'm4 g1 .. y+relu ...vd | T.D:128 w=pre4L d=winograd',
                                      'm4 g1 .. y+relu ...v. | T.D:128 w=pre4L d=winograd'],
                            'step': {'lowest': 7, 'runs': (), 'late_at': None, 'late_side': (), 'shallow_evidence': False, 'relu_stored': True},
                            'eval': ['m0 g- C. x0 ....d',
                                     'm4 g- C. y+relu ....d',
                                     'm4 g- C. yp ....d',
                                     'm4 g- C. y+relu ....d',
                                     'm4 g- C. yp ....d',
                                     'm4 g- C. y+relu ....d',
                                     'm4 g- C. y+relu ....d',
                                     'm4 g0 .. yp ....d',
                                     'm4 g0 .. y+relu ....d',
                                     'm4 g0 .. y+relu ....d',
                                     'm4 g1 .. yp ....d',
                                     'm4 g1 .. y+relu ....d',
                                     'm4 g1 .. y+relu .....']},
 'c07b_frozen_all': {'groups': [((7, 8, 9), 60, 60, 576, 768), ((10, 11, 12), 30, 30, 1344, 768)],
                     'group_of': [None, None, None, None, None, None, None, 0, 0, 0, 1, 1, 1],
                     'train': ['m0 g- C. x0 ....d | ...:0 w=-0. d=-',
                               'm4 g- C. y+relu .bcvd | ...:0 w=-0. d=-',
                               'm4 g- C. yp ...vd | ...:0 w=-0. d=-',
                               'm4 g- C. y+relu .bcvd | ...:0 w=-0. d=-',
                               'm4 g- C. yp ...vd | ...:0 w=-0. d=-',
                               'm4 g- C. y+relu .b.vd | ...:0 w=-0. d=-',
                               'm4 g- C. y+relu .b.vd | ...:0 w=-0. d=-',
                               'm4 g0 .. yp ...vd | ...:0 w=-0. d=-',
                               'm4 g0 .. y+relu ...vd | ...:0 w=-0. d=-',
                               'm4 g0 .. y+relu ...vd | ...:0 w=-0. d=-',
                               'm4 g1 .. yp ...vd | ...:0 w=-0. d=-',
                               'm4 g1 .. y+relu ...vd | ...:0 w=-0. d=-',
                               'm4 g1 .. y+relu ...v. | ...:0 w=-0. d=-'],
                     'step': {'lowest': 13, 'runs': (), 'late_at': None, 'late_side': (), 'shallow_evidence': False, 'relu_stored': True},
                     'eval': ['m0 g- C. x0 ....d',
                              'm4 g- C. y+relu ....d',
                              'm4 g- C. yp ....d',
                              'm4 g- C. y+relu ....d',
                              'm4 g- C. yp ....d',
                              'm4 g- C. y+relu ....d',
                              'm4 g- C. y+relu ....d',
                              'm4 g0 .. yp ....d',
                              'm4 g0 .. y+relu ....d',
                              'm4 g0 .. y+relu ....d',
                              'm4 g1 .. yp ....d',
                              'm4 g1 .. y+relu ....d',
                              'm4 g1 .. y+relu .....']},
 'c08_odd_96x80': {'groups': [((2, 3), 48, 40, 64, 128), ((4, 5, 6), 24, 20, 192, 384), ((7, 8, 9), 12, 10, 576, 768)],
                   'group_of': [None, None, 0, 0, 1, 1, 1, 2, 2, 2, None, None, None],
                   'train': ['m0 g- C. x0 ....d | T..:0 w=direct0. d=-',
                             'm4 g- C. y+relu ...vd | T.D:30 w=pre4. d=winograd',
                             'm4 g0 .. yp ...vd | T.D:15 w=pre4L d=unpool',
                             'm4 g0 .. y+relu ...vd | T.D:15 w=pre4L d=winograd',
                             'm4 g1 .. yp ...vd | T.D:8 w=pre4L d=unpool',
                             'm4 g1 .. y+relu ...vd | T.D:8 w=pre4L d=winograd',
                             'm4 g1 .. y+relu ...vd | T.D:8 w=pre4L d=winograd',
                             'm4 g2 .. yp ...vd | T.D:5 w=pre4L d=unpool',
                             'm4 g2 .. y+relu ...vd | T.D:5 w=pre4L d=winograd',
                             'm4 g2 .. y+relu ...vd | T.D:5 w=pre4L d=winograd',
                             'm4 g- C. yp ...vd | T.D:2 w=pre4L d=unpool',
                             'm4 g- C. y+relu ...vd | T.D:2 w=pre4L d=winograd',
                             'm4 g- C. y+relu ...v. | T.D:2 w=pre4L d=winograd'],
                   'step': {'lowest': 0,
                            'runs': ((12, 11, 10), (1, 0)),
                            'late_at': 2,
                            'late_side': (9, 8, 7, 6, 5, 4, 3, 2),
                            'shallow_evidence': True,
                            'relu_stored': True},
                   'eval': ['m0 g- C. x0 ....d',
                            'm4 g- C. y+relu ....d',
                            'm4 g0 .. yp ....d',
                            'm4 g0 .. y+relu ....d',
                            'm4 g1 .. yp ....d',
                            'm4 g1 .. y+relu ....d',
                            'm4 g1 .. y+relu ....d',
                            'm4 g2 .. yp ....d',
                            'm4 g2 .. y+relu ....d',
                            'm4 g2 .. y+relu ....d',
                            'm4 g- C. yp ....d',
                            'm4 g- C. y+relu ....d',
                            'm4 g- C. y+relu .....']},
 'c09_8x1024': {'groups': [],
                'group_of': [None, None, None, None, None, None, None, None, None, None, None, None, None],
                'train': ['m0 g- C. x0 ....d | TG.:0 w=direct0. d=-',
                          'm4 g- C. y+relu .bcvd | TGD:32768 w=pre4. d=gather',
                          'm4 g- C. yp ...vd | T.D:16384 w=pre4L d=gather',
                          'm4 g- C. y+relu .bcvd | T.D:16384 w=pre4L d=winograd',
                          'm4 g- C. yp ...vd | T.D:8192 w=pre4L d=unpool',
                          'm4 g- C. y+relu .b.vd | T.D:8192 w=pre4L d=winograd',
                          'm4 g- C. y+relu .b.vd | T.D:8192 w=pre4L d=winograd',
                          'm4 g- C. yp ...vd | T.D:4096 w=pre4L d=unpool',
                          'm4 g- C. y+relu ...vd | T.D:4096 w=pre4L d=winograd',
                          'm4 g- C. y+relu ...vd | T.D:4096 w=pre4L d=winograd',
                          'm4 g- C. yp ...vd | T.D:1024 w=pre4L d=unpool',
                          'm4 g- C. y+relu ...vd | T.D:1024 w=pre4L d=winograd',
                          'm4 g- C. y+relu ...v. | T.D:1024 w=pre4L d=winograd'],
                'step': {'lowest': 0,
                         'runs': ((12, 11, 10), (9, 8, 7), (6, 5, 4), (3, 2), (1, 0)),
                         'late_at': None,
                         'late_side': (),
                         'shallow_evidence': True,
                         'relu_stored': True},
                'eval': ['m0 g- C. x0 ....d',
                         'm4 g- C. y+relu ....d',
                         'm4 g- C. yp ....d',
                         'm4 g- C. y+relu ....d',
                         'm4 g- C. yp ....d',
                         'm4 g- C. y+relu ....d',
                         'm4 g- C. y+relu ....d',
                         'm4 g- C. yp ....d',
                         'm4 g- C. y+relu ....d',
                         'm4 g- C. y+relu ....d',
                         'm4 g- C. yp ....d',
                         'm4 g- C. y+relu ....d',
                         'm4 g- C. y+relu .....']},
 'c09b_1x1024': {'groups': [],
                 'group_of': [None, None, None, None, None, None, None, None, None, None, None, None, None],
                 'train': ['m0 g- C. x0 ....d | TG.:0 w=direct0. d=-',
                           'm4 g- C. y+relu .bcvd | TGD:4096 w=pre4. d=gather',
                           'm4 g- C. yp ...vd | T.D:2048 w=pre4L d=gather',
                           'm4 g- C. y+relu .bcvd | T.D:2048 w=pre4L d=winograd',
                           'm4 g- C. yp ...vd | T.D:1024 w=pre4L d=unpool',
                           'm4 g- C. y+relu .b.vd | T.D:1024 w=pre4L d=winograd',
                           'm4 g- C. y+relu .b.vd | T.D:1024 w=pre4L d=winograd',
                           'm4 g- C. yp ...vd | T.D:512 w=pre4L d=unpool',
                           'm4 g- C. y+relu ...vd | T.D:512 w=pre4L d=winograd',
                           'm4 g- C. y+relu ...vd | T.D:512 w=pre4L d=winograd',
                           'm4 g- C. yp ...vd | T.D:128 w=pre4L d=unpool',
                           'm4 g- C. y+relu ...vd | T.D:128 w=pre4L d=winograd',
                           'm4 g- C. y+relu ...v. | T.D:128 w=pre4L d=winograd'],
                 'step': {'lowest': 0,
                          'runs': ((12, 11, 10), (9, 8, 7), (6, 5, 4), (3, 2), (1, 0)),
                          'late_at': None,
                          'late_side': (),
                          'shallow_evidence': True,
                          'relu_stored': True},
                 'eval': ['m0 g- C. x0 ....d',
                          'm4 g- C. y+relu ....d',
                          'm4 g- C. yp ....d',
                          'm4 g- C. y+relu ....d',
                          'm4 g- C. yp ....d',
                          'm4 g- C. y+relu ....d',
                          'm4 g- C. y+relu ....d',
                          'm4 g- C. yp ....d',
                          'm4 g- C. y+relu ....d',
                          'm4 g- C. y+relu ....d',
                          'm4 g- C. yp ....d',
                          'm4 g- C. y+relu ....d',
                          'm4 g- C. y+relu .....']},
 'c10_f2_min128': {'groups': [((7, 8, 9), 60, 60, 576, 768), ((10, 11, 12), 30, 30, 1344, 768)],
                   'group_of': [None, None, None, None, None, None, None, 0, 0, 0, 1, 1, 1],
                   'train': ['m0 g- C. x0 y.... | T..:0 w=direct0. d=-',
                             'm0 g- C. yr ..... | T..:0 w=direct0. d=direct',
                             'm0 g- C. yp ....d | T..:0 w=direct0. d=direct+pool',
                             'm2 g- C. y+relu ...vd | T..:0 w=winograd_v2. d=winograd',
                             'm2 g- C. yp ...vd | T..:0 w=winograd_v2. d=winograd+pool',
                             'm2 g- C. y+relu ...vd | T..:0 w=winograd_v2. d=winograd',
                             'm2 g- C. y+relu ...vd | T..:0 w=winograd_v2. d=winograd',
                             'm2 g0 .. yp ...vd | T..:0 w=winograd_v2. d=winograd+pool',
                             'm2 g0 .. y+relu ...vd | T..:0 w=winograd_v2. d=winograd',
                             'm2 g0 .. y+relu ...vd | T..:0 w=winograd_v2. d=winograd',
                             'm2 g1 .. yp ...vd | T..:0 w=winograd_v2. d=winograd+pool',
                             'm2 g1 .. y+relu ...vd | T..:0 w=winograd_v2. d=winograd',
                             'm2 g1 .. y+relu ...v. | T..:0 w=winograd_v2. d=winograd'],
                   'step': {'lowest': 0,
                            'runs': ((6, 5, 4), (3, 2), (1, 0)),
                            'late_at': 2,
                            'late_side': (12, 11, 10, 9, 8, 7),
                            'shallow_evidence': True,
                            'relu_stored': True},
                   'eval': ['m0 g- C. x0 y....',
                            'm0 g- C. yr .....',
                            'm0 g- C. yp ....d',
                            'm2 g- C. y+relu ....d',
                            'm2 g- C. yp ....d',
                            'm2 g- C. y+relu ....d',
                            'm2 g- C. y+relu ....d',
                            'm2 g0 .. yp ....d',
                            'm2 g0 .. y+relu ....d',
                            'm2 g0 .. y+relu ....d',
                            'm2 g1 .. yp ....d',
                            'm2 g1 .. y+relu ....d',
                            'm2 g1 .. y+relu .....']}}


def default_rule(tile, min_ci):
    """engine.default_route with the two class attributes it reads given."""
    return lambda ci, co, h, w, B: 0 if ci < min_ci else tile


@pytest.fixture(scope='module')
def queries():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    return (lambda K, N, m=4, tiles=0: int(lib.wesup_winograd_fused_route(K, N, m, int(tiles))),
            lambda B, H, W, C: int(lib.wesup_winograd_bias_rows(B, H, W, C)))


def row(L, backward):
    s = 'm%d g%s %s%s %s%s %s%s%s%s%s' % (L.m, '-' if L.group is None else L.group, 'C' if L.commuted else '.',
                                          'S' if L.side_in_conv else '.', L.src, '+relu' if L.relu_in else '',
                                          'y' if L.write_yr else '.', 'b' if L.write_bits else '.', 'c' if L.write_codes else '.',
                                          'v' if L.keep_v else '.', 'd' if L.defer_side else '.')
    if backward:
        s += ' | %s%s%s:%d w=%s%d%s d=%s%s' % ('T' if L.trainable else '.', 'G' if L.gather else '.', 'D' if L.dual else '.',
                                              L.bias_rows, L.wgrad or '-', L.wgrad_m, 'L' if L.wgrad_late else '.',
                                              L.dgrad or '-', '+pool' if L.pool_bwd else '')
    return s


def plans_of(name, queries):
    B, H, W, Kmax, sw, (tile, min_ci), frozen = CONFIGS[name]
    sw = lp.Switches(**sw)
    groups, group_of = lp.groups_for(B, H, W, Kmax, sw)
    route = lp.route(default_rule(tile, min_ci), sw.conv_winograd, B, H, W)
    return groups, group_of, [lp.build((B, H, W), group_of, route, sw, set(), frozen, train, *queries) for train in (True, False)]


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_plan_equals_what_the_engine_did_before_there_was_a_plan(name, queries):
    want = PARENT[name]
    groups, group_of, (tr, ev) = plans_of(name, queries)
    assert [tuple(g) for g in groups] == want['groups'] and list(group_of) == want['group_of']
    assert [row(L, True) for L in tr.layers] == want['train']
    assert [row(L, False) for L in ev.layers] == want['eval']
    step = want['step']
    # (where nothing is queued late, the position it would be queued at was not observable)
    assert (tr.lowest, tr.runs, tr.late_at if tr.late_side else None, tr.late_side, tr.relu_stored) == \
        (step['lowest'], step['runs'], step['late_at'], step['late_side'], step['relu_stored'])
    if step['shallow_evidence']:        # (work seen at the head of the weight-gradient stream)
        assert tr.shallow_first
    # an evaluation plan has no backward
    assert not ev.train and ev.runs == () and ev.late_side == () and not ev.shallow_first
    assert all(L.wgrad is None and L.dgrad is None and not (L.dual or L.gather or L.keep_v or L.write_bits or L.write_codes)
               for L in ev.layers)
    # what the records say about each other
    for l, L in enumerate(tr.layers):
        assert (L.ci, L.co) == lp.CONV_CH[l] and L.pool == lp.POOL_AFTER[l] and L.m == tr.route[l]
        assert not (L.commuted and L.group is not None) and not (L.side_in_conv and (L.commuted or L.m))
        assert L.dgrad is None or (l > tr.lowest and (L.dgrad == 'gather') == tr.layers[l - 1].gather)
        assert (L.wgrad == 'pre') == L.dual and (L.bias_rows > 0) == L.dual and not (L.wgrad_late and not L.dual)
    assert all(len(r) <= 3 and len({tr.layers[l].h for l in r}) == 1 for r in tr.runs)


def test_the_1024_shape_leaves_the_matrix_form_for_conv5(queries):
    groups, group_of, _ = plans_of('c09_8x1024', queries)
    assert list(group_of[10:]) == [None] * 3 and all(g.h * g.w <= 4096 and 3072 * g.h * g.w <= (4 << 20) for g in groups)
    # Kmax that is not a multiple of 4, or a cell count that is not: no matrix form at all / for that resolution
    assert lp.groups_for(4, 480, 480, 578, lp.Switches()) == ((), (None,) * 13)
    assert lp.groups_for(1, 96, 80, 52, lp.Switches())[1] == tuple(PARENT['c08_odd_96x80']['group_of'])
    assert lp.groups_for(4, 480, 480, 576, lp.Switches(matrix_pool=False)) == ((), (None,) * 13)


def test_tiles_and_constants_are_the_engines():
    from wesup_amd import engine, ops
    assert (engine.CONV_CH, engine.CONV_IDX, engine.POOL_AFTER, engine.SIDE_OFF) == (lp.CONV_CH, lp.CONV_IDX, lp.POOL_AFTER, lp.SIDE_OFF)
    for B, H, W in ((4, 480, 480), (1, 96, 80), (3, 37, 51)):
        for m in (2, 4):
            assert lp.tiles(B, H, W, m) == ops.winograd_tiles(B, H, W, m)
    e = engine.WesupEngine
    assert lp.Switches() == lp.Switches(True, True, True, True, True, False, e.matrix_pool, e.fuse_side_fwd, e.WINOGRAD_MIN_CI,
                                        e.WINOGRAD_MIN_CO, e.WINOGRAD_TILE)


def test_the_engine_rebuilds_its_plan_when_its_key_changes_and_only_then(queries):
    import torch
    from wesup_amd import engine
    eng = engine.WesupEngine({'w': torch.zeros(4)}, {'w': torch.zeros(4)})
    b = engine._Bufs()
    b.shape, b.plans = (4, 480, 480), {}
    b.group_of = list(lp.groups_for(4, 480, 480, 576, eng._switches())[1])
    p0 = eng._plan(b, True)
    assert eng._plan(b, True) is p0 and eng._plan(b, True, p0.route) is p0
    assert [row(L, True) for L in p0.layers] == PARENT['c01_default']['train']
    ev = eng._plan(b, False)
    assert ev is not p0 and eng._plan(b, False) is ev and eng._plan(b, True) is p0        # one plan per kind of walk
    assert [row(L, False) for L in ev.layers] == PARENT['c01_default']['eval']
    for change, undo in (
            (lambda: setattr(eng, 'plain', True), lambda: setattr(eng, 'plain', False)),
            (lambda: setattr(eng, 'two_streams', False), lambda: setattr(eng, 'two_streams', True)),
            (lambda: setattr(eng, 'wgrad_winograd', False), lambda: setattr(eng, 'wgrad_winograd', True)),
            (lambda: setattr(eng, 'conv_winograd', False), lambda: setattr(eng, 'conv_winograd', True)),
            (lambda: setattr(eng, 'fuse_pool_fwd', False), lambda: setattr(eng, 'fuse_pool_fwd', True)),
            (lambda: setattr(eng, 'fuse_pool_bwd', False), lambda: setattr(eng, 'fuse_pool_bwd', True)),
            (lambda: setattr(eng, 'fuse_side_fwd', False), lambda: delattr(eng, 'fuse_side_fwd')),
            (lambda: setattr(eng, 'matrix_pool', False), lambda: delattr(eng, 'matrix_pool')),
            (lambda: eng.frozen.update(BACKBONE(3)), lambda: eng.frozen.clear()),
            (lambda: eng._diag_skip.add('wgrad'), lambda: eng._diag_skip.clear()),
            (lambda: setattr(eng, 'route_fn', default_rule(2, 128)), lambda: setattr(eng, 'route_fn', engine.default_route))):
        before = eng._plan(b, True)
        key = eng.plan_key(4, 480, 480)
        change()
        assert eng.plan_key(4, 480, 480) != key
        after = eng._plan(b, True)
        assert after is not before and eng._plan(b, True) is after
        undo()
        assert eng.plan_key(4, 480, 480) == key
    eng.plain = True
    assert [row(L, True) for L in eng._plan(b, True).layers] == PARENT['c02_plain']['train']
    eng.plain = False
    eng.on_tail = eng.on_grads_ready = lambda *a: None          # not part of the key: callbacks do not shape the plan
    eng.max_cached_shapes = 3
    p1 = eng._plan(b, True)
    assert eng._plan(b, True) is p1 and p1 == p0


def test_layer_plan_imports_without_torch():
    code = ('import sys; import wesup_amd.layer_plan as lp; assert "torch" not in sys.modules, "torch imported"; '
            'lp.build((1, 32, 32), lp.groups_for(1, 32, 32, 16, lp.Switches())[1], (0,) + (4,) * 12, lp.Switches(), set(), set(), True, '
            'lambda *a: 0, lambda *a: 0); assert "torch" not in sys.modules; '
            'sw = lp.Switches(); gr, go = lp.groups_for(1, 32, 32, 16, sw); '
            'pl = lp.build((1, 32, 32), go, (0,) + (4,) * 12, sw, set(), set(), True, lambda *a: 2, lambda *a: 3); '
            't = lp.buffers(pl, gr, 16, 32, lambda R, D: 4096); assert lp.nbytes(t) > lp.nbytes(lp.buffers(pl, gr, 16, 32, 0)) > 0; '
            'assert {e.name for e in t} >= {"x0", "y", "V", "G", "dV", "dM", "cls_part", "g.Wm"}; assert "torch" not in sys.modules')
    subprocess.run([sys.executable, '-c', code], cwd=ROOT, check=True, timeout=120)


def table_bytes(B, H, W, Kmax, train=True):
    """What a new set of that shape costs under the default switches, from layer_plan alone (the library answers its size queries
    on the CPU)."""
    from wesup_amd import _lib
    lib = _lib.load()
    sw = lp.Switches()
    groups, group_of = lp.groups_for(B, H, W, Kmax, sw)
    plan = lp.build((B, H, W), group_of, lp.route(default_rule(4, 64), True, B, H, W), sw, set(), set(), train,
                    lambda K, N, m=4, tiles=0: int(lib.wesup_winograd_fused_route(K, N, m, int(tiles))),
                    lambda *a: int(lib.wesup_winograd_bias_rows(*a)))
    return lp.nbytes(lp.buffers(plan, groups, Kmax, 32, lambda R, D: int(lib.wesup_classifier_bwd_workspace_bytes(R, D))))


def test_a_new_shape_evicts_exactly_when_free_plus_idle_memory_is_below_its_table(queries, monkeypatch):
    """WesupEngine._memory_short: a new shape is short exactly when free + idle bytes < 1.1 x its table's bytes -- known before
    any tensor of the set exists, whatever the sets cached so far cost per pixel."""
    import math
    import torch
    from wesup_amd import engine

    def old_set_survives(shape, free, reserved, allocated):
        eng = engine.WesupEngine({'w': torch.zeros(4)}, {'w': torch.zeros(4)})
        monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda device=None: (free, 1 << 40))
        monkeypatch.setattr(torch.cuda, 'memory_reserved', lambda device=None: reserved)
        monkeypatch.setattr(torch.cuda, 'memory_allocated', lambda device=None: allocated)
        eng._bufs[(1, 8, 8, 4)] = engine._Bufs()
        b = eng._get_bufs(*shape, True)
        assert b.x0 is None and b.y == [None] * 13 and list(eng._bufs)[-1] == shape     # a bare record: nothing allocated yet
        return (1, 8, 8, 4) in eng._bufs

    n = table_bytes(4, 480, 480, 576)
    assert 5 << 30 < n < 8 << 30
    enough = math.ceil(1.1 * n)
    assert old_set_survives((4, 480, 480, 576), enough, 0, 0)                   # free memory alone
    assert old_set_survives((4, 480, 480, 576), enough // 2, 3 * enough, 3 * enough - (enough - enough // 2))   # ... with the idle blocks
    assert not old_set_survives((4, 480, 480, 576), enough // 2, 3 * enough, 3 * enough - (enough - enough // 2) + 1)   # one byte less
    assert not old_set_survives((4, 480, 480, 576), enough - 1, 0, 0)
    # many superpixels per pixel: such a set costs more than 16 KiB per pixel -- a per-pixel constant (what the estimate was
    # before any set had been measured) calls this case "not short"
    dense = table_bytes(1, 96, 80, 3072)
    assert dense > 96 * 80 * 16 * 1024
    assert not old_set_survives((1, 96, 80, 3072), 96 * 80 * 16 * 1024, 0, 0)
    assert old_set_survives((1, 96, 80, 3072), math.ceil(1.1 * dense), 0, 0)
    # an evaluation set is sized by the evaluation plan's table
    ev = table_bytes(4, 480, 480, 576, train=False)
    assert ev < n // 2
    eng = engine.WesupEngine({'w': torch.zeros(4)}, {'w': torch.zeros(4)})
    b = eng._get_bufs(4, 480, 480, 576, False)
    assert lp.nbytes(eng._table(b, eng._plan(b, False))) == ev and lp.nbytes(eng._table(b, eng._plan(b, True))) == n


# ---- The buffer sets the PARENT commit (first-use allocation inside the walks) held, per configuration: after one evaluation
# forward and after one training step (forward + backward), each on a fresh engine -- every tensor reachable from the set with its
# name, shape, element type and, for a view, the buffer that owns its storage; the set's bytes (storages counted once); and the
# names of the buffers that no ops.* call of that walk received.  tests/golden/parent_buffer_sets.json is that recording, taken
# from the parent the way the decision tables above were; layer_plan.buffers produced none of it.
# HOW IT WAS TAKEN: by the parent's own engine.py walking forward() / backward() with every ops.* launch replaced by a no-op on
# the host (what a set holds is decided by host code alone; the library's size / route queries were answered by the built
# library).  It was NOT taken on an MI355X: no GPU was to be had when this was written.  The GPU test
# tests/test_buffer_fit_gpu.py checks the same bytes against torch's own storages on the device.
#
# DEAD: what the table leaves out of the parent's training set, by configuration -- dxp[l], the input gradient of layer l + 1 at
# pooled resolution, where that layer has no max-pool backward launch (its input gradient takes the gather / unpool form and
# writes G[l] itself, or it is at or below the lowest trainable layer and has none).  In the recording none of them is handed to
# an ops.* call in any of the eleven configurations.  layer -> bytes, per shape.
DXP = {(4, 480, 480): {1: 4 * 240 * 240 * 64 * 4, 3: 4 * 120 * 120 * 128 * 4, 6: 4 * 60 * 60 * 256 * 4, 9: 4 * 30 * 30 * 512 * 4},
       (1, 96, 80): {1: 48 * 40 * 64 * 4, 3: 24 * 20 * 128 * 4, 6: 12 * 10 * 256 * 4, 9: 6 * 5 * 512 * 4},
       (8, 1024, 1024): {1: 8 * 512 * 512 * 64 * 4, 3: 8 * 256 * 256 * 128 * 4, 6: 8 * 128 * 128 * 256 * 4, 9: 8 * 64 * 64 * 512 * 4},
       (1, 1024, 1024): {1: 512 * 512 * 64 * 4, 3: 256 * 256 * 128 * 4, 6: 128 * 128 * 256 * 4, 9: 64 * 64 * 512 * 4}}
DEAD = {'c01_default': (1, 3, 6, 9),              # 58 982 400 + 29 491 200 + 14 745 600 + 7 372 800 = 110 592 000 bytes
        'c02_plain': (),                          # every pooled layer's input gradient is followed by a max-pool backward
        'c03_plain_unfused': (),
        'c04_direct': (),
        'c05_one_stream': (1, 3, 6, 9),
        'c07a_frozen_to_conv3_3': (1, 3, 6, 9),   # (conv4_1 is the lowest trainable layer: no input gradient at or below it)
        'c07b_frozen_all': (1, 3, 6, 9),
        'c08_odd_96x80': (1, 3, 6, 9),            # 491 520 + 245 760 + 122 880 + 61 440 = 921 600 bytes
        'c09_8x1024': (1, 3, 6, 9),               # 1 006 632 960 bytes
        'c09b_1x1024': (1, 3, 6, 9),              # 125 829 120 bytes
        'c10_f2_min128': ()}


def table_of(name, queries, train):
    from wesup_amd import _lib
    lib = _lib.load()
    B, H, W, Kmax, _, _, _ = CONFIGS[name]
    groups, _, plans = plans_of(name, queries)
    return lp.buffers(plans[0 if train else 1], groups, Kmax, 32, lambda R, D: int(lib.wesup_classifier_bwd_workspace_bytes(R, D)))


def set_name(e):
    return f'groups[{e.layer}].{e.name[2:]}' if e.name.startswith('g.') else e.name if e.layer is None else f'{e.name}[{e.layer}]'


@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_buffer_table_equals_the_set_the_parent_held(name, train, queries):
    import json
    with open(os.path.join(ROOT, 'tests', 'golden', 'parent_buffer_sets.json')) as f:
        rec = json.load(f)[name]
    want = rec['train' if train else 'eval']
    table = table_of(name, queries, train)
    assert len({set_name(e) for e in table}) == len(table)
    got = {set_name(e): [list(e.shape), e.dtype, None if e.group is None else f'groups[{e.group}].{e.name}'] for e in table}
    B, H, W = CONFIGS[name][:3]
    dead = {f'dxp[{l}]': DXP[(B, H, W)][l] for l in DEAD[name]} if train else {}
    for n, nbytes in dead.items():        # itemised: in the parent's set, of that size, never handed to an ops.* call
        shape, dtype, owner = want['bufs'][n]
        assert owner is None and dtype == 'float32' and 4 * shape[0] * shape[1] * shape[2] * shape[3] == nbytes
        assert n in rec['train_never_handed_to_ops']
    assert got == {n: v for n, v in want['bufs'].items() if n not in dead}
    assert lp.nbytes(table) == want['bytes'] - sum(dead.values())
    if name == 'c01_default' and train:
        assert sum(dead.values()) == 110592000
