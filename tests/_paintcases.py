"""The cases of tests/golden/paint.npz (tools/make_paint_golden.py) as arrays and as directories: shared by test_paint_cpu.py
and test_paint_gpu.py."""
import os

import numpy as np


def paint_case(gold, name):
    H, W = (int(v) for v in gold['shape'])
    return tuple(np.unpackbits(gold[f'{k}_{name}'])[:H * W].reshape(H, W) for k in 'SG')


def eval_case(gold, i):
    H, W = (int(v) for v in gold['eval_shape'])
    pred, post = (np.unpackbits(gold[f'eval_{k}{i}'])[:H * W].reshape(H, W) for k in ('pred', 'post'))
    return pred * np.uint8(255), gold[f'eval_gt{i}'], post


def write_eval_dirs(gold, root):
    from PIL import Image
    os.makedirs(root / 'results')
    os.makedirs(root / 'masks')
    for i in range(int(gold['eval_n'])):
        pred, gt, _ = eval_case(gold, i)
        Image.fromarray(pred).save(root / 'results' / f'im{i}.png')
        Image.fromarray(gt).save(root / 'masks' / f'im{i}.png')
    return root / 'results', root / 'masks'
