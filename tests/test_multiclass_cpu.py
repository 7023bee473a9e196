"""The C-way head without a GPU: model and trainer construction, buffer sizing, the host confusion metrics, the command-line
tools' handling of a model with more than two classes, and the presence of the new C ABI entries."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRIES = ['wesup_classifier_fwd_c', 'wesup_classifier_bwd_c_workspace_bytes', 'wesup_classifier_bwd_c', 'wesup_head_fwd_c',
               'wesup_head_bwd_c', 'wesup_classifier_bwd_c_finish', 'wesup_paint_argmax_workspace_bytes', 'wesup_paint_argmax',
               'wesup_seg_confusion']


def test_model_builds_a_c_way_classifier_and_keeps_its_state_dict_layout():
    from wesup_amd.models.wesup import WESUP, WESUPPixelInference
    m3, m2 = WESUP(n_classes=3), WESUP()
    assert m3.classifier[0].weight.shape == (3, 32) and m3.classifier[0].bias.shape == (3,)
    assert m2.classifier[0].weight.shape == (2, 32)
    assert list(m3.state_dict().keys()) == list(m2.state_dict().keys())
    assert WESUPPixelInference(n_classes=5).classifier[0].weight.shape == (5, 32)
    for bad in (1, 17):
        with pytest.raises(ValueError):
            WESUP(n_classes=bad)


def test_initialize_trainer_hands_the_class_count_on():
    from wesup_amd.models import initialize_trainer
    from wesup_amd.utils.data import SyntheticGlasDataset
    t = initialize_trainer('wesup', device='cpu', n_classes=3)
    assert t.model.classifier[0].weight.shape == (3, 32) and t.model.n_classes == 3 and t.kwargs['n_classes'] == 3
    ds = t.get_default_dataset('synthetic:32:32:4:2')
    assert isinstance(ds, SyntheticGlasDataset) and ds.n_classes == 3
    img, pix, pts, seg = ds[0]
    assert pix.shape == (3, 32, 32) and pts.shape == (3, 32, 32)
    t2 = initialize_trainer('wesup', device='cpu')
    assert t2.model.classifier[0].weight.shape == (2, 32) and t2.get_default_dataset('synthetic:32:32:4:2')[0][1].shape == (2, 32, 32)


def test_buffer_table_sizes_sp_pred_by_the_class_count():
    """layer_plan.buffers(..., C=3): sp_pred is (R, 3), everything else as for two classes.  (dpred, the loss gradient, is the step
    runner's state and sized from the masks' class count; tests/test_multiclass_gpu.py checks the gradients it carries.)"""
    from wesup_amd import engine, layer_plan as lp, ops
    B, H, W, Kmax = 2, 64, 48, 64

    def table(params, **kw):
        eng = engine.WesupEngine(params, params)
        groups, group_of = lp.groups_for(B, H, W, Kmax, eng._switches())
        b = engine.WesupEngine._empty_set(B, H, W, Kmax, groups, group_of)
        b.plans = {}
        plan = eng._plan(b, True)
        return eng, b, plan, lp.buffers(plan, b.groups, Kmax, 32, 4096, **kw)

    eng2, b2, plan2, t2 = table({'w': torch.zeros(4)})
    _, _, _, t3 = table({'w': torch.zeros(4)}, C=3)
    assert len(t2) == len(t3)
    diff = [(x, y) for x, y in zip(t2, t3) if x != y]
    assert [(x.name, x.shape, y.shape) for x, y in diff] == [('sp_pred', (B * Kmax, 2), (B * Kmax, 3))]
    assert lp.buffers(plan2, b2.groups, Kmax, 32, 4096, C=2) == t2
    # the engine reads C from the classifier's weight: its own table and its plan key follow
    eng3, b3, plan3, _ = table({'classifier.0.weight': torch.zeros(3, 32)})
    assert eng2.n_classes == 2 and eng3.n_classes == 3
    assert eng2.plan_key(B, H, W) != eng3.plan_key(B, H, W) and eng3.plan_key(B, H, W)[-1] == 3
    by_name = {e.name: e for e in eng3._table(b3, plan3) if e.layer is None}
    assert by_name['sp_pred'].shape == (B * Kmax, 3)
    assert by_name['cls_part'].shape == (max(ops.classifier_bwd_bytes(B * Kmax, 32, 3), 256),)
    assert ops.classifier_bwd_bytes(B * Kmax, 32, 3) == (B * Kmax // 64) * (3 * 32 + 3) * 4
    assert ops.classifier_bwd_bytes(B * Kmax, 32, 2) == ops._lib.load().wesup_classifier_bwd_workspace_bytes(B * Kmax, 32)
    assert ops.head_supported(64, 3) and ops.head_supported(64, 2) and not ops.head_supported(100, 3) and not ops.head_supported(64, 17)


def test_confusion_metrics_on_hand_made_tables():
    from wesup_amd.utils import metrics as M
    # classes 0 and 1 present, class 2 absent from prediction and ground truth: left out of the mean
    t = np.array([[6, 2, 0],
                  [1, 7, 0],
                  [0, 0, 0]])
    d0, d1 = 2 * 6 / (8 + 7 + 1e-7), 2 * 7 / (8 + 9 + 1e-7)
    assert abs(M.dice_from_confusion(t) - (d0 + d1) / 2) < 1e-12
    assert abs(M.accuracy_from_confusion(t) - 13 / 16) < 1e-12
    # a class only the prediction holds counts (with Dice 0)
    t2 = np.array([[4, 0, 2],
                   [0, 4, 0],
                   [0, 0, 0]])
    assert abs(M.dice_from_confusion(t2) - (2 * 4 / (6 + 4 + 1e-7) + 2 * 4 / (4 + 4 + 1e-7) + 0.0) / 3) < 1e-12
    # everything one class: Dice 1 (up to epsilon), accuracy 1
    one = np.zeros((3, 3)); one[1, 1] = 50
    assert abs(M.dice_from_confusion(one) - 1.0) < 1e-8 and M.accuracy_from_confusion(one) == 1.0
    # a batch is the mean over its images
    assert abs(M.dice_from_confusion(np.stack([t, one])) - (M.dice_from_confusion(t) + M.dice_from_confusion(one)) / 2) < 1e-12
    # the host path counts the same table
    P = np.array([[0, 1, 2], [2, 2, 1]]); G = np.array([[0, 1, 1], [2, 0, 1]])
    c = M.confusion(P, G, 3)
    assert c.tolist() == [[1, 0, 1], [0, 2, 1], [0, 0, 1]]
    assert abs(M.accuracy_multiclass(torch.from_numpy(P), torch.from_numpy(G), 3) - 4 / 6) < 1e-12
    assert abs(M.dice_multiclass(P, G, 3) - M.dice_from_confusion(c)) < 1e-12
    with pytest.raises(ValueError):
        M.confusion(np.array([3]), np.array([0]), 3)


def test_trainer_evaluate_uses_the_confusion_definitions_for_more_than_two_classes():
    from wesup_amd.models import initialize_trainer
    from wesup_amd.utils import metrics as M
    P = torch.tensor([[[0, 1, 2], [2, 2, 1]]]); G = torch.tensor([[[0, 1, 1], [2, 0, 1]]])
    t = initialize_trainer('wesup', device='cpu', n_classes=3)
    t.metric_funcs = [M.accuracy, M.dice]
    ev = t.evaluate(P, G)
    assert abs(ev['dice'] - M.dice_multiclass(P[0], G[0], 3)) < 1e-12 and abs(ev['accuracy'] - 4 / 6) < 1e-12
    t2 = initialize_trainer('wesup', device='cpu')
    t2.metric_funcs = [M.accuracy, M.dice]
    B2, G2 = torch.tensor([[[0, 1, 1]]]), torch.tensor([[[0, 1, 0]]])
    assert t2.evaluate(B2, G2)['dice'] == M.dice(B2[0], G2[0])                # two classes: as ever


def test_infer_refuses_multi_scale_class_maps_and_two_class_tools_refuse_the_checkpoint(tmp_path):
    from wesup_amd import infer
    from wesup_amd.models import checkpoint_n_classes, require_two_class_checkpoint
    from wesup_amd.models.wesup import WESUP
    stub = SimpleNamespace(model=SimpleNamespace(n_classes=3), kwargs={})
    with pytest.raises(ValueError, match='class'):
        infer.predict(stub, [], scales=(0.5, 1.0))
    assert infer.predict(stub, [], scales=(0.5,)) == []                         # one scale: fine
    assert infer.predict(stub, [], input_size=(32, 32), scales=(0.5, 1.0)) == []
    assert infer.predict(SimpleNamespace(model=SimpleNamespace(n_classes=2), kwargs={}), [], scales=(0.5, 1.0)) == []
    assert infer.n_classes_of(SimpleNamespace(kwargs={'n_classes': 4})) == 4 and infer.n_classes_of(SimpleNamespace()) == 2
    # class-index PNGs: no x 255
    from PIL import Image
    ds = SimpleNamespace(img_paths=[tmp_path / 'a.png'])
    infer.save_predictions([np.array([[0, 1], [2, 1]])], ds, tmp_path / 'o3', n_classes=3)
    assert np.array(Image.open(tmp_path / 'o3' / 'a.png')).tolist() == [[0, 1], [2, 1]]
    infer.save_predictions([np.array([[0, 1], [1, 1]])], ds, tmp_path / 'o2')
    assert np.array(Image.open(tmp_path / 'o2' / 'a.png')).tolist() == [[0, 255], [255, 255]]
    ck3 = {'model_state_dict': WESUP(n_classes=3).state_dict()}
    ck2 = {'model_state_dict': WESUP().state_dict()}
    assert checkpoint_n_classes(ck3) == 3 and checkpoint_n_classes(ck2) == 2
    require_two_class_checkpoint(ck2, 'x')
    require_two_class_checkpoint(None, 'x')
    with pytest.raises(ValueError, match='3-class'):
        require_two_class_checkpoint(ck3, 'pixel inference')
    path = tmp_path / 'ckpt.pth'
    torch.save(ck3, path)
    from wesup_amd import infer_tile
    with pytest.raises(ValueError, match='3-class'):
        infer_tile._load_pixel_model(str(path), 'cpu')


def test_new_entries_are_declared_and_bound():
    from wesup_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    for name in NEW_ENTRIES:
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in _lib._SIGS, name
    assert re.search(r'#define\s+WESUP_MAX_CLASSES\s+16\b', hdr) and _lib.MAX_CLASSES == 16
    assert _lib.ABI_VERSION == 6
