"""CPU-side checks of the scene-frame value interface (no GPU): the C ABI declares and exports smg_scene_values /
smg_scene_class_values and the binding carries them, the gather of tests/scene_values_ref.py agrees with the point form of
tests/scene_ref.py, the eight Trainer methods refuse before they touch an engine, and get_label_value_scene / backprop_scene map
best_scene_actions' dict onto scene_values and the train_batch_scene_*pixels calls (replaced by recorders here)."""
import numpy as np
import pytest
import torch

from helpers import orc
from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_class_ref
import scene_ref
import scene_values_ref

TRAINER_METHODS = ["scene_values", "scene_object_values", "scene_object_pair_values", "scene_class_values", "scene_class_object_values",
                   "scene_class_object_pair_values", "get_label_value_scene", "backprop_scene"]


def test_scene_values_are_declared_exported_and_bound():
    assert_declared_exported_and_bound(
        "smg_scene_values",
        r"\bint\s+smg_scene_values\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int64_t map_stride,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*int K,\s*const int\*\s*pixels_dev,\s*float\*\s*out_dev,\s*void\*\s*stream\)",
        10, "scene_values", TRAINER_METHODS)
    assert_declared_exported_and_bound(
        "smg_scene_class_values",
        r"\bint\s+smg_scene_class_values\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int n_maps,\s*const float\*\s*affine_host,\s*"
        r"int hm_size,\s*int cls,\s*int K,\s*const int\*\s*pixels_dev,\s*float\*\s*out_dev,\s*void\*\s*stream\)",
        10, "scene_class_values", TRAINER_METHODS)


def test_helper_gather_against_the_point_form():
    """(Validates the REFERENCE, tests/scene_values_ref.py, not the product.)  hm = 240, the 81 pixels 116 .. 124 squared of
    map_harness.s704_scene's block, valid in all 16 rotations: the gather from the map form equals scene_ref.scene_points (torch
    fp64, the same expression on the same corners) to 2 ulp of fp64; the class form is the softmax of the three gathered logits;
    points outside the heightmap are -inf."""
    hm, side = 240, 3
    by, bx = np.meshgrid(np.arange(116, 125), np.arange(116, 125), indexing="ij")
    block = np.stack([by.ravel(), bx.ravel()], axis=-1)
    aff = np.stack([scene_ref.theta(r, 16) for r in range(16)])
    rng = np.random.default_rng(7)
    q = rng.standard_normal((16, side, side))
    q3 = rng.standard_normal((16, 3, side, side))
    pix = np.broadcast_to(block, (16, 81, 2))
    got = scene_values_ref.values(q, aff, hm, pix)
    got3 = scene_values_ref.class_values(q3, aff, hm, pix)
    assert got.shape == (16, 81) and got3.shape == (16, 3, 81) and got.dtype == got3.dtype == np.float64
    for r in range(16):
        want = scene_ref.scene_points(torch.from_numpy(q[r]), aff[r], hm, block).numpy()
        assert np.abs(got[r] - want).max() <= 2.0 ** -51 * np.abs(want).max()
        z = scene_class_ref.scene_class_points(torch.from_numpy(q3[r]), aff[r], hm, block)
        want3 = torch.softmax(z, dim=1).numpy().T
        assert np.abs(got3[r] - want3).max() <= 2.0 ** -50
    # any integer is a legal point: outside the heightmap the value is -inf in every plane, inside it is the map's
    odd = np.asarray([[(-1, 120), (120, 240), (-2 ** 31, 2 ** 31 - 1), (120, 120), (0, 0)]] * 16)
    v, v3 = scene_values_ref.values(q, aff, hm, odd), scene_values_ref.class_values(q3, aff, hm, odd)
    assert np.isneginf(v[:, :3]).all() and np.isneginf(v3[:, :, :3]).all()
    assert np.array_equal(v[:, 3], got[:, 4 * 9 + 4]) and np.array_equal(v3[:, :, 3], got3[:, :, 4 * 9 + 4])
    assert np.isneginf(v[:, 4]).all()                       # the image corner: inside the heightmap, no window centred there
    maps32 = scene_ref.scene_maps(q, aff, hm)[0].astype(np.float32)
    assert scene_values_ref.gather(maps32, odd).dtype == np.float32


def test_trainer_methods_refuse_before_the_engine():
    # (on a CPU trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    d, m = np.zeros((240, 240)), np.ones((3, 240, 240))
    d224, m224 = np.zeros((224, 224)), np.ones((3, 224, 224))                   # S = 640: a 1 x 1 map has no extent
    p1, pn, pp = [(120, 120)], [(120, 120)] * 3, [(120, 120)] * 3               # 3 objects, 3 pairs

    def calls(tr, depth, masks, one=p1, per_object=pn, per_pair=pp):
        return {"scene_values": lambda: tr.scene_values(depth, depth, one),
                "scene_object_values": lambda: tr.scene_object_values(depth, masks, per_object),
                "scene_object_pair_values": lambda: tr.scene_object_pair_values(depth, masks, per_pair),
                "scene_class_values": lambda: tr.scene_class_values(depth, depth, one),
                "scene_class_object_values": lambda: tr.scene_class_object_values(depth, masks, per_object),
                "scene_class_object_pair_values": lambda: tr.scene_class_object_pair_values(depth, masks, per_pair)}
    q_names = ["scene_values", "scene_object_values", "scene_object_pair_values"]
    c_names = ["scene_class_values", "scene_class_object_values", "scene_class_object_pair_values"]
    rl, rc = cpu_trainer('reinforcement'), cpu_trainer('reactive')
    for tr, own, other in ((rl, q_names, c_names), (rc, c_names, q_names)):
        for name in other:                                  # the wrong method
            with pytest.raises(ValueError):
                calls(tr, d, m)[name]()
        for name in own:
            with pytest.raises(ValueError):                 # a 224^2 heightmap
                calls(tr, d224, m224)[name]()
            for pix in ([(120, 120, 1)], [(120.5, 120)], [(120, 240)], [(-1, 3)], np.zeros((2, 2, 2, 2))):
                many = list(pix) * 3 if np.ndim(pix) == 2 else pix      # one such point per object / pair
                with pytest.raises(ValueError):             # wrong shape, non-integer, outside the heightmap
                    calls(tr, d, m, one=pix, per_object=many, per_pair=many)[name]()
            with pytest.raises(RuntimeError):               # every check passed: the engine, which a CPU trainer does not have
                calls(tr, d, m)[name]()
        for name in own[1:]:                                # one pixel list per object / per pair, no fewer
            with pytest.raises(ValueError):
                calls(tr, d, m, per_object=pn[:2], per_pair=pp[:2])[name]()
    with pytest.raises(ValueError):
        rc.scene_class_values(d, d, p1, cls=3)
    with pytest.raises(ValueError):
        rl.scene_object_values(d, m, pn, style=2)
    # fewer than two objects: no pair, nothing runs, nothing is refused
    vals, idx = rl.scene_object_pair_values(d, m[:1], np.zeros((0, 2)))
    assert idx == [] and vals.shape == (0,)


BEST = {"bestg_id": (1, 5), "bestg_pixel": (118, 131), "bestg_conf": 0.25, "bests_id": (2, 9), "bests_pixel": (140, 99), "bests_conf": 0.5,
        "bestgs_num": (0, 2), "bestgs_pixel": (125, 120), "bestgs_conf": 0.125}
ACTIONS = {"grasp": (0, 5, (118, 131), lambda m: m[1]), "suction": (1, 9, (140, 99), lambda m: m[2]),
           "grasp_then_suction": (2, 0, (125, 120), lambda m: m[0] + m[2])}


def scene_and_masks(hm=240):
    rng = np.random.default_rng(2)
    depth = rng.uniform(0.0, 0.1, size=(hm, hm))
    masks = (rng.uniform(size=(3, hm, hm)) < 0.3).astype(np.float64)
    return depth, masks


def test_get_label_value_scene_with_a_recorder(capsys):
    depth, masks = scene_and_masks()
    tr = cpu_trainer('reinforcement')
    seen = []

    def recorder(d, m, pixels, style=0, is_target=False, specific_rotation=-1, return_device=False):
        seen.append(dict(d=d, m=np.array(m), pixels=pixels, style=style, is_target=is_target, rot=specific_rotation, dev=return_device))
        return np.asarray([[0.75]])
    tr.scene_values = recorder
    # the zero-future rows of test_trainer_reward_arithmetic_matches_oracle: the recorder is never called, best may be anything
    for args in (("grasp", 3, 0, 0, 0), ("suction", 1, 1, 0, 0), ("grasp", 1, 0, 1, 0), ("grasp_then_suction", 2, 0, 0, 2.5)):
        got = tr.get_label_value_scene(args[0], args[1], args[2], args[3], args[4], depth, masks, None, 'grasp')
        assert got == orc.label_value("reinforcement", args[0], args[1], args[2], args[3], args[4], 123.0, 0.5)
        assert got == tr.get_label_value(args[0], args[1], args[2], args[3], args[4], depth, masks, masks, (0, 0), (0, 0), (0, 0), (0, 0), 'grasp', 0, 0, 0)
    assert not seen
    # non-terminal rows: one target evaluation at the action `best` names for the exploit action
    for args in (("grasp", 3, 0, 1, 0), ("suction", 2, 1, 0, 0), ("grasp_then_suction", 3, 0, 0, 2.5), ("grasp", 2, 0, 0.5, 0)):
        for exploit, (style, rot, pixel, masked) in ACTIONS.items():
            del seen[:]
            capsys.readouterr()
            got = tr.get_label_value_scene(args[0], args[1], args[2], args[3], args[4], depth, masks, BEST, exploit)
            assert got == orc.label_value("reinforcement", args[0], args[1], args[2], args[3], args[4], 0.75, 0.5)
            assert got[0] == got[1] + 0.5 * 0.75
            assert capsys.readouterr().out == 'Expected reward: %f + %f x %f = %f\n' % (got[1], 0.5, 0.75, got[0])
            assert len(seen) == 1
            call = seen[0]
            assert call["is_target"] is True and call["style"] == style and call["rot"] == rot and call["dev"] is False
            assert np.asarray(call["pixels"]).shape == (1, 2) and tuple(np.asarray(call["pixels"])[0]) == pixel
            assert call["d"] is depth and np.array_equal(call["m"], depth * masked(masks))
    # a None id for the chosen primitive raises and names it; the other primitives' ids do not matter
    for exploit, key in (("grasp", "bestg_id"), ("suction", "bests_id"), ("grasp_then_suction", "bestgs_num")):
        with pytest.raises(ValueError, match=key):
            tr.get_label_value_scene("grasp", 3, 0, 1, 0, depth, masks, dict(BEST, **{key: None}), exploit)
    del seen[:]
    assert tr.get_label_value_scene("grasp", 3, 0, 1, 0, depth, masks, dict(BEST, bests_id=None, bestgs_num=None), "grasp")[0] == 1 + 0.5 * 0.75
    assert len(seen) == 1
    # reactive: get_label_value's tuple and print-out, no forward, best may be None
    tr3 = cpu_trainer('reactive')
    tr3.scene_values = tr3.scene_class_values = recorder
    for args in (("grasp", 3, 0, 0, 0), ("grasp", 3, 0, 1, 0), ("suction", 3, 1, 0, 0), ("grasp_then_suction", 3, 0, 0, 2.5),
                 ("grasp_then_suction", 3, 0, 0, 0.5)):
        capsys.readouterr()
        want = tr3.get_label_value(args[0], args[1], args[2], args[3], args[4], depth, masks, masks, (0, 0), (0, 0), (0, 0), (0, 0), 'grasp', 0, 0, 0)
        said = capsys.readouterr().out
        assert tr3.get_label_value_scene(args[0], args[1], args[2], args[3], args[4], depth, masks, None, 'grasp') == want
        assert capsys.readouterr().out == said == 'Label value: %d\n' % want[0]
        assert want == orc.label_value("reactive", args[0], args[1], args[2], args[3], args[4], 0, 0.5)
    assert len(seen) == 1


@pytest.mark.parametrize("method,step,label", (("reinforcement", "train_batch_scene_pixels", 1.25), ("reactive", "train_batch_scene_class_pixels", 1)))
def test_backprop_scene_with_a_recorder(method, step, label, capsys):
    depth, masks = scene_and_masks()
    tr = cpu_trainer(method)
    seen = []

    def recorder(name):
        def record(*args, **kwargs):
            seen.append((name, args, kwargs))
            return torch.tensor([0.375])
        return record
    tr.train_batch_scene_pixels = recorder("train_batch_scene_pixels")
    tr.train_batch_scene_class_pixels = recorder("train_batch_scene_class_pixels")
    for objects_mask in (masks.copy(), masks.copy().reshape(3, 240, 240, 1)):
        shape = objects_mask.shape
        for action, (style, rot, pixel, masked) in ACTIONS.items():
            del seen[:]
            capsys.readouterr()
            loss = tr.backprop_scene(depth, action, BEST, label, objects_mask)
            assert isinstance(loss, np.ndarray) and loss.shape == () and float(loss) == 0.375
            assert capsys.readouterr().out == 'Training loss: %f\n' % 0.375
            assert objects_mask.shape == shape
            assert len(seen) == 1 and seen[0][0] == step and seen[0][2] == {}
            d, m, st, rots, pixels, labels = seen[0][1]
            assert d is depth and np.array_equal(m, depth * masked(masks)) and st == style
            assert list(rots) == [rot] and np.asarray(pixels).shape == (1, 1, 2) and tuple(np.asarray(pixels)[0, 0]) == pixel
            assert list(labels) == [label]
    with pytest.raises(ValueError, match="bestgs_num"):
        tr.backprop_scene(depth, "grasp_then_suction", dict(BEST, bestgs_num=None, bestgs_pixel=None), label, masks)
    with pytest.raises(ValueError):
        tr.backprop_scene(depth, "push", BEST, label, masks)
