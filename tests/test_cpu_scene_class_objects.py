"""CPU-side checks of the reactive net's per-object scene-frame interface (no GPU): the C ABI declares and exports
smg_scene_class_argmax_objects and the binding carries it, the three Trainer methods refuse before they touch an engine, and the
two numpy references the GPU tests combine - scene_class_ref.scene_class_maps for the values, scene_objects_ref.group_argmax for
the selection and grouping - compose: checked once against a brute-force loop."""
import numpy as np
import pytest

from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_class_ref
import scene_objects_ref
import scene_ref


def test_scene_class_argmax_objects_is_declared_exported_and_bound():
    assert_declared_exported_and_bound(
        "smg_scene_class_argmax_objects",
        r"\bint\s+smg_scene_class_argmax_objects\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*int cls,\s*const double\*\s*masks_dev,\s*int n_masks,\s*const int\*\s*map_mask_a,\s*"
        r"const int\*\s*map_mask_b,\s*const int\*\s*map_group,\s*int n_groups,\s*int\*\s*idx_out_dev,\s*float\*\s*val_out_dev,\s*void\*\s*stream\)",
        15, "scene_class_argmax_objects", ["forward_class_objects", "forward_class_object_pairs", "best_scene_class_actions"])


def test_trainer_methods_refuse_before_the_engine():
    # (on a CPU trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    d, m = np.zeros((240, 240)), np.ones((2, 240, 240))
    d224, m224 = np.zeros((224, 224)), np.ones((2, 224, 224))
    rl, ra = cpu_trainer('reinforcement'), cpu_trainer('reactive')
    for depth, masks in ((d, m), (d224, m224)):             # a reinforcement trainer, whatever the heightmap
        with pytest.raises(ValueError, match="reactive method only"):
            rl.forward_class_objects(depth, masks, 0)
        with pytest.raises(ValueError, match="reactive method only"):
            rl.forward_class_object_pairs(depth, masks)
        with pytest.raises(ValueError, match="reactive method only"):
            rl.best_scene_class_actions(depth, masks)
    with pytest.raises(ValueError, match="styles 0"):
        ra.forward_class_objects(d, m, style=2)
    with pytest.raises(ValueError, match="224"):             # S = 640: a 1 x 1 map has no extent
        ra.best_scene_class_actions(d224, m224)
    with pytest.raises(ValueError, match="cls"):
        ra.best_scene_class_actions(d, m, cls=3)
    for wrong in (np.ones((2, 240, 239)), np.ones((2, 224, 224)), np.ones((240, 240))):
        with pytest.raises(ValueError, match="mask_depth must be"):
            ra.forward_class_objects(d, wrong)
        with pytest.raises(ValueError, match="mask_depth must be"):
            ra.forward_class_object_pairs(d, wrong)
        with pytest.raises(ValueError, match="mask_depth must be"):
            ra.best_scene_class_actions(d, wrong)
    empty = np.ones((0, 240, 240))
    with pytest.raises(ValueError, match="no object"):
        ra.forward_class_objects(d, empty)
    with pytest.raises(ValueError, match="no object"):
        ra.forward_class_object_pairs(d, empty)
    with pytest.raises(ValueError, match="no object"):
        ra.best_scene_class_actions(d, empty)
    # a reactive trainer with valid arguments passes every check and reaches the engine, which a CPU trainer does not have
    with pytest.raises(RuntimeError):
        ra.forward_class_objects(d, m, 1)
    with pytest.raises(RuntimeError):
        ra.forward_class_objects(d224, m224)                 # 224^2 is fine for the maps themselves
    with pytest.raises(RuntimeError):
        ra.forward_class_object_pairs(d, m)
    with pytest.raises(RuntimeError):
        ra.best_scene_class_actions(d, m)
    # the reinforcement entry points keep refusing a reactive trainer
    with pytest.raises(ValueError):
        ra.forward_objects(d224, m224, 0)


def brute_force(maps, masks, mask_a, mask_b, groups, n_groups):
    """The rules spelled out pixel by pixel: selection by != 0 (union), invalid = -inf skipped, a NaN beats a number, then the
    larger value, then the lower flattened index."""
    n_maps, hm, _ = maps.shape
    out = []
    for g in range(n_groups):
        best, at = np.float32(-np.inf), -1
        for m in range(n_maps):
            if groups[m] != g:
                continue
            a, b = mask_a[m], mask_b[m]
            for iy in range(hm):
                for ix in range(hm):
                    sel = (a < 0 and b < 0) or (a >= 0 and masks[a, iy, ix] != 0) or (b >= 0 and masks[b, iy, ix] != 0)
                    v = maps[m, iy, ix]
                    if not sel or np.isneginf(v):
                        continue
                    flat = (m * hm + iy) * hm + ix
                    if at < 0:
                        better = True
                    elif np.isnan(v) != np.isnan(best):
                        better = bool(np.isnan(v))
                    elif np.isnan(v):
                        better = flat < at
                    else:
                        better = v > best or (v == best and flat < at)
                    if better:
                        best, at = v, flat
        out.append((at, best))
    return out


def test_the_two_references_compose():
    """(Validates the REFERENCES, not the product.)  hm = 240, 3 x 3 logits, 4 rotations: plane 0 of the fp64 class maps cast to
    float32, through group_argmax, against the brute-force loop - a rectangle, a union, a -0.0 / NaN mask, the every-pixel form, a
    mask on invalid pixels only (the border rows have no window at hm = 240) and a group without a map."""
    hm, R = 240, 4
    aff = np.stack([scene_ref.theta(r, R) for r in range(R)])
    q = np.random.default_rng(5).standard_normal((R, 3, 3, 3)).astype(np.float32)
    P, valid, _ = scene_class_ref.scene_class_maps(q, aff, hm)
    maps = P[:, 0].astype(np.float32)
    assert np.array_equal(np.isneginf(maps), ~valid) and not valid[:, :40].any() and valid[:, 120, 120].all()
    inside = maps[valid]
    assert inside.min() > 0 and inside.max() < 1
    masks = np.zeros((5, hm, hm))
    masks[0, 112:128, 110:126] = 1.0
    masks[1, 90:110, 100:140] = -1.0
    masks[2] = -0.0
    masks[2, 119, 118] = np.nan
    masks[3, 0:40, :] = 0.5                                  # invalid pixels only
    masks[4, 125:131, 125:131] = 2.0
    mask_a = [0, 1, 2, 3, -1, 0, 4, 2]
    mask_b = [-1, 0, -1, -1, -1, 4, -1, 3]
    groups = [0, 1, 2, 3, 4, 0, 1, 2]
    rep = [0, 1, 2, 3, 0, 1, 2, 3]
    idx, val = scene_objects_ref.group_argmax(maps[rep], masks, mask_a, mask_b, groups, 6)
    ref = brute_force(maps[rep], masks, mask_a, mask_b, groups, 6)
    for g in range(6):
        print("group %d: helper (%d, %s), brute force %s" % (g, idx[g], val[g], ref[g]))
        assert idx[g] == ref[g][0]
        assert np.asarray(val[g]).view(np.uint32) == np.asarray(ref[g][1], dtype=np.float32).view(np.uint32)
    assert (idx[[0, 1, 2, 4]] >= 0).all()
    assert idx[3] == -1 and np.isneginf(val[3])              # all-invalid: selected pixels, none with a window
    assert idx[5] == -1 and np.isneginf(val[5])              # no map
    assert idx[2] % (hm * hm) == 119 * hm + 118              # the NaN of the mask selects one pixel; the -0.0 and the invalid rows none
