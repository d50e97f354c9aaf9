"""CPU-side checks of the per-object scene-frame interface (no GPU): the C ABI declares and exports smg_scene_argmax_objects and
the binding carries it, the numpy restatement of tests/scene_objects_ref.py agrees with a brute-force loop, and the three Trainer
methods refuse before they touch an engine."""
import numpy as np
import pytest

from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_objects_ref


def test_scene_argmax_objects_is_declared_exported_and_bound():
    assert_declared_exported_and_bound(
        "smg_scene_argmax_objects",
        r"\bint\s+smg_scene_argmax_objects\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int64_t map_stride,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*const double\*\s*masks_dev,\s*int n_masks,\s*const int\*\s*map_mask_a,\s*"
        r"const int\*\s*map_mask_b,\s*const int\*\s*map_group,\s*int n_groups,\s*int\*\s*idx_out_dev,\s*float\*\s*val_out_dev,\s*void\*\s*stream\)",
        15, "scene_argmax_objects", ["forward_objects_dense", "forward_object_pairs_dense", "best_scene_actions"])


def brute_force(maps, masks, mask_a, mask_b, groups, n_groups):
    """The rules spelled out pixel by pixel, with argmax_better's comparison."""
    n_maps, hm, _ = maps.shape
    out = []
    for g in range(n_groups):
        best, at = np.float32(-np.inf), -1
        for m in range(n_maps):
            if groups[m] != g:
                continue
            for iy in range(hm):
                for ix in range(hm):
                    a, b = mask_a[m], mask_b[m]
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


def test_helper_against_a_brute_force_loop_on_a_toy():
    """(Validates the REFERENCE, tests/scene_objects_ref.py, not the product.)  6 x 6 maps: 7 maps in 4 groups that are not
    contiguous, ties, a NaN, invalid pixels, mask values -0.0 / NaN / 0.5, a union, the every-pixel form, a group whose mask
    selects invalid pixels only and a group without a map."""
    rng = np.random.default_rng(3)
    hm, n_maps = 6, 7
    maps = rng.integers(-3, 4, size=(n_maps, hm, hm)).astype(np.float32)         # small integers: ties
    maps[:, 0, :] = -np.inf                                                    # row 0 invalid everywhere
    maps[2, 3:, 3:] = -np.inf
    maps[4, 2, 2] = np.nan
    masks = np.zeros((4, hm, hm))
    masks[0, 1:3, 1:4] = 1.0
    masks[1, 2:5, 2:6] = -1.0
    masks[1, 3, 3] = -0.0
    masks[1, 4, 4] = np.nan
    masks[2, 0, :] = 0.5                                                       # invalid pixels only
    masks[3, 5, 5] = 2.0
    mask_a = [0, 1, 0, 2, 1, -1, 3]
    mask_b = [-1, -1, 1, -1, 0, -1, -1]
    groups = [0, 1, 0, 2, 1, 4, 1]
    idx, val = scene_objects_ref.group_argmax(maps, masks, mask_a, mask_b, groups, 5)
    ref = brute_force(maps, masks, mask_a, mask_b, groups, 5)
    for g in range(5):
        print("group %d: helper (%d, %s), brute force %s" % (g, idx[g], val[g], ref[g]))
        assert idx[g] == ref[g][0]
        assert np.asarray(val[g]).view(np.uint32) == np.asarray(ref[g][1], dtype=np.float32).view(np.uint32)
    assert idx[2] == -1 and np.isneginf(val[2])           # selected pixels, none valid
    assert idx[3] == -1 and np.isneginf(val[3])           # no map
    assert np.isnan(val[1]) and idx[1] == (4 * hm + 2) * hm + 2          # the NaN of map 4 wins its group
    assert idx[4] // (hm * hm) == 5 and idx[4] % (hm * hm) >= hm         # every pixel selected, row 0 invalid
    assert not scene_objects_ref.selected(masks, 1, -1)[3, 3] and scene_objects_ref.selected(masks, 1, -1)[4, 4]


def test_trainer_methods_refuse_before_the_engine():
    # (on a CPU trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    d, m = np.zeros((240, 240)), np.ones((2, 240, 240))
    d224, m224 = np.zeros((224, 224)), np.ones((2, 224, 224))                   # S = 640: a 1 x 1 map has no extent
    for tr, depth, masks in ((cpu_trainer('reactive'), d, m), (cpu_trainer('reinforcement'), d224, m224)):
        with pytest.raises(ValueError):
            tr.forward_objects_dense(depth, masks, 0)
        with pytest.raises(ValueError):
            tr.forward_object_pairs_dense(depth, masks)
        with pytest.raises(ValueError):
            tr.best_scene_actions(depth, masks)
    with pytest.raises(ValueError):
        cpu_trainer('reinforcement').forward_objects_dense(d, m, style=2)
    # a large heightmap on a reinforcement trainer passes every check and reaches the engine, which a CPU trainer does not have
    with pytest.raises(RuntimeError):
        cpu_trainer('reinforcement').best_scene_actions(d, m)
