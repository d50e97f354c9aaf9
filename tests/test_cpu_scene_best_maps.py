"""CPU-side checks of the collapsed scene-frame map (no GPU): the C ABI declares and exports smg_scene_best_maps and
smg_scene_class_best_maps and the binding carries them, the numpy restatement of tests/scene_best_ref.py agrees with a brute-force
loop over pixels, and the Trainer methods refuse before they touch an engine."""
import numpy as np
import pytest

from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_best_ref

TAIL = (r"const double\*\s*masks_dev,\s*int n_masks,\s*const int\*\s*map_mask_a,\s*const int\*\s*map_mask_b,\s*const int\*\s*map_group,\s*"
        r"int n_groups,\s*float\*\s*val_out_dev,\s*int\*\s*arg_out_dev,\s*void\*\s*stream\)")


def test_both_exports_are_declared_exported_and_bound():
    hdr = assert_declared_exported_and_bound(
        "smg_scene_best_maps",
        r"\bint\s+smg_scene_best_maps\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int64_t map_stride,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*" + TAIL,
        15, "scene_best_maps", ["best_rotation_map", "best_rotation_object_maps"])
    assert_declared_exported_and_bound(
        "smg_scene_class_best_maps",
        r"\bint\s+smg_scene_class_best_maps\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*int cls,\s*" + TAIL,
        15, "scene_class_best_maps", ["best_rotation_class_map", "best_rotation_class_object_maps"])
    for word in ("(-inf, -1)", "masks_dev == NULL with n_masks == 0", "lowest m on ties", "bit for bit", "n_groups * hm_size^2 beyond int32"):
        assert word in hdr, word


def brute_force(maps, masks, mask_a, mask_b, groups, n_groups):
    """The rules spelled out pixel by pixel: the candidates of (group, pixel) in ascending map order, a later one replacing the
    held one only when it is strictly better - a NaN over a number, a larger number over a smaller - so the lowest map keeps a tie
    and the first NaN stays."""
    n_maps, hm, _ = maps.shape
    val = np.full((n_groups, hm, hm), -np.inf, dtype=np.float32)
    arg = np.full((n_groups, hm, hm), -1, dtype=np.int32)
    for g in range(n_groups):
        for iy in range(hm):
            for ix in range(hm):
                for m in range(n_maps):
                    if groups[m] != g:
                        continue
                    a, b = mask_a[m], mask_b[m]
                    sel = (a < 0 and b < 0) or (a >= 0 and masks[a, iy, ix] != 0) or (b >= 0 and masks[b, iy, ix] != 0)
                    v = maps[m, iy, ix]
                    if not sel or np.isneginf(v):
                        continue
                    held = val[g, iy, ix]
                    if arg[g, iy, ix] < 0 or (np.isnan(v) and not np.isnan(held)) or (not np.isnan(held) and v > held):
                        val[g, iy, ix], arg[g, iy, ix] = v, m
    return val, arg


def toy():
    """6 x 6 maps, 8 maps in 4 groups that are not contiguous plus a group without a map: ties (small integers, and map 7 a copy
    of map 1), NaNs in two maps of one group at the same pixel, invalid pixels, mask values -0.0 / NaN / 0.5, a union, the
    every-pixel form, and a group whose mask selects invalid pixels only."""
    rng = np.random.default_rng(5)
    hm, n_maps = 6, 8
    maps = rng.integers(-3, 4, size=(n_maps, hm, hm)).astype(np.float32)
    maps[:, 0, :] = -np.inf
    maps[2, 3:, 3:] = -np.inf
    maps[4, 2, 2] = np.nan
    maps[7] = maps[1]
    maps[7, 2, 2] = np.nan                   # behind map 4's NaN in group 1: the first stays
    maps[7, 4, 5] = np.nan                   # the only NaN of that pixel
    masks = np.zeros((4, hm, hm))
    masks[0, 1:3, 1:4] = 1.0
    masks[1, 2:5, 2:6] = -1.0
    masks[1, 3, 3] = -0.0
    masks[1, 4, 4] = np.nan
    masks[2, 0, :] = 0.5
    masks[3, 5, 5] = 2.0
    return maps, masks, [0, 1, 0, 2, 1, -1, 3, 1], [-1, -1, 1, -1, 0, -1, -1, -1], [0, 1, 0, 2, 1, 4, 1, 1]


def same(a, b):
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_helper_against_a_brute_force_loop_on_a_toy():
    """(Validates the REFERENCE, tests/scene_best_ref.py, not the product.)"""
    maps, masks, mask_a, mask_b, groups = toy()
    got = scene_best_ref.group_best(maps, masks, mask_a, mask_b, groups, 5)
    same(got, brute_force(maps, masks, mask_a, mask_b, groups, 5))
    val, arg = got
    assert val.dtype == np.float32 and arg.dtype == np.int32 and val.shape == arg.shape == (5, 6, 6)
    assert (arg[2] == -1).all() and np.isneginf(val[2]).all()                  # mask 2 selects row 0 alone, which is invalid
    assert (arg[3] == -1).all() and np.isneginf(val[3]).all()                  # a group without a map
    assert (arg[:, 0, :] == -1).all()                                          # a pixel without a candidate, in every group
    assert (arg[4, 1:] == 5).all() and np.array_equal(val[4, 1:], maps[5, 1:])                 # one map, every pixel
    assert np.isnan(val[1, 2, 2]) and arg[1, 2, 2] == 4                        # two NaNs at one pixel: the first map's
    assert np.isnan(val[1, 4, 5]) and arg[1, 4, 5] == 7                        # a NaN beats the numbers of the lower maps
    assert arg[1, 3, 3] == -1                                                  # -0.0 does not select
    assert arg[1, 4, 4] in (1, 4, 7)                                           # a NaN mask value selects
    assert arg[1, 5, 5] == 6 and val[1, 5, 5] == maps[6, 5, 5] and (arg[1] == 6).sum() == 1   # mask 3's one pixel: map 6 alone, and nowhere else
    tie = (maps[1] == maps[7]) & (masks[1] != 0) & (arg[1] >= 0) & (arg[1] != 4) & (arg[1] != 6)
    assert tie.any() and not (arg[1][tie] == 7).any()                          # map 7 repeats map 1: the lower map keeps every tie
    assert set(np.unique(arg[0])) <= {-1, 0, 2}                                # the union (0 | 1) of map 2 and the plain mask 0 of map 0


def test_masks_of_none_is_the_every_pixel_form():
    maps, masks, _, _, groups = toy()
    none = [-1] * 8
    a = scene_best_ref.group_best(maps, None, none, none, groups, 5)
    same(a, scene_best_ref.group_best(maps, masks, none, none, groups, 5))
    same(a, brute_force(maps, masks, none, none, groups, 5))
    # one group, call order: np.max / np.argmax over axis 0 with the invalid pixels at -1
    val, arg = scene_best_ref.group_best(maps, None, none, none, [0] * 8, 1)
    assert np.array_equal(val[0].view(np.uint32), np.max(maps, axis=0).view(np.uint32))
    assert np.array_equal(arg[0], np.where(np.isneginf(np.max(maps, axis=0)), -1, np.argmax(maps, axis=0)))
    with pytest.raises(AssertionError):
        scene_best_ref.group_best(maps, None, [0] + none[1:], none, groups, 5)


def test_trainer_methods_refuse_before_the_engine():
    # (on a CPU trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    d, m = np.zeros((240, 240)), np.ones((2, 240, 240))
    d224, m224 = np.zeros((224, 224)), np.ones((2, 224, 224))                   # S = 640: a 1 x 1 map has no extent
    rl, re = cpu_trainer('reinforcement'), cpu_trainer('reactive')
    with pytest.raises(ValueError):
        re.best_rotation_map(d, d)
    with pytest.raises(ValueError):
        re.best_rotation_object_maps(d, m)
    with pytest.raises(ValueError):
        rl.best_rotation_class_map(d, d)
    with pytest.raises(ValueError):
        rl.best_rotation_class_object_maps(d, m)
    with pytest.raises(ValueError):
        rl.best_rotation_map(d224, d224)
    with pytest.raises(ValueError):
        rl.best_rotation_object_maps(d224, m224)
    with pytest.raises(ValueError):
        re.best_rotation_class_map(d224, d224)
    with pytest.raises(ValueError):
        re.best_rotation_class_object_maps(d224, m224)
    for cls in (3, -1):
        with pytest.raises(ValueError):
            re.best_rotation_class_map(d, d, cls=cls)
        with pytest.raises(ValueError):
            re.best_rotation_class_object_maps(d, m, cls=cls)
    for style in (2, 3):                                                        # style 2 is rotation 0 alone: not offered
        with pytest.raises(ValueError):
            rl.best_rotation_map(d, d, style=style)
        with pytest.raises(ValueError):
            rl.best_rotation_object_maps(d, m, style=style)
        with pytest.raises(ValueError):
            re.best_rotation_class_map(d, d, style=style)
        with pytest.raises(ValueError):
            re.best_rotation_class_object_maps(d, m, style=style)
    with pytest.raises(ValueError):
        re.best_rotation_class_object_maps(d, np.ones((2, 200, 240)))           # masks unlike the heightmap
    # legal arguments pass every check and reach the engine, which a CPU trainer does not have
    with pytest.raises(RuntimeError):
        rl.best_rotation_map(d, d, style=1, is_target=True)
    with pytest.raises(RuntimeError):
        rl.best_rotation_object_maps(d, m, on_object=False)
    with pytest.raises(RuntimeError):
        re.best_rotation_class_map(d, d, cls=2)
    with pytest.raises(RuntimeError):
        re.best_rotation_class_object_maps(d, m, style=1, cls=1)
