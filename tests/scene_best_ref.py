"""numpy restatement of smg_scene_best_maps' / smg_scene_class_best_maps' collapse (include/smg_hip.h), the reference of
tests/test_cpu_scene_best_maps.py and tests/test_gpu_scene_best_maps.py.  Plain helper module, no tests.

Like scene_objects_ref it starts from scene-frame maps that already exist - smg_scene_maps' (smg_scene_class_maps') output, or
scene_ref.scene_maps' - so the geometry is not restated here: what is restated is which pixels a map sees and how the maps of a group
compete at one pixel."""
import numpy as np

from scene_objects_ref import selected


def group_best(maps, masks, mask_a, mask_b, groups, n_groups):
    """maps float32 [n_maps, hm, hm] (-inf = no window), masks [n_masks, hm, hm] or None (every term must then be -1), mask_a /
    mask_b / groups n_maps ints each -> (val float32 [n_groups, hm, hm], arg int32 [n_groups, hm, hm]): per group and pixel
    np.argmax (the lowest map on ties, the first NaN wins) over the group's maps in call order, a map counting at a pixel only
    where its mask terms select it (the bit-pattern rule: not exactly 0) and it is not -inf there; (-inf, -1) where no map counts."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.ndim == 3
    n_maps, hm = maps.shape[0], maps.shape[1]
    assert len(mask_a) == len(mask_b) == len(groups) == n_maps
    if masks is None:
        assert all(a < 0 for a in mask_a) and all(b < 0 for b in mask_b)
        masks = np.zeros((0, hm, hm))
    val = np.full((n_groups, hm, hm), -np.inf, dtype=np.float32)
    arg = np.full((n_groups, hm, hm), -1, dtype=np.int32)
    for g in range(n_groups):
        mine = [m for m in range(n_maps) if groups[m] == g]
        if not mine:
            continue
        stack = np.stack([np.where(selected(masks, mask_a[m], mask_b[m]), maps[m], np.float32(-np.inf)) for m in mine])
        k = np.argmax(stack, axis=0)                    # the first NaN, else the first of the largest
        v = np.take_along_axis(stack, k[None], axis=0)[0]
        have = ~np.isneginf(v)                          # (a NaN is not -inf: it counts)
        val[g] = v
        arg[g] = np.where(have, np.asarray(mine, dtype=np.int32)[k], -1)
    return val, arg
