"""numpy restatement of smg_scene_argmax_objects' selection and grouping (include/smg_hip.h), the reference of
tests/test_cpu_scene_objects.py and tests/test_gpu_scene_objects.py.  Plain helper module, no tests.

It starts from scene-frame maps that already exist - smg_scene_maps' output, or scene_ref.scene_maps' - so the geometry is not
restated here: what is restated is which pixels a map sees and how the maps of a group compete."""
import numpy as np


def selected(masks, a, b):
    """bool [hm, hm]: the pixels mask terms a / b select - not exactly 0 (so -0.0 does not select and a NaN does); index -1 = no
    such term, both -1 = every pixel."""
    masks = np.asarray(masks)
    if a < 0 and b < 0:
        return np.ones(masks.shape[1:], dtype=bool)
    sel = np.zeros(masks.shape[1:], dtype=bool)
    for t in (a, b):
        if t >= 0:
            sel |= masks[t] != 0
    return sel


def group_argmax(maps, masks, mask_a, mask_b, groups, n_groups):
    """maps float32 [n_maps, hm, hm] (-inf = invalid), masks [n_masks, hm, hm], mask_a / mask_b / groups n_maps ints each ->
    (idx int64 [n_groups], val float32 [n_groups]): per group np.argmax (lowest index on ties, the first NaN wins) over the
    selected valid pixels of the group's maps, as a flattened index into [n_maps, hm, hm]; (-1, -inf) for a group with no map or
    no selected valid pixel."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.ndim == 3
    n_maps, npix = maps.shape[0], maps.shape[1] * maps.shape[2]
    assert len(mask_a) == len(mask_b) == len(groups) == n_maps
    idx = np.full(n_groups, -1, dtype=np.int64)
    val = np.full(n_groups, -np.inf, dtype=np.float32)
    for g in range(n_groups):
        cand_i, cand_v = [], []
        for m in range(n_maps):
            if groups[m] != g:
                continue
            see = (selected(masks, mask_a[m], mask_b[m]) & ~np.isneginf(maps[m])).ravel()
            at = np.flatnonzero(see)
            cand_i.append(m * npix + at)
            cand_v.append(maps[m].ravel()[at])
        if cand_i and sum(len(c) for c in cand_i):
            ci, cv = np.concatenate(cand_i), np.concatenate(cand_v)
            k = int(np.argmax(cv))              # candidates are in ascending flattened order: the lowest index on ties
            idx[g], val[g] = ci[k], cv[k]
    return idx, val
