"""numpy restatement of smg_scene_topk_objects' greedy rule (include/smg_hip.h), the reference of tests/test_cpu_scene_topk.py and
tests/test_gpu_scene_topk.py.  Plain helper module, no tests.

Like scene_objects_ref it starts from scene-frame maps that already exist - smg_scene_maps' output, a plane of
smg_scene_class_maps', or scene_ref.scene_maps' - and reuses scene_objects_ref.selected: what is restated here is the ranks.  Rank
j of a group is np.argmax (the first NaN wins, the lowest flattened index on ties) over the group's selected valid pixels whose
HEIGHTMAP pixel (iy, ix) - in whichever map of the group - lies farther than `radius` from every earlier pick of the group:
(iy - py)^2 + (ix - px)^2 > radius^2 in integers.  When nothing is left the rank and all later ones are (-1, -inf)."""
import numpy as np

from scene_objects_ref import selected


def group_topk(maps, masks, mask_a, mask_b, groups, n_groups, K, radius):
    """maps float32 [n_maps, hm, hm] (-inf = invalid), masks [n_masks, hm, hm], mask_a / mask_b / groups n_maps ints each ->
    (idx int64 [n_groups, K], val float32 [n_groups, K]), the index flattened into [n_maps, hm, hm]."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.ndim == 3 and K >= 1 and radius >= 0
    n_maps, hm = maps.shape[0], maps.shape[1]
    npix = hm * maps.shape[2]
    assert len(mask_a) == len(mask_b) == len(groups) == n_maps
    idx = np.full((n_groups, K), -1, dtype=np.int64)
    val = np.full((n_groups, K), -np.inf, dtype=np.float32)
    for g in range(n_groups):
        cand_i, cand_v = [], []
        for m in range(n_maps):
            if groups[m] != g:
                continue
            at = np.flatnonzero((selected(masks, mask_a[m], mask_b[m]) & ~np.isneginf(maps[m])).ravel())
            cand_i.append(m * npix + at)
            cand_v.append(maps[m].ravel()[at])
        if not cand_i:
            continue
        ci, cv = np.concatenate(cand_i), np.concatenate(cand_v)       # ascending flattened order: np.argmax takes the lowest on ties
        cy, cx = (ci % npix) // hm, ci % hm
        for j in range(K):
            if not len(ci):
                break
            k = int(np.argmax(cv))
            idx[g, j], val[g, j] = ci[k], cv[k]
            keep = (cy - cy[k]) ** 2 + (cx - cx[k]) ** 2 > int(radius) ** 2
            ci, cv, cy, cx = ci[keep], cv[keep], cy[keep], cx[keep]
    return idx, val
