"""CPU-side checks of the K-best-per-object scene-frame interface (no GPU): the C ABI declares and exports smg_scene_topk_objects
and smg_scene_class_topk_objects and the binding carries them, the greedy numpy restatement of tests/scene_topk_ref.py agrees with a
brute-force loop, the Trainer methods refuse before they touch an engine, and the K / radius cases of tests/test_gpu_scene_topk.py
fill the ranks that module says they fill."""
import numpy as np
import pytest

from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_objects_ref
import scene_ref
import scene_topk_ref
import test_gpu_scene_topk as gpu_side

TAIL = (r"const double\*\s*masks_dev,\s*int n_masks,\s*const int\*\s*map_mask_a,\s*const int\*\s*map_mask_b,\s*const int\*\s*map_group,\s*"
        r"int n_groups,\s*int K,\s*int radius,\s*int\*\s*idx_out_dev,\s*float\*\s*val_out_dev,\s*void\*\s*stream\)")


def test_both_exports_are_declared_exported_and_bound():
    hdr = assert_declared_exported_and_bound(
        "smg_scene_topk_objects",
        r"\bint\s+smg_scene_topk_objects\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int64_t map_stride,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*" + TAIL,
        17, "scene_topk_objects", ["ranked_scene_actions", "ranked_to_best"])
    assert_declared_exported_and_bound(
        "smg_scene_class_topk_objects",
        r"\bint\s+smg_scene_class_topk_objects\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*int cls,\s*" + TAIL,
        17, "scene_class_topk_objects", ["ranked_scene_class_actions"])
    for word in ("radius^2", "(-1, -inf)", "K > 32", "radius < 0", "n_groups * K beyond int32", "bit for bit"):
        assert word in hdr, word


def better(v, flat, best, at):
    """argmax_better's comparison: a NaN wins, then the larger value, then the lower flattened index."""
    if at < 0:
        return True
    if np.isnan(v) != np.isnan(best):
        return bool(np.isnan(v))
    if np.isnan(v):
        return flat < at
    return v > best or (v == best and flat < at)


def brute_force(maps, masks, mask_a, mask_b, groups, n_groups, K, radius):
    """The rules spelled out pixel by pixel: every rank walks every (map, pixel) of the group and tests it against every earlier pick."""
    n_maps, hm, _ = maps.shape
    out = []
    for g in range(n_groups):
        picks = []
        for _ in range(K):
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
                        if any((iy - (p % (hm * hm)) // hm) ** 2 + (ix - p % hm) ** 2 <= radius * radius for p, _ in picks):
                            continue
                        flat = (m * hm + iy) * hm + ix
                        if better(v, flat, best, at):
                            best, at = v, flat
            picks.append((at, best))
        out.append(picks)
    return out


def toy():
    """test_cpu_scene_objects.py's toy: 6 x 6 maps, 7 maps in 4 groups that are not contiguous, ties (small integers), a NaN,
    invalid pixels, mask values -0.0 / NaN / 0.5, a union, the every-pixel form, a group whose mask selects invalid pixels only
    and a group without a map."""
    rng = np.random.default_rng(3)
    hm, n_maps = 6, 7
    maps = rng.integers(-3, 4, size=(n_maps, hm, hm)).astype(np.float32)
    maps[:, 0, :] = -np.inf
    maps[2, 3:, 3:] = -np.inf
    maps[4, 2, 2] = np.nan
    masks = np.zeros((4, hm, hm))
    masks[0, 1:3, 1:4] = 1.0
    masks[1, 2:5, 2:6] = -1.0
    masks[1, 3, 3] = -0.0
    masks[1, 4, 4] = np.nan
    masks[2, 0, :] = 0.5
    masks[3, 5, 5] = 2.0
    return maps, masks, [0, 1, 0, 2, 1, -1, 3], [-1, -1, 1, -1, 0, -1, -1], [0, 1, 0, 2, 1, 4, 1]


def separated_and_descending(idx, val, hm, radius):
    for g in range(idx.shape[0]):
        have = [j for j in range(idx.shape[1]) if idx[g, j] >= 0]
        assert have == list(range(len(have)))                      # a -1 is followed by -1 only
        assert np.isneginf(val[g, len(have):]).all()
        pix = [divmod(int(idx[g, j]) % (hm * hm), hm) for j in have]
        for a in range(len(pix)):
            for b in range(a):
                assert (pix[a][0] - pix[b][0]) ** 2 + (pix[a][1] - pix[b][1]) ** 2 > radius * radius
        v = [val[g, j] for j in have if not np.isnan(val[g, j])]
        assert all(v[j + 1] <= v[j] for j in range(len(v) - 1))   # values never increase with rank, NaNs aside
        nan = [j for j in have if np.isnan(val[g, j])]
        assert nan == list(range(len(nan)))                        # the NaNs come first


@pytest.mark.parametrize("K,radius", ((1, 0), (4, 0), (5, 1), (3, 2), (6, 9)))
def test_helper_against_a_brute_force_loop_on_a_toy(K, radius):
    """(Validates the REFERENCE, tests/scene_topk_ref.py, not the product.)"""
    maps, masks, mask_a, mask_b, groups = toy()
    idx, val = scene_topk_ref.group_topk(maps, masks, mask_a, mask_b, groups, 5, K, radius)
    ref = brute_force(maps, masks, mask_a, mask_b, groups, 5, K, radius)
    for g in range(5):
        print("group %d: helper %s, brute force %s" % (g, list(zip(idx[g].tolist(), val[g].tolist())), ref[g]))
        for j in range(K):
            assert idx[g, j] == ref[g][j][0]
            assert np.asarray(val[g, j]).view(np.uint32) == np.asarray(ref[g][j][1], dtype=np.float32).view(np.uint32)
    separated_and_descending(idx, val, 6, radius)
    # rank 0, and the whole K = 1 call, are scene_objects_ref.group_argmax
    i0, v0 = scene_objects_ref.group_argmax(maps, masks, mask_a, mask_b, groups, 5)
    assert np.array_equal(idx[:, 0], i0) and np.array_equal(val[:, 0].view(np.uint32), v0.view(np.uint32))
    assert (idx[2] == -1).all() and (idx[3] == -1).all() and np.isneginf(val[2:4]).all()      # invalid pixels only; no map
    assert np.isnan(val[1, 0]) and idx[1, 0] == (4 * 6 + 2) * 6 + 2                           # the NaN of map 4 wins rank 0 of its group
    if radius == 9:
        assert (idx[:, 1:] == -1).all()                            # the disc covers the 6 x 6 image: every group is exhausted after rank 0
    if (K, radius) == (4, 0):
        # radius 0 removes the picked PIXEL in every map of the group: group 1's ranks are four different pixels
        assert len({int(i) % 36 for i in idx[1]}) == 4
        # group 4 is one map with every pixel selected: the ranks are its four largest values in np.argsort's stable order
        order = np.argsort(-maps[5].ravel(), kind="stable")[:4]
        assert [int(i) - 5 * 36 for i in idx[4]] == order.tolist()


def test_a_tie_takes_the_lowest_index_then_the_next_outside_the_disc():
    maps = np.full((2, 5, 5), 0.25, dtype=np.float32)
    masks = np.ones((1, 5, 5))
    idx, val = scene_topk_ref.group_topk(maps, masks, [0, 0], [-1, -1], [0, 0], 1, 4, 2)
    assert [divmod(int(i), 25) for i in idx[0]] == [(0, 0), (0, 3), (0, 11), (0, 14)] and (val == np.float32(0.25)).all()
    idx, _ = scene_topk_ref.group_topk(maps, masks, [0, 0], [-1, -1], [0, 0], 1, 3, 0)
    assert idx[0].tolist() == [0, 1, 2]                            # never pixel 0 of the second map


def test_trainer_methods_refuse_before_the_engine():
    # (on a CPU trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    d, m = np.zeros((240, 240)), np.ones((2, 240, 240))
    d224, m224 = np.zeros((224, 224)), np.ones((2, 224, 224))                   # S = 640: a 1 x 1 map has no extent
    rl, re = cpu_trainer('reinforcement'), cpu_trainer('reactive')
    with pytest.raises(ValueError):
        re.ranked_scene_actions(d, m, 2, 1)
    with pytest.raises(ValueError):
        rl.ranked_scene_class_actions(d, m, 2, 1)
    with pytest.raises(ValueError):
        rl.ranked_scene_actions(d224, m224, 2, 1)
    with pytest.raises(ValueError):
        re.ranked_scene_class_actions(d224, m224, 2, 1)
    with pytest.raises(ValueError):
        re.ranked_scene_class_actions(d, m, 2, 1, cls=3)
    for k, radius in ((0, 1), (33, 1), (2, -1), (2.5, 1)):
        with pytest.raises(ValueError):
            rl.ranked_scene_actions(d, m, k, radius)
        with pytest.raises(ValueError):
            re.ranked_scene_class_actions(d, m, k, radius)
    # legal arguments pass every check and reach the engine, which a CPU trainer does not have
    with pytest.raises(RuntimeError):
        rl.ranked_scene_actions(d, m, 32, 0)
    with pytest.raises(RuntimeError):
        re.ranked_scene_class_actions(d, m, 1, 7)


def test_ranked_to_best():
    from trainer import Trainer
    ranked = {"grasp": [(2, 3, (10, 11), 0.9), (2, 1, (30, 11), 0.7)], "suction": [], "pairs": [((0, 2), (5, 6), 0.4)]}
    best = Trainer.ranked_to_best({"ranked": ranked, "per_object": {}}, "grasp", 1)
    assert best == dict(bestg_id=(2, 1), bestg_pixel=(30, 11), bestg_conf=0.7, bests_id=None, bests_pixel=None, bests_conf=-np.inf,
                        bestgs_num=None, bestgs_pixel=None, bestgs_conf=0)
    depth, masks = np.ones((40, 40)), np.stack([np.full((40, 40), float(k + 1)) for k in range(3)])
    m, style, rot, pixel = Trainer._scene_action("test", best, "grasp", depth, masks)
    assert (style, rot, pixel) == (0, 1, (30, 11)) and (m == 3.0).all()
    pair = Trainer.ranked_to_best(ranked, "grasp_then_suction", 0)
    assert (pair["bestgs_num"], pair["bestgs_pixel"], pair["bestgs_conf"], pair["bestg_id"]) == ((0, 2), (5, 6), 0.4, None)
    m, style, rot, pixel = Trainer._scene_action("test", pair, "grasp_then_suction", depth, masks)
    assert (style, rot, pixel) == (2, 0, (5, 6)) and (m == 4.0).all()
    for action, j in (("suction", 0), ("grasp", 2), ("grasp", -1), ("push", 0)):
        with pytest.raises(ValueError):
            Trainer.ranked_to_best(ranked, action, j)


@pytest.mark.parametrize("hm,S,side", gpu_side.SHAPES)
def test_the_gpu_cases_fill_the_ranks_they_claim(hm, S, side):
    """tests/test_gpu_scene_topk.py's main case - 80 maps, rotation-major, test_gpu_scene_objects.py's rectangles - on
    scene_ref.scene_maps of the same seeded maps: for every (K, radius) of CASES the centre, straddling and whole-image masks
    fill every rank, the one-pixel mask is exhausted after rank 0 and the mask without a window has no rank at all.  So the GPU
    test cannot pass on empty ranks, and its exhaustion case has a -1 tail to write."""
    assert scene_ref.geometry(hm)[1:] == (S, side)
    aff16 = gpu_side.affines()
    q16 = np.random.default_rng(S + 3).standard_normal((16, side, side)).astype(np.float32)
    maps16 = scene_ref.scene_maps(q16, aff16, hm)[0].astype(np.float32)
    masks = gpu_side.rect_masks(hm)
    rep = np.repeat(np.arange(16), 5)
    for K, radius in gpu_side.CASES:
        idx, val = scene_topk_ref.group_topk(maps16[rep], masks, n_groups=5, K=K, radius=radius, **gpu_side.ALL80)
        print("hm %d K %d radius %d: ranks filled per group %s" % (hm, K, radius, (idx >= 0).sum(1).tolist()))
        assert (idx[[gpu_side.CENTRE, gpu_side.STRADDLE, gpu_side.WHOLE]] >= 0).all()
        assert idx[gpu_side.ONE, 0] >= 0 and (idx[gpu_side.ONE, 1:] == -1).all()
        assert (idx[gpu_side.OUTSIDE] == -1).all()
        separated_and_descending(idx, val, hm, radius)
        assert len({int(i) // (hm * hm) // 5 for i in idx[gpu_side.WHOLE]}) > 1 or K < 32
