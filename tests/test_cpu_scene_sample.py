"""CPU-side checks of the Boltzmann exploration interface (no GPU): the C ABI declares and exports smg_scene_sample_objects and
smg_scene_class_sample_objects and the binding carries them; the noise of tests/scene_sample_ref.py is the stated hash (its mix is
synthetic._splitmix64 bit for bit, u is exact at both ends); group_sample agrees with a brute-force loop; draw d does not depend on
n_draws; a large beta gives scene_objects_ref.group_argmax; 4096 draws follow softmax(beta v) by Pearson's chi^2 (and do not follow
beta / 2 or 2 beta); the comparison rule skips no draw of the inputs of tests/test_gpu_scene_sample.py; and the Trainer methods
refuse before they touch an engine."""
import numpy as np
import pytest

from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_objects_ref
import scene_ref
import scene_sample_ref
import test_gpu_scene_sample as gpu_side

TAIL = (r"const double\*\s*masks_dev,\s*int n_masks,\s*const int\*\s*map_mask_a,\s*const int\*\s*map_mask_b,\s*const int\*\s*map_group,\s*"
        r"int n_groups,\s*int n_draws,\s*double beta,\s*uint64_t seed,\s*int\*\s*idx_out_dev,\s*float\*\s*val_out_dev,\s*void\*\s*stream\)")


def test_both_exports_are_declared_exported_and_bound():
    hdr = assert_declared_exported_and_bound(
        "smg_scene_sample_objects",
        r"\bint\s+smg_scene_sample_objects\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int64_t map_stride,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*" + TAIL,
        18, "scene_sample_objects", ["sampled_scene_actions", "ranked_to_best"])
    assert_declared_exported_and_bound(
        "smg_scene_class_sample_objects",
        r"\bint\s+smg_scene_class_sample_objects\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*int cls,\s*" + TAIL,
        18, "scene_class_sample_objects", ["sampled_scene_class_actions"])
    for word in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "(h >> 12) + 0.5", "-log(-log(u))", "fma(beta, (double) v, G)",
                 "(-1, -inf)", "n_draws > 32", "n_groups * n_draws beyond int32", "negative, NaN or infinite", "Draw d does not depend on n_draws"):
        assert word in hdr, word


def test_the_noise_is_the_stated_hash():
    import synthetic
    x = np.concatenate([np.arange(5, dtype=np.uint64), np.asarray([2 ** 64 - 1, 2 ** 63, 0x0123456789ABCDEF], dtype=np.uint64),
                        np.random.default_rng(0).integers(0, 2 ** 64, size=1000, dtype=np.uint64)])
    assert np.array_equal(scene_sample_ref.mix(x), synthetic._splitmix64(x))
    # mix(0) against the finaliser written out in Python integers
    z = 0x9E3779B97F4A7C15
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert int(scene_sample_ref.mix(np.uint64(0))) == z ^ (z >> 31)
    # u is exact at the ends and strictly inside (0, 1); G is finite there
    ends = scene_sample_ref.unit(np.asarray([0, 2 ** 64 - 1], dtype=np.uint64))
    assert ends[0] == 2.0 ** -53 and ends[1] == 1.0 - 2.0 ** -53 and 0.0 < ends[0] and ends[1] < 1.0
    g_ends = -np.log(-np.log(ends))
    print("G at the ends of u: %.4f, %.4f" % (g_ends[0], g_ends[1]))
    assert np.isfinite(g_ends).all() and -3.62 < g_ends[0] < -3.60 and 36.73 < g_ends[1] < 36.75
    # the counter: seed, draw and index enter as seed + (d << 32) + i mod 2^64
    seed, d, flat = 2 ** 64 - 5, 3, np.asarray([0, 7, 2 ** 31 - 1])
    x = np.asarray([(seed + (d << 32) + int(i)) % 2 ** 64 for i in flat], dtype=np.uint64)
    want = -np.log(-np.log(scene_sample_ref.unit(scene_sample_ref.mix(scene_sample_ref.mix(x)))))
    assert np.array_equal(scene_sample_ref.gumbel(seed, d, flat), want)
    G = scene_sample_ref.gumbel(1, 0, np.arange(100000))
    assert np.isfinite(G).all() and abs(G.mean() - 0.5772) < 0.02 and abs(G.var() - np.pi ** 2 / 6) < 0.05      # a standard Gumbel's moments
    s = scene_sample_ref.scores(np.asarray([1.5, np.nan], dtype=np.float32), 3.0, 1, 0, np.asarray([4, 5]))
    assert s.dtype == np.float32 and s[0] == np.float32(4.5 + G[4]) and np.isnan(s[1])


def better(v, flat, best, at):
    """argmax_better's comparison: a NaN wins, then the larger value, then the lower flattened index."""
    if at < 0:
        return True
    if np.isnan(v) != np.isnan(best):
        return bool(np.isnan(v))
    if np.isnan(v):
        return flat < at
    return v > best or (v == best and flat < at)


def brute_force(maps, masks, mask_a, mask_b, groups, n_groups, n_draws, beta, seed):
    """The rules spelled out candidate by candidate: every draw walks every (map, pixel) of the group, hashes its own flattened
    index and keeps the best score by argmax_better's rules."""
    n_maps, hm, _ = maps.shape
    out = []
    for g in range(n_groups):
        picks = []
        for d in range(n_draws):
            best, at, held = np.float32(-np.inf), -1, np.float32(-np.inf)
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
                        sc = scene_sample_ref.scores(np.asarray([v], dtype=np.float32), beta, seed, d, np.asarray([flat]))[0]
                        if better(sc, flat, best, at):
                            best, at, held = sc, flat, v
            picks.append((at, held))
        out.append(picks)
    return out


def toy():
    """test_cpu_scene_objects.py's toy: 6 x 6 maps, 7 maps in 4 groups that are not contiguous, small integers, a NaN, invalid
    pixels, mask values -0.0 / NaN / 0.5, a union, the every-pixel form, a group whose mask selects invalid pixels only and a
    group without a map."""
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


@pytest.mark.parametrize("n_draws,beta,seed", ((1, 0.0, 0), (5, 3.0, 7), (3, 0.75, 2 ** 64 - 1)))
def test_helper_against_a_brute_force_loop_on_a_toy(n_draws, beta, seed):
    """(Validates the REFERENCE, tests/scene_sample_ref.py, not the product.)"""
    maps, masks, mask_a, mask_b, groups = toy()
    idx, val, gap = scene_sample_ref.group_sample(maps, masks, mask_a, mask_b, groups, 5, n_draws, beta, seed)
    ref = brute_force(maps, masks, mask_a, mask_b, groups, 5, n_draws, beta, seed)
    for g in range(5):
        print("group %d: helper %s, brute force %s, gaps %s" % (g, list(zip(idx[g].tolist(), val[g].tolist())), ref[g], gap[g].tolist()))
        for d in range(n_draws):
            assert idx[g, d] == ref[g][d][0]
            assert np.asarray(val[g, d]).view(np.uint32) == np.asarray(ref[g][d][1], dtype=np.float32).view(np.uint32)
    assert (idx[2] == -1).all() and (idx[3] == -1).all() and np.isneginf(val[2:4]).all()      # invalid pixels only; no map
    assert np.isnan(val[1]).all() and (idx[1] == (4 * 6 + 2) * 6 + 2).all()                   # the NaN of map 4 wins every draw of its group
    assert (gap[[0, 4]] > 0).all() and np.isinf(gap[1:4]).all()
    _, _, gap2, s1, s2 = scene_sample_ref.group_sample_scores(maps, masks, mask_a, mask_b, groups, 5, n_draws, beta, seed)
    assert np.array_equal(gap2, gap) and np.isnan(s1[1]).all() and scene_sample_ref.compared(gap, s1, s2)[1:4].all()      # a NaN's win hangs on no rounding
    if beta == 0.0:
        # beta = 0: uniform over the candidates, whatever their values - the argmax of the noise alone
        for g in (0, 4):
            cand = np.concatenate([m * 36 + np.flatnonzero((scene_objects_ref.selected(masks, mask_a[m], mask_b[m]) & ~np.isneginf(maps[m])).ravel())
                                   for m in range(7) if groups[m] == g])
            assert idx[g, 0] == cand[int(np.argmax(scene_sample_ref.gumbel(seed, 0, cand).astype(np.float32)))]


def test_a_draw_does_not_depend_on_the_number_of_draws():
    maps, masks, mask_a, mask_b, groups = toy()
    i8, v8, g8 = scene_sample_ref.group_sample(maps, masks, mask_a, mask_b, groups, 5, 8, 3.0, 11)
    i3, v3, g3 = scene_sample_ref.group_sample(maps, masks, mask_a, mask_b, groups, 5, 3, 3.0, 11)
    assert np.array_equal(i3, i8[:, :3]) and np.array_equal(v3.view(np.uint32), v8[:, :3].view(np.uint32)) and np.array_equal(g3, g8[:, :3])
    other = scene_sample_ref.group_sample(maps, masks, mask_a, mask_b, groups, 5, 8, 3.0, 12)[0]
    assert (other != i8).any()
    assert len({int(i) for i in i8[4]}) > 1                        # the draws of a group differ from one another


def test_a_large_beta_is_the_argmax():
    """beta (v1 - v2) > 41, the width of G's range (40.35) rounded up: the noise cannot reorder the two best values, so every draw
    is scene_objects_ref.group_argmax.  The toy's values are distinct multiples of 1/8 per group here (a tie would be decided by
    the noise), and beta = 512 keeps beta |v| below 2^16, where a float32 score still resolves 2^-7."""
    maps, masks, mask_a, mask_b, groups = toy()
    maps = np.where(np.isfinite(maps), np.random.default_rng(4).permutation(7 * 36).reshape(7, 6, 6) * 0.125, maps).astype(np.float32)
    beta = 512.0
    assert beta * 0.125 > 41
    idx, val, gap = scene_sample_ref.group_sample(maps, masks, mask_a, mask_b, groups, 5, 16, beta, 5)
    bi, bv = scene_objects_ref.group_argmax(maps, masks, mask_a, mask_b, groups, 5)
    for d in range(16):
        assert np.array_equal(idx[:, d], bi) and np.array_equal(val[:, d].view(np.uint32), bv.view(np.uint32))
    assert (gap[[0, 1, 4]] > 41 - 40.35).all()


def test_distribution_of_4096_draws():
    """The distribution case of tests/test_gpu_scene_sample.py on scene_ref.scene_maps: hm = 240 (S = 704, 3 x 3 maps), 32 maps
    with identical q and rotation 0, each its own group, one mask = the 10 x 10 box of rows and columns 115 .. 124; 32 draws x 4
    seeds = 4096 draws of a pixel.  Pearson's chi^2 against softmax(beta v) in float64, bins merged in ascending probability until
    each expects >= 5, must lie below df + 4 sqrt(2 df) for beta = 0 and beta = 3; against beta / 2 and 2 beta it must lie above."""
    hm = gpu_side.DIST_HM
    assert scene_ref.geometry(hm)[1:] == (704, 3)
    aff = np.tile(scene_ref.theta(0, 16), (32, 1))
    maps, valid, _ = scene_ref.scene_maps(np.tile(gpu_side.dist_q(), (32, 1, 1)), aff, hm)
    maps = maps.astype(np.float32)
    lo, hi = gpu_side.DIST_BOX
    assert (lo, hi) == (115, 125) and valid[:, lo:hi, lo:hi].all()                # the box is valid
    masks = gpu_side.dist_mask()
    v = maps[0, lo:hi, lo:hi].ravel()
    print("values on the box: %.4f .. %.4f" % (v.min(), v.max()))
    for beta in gpu_side.DIST_BETAS:
        picks, skipped = [], 0
        for seed in gpu_side.DIST_SEEDS:
            idx, val, gap, s1, s2 = scene_sample_ref.group_sample_scores(maps, masks, n_draws=32, beta=beta, seed=seed, **gpu_side.DIST)
            skipped += int((~scene_sample_ref.compared(gap, s1, s2)).sum())
            picks.append(idx)
        assert skipped * 1000 <= 4096
        gpu_side.assert_distribution(gpu_side.dist_counts(picks), v, beta, "restatement")


@pytest.mark.parametrize("hm", (240, 239))
def test_the_rule_skips_no_draw_of_the_gpu_cases(hm):
    """tests/test_gpu_scene_sample.py's picks case on scene_ref.scene_maps of the same seeded maps: the groups it says have
    candidates have them, the comparison rule compares every draw (the cap is 1 in 1000), and the picks come from both launches."""
    aff = gpu_side.picks_affines()
    masks = gpu_side.masks_for(hm)
    total = skipped = 0
    for q_seed, n_draws, beta, seed in ((hm, gpu_side.PICKS_DRAWS, gpu_side.PICKS_BETA, gpu_side.SEED), (1, 32, 0.0, gpu_side.SEED + 1),
                                        (3, 8, gpu_side.PICKS_BETA, gpu_side.SEED)):
        maps = scene_ref.scene_maps(gpu_side.picks_q(q_seed), aff, hm)[0].astype(np.float32)
        idx, val, gap, s1, s2 = scene_sample_ref.group_sample_scores(maps, masks, n_draws=n_draws, beta=beta, seed=seed, **gpu_side.PICKS)
        cmp = scene_sample_ref.compared(gap, s1, s2)
        with np.errstate(invalid="ignore"):
            rel = np.where(np.isfinite(gap), gap / np.maximum(np.abs(s1), np.abs(s2)), np.inf)
        print("hm %d q %d beta %g: %d draws, %d not compared, smallest relative gap %.3g" % (hm, q_seed, beta, cmp.size, int((~cmp).sum()), rel.min()))
        total += cmp.size
        skipped += int((~cmp).sum())
        assert (idx[[0, 1, 3]] >= 0).all() and (idx[[2, 4]] == -1).all()
        assert {bool(int(i) // (hm * hm) >= 32) for i in idx[[0, 1, 3]].ravel()} == {False, True}
        assert np.isinf(gap[[2, 4]]).all() and np.isfinite(gap[[0, 1, 3]]).all()
    assert skipped * 1000 <= total


def test_trainer_methods_refuse_before_the_engine():
    # (on a CPU trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    d, m = np.zeros((240, 240)), np.ones((2, 240, 240))
    d224, m224 = np.zeros((224, 224)), np.ones((2, 224, 224))                   # S = 640: a 1 x 1 map has no extent
    rl, re = cpu_trainer('reinforcement'), cpu_trainer('reactive')
    with pytest.raises(ValueError):
        re.sampled_scene_actions(d, m, 2, 1.0, 0)
    with pytest.raises(ValueError):
        rl.sampled_scene_class_actions(d, m, 2, 1.0, 0)
    with pytest.raises(ValueError):
        rl.sampled_scene_actions(d224, m224, 2, 1.0, 0)
    with pytest.raises(ValueError):
        re.sampled_scene_class_actions(d224, m224, 2, 1.0, 0)
    with pytest.raises(ValueError):
        re.sampled_scene_class_actions(d, m, 2, 1.0, 0, cls=3)
    for n_draws, temperature, seed in ((0, 1.0, 0), (33, 1.0, 0), (2.5, 1.0, 0), (2, 0.0, 0), (2, -0.5, 0), (2, float("nan"), 0), (2, float("-inf"), 0),
                                       (2, 1.0, -1), (2, 1.0, 2 ** 64), (2, 1.0, 1.5)):
        with pytest.raises(ValueError):
            rl.sampled_scene_actions(d, m, n_draws, temperature, seed)
        with pytest.raises(ValueError):
            re.sampled_scene_class_actions(d, m, n_draws, temperature, seed)
    # legal arguments pass every check and reach the engine, which a CPU trainer does not have
    with pytest.raises(RuntimeError):
        rl.sampled_scene_actions(d, m, 32, float("inf"), 2 ** 64 - 1, joint=True)
    with pytest.raises(RuntimeError):
        re.sampled_scene_class_actions(d, m, 1, 0.01, 0)
    from trainer import Trainer
    assert Trainer._style_seed(2 ** 64 - 1, 0) == 2 ** 64 - 1 and Trainer._style_seed(2 ** 64 - 1, 2) == (2 ** 64 - 1 + 2 * 0x9E3779B97F4A7C15) % 2 ** 64
    assert Trainer._require_draws("t", 3, float("inf"), 5) == (3, 0.0, 5) and Trainer._require_draws("t", 32, 0.25, 0) == (32, 4.0, 0)
