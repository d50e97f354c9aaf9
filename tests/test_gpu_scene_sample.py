"""Boltzmann exploration per object in the scene frame on the MI355X (run with -m gpu): smg_scene_sample_objects and
smg_scene_class_sample_objects on an engine alone with seeded maps fed directly - smg_scene_maps' (smg_scene_class_maps') own output,
masked on the host and pushed through the numpy restatement of tests/scene_sample_ref.py, must give the kernels' picks (index equal,
value bit for bit the map at that index) wherever that module's comparison rule compares a draw - then the limits beta = 0 and
beta -> argmax, the distribution of 4096 draws against softmax(beta v), determinism and independence of n_draws, a NaN, every
refusal, and Trainer.sampled_scene_actions / sampled_scene_class_actions against the maps they kept.  The inputs (PICKS, the
distribution case) are also run through the restatement alone by tests/test_cpu_scene_sample.py, which shows that no draw of them is
skipped by the rule and that the chosen seeds pass the chi^2 bound for the restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

from map_harness import assert_bit_identical, bits, cached_engine, filled, gpu, make_trainer, own_engine, stream  # noqa: F401

import scene_objects_ref
import scene_ref
import scene_sample_ref
import test_gpu_scene_class_objects as class_plane
import test_gpu_scene_objects as one_plane

pytestmark = pytest.mark.gpu

S, SIDE = 704, 3                         # hm = 240 and hm = 239 both pad to S = 704: 3 x 3 maps
CENTRE, STRADDLE, OUTSIDE, ONE, WHOLE = range(5)
affines = one_plane.affines
SEED = 0x0123456789ABCDEF

# The picks case: 40 maps = two launches of 32 + 8, map m has rotation m % 16 and a map of its own.  Groups 0 .. 3 take every
# fourth map - not contiguous, each split by the launch boundary -, group 4 has no map.  Group 0 sees the union of two mask
# terms, group 1 one rectangle, group 2 a mask without a valid pixel, group 3 (term b alone) a single pixel: ten lone candidates.
PICKS = dict(mask_a=[(CENTRE, STRADDLE, OUTSIDE, -1)[m % 4] for m in range(40)], mask_b=[(STRADDLE, -1, -1, ONE)[m % 4] for m in range(40)],
             groups=[m % 4 for m in range(40)], n_groups=5)
PICKS_DRAWS, PICKS_BETA = 8, 3.0


def picks_q(seed, planes=None):
    """Seeded maps of the picks case; the eight maps of the second launch lie 1.0 higher, so that at beta = 3 a group's two maps
    there weigh about as much as its eight of the first launch and the draws come from both."""
    shape = (40, SIDE, SIDE) if planes is None else (40, planes, SIDE, SIDE)
    q = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    if planes is None:
        q[32:] += np.float32(1.0)
    return q


def picks_affines():
    return affines()[np.arange(40) % 16]


def masks_for(hm):
    """test_gpu_scene_objects.py's five masks; at hm = 239 its rectangles of 240 with the one-pixel mask kept inside the window."""
    m = np.zeros((5, hm, hm))
    for k, (_, (y0, y1, x0, x1), _) in enumerate(one_plane.RECTS[240]):
        m[k, y0:y1, x0:x1] = 1.0
    m[WHOLE] = 1.0
    return m


# The distribution case: 32 maps with identical q and rotation 0, each its own group, one mask = the 10 x 10 box of rows and
# columns 115 .. 124; 32 draws x 4 seeds = 4096 draws of a pixel of the box.
DIST_HM, DIST_BOX, DIST_SEEDS, DIST_BETAS = 240, (115, 125), (11, 12, 13, 14), (0.0, 3.0)
DIST = dict(mask_a=[0] * 32, mask_b=[-1] * 32, groups=list(range(32)), n_groups=32)


def dist_q():
    return np.random.default_rng(5).standard_normal((SIDE, SIDE)).astype(np.float32)


def dist_mask():
    m = np.zeros((1, DIST_HM, DIST_HM))
    m[0, DIST_BOX[0]:DIST_BOX[1], DIST_BOX[0]:DIST_BOX[1]] = 1.0
    return m


def dist_counts(idx):
    """Picks [.., 32 groups, 32 draws] (flattened indices) -> how often each of the box's 100 pixels was drawn, row-major."""
    idx = np.asarray(idx).astype(np.int64)
    assert (idx >= 0).all()
    at = idx % (DIST_HM * DIST_HM)
    iy, ix = at // DIST_HM - DIST_BOX[0], at % DIST_HM - DIST_BOX[0]
    assert ((iy >= 0) & (iy < 10) & (ix >= 0) & (ix < 10)).all()
    return np.bincount((iy * 10 + ix).ravel(), minlength=100)


def assert_distribution(counts, v, beta, what):
    """Pearson's chi^2 of the counts against softmax(beta v) in float64 below df + 4 sqrt(2 df); for beta > 0 the same counts
    against beta / 2 and 2 beta above it (the test can fail)."""
    def softmax(b):
        z = b * np.asarray(v, dtype=np.float64)
        e = np.exp(z - z.max())
        return e / e.sum()
    chi, df = scene_sample_ref.chi_square(counts, softmax(beta))
    print("%s beta %g: chi^2 %.1f at df %d (bound %.1f), %d draws" % (what, beta, chi, df, scene_sample_ref.chi_square_bound(df), counts.sum()))
    assert counts.sum() == 4096 and df >= 50
    assert chi < scene_sample_ref.chi_square_bound(df), what
    if beta > 0:
        for other in (beta / 2, 2 * beta):
            chi_o, df_o = scene_sample_ref.chi_square(counts, softmax(other))
            print("%s control beta %g: chi^2 %.1f at df %d (bound %.1f)" % (what, other, chi_o, df_o, scene_sample_ref.chi_square_bound(df_o)))
            assert chi_o > scene_sample_ref.chi_square_bound(df_o), what


def assert_picks(got, maps, masks, n_draws, beta, seed, what, **sel):
    """The kernel's picks against the restatement on the same float32 maps, by the module's comparison rule: every element
    written, the empty pairs exact, a compared draw's index equal, its value bit for bit the map there; at most 1 in 1000 draws
    not compared.  Returns the restatement's (idx, val)."""
    ref_i, ref_v, gap, s1, s2 = scene_sample_ref.group_sample_scores(maps, masks, n_draws=n_draws, beta=beta, seed=seed, **sel)
    idx, val = got[0].astype(np.int64), got[1]
    assert idx.shape == val.shape == ref_i.shape
    cmp = scene_sample_ref.compared(gap, s1, s2)
    with np.errstate(invalid="ignore"):
        rel = np.where(np.isfinite(gap), gap / np.maximum(np.abs(s1), np.abs(s2)), np.inf)
    print("%s: %d draws, %d not compared; smallest relative gap %.3g; kernel draw 0 idx %s" % (what, cmp.size, int((~cmp).sum()), float(rel.min()), idx[:, 0].tolist()))
    assert (~cmp).sum() * 1000 <= cmp.size, what
    empty = ref_i < 0
    assert (idx[empty] == -1).all() and np.isneginf(val[empty]).all(), what
    assert ((idx >= 0) == ~empty).all(), what
    assert np.array_equal(idx[cmp], ref_i[cmp]), what
    have = idx >= 0
    assert np.array_equal(bits(val[have]), bits(maps.ravel()[idx[have]])), what       # the value is the map at the pick, compared or not
    return ref_i, ref_v


@pytest.fixture(scope="module")
def eng1(gpu):
    with own_engine(S, 1, 1) as eng:
        yield eng


@pytest.fixture(scope="module")
def eng3(gpu):
    with own_engine(S, 3, 1) as eng:
        yield eng


def sample(eng, q, aff, hm, masks_dev, mask_a, mask_b, groups, n_groups, n_draws, beta, seed, cls=None):
    """One smg_scene_sample_objects (cls None) or smg_scene_class_sample_objects on outputs prefilled with (-5, -5.0) ->
    (idx int32 [n_groups, n_draws], val float32 [n_groups, n_draws])."""
    idx = torch.full((n_groups, n_draws), -5, dtype=torch.int32, device="cuda")
    val = filled((n_groups, n_draws), -5.0)
    tail = (masks_dev.data_ptr(), int(masks_dev.shape[0]), mask_a, mask_b, groups, n_groups, n_draws, beta, seed, idx.data_ptr(), val.data_ptr(), stream())
    if cls is None:
        eng.scene_sample_objects(q.data_ptr(), q[0].numel(), len(aff), aff, hm, *tail)
    else:
        eng.scene_class_sample_objects(q.data_ptr(), len(aff), aff, hm, cls, *tail)
    return idx.cpu().numpy(), val.cpu().numpy()


@pytest.mark.parametrize("hm", (240, 239))
def test_picks_against_the_restatement(eng1, hm):
    """The picks case on smg_scene_maps' own output.  hm = 239 (57 121 pixels, no multiple of 4) with the masks tensor one double
    off 16-byte alignment takes the guarded mask loads, rows that change inside a thread's four pixels and a ragged last thread."""
    assert scene_ref.geometry(hm)[1:] == (S, SIDE)
    aff = picks_affines()
    q = torch.from_numpy(picks_q(hm)).cuda()
    maps = one_plane.scene_maps(eng1, q, aff, hm)
    masks = masks_for(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    if hm == 239:
        buf = torch.zeros(masks.size + 1, dtype=torch.float64, device="cuda")
        off = buf[1:].view(5, hm, hm)
        off.copy_(masks_dev)
        masks_dev = off
        assert masks_dev.data_ptr() % 16 == 8 and hm * hm % 4 == 1
    got = sample(eng1, q, aff, hm, masks_dev, n_draws=PICKS_DRAWS, beta=PICKS_BETA, seed=SEED, **PICKS)
    assert_picks(got, maps, masks, PICKS_DRAWS, PICKS_BETA, SEED, "hm %d, 40 maps" % hm, **PICKS)
    assert (got[0][[0, 1, 3]] >= 0).all()
    assert (got[0][[2, 4]] == -1).all() and np.isneginf(got[1][[2, 4]]).all()       # no valid pixel; no map
    launches = {int(i) // (hm * hm) >= 32 for i in got[0][[0, 1, 3]].ravel()}
    assert launches == {False, True}                                                # picks from both launches: the carry decided some
    assert len({int(i) for i in got[0][1]}) > 1                                     # the draws differ


def test_beta_0_is_the_argmax_of_the_noise_and_32_draws(eng1):
    """beta = 0: fma(0, v, G) = G whatever the finite v - every draw is the candidate with the largest noise, which this test
    takes from scene_sample_ref.gumbel alone.  n_draws = 32, the most a call takes."""
    hm = 240
    aff = picks_affines()
    q = torch.from_numpy(picks_q(1)).cuda()
    maps = one_plane.scene_maps(eng1, q, aff, hm)
    masks = masks_for(hm)
    got = sample(eng1, q, aff, hm, torch.from_numpy(masks).cuda(), n_draws=32, beta=0.0, seed=SEED + 1, **PICKS)
    assert_picks(got, maps, masks, 32, 0.0, SEED + 1, "beta 0, 32 draws", **PICKS)
    for g in (0, 1, 3):
        cand = np.concatenate([m * hm * hm + np.flatnonzero((scene_objects_ref.selected(masks, PICKS["mask_a"][m], PICKS["mask_b"][m])
                                                            & ~np.isneginf(maps[m])).ravel()) for m in range(40) if m % 4 == g])
        for d in range(32):
            noise = scene_sample_ref.gumbel(SEED + 1, d, cand).astype(np.float32)
            top = np.sort(noise)[-2:]
            assert top[1] > top[0]                                                  # (no tie of the two largest at float32)
            assert got[0][g, d] == cand[int(np.argmax(noise))], (g, d)


def test_a_large_beta_is_the_argmax(eng1):
    """beta (v1 - v2) > 41 - the width of G's range, 40.35, rounded up - for the two best values of every group: the noise cannot
    reorder them, and every draw is smg_scene_argmax_objects' result, index and value bit for bit.  The gap is asserted on the
    kernel's own maps first; beta = 128 / (the smallest gap), and beta |v| stays below 2^16, where a float32 score resolves 2^-7:
    the margin 128 - 41 is not eaten by the rounding of the score."""
    hm = 240
    aff = picks_affines()
    q = torch.from_numpy(picks_q(2)).cuda()
    maps = one_plane.scene_maps(eng1, q, aff, hm)
    masks = masks_for(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    sel = {k: PICKS[k] for k in ("mask_a", "mask_b", "groups")}
    gaps = []
    for g in (0, 1, 3):
        v = np.concatenate([maps[m][scene_objects_ref.selected(masks, sel["mask_a"][m], sel["mask_b"][m]) & ~np.isneginf(maps[m])] for m in range(40) if m % 4 == g])
        top = np.sort(v.astype(np.float64))[-2:]
        gaps.append(top[1] - top[0])
    beta = 128.0 / min(gaps)
    print("gaps of the two best values per group %s, beta %g" % (gaps, beta))
    assert min(gaps) > 0 and beta * min(gaps) > 41 and beta * float(np.abs(maps[np.isfinite(maps)]).max()) < 2.0 ** 16
    best = one_plane.objects(eng1, q, aff, hm, masks_dev, n_groups=5, **sel)
    got = sample(eng1, q, aff, hm, masks_dev, n_draws=8, beta=beta, seed=SEED + 2, **PICKS)
    for d in range(8):
        assert np.array_equal(got[0][:, d], best[0])
        assert_bit_identical(got[1][:, d], best[1])


def test_distribution_of_4096_draws(eng1):
    """The distribution case on the device: four calls (seeds) of 32 groups x 32 draws; the expected probabilities come from the
    kernel's own values (smg_scene_maps on the box)."""
    aff = np.tile(scene_ref.theta(0, 16), (32, 1))
    q = torch.from_numpy(np.tile(dist_q(), (32, 1, 1))).cuda()
    maps = one_plane.scene_maps(eng1, q, aff, DIST_HM)
    box = maps[0, DIST_BOX[0]:DIST_BOX[1], DIST_BOX[0]:DIST_BOX[1]]
    assert np.isfinite(box).all()                                                   # the box is valid
    masks = dist_mask()
    masks_dev = torch.from_numpy(masks).cuda()
    for beta in DIST_BETAS:
        picks = []
        for seed in DIST_SEEDS:
            got = sample(eng1, q, aff, DIST_HM, masks_dev, n_draws=32, beta=beta, seed=seed, **DIST)
            assert_picks(got, maps, masks, 32, beta, seed, "distribution, beta %g seed %d" % (beta, seed), **DIST)
            picks.append(got[0])
        assert_distribution(dist_counts(picks), box.ravel(), beta, "device")


def test_determinism_and_independence_of_the_draws(eng1):
    hm = 240
    aff = picks_affines()
    q = torch.from_numpy(picks_q(3)).cuda()
    masks_dev = torch.from_numpy(masks_for(hm)).cuda()
    a = sample(eng1, q, aff, hm, masks_dev, n_draws=8, beta=PICKS_BETA, seed=SEED, **PICKS)
    b = sample(eng1, q, aff, hm, masks_dev, n_draws=8, beta=PICKS_BETA, seed=SEED, **PICKS)
    assert np.array_equal(a[0], b[0])
    assert_bit_identical(a[1], b[1])
    c = sample(eng1, q, aff, hm, masks_dev, n_draws=3, beta=PICKS_BETA, seed=SEED, **PICKS)
    assert np.array_equal(c[0], a[0][:, :3])                                        # draw d does not depend on n_draws
    assert_bit_identical(c[1], a[1][:, :3])
    other = sample(eng1, q, aff, hm, masks_dev, n_draws=8, beta=PICKS_BETA, seed=SEED ^ 1, **PICKS)
    assert (other[0] != a[0]).any()                                                 # another seed, another noise field
    assert np.array_equal(other[0][[2, 4]], a[0][[2, 4]])                           # (the empty groups stay empty)


def test_a_nan_wins_every_draw_of_its_group(eng1):
    """A NaN map element in ONE map of group 1: its score is NaN in every draw, and by smg_argmax's rules the lowest flattened
    index among the group's NaN candidates wins each of them; the other groups keep their draws."""
    hm = 240
    aff = picks_affines()
    qh = picks_q(4)
    masks = masks_for(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    base = sample(eng1, torch.from_numpy(qh).cuda(), aff, hm, masks_dev, n_draws=8, beta=PICKS_BETA, seed=SEED, **PICKS)
    m = 4 * 2 + 1                                                                   # map 9: group 1, rotation 9
    qh[m, 1, 1] = np.nan
    q = torch.from_numpy(qh).cuda()
    maps = one_plane.scene_maps(eng1, q, aff, hm)
    foot = np.isnan(maps[m]) & (masks[STRADDLE] != 0)
    assert foot.any()
    got = sample(eng1, q, aff, hm, masks_dev, n_draws=8, beta=PICKS_BETA, seed=SEED, **PICKS)
    assert_picks(got, maps, masks, 8, PICKS_BETA, SEED, "a NaN element", **PICKS)
    assert (got[0][1] == m * hm * hm + int(np.flatnonzero(foot.ravel())[0])).all() and np.isnan(got[1][1]).all()
    others = [0, 2, 3, 4]
    assert np.array_equal(got[0][others], base[0][others])
    assert_bit_identical(got[1][others], base[1][others])


def test_class_form_against_the_class_maps(eng3):
    """smg_scene_class_sample_objects for every cls against smg_scene_class_maps' own plane, 40 maps in two launches; group 1 is
    the whole image (both terms -1)."""
    hm = 240
    aff = picks_affines()
    q = torch.from_numpy(picks_q(6, planes=3)).cuda()
    masks = masks_for(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    sel = dict(PICKS, mask_a=[-1 if m % 4 == 1 else a for m, a in enumerate(PICKS["mask_a"])])
    assert sel["mask_a"][1] == sel["mask_b"][1] == -1
    for cls in (0, 1, 2):
        maps = class_plane.class_maps(eng3, q, aff, hm, cls)
        got = sample(eng3, q, aff, hm, masks_dev, n_draws=PICKS_DRAWS, beta=PICKS_BETA, seed=SEED + cls, cls=cls, **sel)
        assert_picks(got, maps, masks, PICKS_DRAWS, PICKS_BETA, SEED + cls, "class form, cls %d" % cls, **sel)
        assert (got[0][[0, 1, 3]] >= 0).all() and (got[0][[2, 4]] == -1).all()
        again = sample(eng3, q, aff, hm, masks_dev, n_draws=PICKS_DRAWS, beta=PICKS_BETA, seed=SEED + cls, cls=cls, **sel)
        assert np.array_equal(got[0], again[0])
        assert_bit_identical(got[1], again[1])


def test_refusals(eng1, eng3):
    """-22, a message that starts with the function's name and names the cause, nothing launched: the outputs keep their fill.
    Every refusal of the argmax_objects entry points, then n_draws < 1, n_draws > 32, n_groups * n_draws beyond int32 and a beta
    that is negative, NaN or infinite."""
    import smg_hip
    L = smg_hip.lib()
    hm, n_draws = 240, 4
    big = 37283                                            # 37 283 x 240^2 > 2^31 - 1
    aff = np.tile(scene_ref.theta(1, 16), (big, 1))
    shifted = aff[:16].copy()
    shifted[7, 5] = 0.25
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))         # noqa: E731
    ints = lambda v: (C.c_int * big)(*([v] * big))                 # noqa: E731
    zero, minus = ints(0), ints(-1)
    q = torch.zeros((16, 3, SIDE, SIDE), device="cuda")
    masks = torch.ones((2, hm, hm), dtype=torch.float64, device="cuda")
    idx = torch.full((3, n_draws), -5, dtype=torch.int32, device="cuda")
    val = filled((3, n_draws), -5.0)
    ok = dict(e=eng1.h, q=q.data_ptr(), stride=SIDE * SIDE, n_maps=16, aff=ptr(aff), hm=hm, cls=0, masks=masks.data_ptr(), n_masks=2, a=zero, b=minus,
              g=zero, n_groups=3, n_draws=n_draws, beta=3.0, seed=SEED, idx=idx.data_ptr(), val=val.data_ptr())

    def call(name, a):
        tail = (a["masks"], a["n_masks"], a["a"], a["b"], a["g"], a["n_groups"], a["n_draws"], a["beta"], a["seed"], a["idx"], a["val"], None)
        if name == b"smg_scene_sample_objects":
            return L.smg_scene_sample_objects(a["e"], a["q"], a["stride"], a["n_maps"], a["aff"], a["hm"], *tail)
        return L.smg_scene_class_sample_objects(a["e"], a["q"], a["n_maps"], a["aff"], a["hm"], a["cls"], *tail)
    one_bad = lambda v: (C.c_int * 16)(*([0] * 15 + [v]))          # noqa: E731
    for name, e_ok, e_640 in ((b"smg_scene_sample_objects", eng1.h, cached_engine(640, 1).h), (b"smg_scene_class_sample_objects", eng3.h, cached_engine(640, 3).h)):
        def refused(word, **change):
            rc = call(name, dict(dict(ok, e=e_ok), **change))
            msg = L.smg_last_error()
            assert rc == -22 and msg.startswith(name + b":") and word in msg, (name, change.keys(), rc, msg)
        for key in ("q", "aff", "masks", "a", "b", "g", "idx", "val"):
            refused(b"NULL", **{key: None})
        refused(b"n_maps < 1", n_maps=0)
        refused(b"n_masks < 1", n_masks=0)
        refused(b"n_groups < 1", n_groups=0)
        for bad in (2, -2):
            refused(b"mask index", a=one_bad(bad))
            refused(b"mask index", b=one_bad(bad))
        for bad in (3, -1):
            refused(b"group outside", g=one_bad(bad))
        refused(b"int32", n_maps=big)
        refused(b"does not pad", hm=320)
        refused(b"does not pad", hm=224)
        refused(b"1 x 1", e=e_640, hm=224)
        refused(b"translation", aff=ptr(shifted))
        refused(b"n_draws < 1", n_draws=0)
        refused(b"n_draws < 1", n_draws=-3)
        refused(b"n_draws exceeds", n_draws=33)
        refused(b"n_groups * n_draws", n_groups=0x7fffffff // 32 + 1, n_draws=32)
        for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
            refused(b"beta", beta=bad)
        if name == b"smg_scene_sample_objects":
            refused(b"negative map_stride", stride=-1)
        else:
            refused(b"head_out", e=eng1.h)
            refused(b"cls must be", cls=3)
            refused(b"cls must be", cls=-1)
    with pytest.raises(smg_hip.SmgError):
        eng1.scene_sample_objects(q.data_ptr(), SIDE * SIDE, 16, shifted, hm, masks.data_ptr(), 2, [0] * 16, [-1] * 16, [0] * 16, 3, n_draws, 3.0, SEED,
                                  idx.data_ptr(), val.data_ptr(), stream())
    with pytest.raises(smg_hip.SmgError):
        eng3.scene_class_sample_objects(q.data_ptr(), 16, aff[:16], hm, 0, masks.data_ptr(), 2, [0] * 16, [-1] * 16, [0] * 16, 3, 33, 3.0, SEED,
                                        idx.data_ptr(), val.data_ptr(), stream())
    torch.cuda.synchronize()
    assert bool((idx == -5).all()) and bool((val == -5.0).all())
    # and the accepted calls write every element: group 0 four draws of the constant map, groups 1 and 2 (no map) the empty pairs
    for name, e_ok, value in ((b"smg_scene_sample_objects", eng1.h, np.float32(0.0)), (b"smg_scene_class_sample_objects", eng3.h, class_plane.THIRD)):
        for seed in (0, 2 ** 64 - 1):                      # the ends of the seed's range
            idx.fill_(-5)
            val.fill_(-5.0)
            assert call(name, dict(ok, e=e_ok, seed=seed)) == 0
            i, v = idx.cpu().numpy(), val.cpu().numpy()
            assert (i[0] >= 0).all() and (v[0] == value).all() and (i[1:] == -1).all() and np.isneginf(v[1:]).all()


# ---- the Trainer's methods ---------------------------------------------------------------------------------------------------------
HM, R, DRAWS_TR, TEMPERATURE_TR, SEED_TR = 240, 16, 4, 0.25, 2 ** 63 + 12345      # (1 / 0.25 = 4 exactly)
STEP = 0x9E3779B97F4A7C15


def scene():
    """A 240^2 heightmap (S = 704, 3 x 3 maps) and two objects inside the part of it that has a window in every rotation."""
    import synthetic
    depth, _ = synthetic.heightmap_scene(8, size=HM)
    obj = np.zeros((2, HM, HM))
    obj[0, 112:128, 110:120] = 1.0
    obj[1, 114:126, 121:131] = 1.0
    return depth, obj


def kept_maps(kept, name, planes, cls, per):
    """smg_scene_maps' / smg_scene_class_maps' output for the maps a Trainer method kept for one primitive."""
    q = kept[name]
    n = q.shape[0]
    aff = affines(R)[np.arange(n) % per] if per > 1 else np.tile(scene_ref.theta(0, R), (n, 1))
    if planes == 1:
        return one_plane.scene_maps(cached_engine(S, 1), q.reshape(n, SIDE, SIDE), aff, HM)
    return class_plane.class_maps(cached_engine(S, 3), q, aff, HM, cls)


def check_sampled(tr, call, planes, cls=0):
    depth, obj = scene()
    beta = 1.0 / TEMPERATURE_TR
    res = call(tr, depth, obj, DRAWS_TR, TEMPERATURE_TR, SEED_TR, is_ets=False)
    assert set(res) == {"per_object", "pairs", "per_pair", "ranked"} and res["pairs"] == [] and res["per_pair"] == []
    kept = tr._last_object_q
    assert set(kept) == {"grasp", "suction"}
    refs = {}
    for style, name in enumerate(("grasp", "suction")):
        maps = kept_maps(kept, name, planes, cls, R)
        sel = dict(mask_a=[k for k in range(2) for _ in range(R)], mask_b=[-1] * (2 * R), groups=[k for k in range(2) for _ in range(R)], n_groups=2)
        seed = (SEED_TR + style * STEP) % 2 ** 64
        ref_i, ref_v, gap, s1, s2 = scene_sample_ref.group_sample_scores(maps, obj, n_draws=DRAWS_TR, beta=beta, seed=seed, **sel)
        assert scene_sample_ref.compared(gap, s1, s2).all() and (ref_i >= 0).all()
        refs[name] = (maps, seed)
        lists = res["per_object"][name]
        assert len(lists) == 2
        for k in range(2):
            want = [((int(i) // (HM * HM)) % R, ((int(i) // HM) % HM, int(i) % HM), float(v)) for i, v in zip(ref_i[k], ref_v[k])]
            print("%s object %d: %s" % (name, k, lists[k]))
            assert lists[k] == want, (name, k)
        flat = [(k,) + e for k in range(2) for e in lists[k]]
        assert sorted(res["ranked"][name]) == sorted(flat)
        confs = [e[3] for e in res["ranked"][name]]
        assert confs == sorted(confs, reverse=True)
    assert res["ranked"]["pairs"] == []
    # joint: one group of all the primitive's maps, and the pairs' one group
    joint = call(tr, depth, obj, DRAWS_TR, TEMPERATURE_TR, SEED_TR, is_ets=True, joint=True)
    assert set(joint) == {"joint", "pairs", "per_pair", "ranked"} and joint["pairs"] == [(0, 1)] and joint["per_pair"] == []
    kept = tr._last_object_q
    assert set(kept) == {"grasp", "suction", "pairs"}
    for style, name in enumerate(("grasp", "suction", "pairs")):
        per = 1 if name == "pairs" else R
        maps = kept_maps(kept, name, planes, cls, per)
        n = maps.shape[0]
        sel = (dict(mask_a=[0], mask_b=[1]) if name == "pairs" else dict(mask_a=[k for k in range(2) for _ in range(R)], mask_b=[-1] * n))
        seed = (SEED_TR + style * STEP) % 2 ** 64
        ref_i, ref_v, gap, s1, s2 = scene_sample_ref.group_sample_scores(maps, obj, groups=[0] * n, n_groups=1, n_draws=DRAWS_TR, beta=beta, seed=seed, **sel)
        assert scene_sample_ref.compared(gap, s1, s2).all() and (ref_i >= 0).all()
        if name == "pairs":
            want = [((0, 1), ((int(i) // HM) % HM, int(i) % HM), float(v)) for i, v in zip(ref_i[0], ref_v[0])]
        else:
            want = [(int(i) // (HM * HM) // R, (int(i) // (HM * HM)) % R, ((int(i) // HM) % HM, int(i) % HM), float(v)) for i, v in zip(ref_i[0], ref_v[0])]
        print("joint %s: %s" % (name, joint["joint"][name]))
        assert joint["joint"][name] == want, name
        assert sorted(joint["ranked"][name]) == sorted(want)
        confs = [e[-1] for e in joint["ranked"][name]]
        assert confs == sorted(confs, reverse=True)
    return res, refs


def test_sampled_scene_actions(gpu):
    tr = make_trainer('reinforcement', 4, R=R)
    res, refs = check_sampled(tr, lambda t, *a, **k: t.sampled_scene_actions(*a, **k), 1)
    depth, obj = scene()
    # a temperature small enough for the gap condition gives best_scene_actions' entries in every draw
    best = tr.best_scene_actions(depth, obj, is_ets=False)
    cold_maps = {name: kept_maps(tr._last_object_q, name, 1, 0, R) for name in ("grasp", "suction")}
    gaps = []
    for name in ("grasp", "suction"):
        for k in range(2):
            v = np.concatenate([cold_maps[name][k * R + r][(obj[k] != 0) & ~np.isneginf(cold_maps[name][k * R + r])] for r in range(R)]).astype(np.float64)
            top = np.sort(v)[-2:]
            gaps.append(top[1] - top[0])
    beta = 128.0 / min(gaps)
    print("gaps of the two best values per object %s, beta %g" % (gaps, beta))
    assert min(gaps) > 0 and beta * min(gaps) > 41 and beta * max(float(np.abs(m[np.isfinite(m)]).max()) for m in cold_maps.values()) < 2.0 ** 16
    cold = tr.sampled_scene_actions(depth, obj, 3, 1.0 / beta, 5, is_ets=False)
    for name in ("grasp", "suction"):
        for k in range(2):
            assert cold["per_object"][name][k] == [best["per_object"][name][k]] * 3, (name, k)
    target = tr.sampled_scene_actions(depth, obj, 3, 1.0 / beta, 5, is_ets=False, is_target=True)
    assert [len(x) for x in target["per_object"]["suction"]] == [3, 3]
    uniform = tr.sampled_scene_actions(depth, obj, 2, float("inf"), 5, is_ets=False)
    assert all(len(x) == 2 for x in uniform["per_object"]["grasp"])
    with pytest.raises(ValueError):
        tr.sampled_scene_class_actions(depth, obj, 2, 1.0, 0)
    for n_draws, temperature, seed in ((0, 1.0, 0), (33, 1.0, 0), (2.5, 1.0, 0), (2, 0.0, 0), (2, -1.0, 0), (2, float("nan"), 0), (2, 1.0, -1), (2, 1.0, 2 ** 64),
                                       (2, 1.0, 0.5)):
        with pytest.raises(ValueError):
            tr.sampled_scene_actions(depth, obj, n_draws, temperature, seed)


def test_sampled_scene_class_actions(gpu):
    tr = make_trainer('reactive', 4, R=R)
    check_sampled(tr, lambda t, *a, **k: t.sampled_scene_class_actions(*a, **k), 3)
    depth, obj = scene()
    one = tr.sampled_scene_class_actions(depth, obj, 2, 0.5, 9, is_ets=False, cls=1)
    maps = kept_maps(tr._last_object_q, "grasp", 3, 1, R)
    for k in range(2):
        for rot, (iy, ix), conf in one["per_object"]["grasp"][k]:
            assert conf == float(maps[k * R + rot, iy, ix]) and obj[k, iy, ix] != 0
    with pytest.raises(ValueError):
        tr.sampled_scene_actions(depth, obj, 2, 1.0, 0)
    with pytest.raises(ValueError):
        tr.sampled_scene_class_actions(depth, obj, 2, 1.0, 0, cls=3)
    with pytest.raises(ValueError):
        tr.sampled_scene_class_actions(depth, obj, 33, 1.0, 0)


@pytest.mark.parametrize("action,style", (("grasp", 0), ("grasp_then_suction", 2)))
def test_a_sampled_action_goes_through_backprop_scene(gpu, action, style):
    """ranked_to_best on a DRAW: backprop_scene takes it as it takes best_scene_actions' dict, and the step is
    train_batch_scene_pixels on that (object, rotation, pixel) - loss and the head's conv1 weight gradient bit for bit."""
    depth, obj = scene()
    a, b = make_trainer('reinforcement', 4, R=R), make_trainer('reinforcement', 4, R=R)
    res = a.sampled_scene_actions(depth, obj, 3, 0.5, 21, joint=(style == 2))
    best = a.ranked_to_best(res, action, 1)
    if style == 2:
        (g, s), rot, pixel, conf = best["bestgs_num"], 0, best["bestgs_pixel"], best["bestgs_conf"]
        m = depth * (obj[g] + obj[s])
        assert ((g, s), pixel, conf) == res["ranked"]["pairs"][1] and ((g, s), pixel, conf) in res["joint"]["pairs"]
    else:
        (k, rot), pixel, conf = best["bestg_id"], best["bestg_pixel"], best["bestg_conf"]
        m = depth * obj[k]
        assert (k, rot, pixel, conf) == res["ranked"]["grasp"][1] and (rot, pixel, conf) in res["per_object"]["grasp"][k]
    label = conf + 0.4
    loss_a = a.backprop_scene(depth, action, best, label, obj)
    loss_b = b.train_batch_scene_pixels(depth, m, style, [rot], [[pixel]], [label]).cpu().numpy()
    print("%s draw %s rot %d pixel %s: loss %.7f (backprop_scene), %.7f (train_batch_scene_pixels)" % (action, best, rot, pixel, float(loss_a), float(loss_b[0])))
    assert 0.0 < float(loss_a) < 0.1
    assert_bit_identical(loss_a.reshape(1), loss_b)
    name = ("graspnet_val.grasp-val-", None, "suctionnet_val.suction-val-")[style] + "conv1.weight"
    ga, gb = dict(a.model.named_parameters())[name].grad, dict(b.model.named_parameters())[name].grad
    assert float(ga.abs().max()) > 0
    assert_bit_identical(ga, gb)
