"""The K best separated actions per object in the scene frame on the MI355X (run with -m gpu): smg_scene_topk_objects and
smg_scene_class_topk_objects on an engine alone with synthetic maps - smg_scene_maps' (smg_scene_class_maps') own output, masked on
the host and pushed through the numpy greedy restatement of tests/scene_topk_ref.py, must give the kernels' indices, and the values
bit for bit - then Trainer.ranked_scene_actions / ranked_scene_class_actions against the maps they kept pushed through scene_ref /
scene_class_ref in fp64, and ranked_to_best through backprop_scene.  The rectangle masks, their valid-pixel counts and the map
layouts are test_gpu_scene_objects.py's; tests/test_cpu_scene_topk.py shows on the CPU that CASES fill every rank of the three
large masks and leave the one-pixel mask a -1 tail."""
import ctypes as C

import numpy as np
import pytest
import torch

from map_harness import assert_bit_identical, bits, cached_engine, filled, gpu, make_trainer, stream  # noqa: F401

import scene_ref
import scene_topk_ref
import test_gpu_scene_class_objects as class_plane
import test_gpu_scene_objects as one_plane

pytestmark = pytest.mark.gpu

SHAPES = ((240, 704, 3), (320, 928, 10))
CASES = ((32, 1), (4, 5))                # (K, radius): the most ranks with the smallest disc (5 pixels), and a disc of 81 pixels
CENTRE, STRADDLE, OUTSIDE, ONE, WHOLE = range(5)
affines, rect_masks, rotation_major = one_plane.affines, one_plane.rect_masks, one_plane.rotation_major
ALL80 = dict(mask_a=[m % 5 for m in range(80)], mask_b=[-1] * 80, groups=[m % 5 for m in range(80)])      # m = 5 r + k, group = mask = k


def topk(eng, q, aff, hm, masks_dev, mask_a, mask_b, groups, n_groups, K, radius, cls=None):
    """One smg_scene_topk_objects (cls None) or smg_scene_class_topk_objects on outputs prefilled with (-5, -5.0) ->
    (idx int32 [n_groups, K], val float32 [n_groups, K])."""
    idx = torch.full((n_groups, K), -5, dtype=torch.int32, device="cuda")
    val = filled((n_groups, K), -5.0)
    tail = (masks_dev.data_ptr(), int(masks_dev.shape[0]), mask_a, mask_b, groups, n_groups, K, radius, idx.data_ptr(), val.data_ptr(), stream())
    if cls is None:
        eng.scene_topk_objects(q.data_ptr(), q[0].numel(), len(aff), aff, hm, *tail)
    else:
        eng.scene_class_topk_objects(q.data_ptr(), len(aff), aff, hm, cls, *tail)
    return idx.cpu().numpy(), val.cpu().numpy()


def assert_equals_helper(got, maps, masks, mask_a, mask_b, groups, n_groups, K, radius, what):
    """The kernel's ranks against the greedy helper on the same float32 maps: indices equal, values bit for bit, every element
    written, picks of a group pairwise farther apart than the radius."""
    ref_i, ref_v = scene_topk_ref.group_topk(maps, masks, mask_a, mask_b, groups, n_groups, K, radius)
    filled_ranks = (ref_i >= 0).sum(1)
    print("%s: K %d radius %d, ranks filled per group %s; kernel rank 0 idx %s" % (what, K, radius, filled_ranks.tolist(), got[0][:, 0].tolist()))
    assert got[0].shape == got[1].shape == (n_groups, K)
    assert np.array_equal(got[0].astype(np.int64), ref_i), what
    assert np.array_equal(bits(got[1]), bits(ref_v)), what
    hm = maps.shape[1]
    for g in range(n_groups):
        pix = [divmod(int(i) % (hm * hm), hm) for i in got[0][g] if i >= 0]
        for a in range(len(pix)):
            for b in range(a):
                assert (pix[a][0] - pix[b][0]) ** 2 + (pix[a][1] - pix[b][1]) ** 2 > radius * radius, (what, g, pix[a], pix[b])
        assert (got[0][g][len(pix):] == -1).all() and np.isneginf(got[1][g][len(pix):]).all()      # the tail, and nothing after it
    return ref_i, ref_v


def assert_rank0_is_the_argmax(got, best):
    assert np.array_equal(got[0][:, 0], best[0])
    assert_bit_identical(got[1][:, 0], best[1])


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_ranks_of_masked_maps_against_the_helper(gpu, hm, S, side):
    """16 rotations x 5 masks = 80 maps, rotation-major (m = 5 r + k, group = k): three launches of 32 / 32 / 16 maps per round, so
    every rank of every group is carried twice, and a group's picks come from maps of all three launches."""
    assert scene_ref.geometry(hm)[1:] == (S, side)
    eng = cached_engine(S, 1)
    aff16 = affines()
    q16 = torch.from_numpy(np.random.default_rng(S + 3).standard_normal((16, side, side)).astype(np.float32)).cuda()
    maps16 = one_plane.scene_maps(eng, q16, aff16, hm)
    masks = rect_masks(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    q80, aff80, rep = rotation_major(q16, aff16, 5)
    best = one_plane.objects(eng, q80, aff80, hm, masks_dev, n_groups=5, **ALL80)
    one = topk(eng, q80, aff80, hm, masks_dev, n_groups=5, K=1, radius=3, **ALL80)
    assert one[0].shape == (5, 1)
    assert_rank0_is_the_argmax(one, best)
    for K, radius in CASES:
        got = topk(eng, q80, aff80, hm, masks_dev, n_groups=5, K=K, radius=radius, **ALL80)
        assert_equals_helper(got, maps16[rep], masks, n_groups=5, K=K, radius=radius, what="hm %d, 80 maps" % hm, **ALL80)
        assert_rank0_is_the_argmax(got, best)
        assert (got[0][[CENTRE, STRADDLE, WHOLE]] >= 0).all()                              # every rank filled
        assert (got[0][OUTSIDE] == -1).all() and np.isneginf(got[1][OUTSIDE]).all()         # no pixel with a window
        assert got[0][ONE, 0] >= 0 and (got[0][ONE, 1:] == -1).all() and np.isneginf(got[1][ONE, 1:]).all()      # a mask smaller than the disc
        rots = {int(i) // (hm * hm) // 5 for i in got[0][WHOLE]}
        assert K < 32 or len(rots) > 1                                                      # the picks of a group come from several of its maps
        again = topk(eng, q80, aff80, hm, masks_dev, n_groups=5, K=K, radius=radius, **ALL80)
        assert np.array_equal(got[0], again[0])
        assert_bit_identical(got[1], again[1])
    # groups that are no function of the mask: (rotation parity) x mask, in descending order, and the every-pixel form (-1, -1)
    groups2 = [9 - (2 * (m % 5) + (m // 5) % 2) for m in range(80)]
    mask_a2 = [-1 if m % 5 == WHOLE else m % 5 for m in range(80)]
    got2 = topk(eng, q80, aff80, hm, masks_dev, mask_a2, ALL80["mask_b"], groups2, 11, 4, 5)
    assert_equals_helper(got2, maps16[rep], masks, mask_a2, ALL80["mask_b"], groups2, 11, 4, 5, "hm %d, 11 groups" % hm)
    assert (got2[0][10] == -1).all() and np.isneginf(got2[1][10]).all()                      # a group without a map


def test_guarded_mask_loads_give_the_same_results(gpu):
    """The masks tensor one double off 16-byte alignment takes the guarded 8-byte loads: the same ranks as the aligned tensor.
    hm = 239 (57 121 pixels, no multiple of 4, the same S = 704) takes them too, with rows that change inside a thread's four
    pixels and a last thread whose four pixels run past the map."""
    S, side, K, radius = 704, 3, 4, 5
    eng = cached_engine(S, 1)
    aff16 = affines()
    q16 = torch.from_numpy(np.random.default_rng(21).standard_normal((16, side, side)).astype(np.float32)).cuda()
    q80, aff80, rep = rotation_major(q16, aff16, 5)
    hm = 240
    masks = rect_masks(hm)
    aligned = torch.from_numpy(masks).cuda()
    buf = torch.zeros(masks.size + 1, dtype=torch.float64, device="cuda")
    off = buf[1:].view(5, hm, hm)
    off.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 8
    a = topk(eng, q80, aff80, hm, aligned, n_groups=5, K=K, radius=radius, **ALL80)
    b = topk(eng, q80, aff80, hm, off, n_groups=5, K=K, radius=radius, **ALL80)
    assert_equals_helper(b, one_plane.scene_maps(eng, q16, aff16, hm)[rep], masks, n_groups=5, K=K, radius=radius, what="hm 240, masks 8 bytes off", **ALL80)
    assert np.array_equal(a[0], b[0])
    assert_bit_identical(a[1], b[1])
    hm = 239
    assert scene_ref.geometry(hm)[1:] == (S, side) and hm * hm % 4 == 1
    masks = np.zeros((5, hm, hm))
    for k, (_, (y0, y1, x0, x1), _) in enumerate(one_plane.RECTS[240]):
        masks[k, y0:y1, x0:x1] = 1.0
    masks[WHOLE] = 1.0
    masks[ONE] = 0.0
    masks[ONE, hm - 1, hm - 1] = 1.0                       # the very last pixel (no window is centred there: an empty group)
    c = topk(eng, q80, aff80, hm, torch.from_numpy(masks).cuda(), n_groups=5, K=K, radius=radius, **ALL80)
    assert_equals_helper(c, one_plane.scene_maps(eng, q16, aff16, hm)[rep], masks, n_groups=5, K=K, radius=radius, what="hm 239", **ALL80)
    assert (c[0][ONE] == -1).all() and (c[0][CENTRE] >= 0).all()


def test_unions_ties_radius_0_and_exhaustion(gpu):
    """test_gpu_scene_objects.py's seven masks (unions that cancel as a sum, 0.5 / 2.0 / NaN select, -0.0 does not) on four
    rotations.  On a constant map every candidate ties: the ranks are the greedy rule on the flattened order alone.  radius 0
    removes the picked pixel only - in all four rotations of its group, or rank 1 would be the same pixel one rotation on.  The
    6 x 6 overlap masks and the 3 x 3 block lie inside the disc of radius 8 around any of their pixels: exhausted after rank 0."""
    hm, S, side = 240, 704, 3
    eng = cached_engine(S, 1)
    R = 4
    aff = affines(R)
    masks = np.zeros((7, hm, hm))
    masks[0, 112:128, 110:126] = 0.5
    masks[1, 90:110, 100:140] = 2.0
    masks[1, 95, 120] = np.nan
    masks[2, 115:130, 115:130] = 1.0
    masks[2, 100:115, 100:130] = 1.0
    masks[3, 115:130, 115:130] = -1.0
    masks[3, 130:140, 115:140] = -1.0
    masks[4, 117:123, 117:123] = 1.0
    masks[5, 117:123, 117:123] = -1.0
    masks[6] = -0.0
    masks[6, 119, 118] = np.nan
    masks[6, 121:124, 117:120] = 3.0
    masks_dev = torch.from_numpy(masks).cuda()
    pairs = ((0, 1), (2, 3), (4, 5), (6, -1), (-1, 6))
    sel = dict(mask_a=[pairs[m % 5][0] for m in range(5 * R)], mask_b=[pairs[m % 5][1] for m in range(5 * R)], groups=[m % 5 for m in range(5 * R)])
    rep = np.repeat(np.arange(R), 5)
    q = torch.from_numpy(np.random.default_rng(31).standard_normal((R, side, side)).astype(np.float32)).cuda()
    maps = one_plane.scene_maps(eng, q, aff, hm)
    q20 = q[torch.from_numpy(rep).cuda()].contiguous()
    for K, radius in ((6, 0), (6, 3), (3, 8)):
        got = topk(eng, q20, aff[rep], hm, masks_dev, n_groups=5, K=K, radius=radius, **sel)
        assert_equals_helper(got, maps[rep], masks, n_groups=5, K=K, radius=radius, what="unions, random maps", **sel)
    assert (got[0][2:, 0] >= 0).all() and (got[0][2:, 1:] == -1).all()         # radius 8: the small masks are gone after rank 0
    assert (got[0][:2] >= 0).all()
    # a constant map: all selected valid pixels tie
    qc = torch.full((5 * R, side, side), 0.375, dtype=torch.float32, device="cuda")
    mapc = one_plane.scene_maps(eng, qc[:R], aff, hm)
    for K, radius in ((6, 0), (5, 2)):
        got = topk(eng, qc, aff[rep], hm, masks_dev, n_groups=5, K=K, radius=radius, **sel)
        assert_equals_helper(got, mapc[rep], masks, n_groups=5, K=K, radius=radius, what="unions, constant maps", **sel)
        assert (got[1][got[0] >= 0] == np.float32(0.375)).all()
        assert [int(i) // (hm * hm) for i in got[0][:, 0]] == [0, 1, 2, 3, 4]                 # rotation 0's map of each group
    got0 = topk(eng, qc, aff[rep], hm, masks_dev, n_groups=5, K=3, radius=0, **sel)
    first = [[divmod(int(i) % (hm * hm), hm) for i in row] for row in got0[0]]
    assert first[2] == [(117, 117), (117, 118), (117, 119)]                     # radius 0: the next pixel, not (117, 117) of rotation 1
    assert first[3] == first[4] == [(119, 118), (121, 117), (121, 118)]         # the NaN selects, the -0.0 around it does not
    assert [int(i) // (hm * hm) for i in got0[0][2]] == [2, 2, 2]


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_a_nan_wins_its_rank_and_is_suppressed_like_any_pick(gpu, hm, S, side):
    """A NaN map element in ONE map of a group: the first selected pixel of its footprint is rank 0 of that group, the NaN pixels
    outside the pick's disc take the next ranks in flattened order, and the other groups keep their ranks."""
    eng = cached_engine(S, 1)
    aff16 = affines()
    masks = rect_masks(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    rep = np.repeat(np.arange(16), 5)
    q16 = torch.from_numpy(np.random.default_rng(S + 11).standard_normal((16, side, side)).astype(np.float32)).cuda()
    q80 = q16[torch.from_numpy(rep).cuda()].contiguous()
    K, radius = 4, 5
    base = topk(eng, q80, aff16[rep], hm, masks_dev, n_groups=5, K=K, radius=radius, **ALL80)
    el = (side // 2, side // 2) if side == 3 else (4, 4)
    m = 5 * 0 + CENTRE
    qn = q80.clone()
    qn[m, el[0], el[1]] = float("nan")
    maps = one_plane.scene_maps(eng, qn, aff16[rep], hm)
    foot = np.isnan(maps[m]) & (masks[CENTRE] != 0)
    assert foot.any()
    got = topk(eng, qn, aff16[rep], hm, masks_dev, n_groups=5, K=K, radius=radius, **ALL80)
    assert_equals_helper(got, maps, masks, n_groups=5, K=K, radius=radius, what="hm %d, a NaN element" % hm, **ALL80)
    assert np.isnan(got[1][CENTRE, 0]) and got[0][CENTRE, 0] == m * hm * hm + int(np.flatnonzero(foot.ravel())[0])
    others = [g for g in range(5) if g != CENTRE]
    assert np.array_equal(got[0][others], base[0][others])
    assert_bit_identical(got[1][others], base[1][others])


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_class_form_against_the_class_maps(gpu, hm, S, side):
    """smg_scene_class_topk_objects for every cls against smg_scene_class_maps' own plane, 80 maps in three launches; rank 0 and
    the K = 1 call are smg_scene_class_argmax_objects."""
    eng = cached_engine(S, 3)
    aff16 = affines()
    q16 = class_plane.logits(S + 5, 16, side)
    masks = rect_masks(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    q80, aff80, rep = rotation_major(q16, aff16, 5)
    for cls, (K, radius) in ((0, CASES[1]), (1, CASES[0]), (2, CASES[1])):
        maps16 = class_plane.class_maps(eng, q16, aff16, hm, cls)
        best = class_plane.objects(eng, q80, aff80, hm, cls, masks_dev, n_groups=5, **ALL80)
        got = topk(eng, q80, aff80, hm, masks_dev, n_groups=5, K=K, radius=radius, cls=cls, **ALL80)
        assert_equals_helper(got, maps16[rep], masks, n_groups=5, K=K, radius=radius, what="hm %d cls %d" % (hm, cls), **ALL80)
        assert_rank0_is_the_argmax(got, best)
        assert (got[0][[CENTRE, STRADDLE, WHOLE]] >= 0).all() and (got[0][OUTSIDE] == -1).all() and (got[0][ONE, 1:] == -1).all()
        one = topk(eng, q80, aff80, hm, masks_dev, n_groups=5, K=1, radius=0, cls=cls, **ALL80)
        assert_rank0_is_the_argmax(one, best)
        again = topk(eng, q80, aff80, hm, masks_dev, n_groups=5, K=K, radius=radius, cls=cls, **ALL80)
        assert np.array_equal(got[0], again[0])
        assert_bit_identical(got[1], again[1])


def test_refusals(gpu):
    """-22, a message that starts with the function's name and names the cause, nothing launched: the outputs keep their fill.
    Every refusal of the argmax_objects entry points, then K < 1, K > 32, radius < 0 and n_groups * K beyond int32."""
    import smg_hip
    L = smg_hip.lib()
    hm, side, K = 240, 3, 4
    eng, eng3, eng640 = cached_engine(704, 1), cached_engine(704, 3), cached_engine(640, 1)
    big = 37283                                            # 37 283 x 240^2 > 2^31 - 1
    aff = np.tile(scene_ref.theta(1, 16), (big, 1))
    shifted = aff[:16].copy()
    shifted[7, 5] = 0.25
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))         # noqa: E731
    ints = lambda v: (C.c_int * big)(*([v] * big))                 # noqa: E731
    zero, minus = ints(0), ints(-1)
    q = torch.zeros((16, 3, side, side), device="cuda")
    masks = torch.ones((2, hm, hm), dtype=torch.float64, device="cuda")
    idx = torch.full((3, K), -5, dtype=torch.int32, device="cuda")
    val = filled((3, K), -5.0)
    ok = dict(e=eng.h, q=q.data_ptr(), stride=side * side, n_maps=16, aff=ptr(aff), hm=hm, cls=0, masks=masks.data_ptr(), n_masks=2, a=zero, b=minus,
              g=zero, n_groups=3, K=K, radius=2, idx=idx.data_ptr(), val=val.data_ptr())

    def call(name, a):
        tail = (a["masks"], a["n_masks"], a["a"], a["b"], a["g"], a["n_groups"], a["K"], a["radius"], a["idx"], a["val"], None)
        if name == b"smg_scene_topk_objects":
            return L.smg_scene_topk_objects(a["e"], a["q"], a["stride"], a["n_maps"], a["aff"], a["hm"], *tail)
        return L.smg_scene_class_topk_objects(a["e"], a["q"], a["n_maps"], a["aff"], a["hm"], a["cls"], *tail)
    one_bad = lambda v: (C.c_int * 16)(*([0] * 15 + [v]))          # noqa: E731
    for name, e_ok, e_640 in ((b"smg_scene_topk_objects", eng.h, eng640.h), (b"smg_scene_class_topk_objects", eng3.h, cached_engine(640, 3).h)):
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
        refused(b"K < 1", K=0)
        refused(b"K < 1", K=-3)
        refused(b"K exceeds", K=33)
        refused(b"radius < 0", radius=-1)
        refused(b"n_groups * K", n_groups=0x7fffffff // 32 + 1, K=32)
        if name == b"smg_scene_topk_objects":
            refused(b"negative map_stride", stride=-1)
        else:
            refused(b"head_out", e=eng.h)
            refused(b"cls must be", cls=3)
            refused(b"cls must be", cls=-1)
    with pytest.raises(smg_hip.SmgError):
        eng.scene_topk_objects(q.data_ptr(), side * side, 16, shifted, hm, masks.data_ptr(), 2, [0] * 16, [-1] * 16, [0] * 16, 3, K, 2,
                               idx.data_ptr(), val.data_ptr(), stream())
    with pytest.raises(smg_hip.SmgError):
        eng3.scene_class_topk_objects(q.data_ptr(), 16, aff[:16], hm, 0, masks.data_ptr(), 2, [0] * 16, [-1] * 16, [0] * 16, 3, 33, 2,
                                      idx.data_ptr(), val.data_ptr(), stream())
    torch.cuda.synchronize()
    assert bool((idx == -5).all()) and bool((val == -5.0).all())
    # and the accepted calls write every element: group 0 four ranks of the constant map, groups 1 and 2 (no map) the empty pairs
    for name, e_ok, value in ((b"smg_scene_topk_objects", eng.h, np.float32(0.0)), (b"smg_scene_class_topk_objects", eng3.h, class_plane.THIRD)):
        idx.fill_(-5)
        val.fill_(-5.0)
        assert call(name, dict(ok, e=e_ok)) == 0
        i, v = idx.cpu().numpy(), val.cpu().numpy()
        assert (i[0] >= 0).all() and (v[0] == value).all() and (i[1:] == -1).all() and np.isneginf(v[1:]).all()
        assert call(name, dict(ok, e=e_ok, radius=0x7fffffff)) == 0            # a radius beyond the image: rank 0 alone
        i = idx.cpu().numpy()
        assert i[0, 0] >= 0 and (i[0, 1:] == -1).all()


# ---- the Trainer's methods ---------------------------------------------------------------------------------------------------------
HM, R, K_TR, RADIUS_TR = 320, 4, 4, 6


def scene():
    """A 320^2 heightmap and objects 2 to 5 of the synthetic scene: object 2 has no pixel with a window, the others 210 / 351 /
    1020 in every rotation of 4 (test_gpu_scene_objects.py's test_best_scene_actions counts them)."""
    import synthetic
    depth, masks = synthetic.heightmap_scene(8, size=HM)
    return depth, masks[[2, 3, 4, 5]]


def check_ranked(res, best, kept, obj, entry_check, planes):
    """ranked_scene_*_actions' result `res` against best_scene_*_actions' `best` of a twin trainer and against the kept maps in
    fp64: rank 0 is the best entry (same index, confidence within check_entry's 2^-23), every entry passes check_entry on the
    object's pixels outside the discs of the ranks before it, the lists are separated, and `ranked` is in np.argmax's order."""
    aff = affines(R)
    pair_list = [(g, s) for g in range(4) for s in range(g + 1, 4)]
    assert set(res) == {"per_object", "pairs", "per_pair", "ranked"} and res["pairs"] == pair_list
    yy, xx = np.mgrid[0:HM, 0:HM]

    def check_list(entries, qd, aff_, sel, first, what):
        assert len(entries) <= K_TR
        if first is None:
            assert entries == [], what
            return
        assert entries[0][:2] == first[:2] and abs(entries[0][2] - first[2]) <= 2.0 ** -23 * abs(first[2]), what
        left = sel.copy()
        for j, e in enumerate(entries):
            entry_check(e, qd, aff_, HM, left, "%s rank %d" % (what, j))
            left &= (yy - e[1][0]) ** 2 + (xx - e[1][1]) ** 2 > RADIUS_TR ** 2
        if len(entries) < K_TR:                                                  # exhausted: no pixel with a window is left
            assert not (scene_ref.scene_maps(np.zeros((len(aff_), 10, 10)), aff_, HM)[1] & left[None]).any(), what

    for name in ("grasp", "suction"):
        qd = kept[name].cpu().numpy().reshape((4, R) + planes + (10, 10))
        lists = res["per_object"][name]
        assert len(lists) == 4 and lists[0] == []
        for k in range(4):
            check_list(lists[k], qd[k], aff, obj[k] != 0, best["per_object"][name][k], "%s object %d" % (name, k))
        flat = [(k,) + e for k in range(4) for e in lists[k]]
        assert sorted(res["ranked"][name]) == sorted(flat)
        order, confs = [], [e[3] for e in flat]
        while len(order) < len(flat):
            i = int(np.argmax(confs))
            order.append(flat[i])
            confs[i] = -np.inf
        assert res["ranked"][name] == order
        print("%s: %s ranks per object, ranked confs %s" % (name, [len(x) for x in lists], [round(e[3], 5) for e in order]))
        assert max(len(x) for x in lists) == K_TR and all(len(x) >= 1 for x in lists[1:])
        key = "bestg" if name == "grasp" else "bests"
        assert order[0][:3] == (best[key + "_id"][0], best[key + "_id"][1], best[key + "_pixel"])
    qp = kept["pairs"].cpu().numpy().reshape((6, 1) + planes + (10, 10))
    assert len(res["per_pair"]) == 6
    firsts = []
    for j, (g, s) in enumerate(pair_list):
        entries = res["per_pair"][j]
        assert 1 <= len(entries) <= K_TR
        firsts.append(entries[0])
        check_list(entries, qp[j], aff[:1], (obj[g] != 0) | (obj[s] != 0), entries[0], "pair (%d, %d)" % (g, s))
    top = int(np.argmax([e[2] for e in firsts]))
    assert (best["bestgs_num"], best["bestgs_pixel"]) == (pair_list[top], firsts[top][1])
    assert abs(best["bestgs_conf"] - firsts[top][2]) <= 2.0 ** -23 * abs(firsts[top][2])
    assert res["ranked"]["pairs"][0] == (pair_list[top], firsts[top][1], firsts[top][2])
    confs = [e[2] for e in res["ranked"]["pairs"]]
    assert confs == sorted(confs, reverse=True) and len(confs) == sum(len(x) for x in res["per_pair"])


def test_ranked_scene_actions(gpu):
    depth, obj = scene()
    a, b = make_trainer('reinforcement', 4, R=R), make_trainer('reinforcement', 4, R=R)
    best = a.best_scene_actions(depth, obj)
    res = b.ranked_scene_actions(depth, obj, K_TR, RADIUS_TR)
    check_ranked(res, best, b._last_object_q, obj, one_plane.check_entry, ())
    # without the pair pass and on the target net; one object without a pixel with a window
    alone = b.ranked_scene_actions(depth, obj[:2], 2, 0, is_ets=False, is_target=True)
    assert alone["pairs"] == [] and alone["per_pair"] == [] and alone["ranked"]["pairs"] == [] and set(b._last_object_q) == {"grasp", "suction"}
    assert alone["per_object"]["grasp"][0] == [] and len(alone["per_object"]["grasp"][1]) == 2
    assert [e[0] for e in alone["ranked"]["suction"]] == [1, 1]
    empty = b.ranked_scene_actions(depth, obj[:1], 3, 1)
    assert empty["per_object"] == {"grasp": [[]], "suction": [[]]} and empty["ranked"] == {"grasp": [], "suction": [], "pairs": []}
    with pytest.raises(ValueError):
        b.ranked_to_best(empty, "grasp", 0)
    with pytest.raises(ValueError):
        b.ranked_scene_class_actions(depth, obj, 2, 1)


def test_ranked_scene_class_actions(gpu):
    depth, obj = scene()
    a, b = make_trainer('reactive', 4, R=R), make_trainer('reactive', 4, R=R)
    best = a.best_scene_class_actions(depth, obj)
    res = b.ranked_scene_class_actions(depth, obj, K_TR, RADIUS_TR)
    check_ranked(res, best, b._last_object_q, obj,
                 lambda e, qd, aff_, hm, sel, what: class_plane.check_entry(e, qd, aff_, hm, sel, 0, what), (3,))
    # another class, without the pair pass: rank 0 is best_scene_class_actions' entry for that class
    best1 = a.best_scene_class_actions(depth, obj[1:3], is_ets=False, cls=1)
    res1 = b.ranked_scene_class_actions(depth, obj[1:3], 2, 3, is_ets=False, cls=1)
    assert res1["pairs"] == [] and res1["ranked"]["pairs"] == []
    for name in ("grasp", "suction"):
        for k in (0, 1):
            first, entries = best1["per_object"][name][k], res1["per_object"][name][k]
            assert len(entries) == 2 and entries[0][:2] == first[:2] and abs(entries[0][2] - first[2]) <= 2.0 ** -23 * abs(first[2])
            assert entries[1][2] <= entries[0][2] and entries[1][1] != entries[0][1]
    with pytest.raises(ValueError):
        b.ranked_scene_actions(depth, obj, 2, 1)


@pytest.mark.parametrize("action,style", (("grasp", 0), ("grasp_then_suction", 2)))
def test_a_fallback_goes_through_backprop_scene(gpu, action, style):
    """ranked_to_best on the SECOND entry of the primitive's ranked list: backprop_scene takes it as it takes best_scene_actions'
    dict, and the step is train_batch_scene_pixels on that (object, rotation, pixel) - loss and the head's conv1 weight gradient
    bit for bit."""
    depth, obj = scene()
    a, b = make_trainer('reinforcement', 4, R=R), make_trainer('reinforcement', 4, R=R)
    res = a.ranked_scene_actions(depth, obj, 3, RADIUS_TR)
    top, best = a.ranked_to_best(res, action, 0), a.ranked_to_best(res["ranked"], action, 1)
    assert set(best) == {"bestg_id", "bestg_pixel", "bestg_conf", "bests_id", "bests_pixel", "bests_conf", "bestgs_num", "bestgs_pixel", "bestgs_conf"}
    if style == 2:
        (g, s), rot, pixel, conf = best["bestgs_num"], 0, best["bestgs_pixel"], best["bestgs_conf"]
        m = depth * (obj[g] + obj[s])
        assert (best["bestg_id"], best["bests_id"]) == (None, None) and (top["bestgs_num"], top["bestgs_pixel"]) != ((g, s), pixel)
        assert ((g, s), pixel, conf) == res["ranked"]["pairs"][1] and conf <= top["bestgs_conf"]
    else:
        (k, rot), pixel, conf = best["bestg_id"], best["bestg_pixel"], best["bestg_conf"]
        m = depth * obj[k]
        assert (best["bests_id"], best["bestgs_num"], best["bestgs_conf"]) == (None, None, 0)
        assert (k, rot, pixel, conf) == res["ranked"]["grasp"][1] and conf <= top["bestg_conf"]
    label = conf + 0.4
    loss_a = a.backprop_scene(depth, action, best, label, obj)
    loss_b = b.train_batch_scene_pixels(depth, m, style, [rot], [[pixel]], [label]).cpu().numpy()
    print("%s fallback %s rot %d pixel %s: loss %.7f (backprop_scene), %.7f (train_batch_scene_pixels)" % (action, best, rot, pixel, float(loss_a), float(loss_b[0])))
    assert 0.0 < float(loss_a) < 0.1
    assert_bit_identical(loss_a.reshape(1), loss_b)
    name = ("graspnet_val.grasp-val-", None, "suctionnet_val.suction-val-")[style] + "conv1.weight"
    ga, gb = dict(a.model.named_parameters())[name].grad, dict(b.model.named_parameters())[name].grad
    assert float(ga.abs().max()) > 0
    assert_bit_identical(ga, gb)
