"""The collapsed scene-frame map on the MI355X (run with -m gpu): smg_scene_best_maps and smg_scene_class_best_maps on an engine
alone with synthetic maps - smg_scene_maps' (smg_scene_class_maps') own output pushed through the numpy restatement of
tests/scene_best_ref.py must give the kernels' map indices, and the values bit for bit - then the maximum of every group against
smg_scene_argmax_objects, every refusal, and the Trainer's four best_rotation_* methods against the maps they kept.  The rectangle
masks and the map layouts are test_gpu_scene_objects.py's; the outputs are prefilled with (-5, -5) so that an element no launch
wrote would show."""
import ctypes as C

import numpy as np
import pytest
import torch

from map_harness import assert_bit_identical, bits, cached_engine, filled, gpu, make_trainer, stream  # noqa: F401

import scene_best_ref
import scene_ref
import test_gpu_scene_class_objects as class_plane
import test_gpu_scene_objects as one_plane

pytestmark = pytest.mark.gpu

SHAPES = ((240, 704, 3), (320, 928, 10))     # 57 600 pixels = 56 tiles of 1024 and one of 256; 102 400 = 100 whole tiles
CENTRE, STRADDLE, OUTSIDE, ONE, WHOLE = range(5)
affines, rect_masks, rotation_major, scene_maps = one_plane.affines, one_plane.rect_masks, one_plane.rotation_major, one_plane.scene_maps
ALL80 = dict(mask_a=[m % 5 for m in range(80)], mask_b=[-1] * 80, groups=[m % 5 for m in range(80)])      # m = 5 r + k, group = mask = k


def outputs(n_groups, hm, off=(0, 0)):
    """(val float32, arg int32) [n_groups, hm, hm] prefilled with (-5.0, -5), each `off` elements (0 or 1) past a 16-byte boundary."""
    n = n_groups * hm * hm
    vbuf, abuf = filled((n + 1,), -5.0), torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
    val, arg = vbuf[off[0]:off[0] + n].view(n_groups, hm, hm), abuf[off[1]:off[1] + n].view(n_groups, hm, hm)
    assert val.data_ptr() % 16 == 4 * off[0] and arg.data_ptr() % 16 == 4 * off[1]
    return val, arg


def best(eng, q, aff, hm, masks_dev, mask_a, mask_b, groups, n_groups, cls=None, off=(0, 0)):
    """One smg_scene_best_maps (cls None) or smg_scene_class_best_maps on prefilled outputs -> (val float32, arg int32), both
    [n_groups, hm, hm], on the host.  masks_dev None is the call without a masks tensor."""
    val, arg = outputs(n_groups, hm, off)
    tail = (None if masks_dev is None else masks_dev.data_ptr(), 0 if masks_dev is None else int(masks_dev.shape[0]), mask_a, mask_b, groups,
            n_groups, val.data_ptr(), arg.data_ptr(), stream())
    if cls is None:
        eng.scene_best_maps(q.data_ptr(), q[0].numel(), len(aff), aff, hm, *tail)
    else:
        eng.scene_class_best_maps(q.data_ptr(), len(aff), aff, hm, cls, *tail)
    return val.cpu().numpy(), arg.cpu().numpy()


def assert_same(a, b, what=""):
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(bits(a[0]), bits(b[0])), what


def assert_equals_helper(got, maps, masks, mask_a, mask_b, groups, n_groups, what):
    """The kernel's pair against the helper on the same float32 maps: map indices equal, values bit for bit, every element written."""
    ref = scene_best_ref.group_best(maps, masks, mask_a, mask_b, groups, n_groups)
    print("%s: candidates per group %s, maps that win a pixel per group %s" % (
        what, (got[1] >= 0).reshape(n_groups, -1).sum(1).tolist(), [len(np.unique(a[a >= 0])) for a in got[1]]))
    assert got[0].shape == got[1].shape == ref[0].shape and got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert not (got[1] == -5).any() and not (got[0] == -5.0).any(), what
    assert_same(got, ref, what)
    return ref


def assert_empty(got, g):
    assert (got[1][g] == -1).all() and np.isneginf(got[0][g]).all()


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_rotation_major_groups_against_the_helper(gpu, hm, S, side):
    """16 rotations x 5 masks = 80 maps, rotation-major (m = 5 r + k, group = k): three launches of 32 / 32 / 16 maps, so every
    group's pixels are carried through the outputs twice, and a group's winners come from maps of all three launches."""
    assert scene_ref.geometry(hm)[1:] == (S, side)
    eng = cached_engine(S, 1)
    aff16 = affines()
    q16 = torch.from_numpy(np.random.default_rng(S + 3).standard_normal((16, side, side)).astype(np.float32)).cuda()
    maps16 = scene_maps(eng, q16, aff16, hm)
    masks = rect_masks(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    q80, aff80, rep = rotation_major(q16, aff16, 5)
    got = best(eng, q80, aff80, hm, masks_dev, n_groups=6, **ALL80)
    assert_equals_helper(got, maps16[rep], masks, n_groups=6, what="hm %d, 80 maps" % hm, **ALL80)
    assert_empty(got, OUTSIDE)                                      # no pixel with a window
    assert_empty(got, 5)                                            # a sixth group without a map
    for k in (CENTRE, STRADDLE, ONE, WHOLE):
        assert (got[1][k] >= 0).any() and (got[1][k][masks[k] == 0] == -1).all()
    launches = {int(m) // 32 for m in np.unique(got[1][WHOLE][got[1][WHOLE] >= 0])}
    assert launches == {0, 1, 2}                                    # winners from every launch: the carry held and was beaten
    again = best(eng, q80, aff80, hm, masks_dev, n_groups=6, **ALL80)
    assert_same(got, again)
    # groups that are no function of the mask: (rotation parity) x mask, in descending order, and the every-pixel form (-1, -1)
    groups2 = [9 - (2 * (m % 5) + (m // 5) % 2) for m in range(80)]
    mask_a2 = [-1 if m % 5 == WHOLE else m % 5 for m in range(80)]
    got2 = best(eng, q80, aff80, hm, masks_dev, mask_a2, ALL80["mask_b"], groups2, 11)
    assert_equals_helper(got2, maps16[rep], masks, mask_a2, ALL80["mask_b"], groups2, 11, "hm %d, 11 groups" % hm)
    assert_empty(got2, 10)                                          # a group without a map
    # the whole-image groups of either parity, merged by hand, are the whole-image group of the first call
    lo, hi = 9 - (2 * WHOLE + 1), 9 - 2 * WHOLE
    assert np.array_equal(np.fmax(got2[0][lo], got2[0][hi]), got[0][WHOLE])


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_object_major_groups_split_by_the_launch_boundary(gpu, hm, S, side):
    """20 rotations x 4 objects = 80 maps, object-major (m = 20 k + r, group = k), the layout of the Trainer's call: group 1 (maps
    20 .. 39) is split by the launch boundary at map 32, and the later launches hold no map of the earlier groups - their
    workgroups must leave what the first launch wrote."""
    eng = cached_engine(S, 1)
    aff20 = affines(20)
    q20 = torch.from_numpy(np.random.default_rng(S + 7).standard_normal((20, side, side)).astype(np.float32)).cuda()
    maps20 = scene_maps(eng, q20, aff20, hm)
    masks = rect_masks(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    rep = np.tile(np.arange(20), 4)
    q80, aff80 = q20.repeat(4, 1, 1).contiguous(), aff20[rep]
    which = (CENTRE, STRADDLE, WHOLE, ONE)
    sel = dict(mask_a=[which[m // 20] for m in range(80)], mask_b=[-1] * 80, groups=[m // 20 for m in range(80)])
    got = best(eng, q80, aff80, hm, masks_dev, n_groups=4, **sel)
    assert_equals_helper(got, maps20[rep], masks, n_groups=4, what="hm %d, object-major" % hm, **sel)
    for g in range(4):
        won = np.unique(got[1][g][got[1][g] >= 0])
        assert len(won) and won.min() >= 20 * g and won.max() < 20 * (g + 1)
    won = np.unique(got[1][1][got[1][1] >= 0])
    assert (won < 32).any() and (won >= 32).any()                   # group 1 has winners on both sides of the boundary
    # every pixel of every object (the on_object=False form): no masks tensor at all
    none = dict(mask_a=[-1] * 80, mask_b=[-1] * 80, groups=sel["groups"])
    free = best(eng, q80, aff80, hm, None, n_groups=4, **none)
    assert_equals_helper(free, maps20[rep], None, n_groups=4, what="hm %d, object-major, every pixel" % hm, **none)
    for g in range(1, 4):                                           # four copies of the same 20 maps: the same picture, the indices 20 g on
        assert np.array_equal(bits(free[0][g]), bits(free[0][0]))
        assert np.array_equal(free[1][g], np.where(free[1][0] >= 0, free[1][0] + 20 * g, -1))


def test_unaligned_outputs_and_masks_and_a_ragged_map(gpu):
    """hm = 240: outputs one float / one int and the masks one double off 16-byte alignment take the guarded 4-byte stores (and
    carry loads) and 8-byte mask loads - each output on its own, then everything at once: the same results as the aligned call.
    hm = 239 (57 121 pixels, no multiple of 4, the same S = 704) takes them whatever the alignment, with rows that change inside a
    thread's four pixels and a last thread whose four pixels run past the map."""
    S, side = 704, 3
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
    a = best(eng, q80, aff80, hm, aligned, n_groups=5, **ALL80)
    assert_equals_helper(a, scene_maps(eng, q16, aff16, hm)[rep], masks, n_groups=5, what="hm 240, aligned", **ALL80)
    for m, o in ((aligned, (1, 0)), (aligned, (0, 1)), (off, (0, 0)), (off, (1, 1))):
        assert_same(a, best(eng, q80, aff80, hm, m, n_groups=5, off=o, **ALL80), "masks %d bytes off, outputs %s elements off" % (m.data_ptr() % 16, o))
    hm = 239
    assert scene_ref.geometry(hm)[1:] == (S, side) and hm * hm % 4 == 1
    masks = np.zeros((5, hm, hm))
    for k, (_, (y0, y1, x0, x1), _) in enumerate(one_plane.RECTS[240]):
        masks[k, y0:y1, x0:x1] = 1.0
    masks[WHOLE] = 1.0
    masks[ONE] = 0.0
    masks[ONE, hm - 1, hm - 1] = 1.0                       # the very last pixel (no window is centred there: an empty group)
    maps = scene_maps(eng, q16, aff16, hm)[rep]
    masks_dev = torch.from_numpy(masks).cuda()
    buf = torch.zeros(masks.size + 1, dtype=torch.float64, device="cuda")
    off = buf[1:].view(5, hm, hm)
    off.copy_(masks_dev)
    c = best(eng, q80, aff80, hm, masks_dev, n_groups=5, **ALL80)
    assert_equals_helper(c, maps, masks, n_groups=5, what="hm 239", **ALL80)
    assert_empty(c, ONE)
    assert (c[1][CENTRE] >= 0).any()
    assert_same(c, best(eng, q80, aff80, hm, off, n_groups=5, off=(1, 1), **ALL80), "hm 239, everything off")


def test_ties_take_the_lower_map(gpu):
    """Every rotation of 4 twice in one group with identical q (m and m + 4): every pixel ties, and the lower map keeps it - also
    across the launch boundary, with the copies 32 maps on.  A constant map ties all rotations: rotation 0 wherever it has a window."""
    hm, S, side = 240, 704, 3
    eng = cached_engine(S, 1)
    aff4 = affines()[:4]                                            # 0 / 22.5 / 45 / 67.5 degrees: four different squares of windows
    q4 = torch.from_numpy(np.random.default_rng(41).standard_normal((4, side, side)).astype(np.float32)).cuda()
    maps4 = scene_maps(eng, q4, aff4, hm)
    for copies in (2, 9):                                           # 8 maps in one launch; 36 maps: the copies of launch 1 behind the boundary
        rep = np.tile(np.arange(4), copies)
        n = len(rep)
        sel = dict(mask_a=[-1] * n, mask_b=[-1] * n, groups=[0] * n)
        got = best(eng, q4.repeat(copies, 1, 1).contiguous(), aff4[rep], hm, None, n_groups=1, **sel)
        assert_equals_helper(got, maps4[rep], None, n_groups=1, what="%d copies" % copies, **sel)
        assert 0 <= got[1].max() <= 3                               # never a copy
    qc = torch.full((4, side, side), 0.375, dtype=torch.float32, device="cuda")
    mapc = scene_maps(eng, qc, aff4, hm)
    sel = dict(mask_a=[-1] * 4, mask_b=[-1] * 4, groups=[0] * 4)
    got = best(eng, qc, aff4, hm, None, n_groups=1, **sel)
    assert_equals_helper(got, mapc, None, n_groups=1, what="constant maps", **sel)
    assert (got[1][0][~np.isneginf(mapc[0])] == 0).all() and (got[0][got[1] >= 0] == np.float32(0.375)).all()
    assert (got[1] > 0).any()                                       # and another rotation where rotation 0 has no window


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_a_nan_wins_its_pixels_and_the_first_map_keeps_them(gpu, hm, S, side):
    """A NaN element in two maps of the whole-image group (rotations 2 and 3 of 16): every pixel whose four corners touch the
    element is NaN, the lower map has the pixels both footprints cover, and no other pixel and no other group changes."""
    eng = cached_engine(S, 1)
    aff16 = affines()
    masks = rect_masks(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    rep = np.repeat(np.arange(16), 5)
    q16 = torch.from_numpy(np.random.default_rng(S + 11).standard_normal((16, side, side)).astype(np.float32)).cuda()
    q80 = q16[torch.from_numpy(rep).cuda()].contiguous()
    base = best(eng, q80, aff16[rep], hm, masks_dev, n_groups=5, **ALL80)
    el = (side // 2, side // 2) if side == 3 else (4, 4)
    ma, mb = 5 * 2 + WHOLE, 5 * 3 + WHOLE
    qn = q80.clone()
    qn[ma, el[0], el[1]] = float("nan")
    qn[mb, el[0], el[1]] = float("nan")
    maps = scene_maps(eng, qn, aff16[rep], hm)
    fa, fb = np.isnan(maps[ma]), np.isnan(maps[mb])
    print("hm %d: footprints %d and %d pixels, %d in both, %d in the second alone" % (hm, fa.sum(), fb.sum(), (fa & fb).sum(), (fb & ~fa).sum()))
    assert (fa & fb).any() and (fb & ~fa).any() and (fa & ~fb).any()
    got = best(eng, qn, aff16[rep], hm, masks_dev, n_groups=5, **ALL80)
    assert_equals_helper(got, maps, masks, n_groups=5, what="hm %d, two NaN elements" % hm, **ALL80)
    assert np.array_equal(np.isnan(got[0][WHOLE]), fa | fb)
    assert (got[1][WHOLE][fa] == ma).all() and (got[1][WHOLE][fb & ~fa] == mb).all()
    rest = ~(fa | fb)
    assert np.array_equal(got[1][WHOLE][rest], base[1][WHOLE][rest]) and np.array_equal(bits(got[0][WHOLE][rest]), bits(base[0][WHOLE][rest]))
    others = [CENTRE, STRADDLE, OUTSIDE, ONE]
    assert_same((got[0][others], got[1][others]), (base[0][others], base[1][others]))


def test_union_masks(gpu):
    """test_gpu_scene_objects.py's seven masks (unions that cancel as a sum, 0.5 / 2.0 / NaN select, -0.0 does not) as terms
    (a, b) on four rotations, on random and on constant maps."""
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
    got = best(eng, q[torch.from_numpy(rep).cuda()].contiguous(), aff[rep], hm, masks_dev, n_groups=5, **sel)
    assert_equals_helper(got, scene_maps(eng, q, aff, hm)[rep], masks, n_groups=5, what="unions, random maps", **sel)
    qc = torch.full((5 * R, side, side), 0.375, dtype=torch.float32, device="cuda")
    gotc = best(eng, qc, aff[rep], hm, masks_dev, n_groups=5, **sel)
    assert_equals_helper(gotc, scene_maps(eng, qc[:R], aff, hm)[rep], masks, n_groups=5, what="unions, constant maps", **sel)
    have = gotc[1] >= 0
    assert have[1, 115:130, 115:130].all()                                     # +1 and -1 on the overlap still select it
    assert have[2, 117:123, 117:123].all() and have[2].sum() == 36             # two masks that ARE the overlap: nothing else
    assert np.array_equal(have[3], have[4])                                    # a term at either place
    assert sorted(zip(*np.nonzero(have[3]))) == sorted([(119, 118)] + [(y, x) for y in range(121, 124) for x in range(117, 120)])      # the NaN selects, -0.0 does not


def test_no_masks_tensor_is_the_every_pixel_form(gpu):
    """masks_dev NULL with n_masks 0 - the sweep form, one group of 16 rotations - equals the (-1, -1) terms on a real tensor, and
    np.max / np.argmax over smg_scene_maps' output."""
    hm, S, side = 240, 704, 3
    eng = cached_engine(S, 1)
    aff16 = affines()
    q16 = torch.from_numpy(np.random.default_rng(51).standard_normal((16, side, side)).astype(np.float32)).cuda()
    maps16 = scene_maps(eng, q16, aff16, hm)
    sel = dict(mask_a=[-1] * 16, mask_b=[-1] * 16, groups=[0] * 16)
    a = best(eng, q16, aff16, hm, None, n_groups=1, **sel)
    b = best(eng, q16, aff16, hm, torch.zeros((2, hm, hm), dtype=torch.float64, device="cuda"), n_groups=1, **sel)
    assert_equals_helper(a, maps16, None, n_groups=1, what="no masks tensor", **sel)
    assert_same(a, b)
    top = maps16.max(0)
    assert np.array_equal(bits(a[0][0]), bits(top)) and np.array_equal(a[1][0], np.where(np.isneginf(top), -1, maps16.argmax(0)))


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_class_form_against_the_class_maps(gpu, hm, S, side):
    """smg_scene_class_best_maps for every cls against smg_scene_class_maps' own plane of the same 80 logit maps, a NaN in one
    logit plane of one map: all three probabilities of its footprint are NaN, and that map wins those pixels of its group."""
    eng = cached_engine(S, 3)
    aff16 = affines()
    q16 = class_plane.logits(S + 5, 16, side)
    masks = rect_masks(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    q80, aff80, rep = rotation_major(q16, aff16, 5)
    m_nan = 5 * 4 + WHOLE
    q80[m_nan, 1, side // 2, side // 2] = float("nan")
    for cls in (0, 1, 2):
        maps80 = class_plane.class_maps(eng, q80, aff80, hm, cls)
        foot = np.isnan(maps80[m_nan])
        assert foot.any() and not np.isnan(np.delete(maps80, m_nan, axis=0)).any()
        got = best(eng, q80, aff80, hm, masks_dev, n_groups=6, cls=cls, **ALL80)
        assert_equals_helper(got, maps80, masks, n_groups=6, what="hm %d cls %d" % (hm, cls), **ALL80)
        assert_empty(got, OUTSIDE)
        assert_empty(got, 5)
        assert np.array_equal(np.isnan(got[0][WHOLE]), foot) and (got[1][WHOLE][foot] == m_nan).all() and not np.isnan(got[0][:WHOLE]).any()
        ok = got[1] >= 0
        assert (got[0][ok & ~np.isnan(got[0])] > 0).all() and (got[0][ok & ~np.isnan(got[0])] < 1).all()
        assert_same(got, best(eng, q80, aff80, hm, masks_dev, n_groups=6, cls=cls, **ALL80))
    free = best(eng, q80, aff80, hm, None, [-1] * 80, [-1] * 80, ALL80["groups"], 5, cls=1)
    assert_equals_helper(free, class_plane.class_maps(eng, q80, aff80, hm, 1), None, [-1] * 80, [-1] * 80, ALL80["groups"], 5, "hm %d cls 1, no masks" % hm)


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_group_maximum_is_the_argmax_objects_result(gpu, hm, S, side):
    """Per group the maximum of val is smg_scene_argmax_objects' value, bit for bit, and an empty group is empty in both.  Where
    the maximum is attained at ONE (map, pixel) of the group - asserted on smg_scene_maps' output first - the (map, pixel) read off
    the collapsed map is the argmax's.  (On a tie across pixels the two legitimately differ: the argmax orders by the flattened
    [m][pixel] index, the collapsed map read row-major gives the lowest pixel first, then the lowest map.)"""
    eng = cached_engine(S, 1)
    aff16 = affines()
    q16 = torch.from_numpy(np.random.default_rng(S + 3).standard_normal((16, side, side)).astype(np.float32)).cuda()
    maps80 = scene_maps(eng, q16, aff16, hm)[np.repeat(np.arange(16), 5)]
    masks = rect_masks(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    q80, aff80, _ = rotation_major(q16, aff16, 5)
    idx, top = one_plane.objects(eng, q80, aff80, hm, masks_dev, n_groups=5, **ALL80)
    val, arg = best(eng, q80, aff80, hm, masks_dev, n_groups=5, **ALL80)
    unique = 0
    for g in range(5):
        if idx[g] < 0:
            assert_empty((val, arg), g)
            continue
        assert np.array_equal(bits(val[g].max()), bits(top[g]))
        seen = np.where(masks[g][None] != 0, maps80[g::5], -np.inf)           # the group's 16 maps on its pixels
        assert (seen == top[g]).sum() == 1                                   # attained once: the decode below is determined
        unique += 1
        pix = int(np.argmax(val[g]))
        assert int(arg[g].ravel()[pix]) * hm * hm + pix == idx[g]
    assert unique == 4


def test_refusals(gpu):
    """-22, a message that starts with the function's name and names the cause, nothing launched: the outputs keep their fill."""
    import smg_hip
    L = smg_hip.lib()
    hm, side = 240, 3
    eng, eng3, eng640 = cached_engine(704, 1), cached_engine(704, 3), cached_engine(640, 1)
    big = 37283                                            # 37 283 x 240^2 > 2^31 - 1
    assert big * hm * hm > 0x7fffffff >= (big - 1) * hm * hm
    aff = np.stack([scene_ref.theta(r, 16) for r in range(16)])
    shifted = aff.copy()
    shifted[7, 5] = 0.25
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))         # noqa: E731
    ints = lambda v: (C.c_int * 16)(*([v] * 16))                   # noqa: E731
    one_bad = lambda v: (C.c_int * 16)(*([0] * 15 + [v]))          # noqa: E731
    one_bad_minus = lambda v: (C.c_int * 16)(*([-1] * 15 + [v]))   # noqa: E731
    zero, minus = ints(0), ints(-1)
    q = torch.zeros((16, 3, side, side), device="cuda")
    masks = torch.ones((2, hm, hm), dtype=torch.float64, device="cuda")
    val, arg = outputs(3, hm)
    ok = dict(e=eng.h, q=q.data_ptr(), stride=side * side, n_maps=16, aff=ptr(aff), hm=hm, cls=0, masks=masks.data_ptr(), n_masks=2, a=zero, b=minus,
              g=zero, n_groups=3, val=val.data_ptr(), arg=arg.data_ptr())

    def call(name, a):
        tail = (a["masks"], a["n_masks"], a["a"], a["b"], a["g"], a["n_groups"], a["val"], a["arg"], None)
        if name == b"smg_scene_best_maps":
            return L.smg_scene_best_maps(a["e"], a["q"], a["stride"], a["n_maps"], a["aff"], a["hm"], *tail)
        return L.smg_scene_class_best_maps(a["e"], a["q"], a["n_maps"], a["aff"], a["hm"], a["cls"], *tail)
    for name, e_ok, e_other, e_640 in ((b"smg_scene_best_maps", eng.h, eng3.h, eng640.h),
                                       (b"smg_scene_class_best_maps", eng3.h, eng.h, cached_engine(640, 3).h)):
        def refused(word, **change):
            rc = call(name, dict(dict(ok, e=e_ok), **change))
            msg = L.smg_last_error()
            assert rc == -22 and msg.startswith(name + b":") and word in msg, (name, change.keys(), rc, msg)
        for key in ("q", "aff", "a", "b", "g", "val", "arg"):
            refused(b"NULL", **{key: None})
        refused(b"n_maps < 1", n_maps=0)
        refused(b"head_out", e=e_other)
        refused(b"n_masks < 0", n_masks=-1)
        refused(b"masks_dev is NULL with n_masks > 0", masks=None)
        refused(b"masks_dev is not NULL with n_masks == 0", n_masks=0, a=minus)
        refused(b"mask index", masks=None, n_masks=0)              # no masks tensor: every term must be -1
        refused(b"mask index", masks=None, n_masks=0, a=minus, b=one_bad_minus(0))
        for bad in (2, -2):
            refused(b"mask index", a=one_bad(bad))
            refused(b"mask index", b=one_bad_minus(bad))
        refused(b"n_groups < 1", n_groups=0)
        refused(b"n_groups < 1", n_groups=-4)
        for bad in (3, -1):
            refused(b"group outside", g=one_bad(bad))
        refused(b"int32", n_groups=big)
        refused(b"does not pad", hm=320)
        refused(b"does not pad", hm=224)
        refused(b"1 x 1", e=e_640, hm=224)
        refused(b"translation", aff=ptr(shifted))
        if name == b"smg_scene_best_maps":
            refused(b"negative map_stride", stride=-1)
        else:
            refused(b"cls must be", cls=3)
            refused(b"cls must be", cls=-1)
    with pytest.raises(smg_hip.SmgError):
        eng.scene_best_maps(q.data_ptr(), side * side, 16, shifted, hm, masks.data_ptr(), 2, [0] * 16, [-1] * 16, [0] * 16, 3,
                            val.data_ptr(), arg.data_ptr(), stream())
    with pytest.raises(smg_hip.SmgError):
        eng3.scene_class_best_maps(q.data_ptr(), 16, aff, hm, 0, None, 0, [-1] * 16, [-1] * 16, [3] * 16, 3, val.data_ptr(), arg.data_ptr(), stream())
    with pytest.raises(ValueError):
        eng.scene_best_maps(q.data_ptr(), side * side, 16, aff, hm, None, 0, [-1] * 15, [-1] * 16, [0] * 16, 3, val.data_ptr(), arg.data_ptr(), stream())
    torch.cuda.synchronize()
    assert bool((val == -5.0).all()) and bool((arg == -5).all())
    # and the accepted calls write every element: group 0 the constant map wherever a rotation has a window, groups 1 and 2 (no map) empty
    _, valid, _ = scene_ref.scene_maps(np.zeros((16, side, side)), aff, hm)
    for name, e_ok, value in ((b"smg_scene_best_maps", eng.h, np.float32(0.0)), (b"smg_scene_class_best_maps", eng3.h, class_plane.THIRD)):
        val.fill_(-5.0)
        arg.fill_(-5)
        assert call(name, dict(ok, e=e_ok)) == 0
        v, a = val.cpu().numpy(), arg.cpu().numpy()
        assert np.array_equal(a[0] >= 0, valid.any(0)) and (v[0][a[0] >= 0] == value).all()
        assert np.array_equal(a[0][a[0] >= 0], valid.argmax(0)[a[0] >= 0])    # all 16 maps tie: the first rotation with a window
        assert_empty((v, a), 1)
        assert_empty((v, a), 2)
        assert np.isneginf(v[0][a[0] < 0]).all() and (a[0][a[0] < 0] == -1).all()


# ---- the Trainer's methods ---------------------------------------------------------------------------------------------------------
HM, R = 320, 4


def scene():
    """A 320^2 heightmap and objects 2 to 5 of the synthetic scene: object 2 has no pixel with a window, the others 210 / 351 /
    1020 in every rotation of 4 (test_gpu_scene_objects.py's test_best_scene_actions counts them)."""
    import synthetic
    depth, masks = synthetic.heightmap_scene(8, size=HM)
    return depth, masks[[2, 3, 4, 5]]


def reduce_axis0(maps):
    """np.max / np.argmax of [R, hm, hm] maps over the rotations, -1 where every rotation is -inf."""
    top = maps.max(0)
    return top, np.where(np.isneginf(top), -1, maps.argmax(0)).astype(np.int32)


def test_best_rotation_map(gpu):
    """best_rotation_map on trainer b against forward_scene's max / argmax over axis 0 on its twin a, both styles; then
    is_target=True with a target net that differs from the online one, and the device form."""
    import synthetic
    from helpers import orc
    depth, obj = scene()
    md = depth * obj[3]
    a, b = make_trainer('reinforcement', 4, R=R), make_trainer('reinforcement', 4, R=R)
    tops = []
    for style in (0, 1):
        ref = a.forward_scene(depth, md, style)
        conf, rot = b.best_rotation_map(depth, md, style)
        top, at = reduce_axis0(ref)
        print("style %d: %d pixels with a window, rotations won %s, max conf %.6f" % (style, (rot >= 0).sum(), np.bincount(rot[rot >= 0], minlength=R).tolist(), conf.max()))
        assert conf.dtype == np.float64 and rot.dtype == np.int32 and conf.shape == rot.shape == (HM, HM)
        assert np.array_equal(conf, top) and np.array_equal(rot, at)
        assert (rot == -1).any() and len(np.unique(rot[rot >= 0])) > 1
        tops.append(top)
    other = synthetic.make_state_dict(orc.state_layout(1), 9)
    for t in (a, b):
        t.model_target.load_state_dict({k: torch.from_numpy(v) for k, v in other.items()})
    top_t, at_t = reduce_axis0(a.forward_scene(depth, md, 0, is_target=True))
    val, rot_dev = b.best_rotation_map(depth, md, 0, is_target=True, return_device=True)
    assert val.is_cuda and val.dtype == torch.float32 and rot_dev.dtype == torch.int32 and tuple(val.shape) == tuple(rot_dev.shape) == (HM, HM)
    assert np.array_equal(val.cpu().numpy().astype(np.float64), top_t) and np.array_equal(rot_dev.cpu().numpy(), at_t)
    assert not np.array_equal(top_t, tops[0])                           # the target net's picture, not the online net's


def test_best_rotation_object_maps(gpu):
    """best_rotation_object_maps on trainer b, on_object True and False, against the maps it kept - which are
    forward_objects_dense's on the twin a - pushed through smg_scene_maps and the helper; its per-object maximum against
    best_scene_actions' per_object entries of the twin (confidence bit-equal in float32; rotation and pixel equal where the
    maximum is attained once)."""
    depth, obj = scene()
    a, b = make_trainer('reinforcement', 4, R=R), make_trainer('reinforcement', 4, R=R)
    n = len(obj)
    aff = affines(R)[np.tile(np.arange(R), n)]
    groups = [j // R for j in range(n * R)]
    entries = a.best_scene_actions(depth, obj, is_ets=False)["per_object"]
    for style, name in ((0, "grasp"), (1, "suction")):
        dense = a.forward_objects_dense(depth, obj, style, return_device=True)
        for on_object in (True, False):
            conf, rot = b.best_rotation_object_maps(depth, obj, style, on_object=on_object)
            assert conf.dtype == np.float64 and rot.dtype == np.int32 and conf.shape == rot.shape == (n, HM, HM)
            kept = b._last_object_q[name]
            assert_bit_identical(kept.reshape(dense.shape), dense)
            maps = scene_maps(cached_engine(928, 1), kept.reshape(n * R, 10, 10), aff, HM)
            mask_a = groups if on_object else [-1] * (n * R)
            val, arg = scene_best_ref.group_best(maps, obj if on_object else None, mask_a, [-1] * (n * R), groups, n)
            assert np.array_equal(conf, val.astype(np.float64)) and np.array_equal(rot, np.where(arg >= 0, arg % R, -1))
            print("%s on_object %s: pixels with a candidate per object %s" % (name, on_object, (rot >= 0).reshape(n, -1).sum(1).tolist()))
            if on_object:
                assert all(int((rot[k] >= 0).sum()) >= c and ((rot[k] >= 0).sum() > 0) == (c > 0) for k, c in enumerate((0, 210, 351, 1020)))     # (per rotation: 0 / 210 / 351 / 1020)
                assert all((rot[k][obj[k] == 0] == -1).all() for k in range(n))
                for k in range(n):
                    if entries[name][k] is None:
                        assert (rot[k] == -1).all() and np.isneginf(conf[k]).all()
                        continue
                    r_best, pixel, c_best = entries[name][k]
                    assert np.array_equal(bits(np.float32(conf[k].max())), bits(np.float32(c_best)))
                    seen = np.where(obj[k][None] != 0, maps[R * k:R * (k + 1)], -np.inf)
                    assert (seen == np.float32(c_best)).sum() == 1
                    assert (int(rot[k][pixel]), conf[k][pixel]) == (r_best, c_best) and np.unravel_index(np.argmax(conf[k]), conf[k].shape) == pixel
            else:
                assert all(np.array_equal(rot[k] >= 0, rot[0] >= 0) for k in range(n)) and (rot[0] >= 0).sum() > 1020
    val, rot_dev = b.best_rotation_object_maps(depth, obj, 0, is_target=True, return_device=True)
    assert val.is_cuda and val.dtype == torch.float32 and rot_dev.dtype == torch.int32 and tuple(val.shape) == tuple(rot_dev.shape) == (n, HM, HM)
    for call in (lambda: b.best_rotation_object_maps(depth, obj, 2), lambda: b.best_rotation_map(depth, depth, 2),
                 lambda: b.best_rotation_class_map(depth, depth), lambda: b.best_rotation_class_object_maps(depth, obj),
                 lambda: b.best_rotation_object_maps(depth, obj[:, :200])):
        with pytest.raises(ValueError):
            call()
    d224 = np.zeros((224, 224))
    with pytest.raises(ValueError):
        b.best_rotation_map(d224, d224)
    with pytest.raises(ValueError):
        b.best_rotation_object_maps(d224, np.ones((1, 224, 224)))


def test_best_rotation_class_maps(gpu):
    """The reactive pair of methods: best_rotation_class_object_maps against forward_class_objects(logits=True) of the twin pushed
    through smg_scene_class_maps and the helper, best_rotation_class_map against forward_scene_class_maps(cls) reduced over axis 0."""
    depth, obj = scene()
    a, b = make_trainer('reactive', 4, R=R), make_trainer('reactive', 4, R=R)
    n = len(obj)
    aff = affines(R)[np.tile(np.arange(R), n)]
    groups = [j // R for j in range(n * R)]
    for style, cls, on_object in ((0, 0, True), (1, 1, False), (0, 2, True)):
        logits = a.forward_class_objects(depth, obj, style, logits=True, return_device=True)
        conf, rot = b.best_rotation_class_object_maps(depth, obj, style, on_object=on_object, cls=cls)
        kept = b._last_object_q["grasp" if style == 0 else "suction"]
        assert_bit_identical(kept.reshape(logits.shape), logits)
        maps = class_plane.class_maps(cached_engine(928, 3), kept.reshape(n * R, 3, 10, 10).contiguous(), aff, HM, cls)
        mask_a = groups if on_object else [-1] * (n * R)
        val, arg = scene_best_ref.group_best(maps, obj if on_object else None, mask_a, [-1] * (n * R), groups, n)
        assert conf.dtype == np.float64 and rot.dtype == np.int32 and conf.shape == rot.shape == (n, HM, HM)
        assert np.array_equal(conf, val.astype(np.float64)) and np.array_equal(rot, np.where(arg >= 0, arg % R, -1))
        assert (rot >= 0).any() and (conf[rot >= 0] >= 0).all() and (conf[rot >= 0] <= 1).all()
        if on_object:
            best_k = a.best_scene_class_actions(depth, obj, is_ets=False, cls=cls)["per_object"]["grasp" if style == 0 else "suction"]
            for k in range(n):
                if best_k[k] is None:
                    assert (rot[k] == -1).all()
                else:
                    assert np.array_equal(bits(np.float32(conf[k].max())), bits(np.float32(best_k[k][2])))
    md = depth * obj[3]
    for style, cls in ((0, 0), (1, 2)):
        top, at = reduce_axis0(a.forward_scene_class_maps(depth, md, style, cls=cls))
        conf, rot = b.best_rotation_class_map(depth, md, style, cls=cls)
        assert np.array_equal(conf, top) and np.array_equal(rot, at) and (rot == -1).any() and len(np.unique(rot[rot >= 0])) > 1
    val, rot_dev = b.best_rotation_class_map(depth, md, return_device=True)
    assert val.is_cuda and val.dtype == torch.float32 and rot_dev.dtype == torch.int32
    for call in (lambda: b.best_rotation_class_map(depth, md, cls=3), lambda: b.best_rotation_class_object_maps(depth, obj, cls=-1),
                 lambda: b.best_rotation_class_map(depth, md, style=2), lambda: b.best_rotation_map(depth, md),
                 lambda: b.best_rotation_object_maps(depth, obj), lambda: b.best_rotation_class_object_maps(depth, obj[:0])):
        with pytest.raises(ValueError):
            call()
    d224 = np.zeros((224, 224))
    with pytest.raises(ValueError):
        b.best_rotation_class_map(d224, d224)
    with pytest.raises(ValueError):
        b.best_rotation_class_object_maps(d224, np.ones((1, 224, 224)))
