"""Per-object best actions of the reactive net in the scene frame on the MI355X (run with -m gpu): smg_scene_class_argmax_objects on
an engine alone with synthetic logits - smg_scene_class_maps' own output (gated against fp64 by test_gpu_scene_class_maps.py),
masked on the host and pushed through the numpy restatement of tests/scene_objects_ref.py, must give the kernel's index, and the
value bit for bit - then Trainer.best_scene_class_actions against its own kept logits pushed through scene_class_ref, and
forward_class_objects / forward_class_object_pairs against per-object loops of forward_class_maps and of the reactive forward.
The rectangle masks, their valid-pixel counts and the map layouts are test_gpu_scene_objects.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

from map_harness import assert_bit_identical, cached_engine, filled, gpu, make_trainer, stream  # noqa: F401

import scene_class_ref
import scene_ref
import test_gpu_scene_objects as one_plane

pytestmark = pytest.mark.gpu

SHAPES = one_plane.SHAPES                # hm = 240 / 320: 3 x 3 / 10 x 10 logits, an interior and a ragged last tile
RECTS = one_plane.RECTS
CENTRE, STRADDLE, OUTSIDE, ONE, WHOLE = range(5)
NAME = b"smg_scene_class_argmax_objects"
affines, rect_masks, rotation_major, assert_equals_helper = (one_plane.affines, one_plane.rect_masks, one_plane.rotation_major,
                                                              one_plane.assert_equals_helper)
THIRD = np.float32(1.0 / 3.0)            # (float)(1.0 / 3.0): what three equal logits give in every plane

ALL80 = dict(mask_a=[m % 5 for m in range(80)], mask_b=[-1] * 80, groups=[m % 5 for m in range(80)])      # m = 5 r + k, group = mask = k


def logits(seed, n, side):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, 3, side, side)).astype(np.float32)).cuda()


def class_maps(eng, q, aff, hm, cls):
    """smg_scene_class_maps' plane `cls` for the logits q [n, 3, OH, OW]: the yardstick's input."""
    out = filled((len(aff), hm, hm), 7.0)
    eng.scene_class_maps(q.data_ptr(), len(aff), aff, hm, cls, out.data_ptr(), stream())
    return out.cpu().numpy()


def objects(eng, q, aff, hm, cls, masks_dev, mask_a, mask_b, groups, n_groups):
    """One smg_scene_class_argmax_objects on outputs prefilled with (-5, -5.0) -> (idx int32 [n_groups], val float32 [n_groups])."""
    idx = torch.full((n_groups,), -5, dtype=torch.int32, device="cuda")
    val = filled((n_groups,), -5.0)
    eng.scene_class_argmax_objects(q.data_ptr(), len(aff), aff, hm, cls, masks_dev.data_ptr(), int(masks_dev.shape[0]), mask_a, mask_b,
                                   groups, n_groups, idx.data_ptr(), val.data_ptr(), stream())
    return idx.cpu().numpy(), val.cpu().numpy()


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_groups_of_masked_class_maps_against_the_helper(gpu, hm, S, side):
    """16 rotations x 5 masks = 80 maps, rotation-major (m = 5 r + k, group = k): three launches of 32 / 32 / 16 maps, so every
    group's result is carried twice.  For every class the yardstick is smg_scene_class_maps' own plane."""
    assert scene_ref.geometry(hm)[1:] == (S, side)
    eng = cached_engine(S, 3)
    aff16 = affines()
    q16 = logits(S + 5, 16, side)
    masks = rect_masks(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    q80, aff80, rep = rotation_major(q16, aff16, 5)
    for cls in (0, 1, 2):
        maps16 = class_maps(eng, q16, aff16, hm, cls)
        valid = ~np.isneginf(maps16)
        for name, (y0, y1, x0, x1), (lo, hi) in RECTS[hm]:
            c = valid[:, y0:y1, x0:x1].reshape(16, -1).sum(1)
            assert (int(c.min()), int(c.max())) == (lo, hi), name
        got = objects(eng, q80, aff80, hm, cls, masks_dev, n_groups=5, **ALL80)
        assert_equals_helper(got, maps16[rep], masks, n_groups=5, what="hm %d cls %d, 80 maps" % (hm, cls), **ALL80)
        assert got[0][OUTSIDE] == -1 and np.isneginf(got[1][OUTSIDE])
        assert (got[0][[CENTRE, STRADDLE, ONE, WHOLE]] >= 0).all() and (got[1][[CENTRE, STRADDLE, ONE, WHOLE]] > 0).all()
        # the whole-image group is smg_scene_class_argmax on its 16 maps, the index remapped to the 80
        i16 = torch.full((1,), -5, dtype=torch.int32, device="cuda")
        v16 = filled((1,), -5.0)
        eng.scene_class_argmax(q16.data_ptr(), 16, aff16, hm, cls, i16.data_ptr(), v16.data_ptr(), stream())
        r, pix = divmod(int(i16.cpu()[0]), hm * hm)
        assert got[0][WHOLE] == (5 * r + WHOLE) * hm * hm + pix
        assert_bit_identical(got[1][WHOLE:WHOLE + 1], v16)
        again = objects(eng, q80, aff80, hm, cls, masks_dev, n_groups=5, **ALL80)
        assert np.array_equal(got[0], again[0])
        assert_bit_identical(got[1], again[1])
    # groups that are no function of the mask: (rotation parity) x mask, in descending order, and the every-pixel form (-1, -1)
    groups2 = [9 - (2 * (m % 5) + (m // 5) % 2) for m in range(80)]
    mask_a2 = [-1 if m % 5 == WHOLE else m % 5 for m in range(80)]
    got2 = objects(eng, q80, aff80, hm, 2, masks_dev, mask_a2, ALL80["mask_b"], groups2, 11)
    assert_equals_helper(got2, maps16[rep], masks, mask_a2, ALL80["mask_b"], groups2, 11, "hm %d cls 2, 11 groups" % hm)
    assert got2[0][10] == -1 and np.isneginf(got2[1][10])          # a group without a map


def test_guarded_mask_loads_give_the_same_results(gpu):
    """hm = 240: the masks tensor one double off 16-byte alignment takes the guarded 8-byte loads: the same results as the aligned
    tensor.  hm = 239 (57 121 pixels, no multiple of 4, the same S = 704) takes them too, with a last thread whose four pixels run
    past the map."""
    S, side = 704, 3
    eng = cached_engine(S, 3)
    aff16 = affines()
    q16 = logits(23, 16, side)
    q80, aff80, rep = rotation_major(q16, aff16, 5)
    hm = 240
    masks = rect_masks(hm)
    aligned = torch.from_numpy(masks).cuda()
    buf = torch.zeros(masks.size + 1, dtype=torch.float64, device="cuda")
    off = buf[1:].view(5, hm, hm)
    off.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 8
    a = objects(eng, q80, aff80, hm, 0, aligned, n_groups=5, **ALL80)
    b = objects(eng, q80, aff80, hm, 0, off, n_groups=5, **ALL80)
    assert_equals_helper(b, class_maps(eng, q16, aff16, hm, 0)[rep], masks, n_groups=5, what="hm 240, masks 8 bytes off", **ALL80)
    assert np.array_equal(a[0], b[0])
    assert_bit_identical(a[1], b[1])
    hm = 239
    assert scene_ref.geometry(hm)[1:] == (S, side) and hm * hm % 4 == 1
    masks = np.zeros((5, hm, hm))
    for k, (_, (y0, y1, x0, x1), _) in enumerate(RECTS[240]):
        masks[k, y0:y1, x0:x1] = 1.0
    masks[WHOLE] = 1.0
    masks[ONE] = 0.0
    masks[ONE, hm - 1, hm - 1] = 1.0                       # the very last pixel (no window is centred there: an empty group)
    c = objects(eng, q80, aff80, hm, 0, torch.from_numpy(masks).cuda(), n_groups=5, **ALL80)
    assert_equals_helper(c, class_maps(eng, q16, aff16, hm, 0)[rep], masks, n_groups=5, what="hm 239", **ALL80)
    assert c[0][ONE] == -1 and c[0][CENTRE] >= 0


def test_union_of_two_masks_and_what_selects(gpu):
    """mask_a | mask_b, never their sum: +1 and -1 on an overlap still select it.  0.5, 2.0 and NaN select, -0.0 does not."""
    hm, S, side = 240, 704, 3
    eng = cached_engine(S, 3)
    R = 4
    aff = affines(R)
    masks = np.zeros((7, hm, hm))
    masks[0, 112:128, 110:126] = 0.5                       # centre
    masks[1, 90:110, 100:140] = 2.0                        # straddle
    masks[1, 95, 120] = np.nan
    masks[2, 115:130, 115:130] = 1.0                       # two overlapping rectangles that cancel on the overlap [115:130, 115:130] ...
    masks[2, 100:115, 100:130] = 1.0
    masks[3, 115:130, 115:130] = -1.0
    masks[3, 130:140, 115:140] = -1.0
    masks[4, 117:123, 117:123] = 1.0                       # ... and two that ARE the overlap: nothing else is selected
    masks[5, 117:123, 117:123] = -1.0
    masks[6] = -0.0                                        # -0.0 everywhere but one pixel with a NaN and a block of 3.0 behind it
    masks[6, 119, 118] = np.nan
    masks[6, 121:124, 117:120] = 3.0
    assert (masks[2] + masks[3])[115:130, 115:130].max() == 0 and (masks[4] + masks[5]).max() == 0
    masks_dev = torch.from_numpy(masks).cuda()
    pairs = ((0, 1), (2, 3), (4, 5), (6, -1), (-1, 6))
    mask_a = [pairs[m % 5][0] for m in range(5 * R)]
    mask_b = [pairs[m % 5][1] for m in range(5 * R)]
    groups = [m % 5 for m in range(5 * R)]
    rep = np.repeat(np.arange(R), 5)
    q = logits(33, R, side)
    for cls in (0, 1):
        maps = class_maps(eng, q, aff, hm, cls)
        got = objects(eng, q[torch.from_numpy(rep).cuda()].contiguous(), aff[rep], hm, cls, masks_dev, mask_a, mask_b, groups, 5)
        assert_equals_helper(got, maps[rep], masks, mask_a, mask_b, groups, 5, "unions, random logits, cls %d" % cls)
    # constant logits: P = 1/3 in every plane, all selected valid pixels tie, so each group's result IS its first selected valid
    # pixel of rotation 0
    qc = torch.full((5 * R, 3, side, side), 0.375, dtype=torch.float32, device="cuda")
    mapc = class_maps(eng, qc[:R], aff, hm, 0)
    assert mapc[0, 104:136, 104:136].min() == THIRD == mapc[0, 104:136, 104:136].max()      # rotation 0's windows
    assert np.isneginf(mapc[0, 103]).all() and np.isneginf(mapc[0, :, 103]).all()
    for cls in (0, 1, 2):
        got = objects(eng, qc, aff[rep], hm, cls, masks_dev, mask_a, mask_b, groups, 5)
        assert_equals_helper(got, mapc[rep], masks, mask_a, mask_b, groups, 5, "unions, constant logits, cls %d" % cls)
        assert (got[1] == THIRD).all()
        assert [int(i) // (hm * hm) for i in got[0]] == [0, 1, 2, 3, 4]       # rotation 0's map of each group
        first = [divmod(int(i) % (hm * hm), hm) for i in got[0]]
        assert first[0] == (104, 104)                          # the union's first pixel with a window lies in mask_b
        assert first[1] == (104, 104)
        assert first[2] == (117, 117)                          # +1 and -1: the overlap is selected
        assert first[3] == first[4] == (119, 118)              # the NaN selects, the -0.0 above it does not; a term at either place


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_nan_logits(gpu, hm, S, side):
    """A NaN in ONE plane of one map element makes all three probabilities NaN over its interpolation footprint: where that reaches
    a selected pixel it wins its group, for every class, and only that group; where it misses the mask it changes nothing."""
    eng = cached_engine(S, 3)
    aff16 = affines()
    masks = rect_masks(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    rep = np.repeat(np.arange(16), 5)
    # every map its own copy of its rotation's logits, so that a NaN sits in ONE map
    q80 = logits(S + 13, 16, side)[torch.from_numpy(rep).cuda()].contiguous()
    base = {cls: objects(eng, q80, aff16[rep], hm, cls, masks_dev, n_groups=5, **ALL80) for cls in (0, 1, 2)}
    el = (side // 2, side // 2) if side == 3 else (4, 4)   # an element beside the map's centre: its footprint covers the image centre
    for k, reaches, plane in ((CENTRE, True, 1), (STRADDLE, side == 3, 2)):
        m = 5 * 0 + k                                      # rotation 0's map of group k
        qn = q80.clone()
        qn[m, plane, el[0], el[1]] = float("nan")
        foot = np.isnan(class_maps(eng, qn[m:m + 1], aff16[:1], hm, 0)[0])
        assert foot.any() and bool((foot & (masks[k] != 0)).any()) == reaches, (k, int(foot.sum()))
        for cls in (0, 1, 2):
            assert np.array_equal(np.isnan(class_maps(eng, qn[m:m + 1], aff16[:1], hm, cls)[0]), foot)
            got = objects(eng, qn, aff16[rep], hm, cls, masks_dev, n_groups=5, **ALL80)
            others = [g for g in range(5) if g != k or not reaches]
            assert np.array_equal(got[0][others], base[cls][0][others])
            assert_bit_identical(got[1][others], base[cls][1][others])
            if reaches:
                assert np.isnan(got[1][k]) and got[0][k] == m * hm * hm + int(np.flatnonzero((foot & (masks[k] != 0)).ravel())[0])
    if side == 3:
        # on the 3 x 3 map every element's footprint reaches the straddling rectangle: the corner element of rotation 0 and the
        # one-pixel mask at the image centre give the footprint that misses its mask
        qn = q80.clone()
        qn[ONE, 0, 0, 0] = float("nan")
        foot = np.isnan(class_maps(eng, qn[ONE:ONE + 1], aff16[:1], hm, 0)[0])
        assert foot.any() and not (foot & (masks[ONE] != 0)).any()
        got = objects(eng, qn, aff16[rep], hm, 0, masks_dev, n_groups=5, **ALL80)
        assert np.array_equal(got[0], base[0][0])
        assert_bit_identical(got[1], base[0][1])


def test_refusals(gpu):
    """-22, a message that starts with the function's name and names the cause, nothing launched: the outputs keep their fill."""
    import smg_hip
    L = smg_hip.lib()
    hm, side = 240, 3
    eng, eng640, eng_one = cached_engine(704, 3), cached_engine(640, 3), cached_engine(704, 1)
    big = 37283                                            # 37 283 x 240^2 > 2^31 - 1
    assert big * hm * hm > 0x7fffffff >= (big - 1) * hm * hm
    aff = np.tile(scene_ref.theta(1, 16), (big, 1))
    shifted = aff[:16].copy()
    shifted[7, 5] = 0.25
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))         # noqa: E731
    ints = lambda v: (C.c_int * big)(*([v] * big))                 # noqa: E731
    zero, minus = ints(0), ints(-1)
    q = torch.zeros((16, 3, side, side), device="cuda")
    masks = torch.ones((2, hm, hm), dtype=torch.float64, device="cuda")
    idx = torch.full((3,), -5, dtype=torch.int32, device="cuda")
    val = filled((3,), -5.0)
    ok = dict(e=eng.h, q=q.data_ptr(), n_maps=16, aff=ptr(aff), hm=hm, cls=0, masks=masks.data_ptr(), n_masks=2, a=zero, b=minus,
              g=zero, n_groups=3, idx=idx.data_ptr(), val=val.data_ptr())

    def call(**change):
        a = dict(ok, **change)
        return L.smg_scene_class_argmax_objects(a["e"], a["q"], a["n_maps"], a["aff"], a["hm"], a["cls"], a["masks"], a["n_masks"], a["a"], a["b"],
                                                a["g"], a["n_groups"], a["idx"], a["val"], None)

    def refused(word, **change):
        rc = call(**change)
        msg = L.smg_last_error()
        assert rc == -22 and msg.startswith(NAME + b":") and word in msg, (change.keys(), rc, msg)
    for key in ("e", "q", "aff", "masks", "a", "b", "g", "idx", "val"):
        refused(b"NULL", **{key: None})
    refused(b"head_out", e=eng_one.h)
    refused(b"cls", cls=3)
    refused(b"cls", cls=-1)
    refused(b"n_maps < 1", n_maps=0)
    refused(b"n_masks < 1", n_masks=0)
    refused(b"n_groups < 1", n_groups=0)
    one_bad = lambda v: (C.c_int * 16)(*([0] * 15 + [v]))          # noqa: E731
    for bad in (2, -2):
        refused(b"mask index", a=one_bad(bad))
        refused(b"mask index", b=one_bad(bad))
    for bad in (3, -1):
        refused(b"group outside", g=one_bad(bad))
    refused(b"int32", n_maps=big)
    refused(b"does not pad", hm=320)
    refused(b"does not pad", hm=224)
    refused(b"1 x 1", e=eng640.h, hm=224)
    refused(b"translation", aff=ptr(shifted))
    args = (masks.data_ptr(), 2, [0] * 16, [-1] * 16)
    with pytest.raises(smg_hip.SmgError):
        eng.scene_class_argmax_objects(q.data_ptr(), 16, shifted, hm, 0, *args, [0] * 16, 3, idx.data_ptr(), val.data_ptr(), stream())
    with pytest.raises(smg_hip.SmgError):
        eng.scene_class_argmax_objects(q.data_ptr(), 16, aff[:16], hm, 0, *args, [3] * 16, 3, idx.data_ptr(), val.data_ptr(), stream())
    with pytest.raises(smg_hip.SmgError):
        eng.scene_class_argmax_objects(q.data_ptr(), 16, aff[:16], hm, 3, *args, [0] * 16, 3, idx.data_ptr(), val.data_ptr(), stream())
    with pytest.raises(smg_hip.SmgError):
        eng_one.scene_class_argmax_objects(q.data_ptr(), 16, aff[:16], hm, 0, *args, [0] * 16, 3, idx.data_ptr(), val.data_ptr(), stream())
    torch.cuda.synchronize()
    assert bool((idx == -5).all()) and bool((val == -5.0).all())
    # and the accepted call writes every group: group 0 a result (zero logits: P = 1/3), groups 1 and 2 (no map) the empty pair
    assert call() == 0
    assert idx.cpu().tolist()[1:] == [-1, -1] and int(idx[0]) >= 0 and np.isneginf(val.cpu().numpy()[1:]).all()
    assert val.cpu().numpy()[0] == THIRD


def check_entry(entry, qd, aff, hm, sel, cls, what):
    """One reported (rotation, (iy, ix), conf) against the fp64 scene-frame class maps of the logits qd [R, 3, OH, OW] on the
    selected pixels: the gates of test_gpu_scene_class_maps.py."""
    P, valid, _ = scene_class_ref.scene_class_maps(qd, aff, hm)
    ref = P[:, cls]
    rot, (iy, ix), conf = entry
    assert valid[rot, iy, ix] and sel[iy, ix], what
    at = ref[rot, iy, ix]
    top = ref[valid & sel[None]].max()
    print("%s: rotation %d pixel (%d, %d) conf %.7f, fp64 there %.7f, fp64 max %.7f" % (what, rot, iy, ix, conf, at, top))
    assert abs(conf - at) <= 2.0 ** -23 * abs(at), what
    assert conf >= np.float32(top) - 2.0 ** -23 * abs(top), what


def test_best_scene_class_actions(gpu):
    """A 320^2 heightmap, 4 rotations, objects 2 to 5 of the synthetic scene: object 2 has no pixel with a window, the others 210 /
    351 / 1020 in every rotation.  The reference is the call's own kept logits pushed through scene_class_ref and the masks."""
    import synthetic
    hm, R = 320, 4
    tr = make_trainer('reactive', 4, R=R)
    depth, masks = synthetic.heightmap_scene(8, size=hm)
    obj = masks[[2, 3, 4, 5]]
    aff = affines(R)
    _, valid, _ = scene_ref.scene_maps(np.zeros((R, 10, 10)), aff, hm)
    for k, count in enumerate((0, 210, 351, 1020)):
        assert [int((valid[r] & (obj[k] != 0)).sum()) for r in range(R)] == [count] * R
    keys = ("grasp_depth_trunk.features.norm0", "graspnet_val.grasp-val-norm0", "suction_depth_trunk.features.norm0",
            "suctionnet_val.suction-val-norm0", "gs_depth_trunk.features.norm0")
    nbt = lambda: [int(tr.model.state_dict()[k + ".num_batches_tracked"]) for k in keys]         # noqa: E731
    before = nbt()
    best = tr.best_scene_class_actions(depth, obj)
    # the reference's loops (main.py:158-192): per object and rotation the trunk sees two images and the head one; per pair likewise
    assert [a - b for a, b in zip(nbt(), before)] == [2 * 4 * R, 4 * R, 2 * 4 * R, 4 * R + 6, 2 * 6]
    assert set(best) == {"bestg_id", "bestg_pixel", "bestg_conf", "bests_id", "bests_pixel", "bests_conf", "bestgs_num", "bestgs_pixel",
                         "bestgs_conf", "per_object"}
    kept = tr._last_object_q
    for name, key in (("grasp", "bestg"), ("suction", "bests")):
        qd = kept[name].cpu().numpy().reshape(4, R, 3, 10, 10)
        entries = best["per_object"][name]
        assert len(entries) == 4 and entries[0] is None
        for k in (1, 2, 3):
            check_entry(entries[k], qd[k], aff, hm, obj[k] != 0, 0, "%s object %d" % (name, k))
        top = 1 + int(np.argmax([entries[k][2] for k in (1, 2, 3)]))
        assert best[key + "_id"] == (top, entries[top][0]) and best[key + "_pixel"] == entries[top][1] and best[key + "_conf"] == entries[top][2]
    qp = kept["pairs"].cpu().numpy()
    assert qp.shape == (6, 3, 10, 10)
    pair_list = [(g, s) for g in range(4) for s in range(g + 1, 4)]
    g, s = best["bestgs_num"]
    j = pair_list.index((g, s))
    check_entry((0, best["bestgs_pixel"], best["bestgs_conf"]), qp[j:j + 1], aff[:1], hm, (obj[g] != 0) | (obj[s] != 0), 0, "pair (%d, %d)" % (g, s))
    ref = scene_class_ref.scene_class_maps(qp, np.tile(aff[:1], (6, 1)), hm)[0][:, 0]
    tops = [ref[p][valid[0] & ((obj[a] != 0) | (obj[b] != 0))].max() for p, (a, b) in enumerate(pair_list)]
    assert best["bestgs_conf"] >= np.float32(max(tops)) - 2.0 ** -23 * abs(max(tops))
    # another class on the same scene: the entries are P(class 1) of that call's logits
    other = tr.best_scene_class_actions(depth, obj[1:3], is_ets=False, cls=1)
    assert (other["bestgs_num"], other["bestgs_pixel"], other["bestgs_conf"]) == (None, None, 0)
    assert set(tr._last_object_q) == {"grasp", "suction"}
    qd = tr._last_object_q["suction"].cpu().numpy().reshape(2, R, 3, 10, 10)
    for k in (0, 1):
        check_entry(other["per_object"]["suction"][k], qd[k], aff, hm, obj[1 + k] != 0, 1, "suction object %d, class 1" % k)
    # without the pair pass, and with no object that has a pixel with a window
    alone = tr.best_scene_class_actions(depth, obj[:2], is_ets=False)
    assert (alone["bestgs_num"], alone["bestgs_pixel"], alone["bestgs_conf"]) == (None, None, 0)
    assert alone["bestg_id"][0] == 1 and alone["per_object"]["suction"][0] is None
    empty = tr.best_scene_class_actions(depth, obj[:1])
    assert empty["bestg_id"] is None and empty["bests_pixel"] is None and np.isneginf(empty["bestg_conf"]) and np.isneginf(empty["bests_conf"])
    assert empty["per_object"] == {"grasp": [None], "suction": [None]} and empty["bestgs_num"] is None and empty["bestgs_conf"] == 0
    # the dense forms alone: their shapes (test_batched_class_object_maps_equal_the_per_object_loop has their values)
    god = tr.forward_class_objects(depth, obj, 0, return_device=True)
    assert god.is_cuda and god.dtype == torch.float32 and tuple(god.shape) == (4, R, 3, 10, 10)
    assert float((god.sum(dim=2) - 1).abs().max()) < 1e-6
    one, none = tr.forward_class_object_pairs(depth, obj[:1])
    assert none == [] and one.shape == (0, 3, 10, 10) and one.dtype == np.float64
    # the reinforcement entry points keep refusing a reactive trainer
    with pytest.raises(ValueError):
        tr.best_scene_actions(depth, obj)


def test_batched_class_object_maps_equal_the_per_object_loop(gpu):
    """forward_class_objects against a forward_class_maps(depth, depth * mask[k], style) loop on a twin trainer, at the project's
    own atol = 3e-5 (test_batched_object_maps_equal_the_per_object_loop's, for the same effect: tile shapes, hence the fp32
    summation order, depend on the number of streams in a launch); at 224^2 against the reactive Trainer.forward, the reference's
    own call.  Then the BN running buffers of the two trainers agree as test_gpu_parity.py's batched-object test checks them."""
    import synthetic
    hm, R = 240, 4
    depth, masks = synthetic.heightmap_scene(8, size=hm)
    centre = np.zeros((hm, hm))
    centre[112:128, 110:126] = 1.0
    obj = np.stack([masks[5], centre])
    a, b = make_trainer('reactive', 4, R=R), make_trainer('reactive', 4, R=R)
    for style in (0, 1):
        batch = b.forward_class_objects(depth, obj, style, logits=True)
        loop = np.stack([a.forward_class_maps(depth, depth * obj[k], style, logits=True) for k in range(2)])
        assert batch.shape == loop.shape == (2, R, 3, 3, 3) and batch.dtype == np.float64
        print("style %d: max |batch - loop| %.3e (gate 3e-5), max |logit| %.3e" % (style, float(np.abs(batch - loop).max()), float(np.abs(loop).max())))
        np.testing.assert_allclose(batch, loop, rtol=0, atol=3e-5)
    pairs, idx = b.forward_class_object_pairs(depth, obj, logits=True)
    loop = a.forward_class_maps(depth, depth * (obj[0] + obj[1]), 2, logits=True)
    print("style 2: max |batch - loop| %.3e (gate 3e-5)" % float(np.abs(pairs - loop).max()))
    assert idx == [(0, 1)] and pairs.shape == loop.shape == (1, 3, 3, 3)
    np.testing.assert_allclose(pairs, loop, rtol=0, atol=3e-5)
    # 224^2: a 1 x 1 map, whose rotation 0 is what the reactive forward returns
    d224, m224 = synthetic.heightmap_scene(2)
    m224 = m224[:3]
    assert d224.shape == (224, 224)
    for style in (0, 1):
        p = b.forward_class_objects(d224, m224, style)
        assert p.shape == (3, R, 3, 1, 1)
        np.testing.assert_allclose(p.sum(axis=2), 1.0, rtol=0, atol=1e-6)
        loop = np.array([a.forward(d224, d224 * m224[k], style, is_volatile=True) for k in range(3)])
        print("224^2 style %d: P(success) batch %s loop %s" % (style, p[:, 0, 0, 0, 0].tolist(), loop.tolist()))
        np.testing.assert_allclose(p[:, 0, 0, 0, 0], loop, rtol=0, atol=3e-5)
    sa = {k: v.cpu() for k, v in a.model.state_dict().items()}
    sb = {k: v.cpu() for k, v in b.model.state_dict().items()}
    for k in ("grasp_depth_trunk.features.norm0", "suction_depth_trunk.features.norm0", "suction_depth_trunk.features.denseblock3.denselayer9.norm1",
              "graspnet_val.grasp-val-norm1", "suctionnet_val.suction-val-norm1", "gs_depth_trunk.features.norm5"):
        assert int(sa[k + ".num_batches_tracked"]) == int(sb[k + ".num_batches_tracked"]) > 0
        np.testing.assert_allclose(sb[k + ".running_mean"].numpy(), sa[k + ".running_mean"].numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(sb[k + ".running_var"].numpy(), sa[k + ".running_var"].numpy(), rtol=1e-4, atol=1e-5)
