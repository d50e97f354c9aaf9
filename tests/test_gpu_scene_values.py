"""The value of a given action in the scene frame on the MI355X (run with -m gpu): smg_scene_values / smg_scene_class_values on an
engine alone with seeded normal maps - the expected value is smg_scene_maps' / smg_scene_class_maps' own output on the same q
(gated against fp64 by test_gpu_scene_maps.py / test_gpu_scene_class_maps.py), gathered on the host by tests/scene_values_ref.py,
bit for bit - then the Trainer's scene_*_values methods against the maps they kept, and get_label_value_scene / backprop_scene
against the calls they stand for."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import orc
from map_harness import assert_bit_identical, bits, cached_engine, filled, gpu, make_trainer, stream  # noqa: F401

import scene_ref
import scene_values_ref
import test_gpu_scene_maps as one_plane

pytestmark = pytest.mark.gpu

SHAPES = one_plane.SHAPES                # hm = 240 -> S = 704, 3 x 3 maps; hm = 320 -> S = 928, 10 x 10
FILL = 7.0


def affines(n=16):
    return np.stack([scene_ref.theta(r, n) for r in range(n)])


def normal(seed, shape, scale=1.0):
    return torch.from_numpy((scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)).cuda()


def every_pixel(n, hm):
    """int32 [n, hm * hm, 2]: every pixel of every map, row-major."""
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    return np.ascontiguousarray(np.broadcast_to(np.stack([iy.ravel(), ix.ravel()], axis=-1), (n, hm * hm, 2)).astype(np.int32))


def seeded_pixels(seed, n, K, hm):
    """int32 [n, K, 2] in [-3, hm + 3), with a few points at the ends of int32."""
    rng = np.random.default_rng(seed)
    pix = rng.integers(-3, hm + 3, size=(n, K, 2)).astype(np.int32)
    for m, k, c, v in ((0, 0, 0, -2 ** 31), (0, 1, 1, 2 ** 31 - 1), (n - 1, K - 1, 0, 2 ** 31 - 1), (n - 1, K - 1, 1, -2 ** 31), (n // 2, K // 2, 1, -2 ** 31)):
        pix[m, k, c] = v
    return pix


def gpu_maps(eng, q, aff, hm, map_stride=None):
    out = filled((len(aff), hm, hm), FILL)
    eng.scene_maps(q.data_ptr(), q[0].numel() if map_stride is None else map_stride, len(aff), aff, hm, out.data_ptr(), stream())
    return out.cpu().numpy()


def gpu_class_maps(eng, q, aff, hm, cls):
    out = filled((len(aff), 3, hm, hm) if cls < 0 else (len(aff), hm, hm), FILL)
    eng.scene_class_maps(q.data_ptr(), len(aff), aff, hm, cls, out.data_ptr(), stream())
    return out.cpu().numpy()


def gpu_values(eng, q, aff, hm, pix, map_stride=None):
    """One smg_scene_values at the host pixels pix [n, K, 2] -> float32 [n, K], every element written."""
    n, K = pix.shape[:2]
    out = filled((n, K), FILL)
    p = torch.from_numpy(np.ascontiguousarray(pix, dtype=np.int32)).cuda()
    eng.scene_values(q.data_ptr(), q[0].numel() if map_stride is None else map_stride, n, aff, hm, K, p.data_ptr(), out.data_ptr(), stream())
    got = out.cpu().numpy()
    assert not (got == FILL).any()
    return got


def gpu_class_values(eng, q, aff, hm, cls, pix):
    n, K = pix.shape[:2]
    out = filled((n, 3, K) if cls < 0 else (n, K), FILL)
    p = torch.from_numpy(np.ascontiguousarray(pix, dtype=np.int32)).cuda()
    eng.scene_class_values(q.data_ptr(), n, aff, hm, cls, K, p.data_ptr(), out.data_ptr(), stream())
    got = out.cpu().numpy()
    assert not (got == FILL).any()
    return got


def assert_same_but_for_nan(got, want):
    """NaN exactly where `want` is NaN, every other element bit for bit."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])
    return nan


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_whole_image_equals_scene_maps(gpu, hm, S, side):
    """16 maps, K = hm^2: every pixel of every map listed row-major, so the output reshaped IS smg_scene_maps' output."""
    assert scene_ref.geometry(hm)[1:] == (S, side)
    eng = cached_engine(S, 1)
    aff = affines()
    pix = every_pixel(16, hm)
    q = normal(S, (16, side, side))
    got = gpu_values(eng, q, aff, hm, pix).reshape(16, hm, hm)
    maps = gpu_maps(eng, q, aff, hm)
    assert np.isneginf(maps).any() and np.isfinite(maps).any()
    assert_bit_identical(got, maps)
    one_plane.check_maps(got, q.cpu().numpy(), aff, hm, "values, S=%d" % S)
    assert_bit_identical(gpu_values(eng, q, aff, hm, pix).reshape(16, hm, hm), got)          # two calls, one result
    # one class plane of a [16, 3, side, side] tensor: map_stride = 3 side^2
    q3 = normal(S + 1, (16, 3, side, side))
    got = gpu_values(eng, q3[:, 1], aff, hm, pix, map_stride=3 * side * side).reshape(16, hm, hm)
    assert_bit_identical(got, gpu_maps(eng, q3[:, 1], aff, hm, map_stride=3 * side * side))
    one_plane.check_maps(got, q3[:, 1].cpu().numpy(), aff, hm, "values, S=%d, plane 1 of 3" % S)


@pytest.mark.parametrize("K", (5, 257))
def test_ragged_launches_unaligned_buffers_and_points_outside(gpu, K):
    """hm = 240, 70 maps: three launches of 32 + 32 + 6; K = 5 (one ragged workgroup per map) and 257 (two, the second with one
    point).  Points in [-3, hm + 3) and at the ends of int32; the pixel buffer 4 bytes off 8-byte alignment, the output 4 bytes off
    16-byte alignment between guard floats."""
    hm, S, side, n = 240, 704, 3, 70
    eng = cached_engine(S, 1)
    aff = affines(n)
    q = normal(K, (n, side, side))
    pix = seeded_pixels(100 + K, n, K, hm)
    pbuf = torch.zeros(2 * n * K + 1, dtype=torch.int32, device="cuda")
    p = pbuf[1:]
    p.copy_(torch.from_numpy(pix.reshape(-1)))
    obuf = filled((n * K + 2,), FILL)
    out = obuf[1:1 + n * K]
    assert p.data_ptr() % 8 == 4 and out.data_ptr() % 16 == 4
    eng.scene_values(q.data_ptr(), side * side, n, aff, hm, K, p.data_ptr(), out.data_ptr(), stream())
    got = out.cpu().numpy().reshape(n, K)
    assert float(obuf[0]) == FILL and float(obuf[-1]) == FILL
    want = scene_values_ref.gather(gpu_maps(eng, q, aff, hm), pix)
    outside = ((pix < 0) | (pix >= hm)).any(axis=2)
    print("K=%d: %d of %d points outside the heightmap, %d inside without a window, %d with a value"
          % (K, int(outside.sum()), outside.size, int((np.isneginf(want) & ~outside).sum()), int(np.isfinite(want).sum())))
    assert outside.sum() >= 5 and (np.isneginf(want) & ~outside).any() and np.isfinite(want).any()
    assert np.isneginf(got[outside]).all()
    assert_bit_identical(got, want)


def test_a_nan_map_element(gpu):
    hm, S, side = 240, 704, 3
    eng = cached_engine(S, 1)
    aff = affines()
    pix = every_pixel(16, hm)
    q = normal(9, (16, side, side))
    q[9, 1, 1] = float("nan")
    maps = gpu_maps(eng, q, aff, hm)
    got = gpu_values(eng, q, aff, hm, pix).reshape(16, hm, hm)
    nan = assert_same_but_for_nan(got, maps)
    assert nan[9].any() and not np.delete(nan, 9, axis=0).any() and np.isneginf(got[9]).any()


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_class_values_equal_scene_class_maps(gpu, hm, S, side):
    eng = cached_engine(S, 3)
    aff = affines()
    pix = every_pixel(16, hm)
    q = normal(S + 2, (16, 3, side, side), 2.0)
    for cls in (0, 1, 2):
        assert_bit_identical(gpu_class_values(eng, q, aff, hm, cls, pix).reshape(16, hm, hm), gpu_class_maps(eng, q, aff, hm, cls))
    allc = gpu_class_values(eng, q, aff, hm, -1, pix).reshape(16, 3, hm, hm)
    maps = gpu_class_maps(eng, q, aff, hm, -1)
    assert np.isneginf(maps).any() and np.isfinite(maps).any()
    assert_bit_identical(allc, maps)
    # a NaN in one logit plane makes all three probabilities NaN wherever a corner holds it
    q[5, 2, side // 2, side // 2] = float("nan")
    nan = assert_same_but_for_nan(gpu_class_values(eng, q, aff, hm, -1, pix).reshape(16, 3, hm, hm), gpu_class_maps(eng, q, aff, hm, -1))
    assert nan[5].any() and np.array_equal(nan[:, 0], nan[:, 1]) and np.array_equal(nan[:, 0], nan[:, 2]) and not np.delete(nan, 5, axis=0).any()
    assert_same_but_for_nan(gpu_class_values(eng, q, aff, hm, 0, pix).reshape(16, hm, hm), gpu_class_maps(eng, q, aff, hm, 0))


def test_class_values_of_33_maps_at_seeded_points(gpu):
    """33 maps: a second launch of one map; K = 257 seeded points, some outside the heightmap."""
    hm, S, side, n, K = 240, 704, 3, 33, 257
    eng = cached_engine(S, 3)
    aff = affines(n)
    q = normal(33, (n, 3, side, side), 2.0)
    pix = seeded_pixels(34, n, K, hm)
    outside = ((pix < 0) | (pix >= hm)).any(axis=2)
    for cls in (0, 1, 2, -1):
        got = gpu_class_values(eng, q, aff, hm, cls, pix)
        assert got.shape == ((n, 3, K) if cls < 0 else (n, K))
        assert_bit_identical(got, scene_values_ref.gather(gpu_class_maps(eng, q, aff, hm, cls), pix))
        assert np.isneginf(got[:, 0][outside] if cls < 0 else got[outside]).all() and np.isfinite(got).any()


def test_refusals(gpu):
    """-22, a message that starts with the function's name and names the cause, nothing launched: `out` keeps its fill."""
    import smg_hip
    L = smg_hip.lib()
    hm, side = 240, 3
    eng, eng3, eng640, eng640_3 = cached_engine(704, 1), cached_engine(704, 3), cached_engine(640, 1), cached_engine(640, 3)
    aff = affines()
    shifted = aff.copy()
    shifted[7, 5] = 0.25
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))         # noqa: E731
    q = torch.zeros((16, 3, side, side), device="cuda")
    pix = torch.full((16, 4, 2), 120, dtype=torch.int32, device="cuda")
    out = filled((16, 3, 4), FILL)
    big = 2 ** 27                                                   # 16 x 2^27 = 2^31 > 2^31 - 1 >= 16 x (2^27 - 1) + 15
    assert 16 * big > 0x7fffffff >= 15 * big
    ok = dict(e=eng.h, q=q.data_ptr(), stride=side * side, n_maps=16, aff=ptr(aff), hm=hm, cls=0, K=4, pix=pix.data_ptr(), out=out.data_ptr())

    def one(a):
        return L.smg_scene_values(a["e"], a["q"], a["stride"], a["n_maps"], a["aff"], a["hm"], a["K"], a["pix"], a["out"], None)

    def three(a):
        return L.smg_scene_class_values(a["e"], a["q"], a["n_maps"], a["aff"], a["hm"], a["cls"], a["K"], a["pix"], a["out"], None)

    def refused(call, name, base, word, **change):
        rc = call(dict(base, **change))
        msg = L.smg_last_error()
        assert rc == -22 and msg.startswith(name + b":") and word in msg, (name, sorted(change), rc, msg)
    for call, name, base, small in ((one, b"smg_scene_values", ok, eng640.h), (three, b"smg_scene_class_values", dict(ok, e=eng3.h), eng640_3.h)):
        for key in ("e", "q", "aff", "pix", "out"):
            refused(call, name, base, b"NULL", **{key: None})
        refused(call, name, base, b"n_maps < 1", n_maps=0)
        refused(call, name, base, b"n_maps < 1", n_maps=-3)
        refused(call, name, base, b"K < 1", K=0)
        refused(call, name, base, b"K < 1", K=-1)
        refused(call, name, base, b"int32", K=big)
        refused(call, name, base, b"does not pad", hm=320)
        refused(call, name, base, b"does not pad", hm=224)
        refused(call, name, base, b"1 x 1", e=small, hm=224)
        refused(call, name, base, b"translation", aff=ptr(shifted))
    refused(one, b"smg_scene_values", ok, b"negative map_stride", stride=-1)
    for cls in (-2, 3):
        refused(three, b"smg_scene_class_values", dict(ok, e=eng3.h), b"cls", cls=cls)
    refused(three, b"smg_scene_class_values", ok, b"head_out")                         # a one-channel engine
    with pytest.raises(smg_hip.SmgError):
        eng.scene_values(q.data_ptr(), side * side, 16, shifted, hm, 4, pix.data_ptr(), out.data_ptr(), stream())
    with pytest.raises(smg_hip.SmgError):
        eng3.scene_class_values(q.data_ptr(), 16, aff, hm, 3, 4, pix.data_ptr(), out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # the accepted calls write every element: a zero map is 0 at the image centre, three equal logits a third each
    assert one(ok) == 0 and bool((out.reshape(-1)[:64] == 0.0).all()) and bool((out.reshape(-1)[64:] == FILL).all())
    assert three(dict(ok, e=eng3.h, cls=-1)) == 0
    assert_bit_identical(out, np.full((16, 3, 4), 1.0 / 3.0, dtype=np.float32))
    # any head width is accepted by the one-plane form
    assert one(dict(ok, e=eng3.h, stride=3 * side * side)) == 0


# ---- the Trainer ---------------------------------------------------------------------------------------------------------------
HM, R = 320, 4                     # the scene of test_best_scene_actions: S = 928, 10 x 10 maps, objects 2 to 5 of the synthetic scene
POINTS = [(100, 200), (160, 160), (231, 88), (120, 95), (0, 0), (87, 160)]       # four with a window in every quarter turn, two without
NBT_KEYS = ("grasp_depth_trunk.features.norm0", "graspnet_val.grasp-val-norm0", "suction_depth_trunk.features.norm0",
            "suctionnet_val.suction-val-norm0", "gs_depth_trunk.features.norm0")
PAIRS = [(g, s) for g in range(4) for s in range(g + 1, 4)]


def scene():
    import synthetic
    depth, masks = synthetic.heightmap_scene(8, size=HM)
    return depth, masks[[2, 3, 4, 5]]


def nbt(model):
    return [int(model.state_dict()[k + ".num_batches_tracked"]) for k in NBT_KEYS]


def object_pixels(entries):
    """One (iy, ix) per object from best_scene_actions' per_object list; (0, 0) - no window there - for an object without one."""
    return np.asarray([(0, 0) if e is None else e[1] for e in entries])


def test_trainer_scene_values(gpu):
    depth, obj = scene()
    tr = make_trainer('reinforcement', 4, R=R)
    eng = cached_engine(928, 1)
    aff = affines(R)
    md = depth * obj[1]
    pts = np.asarray(POINTS)
    _, valid, _ = scene_ref.scene_maps(np.zeros((R, 10, 10)), aff, HM)
    assert valid[:, pts[:4, 0], pts[:4, 1]].all() and not valid[:, pts[4:, 0], pts[4:, 1]].any()

    def kept_maps(rows):
        q = tr._last_q
        assert tuple(q.shape) == (len(rows), 1, 10, 10)
        return scene_values_ref.gather(gpu_maps(eng, q, aff[rows], HM), np.broadcast_to(pts, (len(rows), 6, 2)))
    for style in (0, 1):
        v = tr.scene_values(depth, md, POINTS, style)
        assert v.dtype == np.float64 and v.shape == (R, 6)
        assert np.isneginf(v[:, 4:]).all() and np.isfinite(v[:, :4]).all()
        assert_bit_identical(v.astype(np.float32), kept_maps(list(range(R))))
    dev = tr.scene_values(depth, md, POINTS, 0, return_device=True)
    assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (R, 6)
    one = tr.scene_values(depth, md, POINTS[1], 0, specific_rotation=2)              # one (iy, ix)
    assert one.shape == (1, 1)
    assert_bit_identical(one.astype(np.float32), kept_maps([2])[:, 1:2])
    before = nbt(tr.model), nbt(tr.model_target)
    gs = tr.scene_values(depth, md, POINTS, 2, is_target=True)
    assert gs.shape == (1, 6)
    assert_bit_identical(gs.astype(np.float32), kept_maps([0]))
    assert nbt(tr.model) == before[0] and [a - b for a, b in zip(nbt(tr.model_target), before[1])] == [0, 0, 0, 1, 2]


def test_trainer_scene_object_values(gpu):
    depth, obj = scene()
    tr = make_trainer('reinforcement', 4, R=R)
    eng = cached_engine(928, 1)
    aff = affines(R)
    best = tr.best_scene_actions(depth, obj)
    rep = np.tile(np.arange(R), 4)
    for style, name in ((0, "grasp"), (1, "suction")):
        entries = best["per_object"][name]
        assert entries[0] is None and all(e is not None for e in entries[1:])
        pix = object_pixels(entries)
        before = nbt(tr.model)
        vals = tr.scene_object_values(depth, obj, pix, style)
        grew = [a - b for a, b in zip(nbt(tr.model), before)]
        assert grew == ([2 * 4 * R, 4 * R, 0, 0, 0] if style == 0 else [0, 0, 2 * 4 * R, 4 * R, 0])
        assert vals.dtype == np.float64 and vals.shape == (4, R) and np.isneginf(vals[0]).all()
        q = tr._last_object_q[name]
        assert tuple(q.shape) == (4 * R, 1, 10, 10)
        maps = gpu_maps(eng, q, aff[rep], HM)
        assert_bit_identical(vals.astype(np.float32).reshape(4 * R, 1), scene_values_ref.gather(maps, np.repeat(pix, R, axis=0)[:, None, :]))
        for k in (1, 2, 3):
            rot, _, conf = entries[k]
            print("%s object %d: value at the best pixel %.7f, best_scene_actions' conf %.7f, |d| %.2e (gate 3e-5)"
                  % (name, k, vals[k, rot], conf, abs(vals[k, rot] - conf)))
            assert abs(vals[k, rot] - conf) <= 3e-5
        # K points per object
        many = np.stack([np.asarray(POINTS)[[k, k + 1, 5]] for k in range(4)])
        dev = tr.scene_object_values(depth, obj, many, style, return_device=True)
        assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (4, R, 3)
        maps = gpu_maps(eng, tr._last_object_q[name], aff[rep], HM)
        assert_bit_identical(dev.reshape(4 * R, 3), scene_values_ref.gather(maps, np.repeat(many, R, axis=0)))
        assert np.isneginf(dev.cpu().numpy()[:, :, 2]).all()
    # pairs: style 2, rotation 0, one point per pair in forward_object_pairs' order
    ppix = np.asarray([POINTS[j % 4] for j in range(6)])
    before = nbt(tr.model)
    vals, idx = tr.scene_object_pair_values(depth, obj, ppix)
    assert [a - b for a, b in zip(nbt(tr.model), before)] == [0, 0, 0, 6, 2 * 6]
    assert idx == PAIRS and vals.dtype == np.float64 and vals.shape == (6,)
    q = tr._last_object_q["pairs"]
    assert tuple(q.shape) == (6, 1, 10, 10)
    assert_bit_identical(vals.astype(np.float32)[:, None], scene_values_ref.gather(gpu_maps(eng, q, np.tile(aff[:1], (6, 1)), HM), ppix[:, None, :]))
    j = PAIRS.index(best["bestgs_num"])
    ppix[j] = best["bestgs_pixel"]
    vals, _ = tr.scene_object_pair_values(depth, obj, ppix[:, None, :], is_target=True)           # (the target net is in sync)
    assert vals.shape == (6, 1)
    print("pair %s: value at the best pixel %.7f, conf %.7f" % (best["bestgs_num"], vals[j, 0], best["bestgs_conf"]))
    assert abs(vals[j, 0] - best["bestgs_conf"]) <= 3e-5
    none, idx = tr.scene_object_pair_values(depth, obj[:1], np.zeros((0, 2)))
    assert idx == [] and none.shape == (0,)


def test_get_label_value_scene_uses_the_target_net(gpu):
    """The target net carries seed 5 where the online net carries seed 4, so the two disagree at the chosen actions - by 0.13 (pair), 0.92
    (suction) and 4.3 (grasp) in the fp32 oracle at S = 928 on the CPU - and a label built from the online net's value would miss the 3e-5 gate."""
    import synthetic
    depth, obj = scene()
    tr = make_trainer('reinforcement', 4, R=R)
    sd = synthetic.make_state_dict(orc.state_layout(1), 5)
    tr.model_target.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    best = tr.best_scene_actions(depth, obj)
    before = nbt(tr.model), nbt(tr.model_target)
    for args in (("grasp", 3, 0, 0, 0), ("suction", 1, 1, 0, 0), ("grasp", 1, 0, 1, 0), ("grasp_then_suction", 2, 0, 0, 2.5)):
        assert tr.get_label_value_scene(args[0], args[1], args[2], args[3], args[4], depth, obj, best, 'grasp') == \
            orc.label_value("reinforcement", args[0], args[1], args[2], args[3], args[4], 123.0, 0.5)
    assert (nbt(tr.model), nbt(tr.model_target)) == before
    for exploit, style in (("grasp", 0), ("suction", 1), ("grasp_then_suction", 2)):
        if style == 2:
            (g, s), rot, pixel = best["bestgs_num"], 0, best["bestgs_pixel"]
            m = depth * (obj[g] + obj[s])
        else:
            key = ("bestg", "bests")[style]
            (k, rot), pixel = best[key + "_id"], best[key + "_pixel"]
            m = depth * obj[k]
        label, reward = tr.get_label_value_scene("grasp", 3, 0, 1, 0, depth, obj, best, exploit)
        assert reward == 1
        v = (label - reward) / 0.5
        target = tr.forward_scene(depth, m, style, is_target=True, specific_rotation=rot)[0, pixel[0], pixel[1]]
        online = tr.forward_scene(depth, m, style, is_target=False, specific_rotation=rot)[0, pixel[0], pixel[1]]
        print("%s: label %.7f = 1 + 0.5 x %.7f; target net there %.7f (|d| %.2e, gate 3e-5), online net %.7f"
              % (exploit, label, v, target, abs(v - target), online))
        assert abs(online - v) > 1e-3
        assert abs(v - target) <= 3e-5


@pytest.mark.parametrize("action,style", (("grasp", 0), ("grasp_then_suction", 2)))
def test_backprop_scene_is_one_train_batch_scene_pixels(gpu, action, style):
    depth, obj = scene()
    a, b = make_trainer('reinforcement', 4, R=R), make_trainer('reinforcement', 4, R=R)
    best = a.best_scene_actions(depth, obj)
    if style == 2:
        (g, s), rot, pixel = best["bestgs_num"], 0, best["bestgs_pixel"]
        m = depth * (obj[g] + obj[s])
    else:
        (k, rot), pixel = best["bestg_id"], best["bestg_pixel"]
        m = depth * obj[k]
    label = best[("bestg_conf", None, "bestgs_conf")[style]] + 0.4
    mask4 = obj.copy().reshape(4, HM, HM, 1)
    loss_a = a.backprop_scene(depth, action, best, label, mask4)
    assert mask4.shape == (4, HM, HM, 1) and isinstance(loss_a, np.ndarray) and loss_a.shape == () and loss_a.dtype == np.float32
    loss_b = b.train_batch_scene_pixels(depth, m, style, [rot], [[pixel]], [label]).cpu().numpy()
    print("%s: loss %.7f (backprop_scene), %.7f (train_batch_scene_pixels)" % (action, float(loss_a), float(loss_b[0])))
    assert loss_b.shape == (1,) and 0.0 < float(loss_a) < 0.1              # |d| = 0.4 up to the 3e-5 between two forwards: 0.08
    assert_bit_identical(loss_a.reshape(1), loss_b)
    name = ("graspnet_val.grasp-val-", "suctionnet_val.suction-val-", "suctionnet_val.suction-val-")[style] + "conv1.weight"
    ga, gb = dict(a.model.named_parameters())[name].grad, dict(b.model.named_parameters())[name].grad
    assert float(ga.abs().max()) > 0
    assert_bit_identical(ga, gb)


def test_trainer_reactive(gpu):
    depth, obj = scene()
    tr = make_trainer('reactive', 4, R=R)
    eng = cached_engine(928, 3)
    aff = affines(R)
    md = depth * obj[1]
    pts = np.broadcast_to(np.asarray(POINTS), (R, 6, 2))
    p = tr.scene_class_values(depth, md, POINTS)
    q = tr._last_q
    assert p.dtype == np.float64 and p.shape == (R, 3, 6) and tuple(q.shape) == (R, 3, 10, 10)
    assert np.isneginf(p[:, :, 4:]).all() and np.abs(p[:, :, :4].sum(axis=1) - 1).max() <= 3 * 2.0 ** -24
    assert_bit_identical(p.astype(np.float32), scene_values_ref.gather(gpu_class_maps(eng, q, aff, HM, -1), pts))
    p1 = tr.scene_class_values(depth, md, POINTS, style=1, cls=1, return_device=True)
    assert p1.is_cuda and p1.dtype == torch.float32 and tuple(p1.shape) == (R, 6)
    assert_bit_identical(p1, scene_values_ref.gather(gpu_class_maps(eng, tr._last_q, aff, HM, 1), pts))
    z = tr.scene_class_values(depth, md, POINTS, specific_rotation=3, logits=True)
    q = tr._last_q
    assert z.shape == (1, 3, 6) and tuple(q.shape) == (1, 3, 10, 10)
    for c in range(3):
        maps = gpu_maps(eng, q[:, c], aff[3:4], HM, map_stride=300)
        assert_bit_identical(z[:, c].astype(np.float32), scene_values_ref.gather(maps, pts[:1]))
    z2 = tr.scene_class_values(depth, md, POINTS, specific_rotation=3, cls=2, logits=True)
    assert z2.shape == (1, 6)
    # per object, at best_scene_class_actions' own pixels
    best = tr.best_scene_class_actions(depth, obj)
    for style, name in ((0, "grasp"), (1, "suction")):
        entries = best["per_object"][name]
        vals = tr.scene_class_object_values(depth, obj, object_pixels(entries), style)
        assert vals.shape == (4, R) and np.isneginf(vals[0]).all() and tuple(tr._last_object_q[name].shape) == (4 * R, 3, 10, 10)
        for k in (1, 2, 3):
            rot, _, conf = entries[k]
            print("%s object %d: P(class 0) at the best pixel %.7f, conf %.7f, |d| %.2e (gate 3e-5)" % (name, k, vals[k, rot], conf, abs(vals[k, rot] - conf)))
            assert abs(vals[k, rot] - conf) <= 3e-5
    ppix = np.asarray([POINTS[j % 4] for j in range(6)])
    j = PAIRS.index(best["bestgs_num"])
    ppix[j] = best["bestgs_pixel"]
    vals, idx = tr.scene_class_object_pair_values(depth, obj, ppix)
    assert idx == PAIRS and vals.shape == (6,) and abs(vals[j] - best["bestgs_conf"]) <= 3e-5
    qp = tr._last_object_q["pairs"]
    assert_bit_identical(vals.astype(np.float32)[:, None], scene_values_ref.gather(gpu_class_maps(eng, qp, np.tile(aff[:1], (6, 1)), HM, 0), ppix[:, None, :]))
    # the one-sample step on the executed action
    b = make_trainer('reactive', 4, R=R)
    (k, rot), pixel = best["bests_id"], best["bests_pixel"]
    label, _ = tr.get_label_value_scene("suction", 3, 0, 0, 0, depth, obj, None, "suction")
    assert label == 1
    loss_a = tr.backprop_scene(depth, "suction", best, label, obj)
    loss_b = b.train_batch_scene_class_pixels(depth, depth * obj[k], 1, [rot], [[pixel]], [label]).cpu().numpy()
    print("reactive suction: loss %.7f (backprop_scene), %.7f (train_batch_scene_class_pixels)" % (float(loss_a), float(loss_b[0])))
    assert loss_a.shape == () and float(loss_a) > 0
    assert_bit_identical(loss_a.reshape(1), loss_b)
