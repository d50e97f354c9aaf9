"""The normaliser of the Boltzmann policy per object in the scene frame on the MI355X (run with -m gpu): smg_scene_softmax_objects
and smg_scene_class_softmax_objects on an engine alone with seeded maps fed directly.  Unless a test says otherwise the rows
{count, vmax, lse, mean} are compared against tests/scene_softmax_ref.py's float64 restatement on smg_scene_maps'
(smg_scene_class_maps') own output: count exact, vmax bit-equal to smg_scene_argmax_objects' val, lse and mean within that module's
gate; the largest error / gate ratio is printed.  Outputs are prefilled, so an unwritten element shows.  The layout, masks and
distribution case are tests/test_gpu_scene_sample.py's, by import.  Then Trainer.scene_policy_stats, merge_policy_stats, with_stats
on the sampled forms and get_label_value_scene_soft against the maps they kept.  The cases' inputs are also run through the
restatement alone by tests/test_cpu_scene_softmax.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from map_harness import cached_engine, gpu, make_trainer, own_engine, stream  # noqa: F401

import scene_ref
import scene_softmax_ref as ref
import test_gpu_scene_class_objects as class_plane
import test_gpu_scene_objects as one_plane
import test_gpu_scene_sample as sample_side
from test_gpu_scene_sample import PICKS, S, SIDE, STRADDLE, masks_for, picks_affines, picks_q

pytestmark = pytest.mark.gpu

FILL = -5.0
BETA = 3.0
# 72 maps = three launches of 32 + 32 + 8 with the picks case's pattern: the carried state is merged twice
WIDE = dict(mask_a=[PICKS["mask_a"][m % 4] for m in range(72)], mask_b=[PICKS["mask_b"][m % 4] for m in range(72)],
            groups=[m % 4 for m in range(72)], n_groups=5)


def wide_affines():
    return one_plane.affines()[np.arange(72) % 16]


def wide_q(seed, later=0.0):
    """Seeded maps of the 72-map case; launch j (maps 32 j ..) lies j * `later` higher."""
    q = np.random.default_rng(seed).standard_normal((72, SIDE, SIDE)).astype(np.float32)
    q[32:64] += np.float32(later)
    q[64:] += np.float32(2 * later)
    return q


# name -> (maps of the call, its affines, selection, beta): the one-plane cases at hm = 240
CASES = {
    "picks": lambda: (picks_q(240), picks_affines(), PICKS, BETA),
    "three launches": lambda: (wide_q(11), wide_affines(), WIDE, BETA),
    "beta 0": lambda: (picks_q(12), picks_affines(), PICKS, 0.0),
    "beta 1e4": lambda: (picks_q(13), picks_affines(), PICKS, 1e4),
    "q + 1000": lambda: (picks_q(14) + np.float32(1000.0), picks_affines(), PICKS, BETA),
    "later launches 50 lower": lambda: (wide_q(15, -50.0), wide_affines(), WIDE, BETA),
    "later launches 1.0 higher": lambda: (wide_q(16, 1.0), wide_affines(), WIDE, BETA),
}
STEEP_OR_SHIFTED = ("beta 1e4", "q + 1000", "later launches 50 lower")
NONEMPTY, EMPTY = [0, 1, 3], [2, 4]


@pytest.fixture(scope="module")
def eng1(gpu):
    with own_engine(S, 1, 1) as eng:
        yield eng


@pytest.fixture(scope="module")
def eng3(gpu):
    with own_engine(S, 3, 1) as eng:
        yield eng


def softmax(eng, q, aff, hm, masks_dev, mask_a, mask_b, groups, n_groups, beta, cls=None):
    """One smg_scene_softmax_objects (cls None) or smg_scene_class_softmax_objects on rows prefilled with -5 -> float64 [n_groups, 4]."""
    rows = torch.full((n_groups, 4), FILL, dtype=torch.float64, device="cuda")
    tail = (masks_dev.data_ptr(), int(masks_dev.shape[0]), mask_a, mask_b, groups, n_groups, beta, rows.data_ptr(), stream())
    if cls is None:
        eng.scene_softmax_objects(q.data_ptr(), q[0].numel(), len(aff), aff, hm, *tail)
    else:
        eng.scene_class_softmax_objects(q.data_ptr(), len(aff), aff, hm, cls, *tail)
    return rows.cpu().numpy()


def check(eng, qh, aff, hm, masks, masks_dev, sel, beta, what, cls=None):
    """The call against the restatement on the engine's own maps and against the argmax call; returns (rows, maps, worst ratios)."""
    q = torch.from_numpy(qh).cuda()
    if cls is None:
        maps = one_plane.scene_maps(eng, q, aff, hm)
        best = one_plane.objects(eng, q, aff, hm, masks_dev, **sel)
    else:
        maps = class_plane.class_maps(eng, q, aff, hm, cls)
        best = class_plane.objects(eng, q, aff, hm, cls, masks_dev, **sel)
    rows = softmax(eng, q, aff, hm, masks_dev, beta=beta, cls=cls, **sel)
    assert not (rows == FILL).any(), what                                          # every element written
    worst = ref.assert_rows(rows, maps, masks, beta, what, **sel)
    vmax32 = rows[:, 1].astype(np.float32)
    assert np.array_equal(vmax32.astype(np.float64), rows[:, 1], equal_nan=True)    # vmax is a float32
    assert np.array_equal(vmax32.view(np.uint32), best[1].view(np.uint32)), what    # ... smg_scene_argmax_objects' val, bit for bit
    return rows, maps, worst


@pytest.mark.parametrize("hm", (240, 239))
def test_picks_against_the_restatement(eng1, hm):
    """The picks case at beta = 3: 40 maps in two launches, non-contiguous groups split by the launch boundary, a union, a group
    with no valid pixel, a single-pixel group and a group with no map.  hm = 239 (57 121 pixels, no multiple of 4) with the masks
    tensor one double off 16-byte alignment takes the guarded mask loads and a ragged last thread."""
    assert scene_ref.geometry(hm)[1:] == (S, SIDE)
    masks = masks_for(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    if hm == 239:
        buf = torch.zeros(masks.size + 1, dtype=torch.float64, device="cuda")
        off = buf[1:].view(5, hm, hm)
        off.copy_(masks_dev)
        masks_dev = off
        assert masks_dev.data_ptr() % 16 == 8 and hm * hm % 4 == 1
    rows, _, _ = check(eng1, picks_q(hm), picks_affines(), hm, masks, masks_dev, PICKS, BETA, "picks, hm %d" % hm)
    assert (rows[NONEMPTY, 0] > 0).all() and rows[3, 0] == 10                       # the single-pixel group: ten lone candidates
    for g in EMPTY:                                                                 # no valid pixel; no map
        assert rows[g, 0] == 0 and np.isneginf(rows[g, 1]) and np.isneginf(rows[g, 2]) and np.isnan(rows[g, 3])


@pytest.mark.parametrize("case", [c for c in CASES if c != "picks"])
def test_cases_against_the_restatement(eng1, case):
    """Three launches (the carry used twice); beta = 0 (lse = log count, the arithmetic mean); beta = 10^4 (nothing overflows, the
    mean is vmax); q + 1000 (a plain exp(beta v) would be inf); later launches 50 lower (their weight underflows, no NaN); later
    launches 1.0 higher (the carried state is rescaled)."""
    hm = 240
    qh, aff, sel, beta = CASES[case]()
    masks = masks_for(hm)
    rows, maps, _ = check(eng1, qh, aff, hm, masks, torch.from_numpy(masks).cuda(), sel, beta, case)
    assert np.isfinite(rows[NONEMPTY]).all()
    if case == "beta 0":
        for g in NONEMPTY:
            v = ref.candidates(maps, masks, sel["mask_a"], sel["mask_b"], sel["groups"], g).astype(np.float64)
            assert abs(rows[g, 2] - np.log(len(v))) <= ref.lse_gate(np.log(len(v)))
            assert abs(rows[g, 3] - v.mean()) <= ref.mean_gate(np.abs(v).max())
    if case == "beta 1e4":
        for g in NONEMPTY:
            assert abs(rows[g, 3] - rows[g, 1]) <= ref.mean_gate(abs(rows[g, 1])), g


def test_a_nan_in_one_map(eng1):
    """A NaN map element in ONE map of group 1: it is counted, vmax, lse and mean of its group are NaN, the others keep their rows
    bit for bit."""
    hm = 240
    aff = picks_affines()
    qh = picks_q(4)
    masks = masks_for(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    base = softmax(eng1, torch.from_numpy(qh).cuda(), aff, hm, masks_dev, beta=BETA, **PICKS)
    m = 4 * 2 + 1                                                                   # map 9: group 1, rotation 9
    qh[m, 1, 1] = np.nan
    rows, maps, _ = check(eng1, qh, aff, hm, masks, masks_dev, PICKS, BETA, "a NaN element")
    assert (np.isnan(maps[m]) & (masks[STRADDLE] != 0)).any()
    assert rows[1, 0] == base[1, 0] and np.isnan(rows[1, 1:]).all()
    others = [0, 2, 3, 4]
    assert np.array_equal(rows[others].view(np.uint64), base[others].view(np.uint64))


def test_class_form_against_the_class_maps(eng3):
    """smg_scene_class_softmax_objects for every cls against smg_scene_class_maps' own plane, 40 maps in two launches; group 1 is
    the whole image (both terms -1)."""
    hm = 240
    aff = picks_affines()
    qh = picks_q(6, planes=3)
    masks = masks_for(hm)
    masks_dev = torch.from_numpy(masks).cuda()
    sel = dict(PICKS, mask_a=[-1 if m % 4 == 1 else a for m, a in enumerate(PICKS["mask_a"])])
    assert sel["mask_a"][1] == sel["mask_b"][1] == -1
    for cls in (0, 1, 2):
        rows, _, _ = check(eng3, qh, aff, hm, masks, masks_dev, sel, BETA, "class form, cls %d" % cls, cls=cls)
        assert (rows[NONEMPTY, 0] > 0).all() and (rows[EMPTY, 0] == 0).all()
        assert (rows[NONEMPTY, 1] <= 1.0).all() and (rows[NONEMPTY, 3] > 0.0).all()


def test_identical_calls_are_bit_identical(eng1, eng3):
    hm = 240
    masks_dev = torch.from_numpy(masks_for(hm)).cuda()
    q = torch.from_numpy(wide_q(3, 1.0)).cuda()
    a = softmax(eng1, q, wide_affines(), hm, masks_dev, beta=BETA, **WIDE)
    b = softmax(eng1, q, wide_affines(), hm, masks_dev, beta=BETA, **WIDE)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    q3 = torch.from_numpy(picks_q(7, planes=3)).cuda()
    a = softmax(eng3, q3, picks_affines(), hm, masks_dev, beta=BETA, cls=1, **PICKS)
    b = softmax(eng3, q3, picks_affines(), hm, masks_dev, beta=BETA, cls=1, **PICKS)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_refusals(eng1, eng3):
    """-22, a message that starts with the function's name and names the cause, nothing launched: the rows keep their fill.  Every
    refusal of the argmax_objects entry points, then a beta that is negative, NaN or infinite and a misaligned stats_out_dev."""
    import smg_hip
    L = smg_hip.lib()
    hm = 240
    big = 37283                                            # 37 283 x 240^2 > 2^31 - 1
    aff = np.tile(scene_ref.theta(1, 16), (big, 1))
    shifted = aff[:16].copy()
    shifted[7, 5] = 0.25
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))         # noqa: E731
    ints = lambda v: (C.c_int * big)(*([v] * big))                 # noqa: E731
    zero, minus = ints(0), ints(-1)
    q = torch.zeros((16, 3, SIDE, SIDE), device="cuda")
    masks = torch.ones((2, hm, hm), dtype=torch.float64, device="cuda")
    rows = torch.full((3, 4), FILL, dtype=torch.float64, device="cuda")
    ok = dict(e=eng1.h, q=q.data_ptr(), stride=SIDE * SIDE, n_maps=16, aff=ptr(aff), hm=hm, cls=0, masks=masks.data_ptr(), n_masks=2, a=zero, b=minus,
              g=zero, n_groups=3, beta=BETA, rows=rows.data_ptr())

    def call(name, a):
        tail = (a["masks"], a["n_masks"], a["a"], a["b"], a["g"], a["n_groups"], a["beta"], a["rows"], None)
        if name == b"smg_scene_softmax_objects":
            return L.smg_scene_softmax_objects(a["e"], a["q"], a["stride"], a["n_maps"], a["aff"], a["hm"], *tail)
        return L.smg_scene_class_softmax_objects(a["e"], a["q"], a["n_maps"], a["aff"], a["hm"], a["cls"], *tail)
    one_bad = lambda v: (C.c_int * 16)(*([0] * 15 + [v]))          # noqa: E731
    for name, e_ok, e_640 in ((b"smg_scene_softmax_objects", eng1.h, cached_engine(640, 1).h), (b"smg_scene_class_softmax_objects", eng3.h, cached_engine(640, 3).h)):
        def refused(word, **change):
            rc = call(name, dict(dict(ok, e=e_ok), **change))
            msg = L.smg_last_error()
            assert rc == -22 and msg.startswith(name + b":") and word in msg, (name, change.keys(), rc, msg)
        for key in ("q", "aff", "masks", "a", "b", "g", "rows"):
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
        for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
            refused(b"beta", beta=bad)
        refused(b"8-byte aligned", rows=rows.data_ptr() + 4)
        if name == b"smg_scene_softmax_objects":
            refused(b"negative map_stride", stride=-1)
        else:
            refused(b"head_out", e=eng1.h)
            refused(b"cls must be", cls=3)
            refused(b"cls must be", cls=-1)
    with pytest.raises(smg_hip.SmgError):
        eng1.scene_softmax_objects(q.data_ptr(), SIDE * SIDE, 16, shifted, hm, masks.data_ptr(), 2, [0] * 16, [-1] * 16, [0] * 16, 3, BETA, rows.data_ptr(), stream())
    with pytest.raises(smg_hip.SmgError):
        eng3.scene_class_softmax_objects(q.data_ptr(), 16, aff[:16], hm, 0, masks.data_ptr(), 2, [0] * 16, [-1] * 16, [0] * 16, 3, -1.0, rows.data_ptr(), stream())
    torch.cuda.synchronize()
    assert bool((rows == FILL).all())
    # and the accepted calls write every element: group 0 the constant map (lse = beta v + log count, mean = v), groups 1 and 2 no map
    for name, e_ok, value in ((b"smg_scene_softmax_objects", eng1.h, np.float32(0.0)), (b"smg_scene_class_softmax_objects", eng3.h, class_plane.THIRD)):
        rows.fill_(FILL)
        assert call(name, dict(ok, e=e_ok)) == 0
        r = rows.cpu().numpy()
        want = BETA * float(value) + np.log(r[0, 0])
        assert r[0, 0] > 0 and r[0, 1] == float(value) and abs(r[0, 2] - want) <= ref.lse_gate(want) and abs(r[0, 3] - float(value)) <= ref.mean_gate(1.0)
        assert (r[1:, 0] == 0).all() and np.isneginf(r[1:, 1:3]).all() and np.isnan(r[1:, 3]).all()


def test_the_draws_follow_the_device_normaliser(eng1):
    """The sample tests' distribution case: 4096 draws of smg_scene_sample_objects on the 10 x 10 box against the probabilities
    exp(beta v - lse) formed with the DEVICE's lse - Pearson's chi^2 under that file's own bound and controls."""
    hm = sample_side.DIST_HM
    aff = np.tile(scene_ref.theta(0, 16), (32, 1))
    q = torch.from_numpy(np.tile(sample_side.dist_q(), (32, 1, 1))).cuda()
    maps = one_plane.scene_maps(eng1, q, aff, hm)
    lo, hi = sample_side.DIST_BOX
    box = maps[0, lo:hi, lo:hi].astype(np.float64).ravel()
    assert np.isfinite(box).all()
    masks_dev = torch.from_numpy(sample_side.dist_mask()).cuda()
    for beta in sample_side.DIST_BETAS:
        rows = softmax(eng1, q, aff, hm, masks_dev, beta=beta, **sample_side.DIST)
        assert (rows[:, 0] == 100).all() and np.array_equal(rows.view(np.uint64), np.tile(rows[:1], (32, 1)).view(np.uint64))
        p = np.exp(beta * box - rows[0, 2])
        assert abs(p.sum() - 1.0) <= 100 * ref.GATE                                 # the device's lse normalises the policy
        picks = [sample_side.sample(eng1, q, aff, hm, masks_dev, n_draws=32, beta=beta, seed=seed, **sample_side.DIST)[0] for seed in sample_side.DIST_SEEDS]
        counts = sample_side.dist_counts(picks)
        chi, df = sample_side.scene_sample_ref.chi_square(counts, p / p.sum())
        bound = sample_side.scene_sample_ref.chi_square_bound(df)
        print("beta %g: chi^2 %.1f of 4096 draws against exp(beta v - lse_device) at df %d (bound %.1f)" % (beta, chi, df, bound))
        assert counts.sum() == 4096 and df >= 50 and chi < bound
        sample_side.assert_distribution(counts, box, beta, "device draws")          # that file's bound and its controls


# ---- the Trainer's methods ---------------------------------------------------------------------------------------------------------
HM, R = sample_side.HM, sample_side.R
TEMPERATURE = sample_side.TEMPERATURE_TR
scene, kept_maps = sample_side.scene, sample_side.kept_maps
FIELDS = ("count", "vmax", "lse", "mean")


def object_sel(n_maps, name, joint):
    if name == "pairs":
        return dict(mask_a=[0], mask_b=[1], groups=[0], n_groups=1)
    groups = [0] * n_maps if joint else [k for k in range(2) for _ in range(R)]
    return dict(mask_a=[k for k in range(2) for _ in range(R)], mask_b=[-1] * n_maps, groups=groups, n_groups=1 if joint else 2)


def assert_stats(stats, kept, obj, temperature, joint, planes=1, cls=0, names=("grasp", "suction", "pairs")):
    """One temperature of scene_policy_stats' dict against the restatement on the kept maps, the derived fields as defined."""
    beta = 1.0 / temperature
    for name in names:
        d = stats[name]
        maps = kept_maps(kept, name, planes, cls, 1 if name == "pairs" else R)
        sel = object_sel(maps.shape[0], name, joint)
        rows = np.stack([d[f] for f in FIELDS], axis=-1)
        ref.assert_rows(rows, maps, obj, beta, "%s%s at T %g" % (name, " joint" if joint else "", temperature), **sel)
        assert np.array_equal(d["entropy"], d["lse"] - beta * d["mean"]) and np.allclose(d["mellowmax"], temperature * (d["lse"] - np.log(d["count"])), rtol=2.0 ** -48, atol=0)
        assert (d["mellowmax"] <= d["mean"]).all() and (d["mean"] <= d["vmax"]).all() and (d["entropy"] <= np.log(d["count"])).all()


def test_scene_policy_stats(gpu):
    tr = make_trainer('reinforcement', 4, R=R)
    depth, obj = scene()
    one = tr.scene_policy_stats(depth, obj, TEMPERATURE)
    assert set(one) == {"grasp", "suction", "pairs"} and one["grasp"]["lse"].shape == (2,) and one["pairs"]["lse"].shape == (1,)
    assert_stats(one, tr._last_object_q, obj, TEMPERATURE, False)
    assert tr.scene_policy_stats(depth, obj, TEMPERATURE, is_ets=False)["pairs"]["count"].shape == (0,)
    temps = (TEMPERATURE, 1.0, 0.05)
    many = tr.scene_policy_stats(depth, obj, temps, is_target=True)
    kept = tr._last_object_q
    assert many["suction"]["mean"].shape == (3, 2) and many["pairs"]["mean"].shape == (3, 1)
    for j, t in enumerate(temps):
        assert_stats({name: {k: v[j] for k, v in many[name].items() if k != "beta"} for name in many}, kept, obj, t, False)
    for f in FIELDS:                                        # (the target net is in sync with the online one here)
        assert np.array_equal(many["grasp"][f][0], one["grasp"][f])
    uniform = tr.scene_policy_stats(depth, obj, float("inf"))
    assert np.array_equal(uniform["grasp"]["mellowmax"], uniform["grasp"]["mean"])
    assert (np.abs(uniform["grasp"]["lse"] - np.log(uniform["grasp"]["count"])) <= ref.GATE * np.log(uniform["grasp"]["count"])).all()
    # merging the per-object rows gives the joint row
    joint = tr.scene_policy_stats(depth, obj, TEMPERATURE, joint=True)
    assert_stats(joint, tr._last_object_q, obj, TEMPERATURE, True)
    for name in ("grasp", "suction"):
        merged, j = tr.merge_policy_stats(one[name]), joint[name]
        assert merged["count"].shape == (1,) and merged["count"][0] == j["count"][0] and merged["vmax"][0] == j["vmax"][0]
        assert abs(merged["lse"][0] - j["lse"][0]) <= ref.lse_gate(j["lse"][0])
        assert abs(merged["mean"][0] - j["mean"][0]) <= ref.mean_gate(max(abs(j["vmax"][0]), abs(j["mean"][0])))
    with pytest.raises(ValueError):
        tr.scene_class_policy_stats(depth, obj, 1.0)
    for bad in (0.0, -1.0, float("nan"), (1.0, 0.0), ()):
        with pytest.raises(ValueError):
            tr.scene_policy_stats(depth, obj, bad)


def test_scene_class_policy_stats(gpu):
    tr = make_trainer('reactive', 4, R=R)
    depth, obj = scene()
    for cls in (0, 2):
        stats = tr.scene_class_policy_stats(depth, obj, TEMPERATURE, cls=cls)
        assert_stats(stats, tr._last_object_q, obj, TEMPERATURE, False, planes=3, cls=cls)
    res = tr.sampled_scene_class_actions(depth, obj, 3, TEMPERATURE, 9, with_stats=True)
    plain = tr.sampled_scene_class_actions(depth, obj, 3, TEMPERATURE, 9)
    assert {k: res[k] for k in plain} == plain and set(res) == set(plain) | {"stats", "logp"}
    assert_stats(res["stats"], tr._last_object_q, obj, TEMPERATURE, False, planes=3)
    with pytest.raises(ValueError):
        tr.scene_policy_stats(depth, obj, 1.0)
    with pytest.raises(ValueError):
        tr.get_label_value_scene_soft('grasp', 2, 0, 1, 0, depth, obj, 1.0, "expected")
    with pytest.raises(ValueError):
        tr.scene_class_policy_stats(depth, obj, 1.0, cls=3)


@pytest.mark.parametrize("joint", (False, True))
def test_with_stats_keeps_the_picks_and_adds_logp(gpu, joint):
    tr = make_trainer('reinforcement', 4, R=R)
    depth, obj = scene()
    args = (depth, obj, sample_side.DRAWS_TR, TEMPERATURE, sample_side.SEED_TR)
    plain = tr.sampled_scene_actions(*args, joint=joint)
    res = tr.sampled_scene_actions(*args, joint=joint, with_stats=True)
    assert set(res) == set(plain) | {"stats", "logp"} and {k: res[k] for k in plain} == plain
    assert_stats(res["stats"], tr._last_object_q, obj, TEMPERATURE, joint)
    beta = 1.0 / TEMPERATURE
    for name in ("grasp", "suction", "pairs"):
        lse = res["stats"][name]["lse"]
        if joint:
            want = [beta * e[-1] - lse[0] for e in res["joint"][name]]
        else:
            lists = res["per_pair"] if name == "pairs" else res["per_object"][name]
            want = [[beta * e[-1] - lse[g] for e in entries] for g, entries in enumerate(lists)]
            assert [len(x) for x in want] == [sample_side.DRAWS_TR] * len(lists)
        assert res["logp"][name] == want and np.asarray(want).dtype == np.float64
        assert (np.asarray(want) < 0).all()                 # every group has more than one candidate


@pytest.mark.parametrize("kind", ("expected", "mellowmax"))
def test_get_label_value_scene_soft(gpu, kind, capsys):
    """A target net that differs from the online one: the label is reward + gamma * (the value recomputed from the TARGET's kept
    maps, all primitives merged), and mellowmax lies between the arithmetic mean of the target's candidates and their Boltzmann
    mean, which lies below the target's best confidence (H <= log count puts mellowmax below the Boltzmann mean, never above)."""
    import synthetic
    from oracle import affordance as orc
    tr = make_trainer('reinforcement', 4, R=R)
    sd = synthetic.make_state_dict(orc.state_layout(1), 5)
    tr.model_target.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    depth, obj = scene()
    online = tr.scene_policy_stats(depth, obj, TEMPERATURE, joint=True)
    expected, reward = tr.get_label_value_scene_soft('grasp', 2, 0, 1, 0, depth, obj, TEMPERATURE, kind)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    kept = tr._last_object_q                                # the target's maps
    vals = []
    for name in ("grasp", "suction", "pairs"):
        maps = kept_maps(kept, name, 1, 0, 1 if name == "pairs" else R)
        sel = object_sel(maps.shape[0], name, True)
        vals.append(ref.candidates(maps, obj, sel["mask_a"], sel["mask_b"], sel["groups"], 0))
    v = np.concatenate(vals)
    count, vmax, lse, mean = ref.stats_of(v, 1.0 / TEMPERATURE)
    want = mean if kind == "expected" else TEMPERATURE * (lse - np.log(count))
    gate = ref.mean_gate(float(np.abs(v).max())) if kind == "expected" else TEMPERATURE * (ref.lse_gate(lse) + 2.0 ** -50)
    print("%s: label %.12f, reward %g + 0.5 x %.12f recomputed from %d target candidates; %s" % (kind, expected, reward, want, count, line))
    assert reward == 1 and abs(expected - (1 + 0.5 * want)) <= 0.5 * gate + 2.0 ** -50
    assert line.startswith('Expected reward: %f + %f x ' % (1, 0.5)) and line.endswith(' = %f' % expected)
    assert abs(ref.stats_of(vals[0], 1.0 / TEMPERATURE)[3] - online["grasp"]["mean"][0]) > 1e-6      # the target differs from the online net
    if kind == "mellowmax":
        best = tr.best_scene_actions(depth, obj, is_target=True)
        top = max(best["bestg_conf"], best["bests_conf"], best["bestgs_conf"])
        assert top == vmax and float(v.astype(np.float64).mean()) <= (expected - 1) / 0.5 <= mean <= top
    # the zero-future cases need no forward
    assert tr.get_label_value_scene_soft('grasp', 2, 0, 0, 0, depth, obj, TEMPERATURE, kind) == (0, 0)
    assert tr.get_label_value_scene_soft('grasp', 1, 0, 1, 0, depth, obj, TEMPERATURE, kind) == (1, 1)
    with pytest.raises(ValueError):
        tr.get_label_value_scene_soft('grasp', 2, 0, 1, 0, depth, obj, TEMPERATURE, "max")
