"""Training the Boltzmann policy per object in the scene frame on the MI355X (run with -m gpu): smg_loss_scene_policy on an engine
alone with seeded maps fed directly.  The reference is tests/scene_policy_ref.py's float64 restatement evaluated on the float32
values smg_scene_maps itself returns for the same q, unselected pixels dropped on the host - the v_i are bit-equal by construction.
Gates (no case is left out of any comparison):
    dq per pair     |device - reference| <= 2^-23 max|reference dq of that pair|      (smg_loss_scene_map's gate: everything before
                    the one float32 store is double and that store is 2^-24 of the element); a pair whose reference dq is all zero
                    must come out exactly zero
    loss per group  |device - reference| <= 2^-23 (|w_nll| (|lse| + beta |v_act|) + |w_ent| (|lse| + beta |mean|))
    stats           bit-equal to a smg_scene_softmax_objects call on the same arguments
The largest error / gate ratios are printed.  Outputs are prefilled, so an unwritten element shows.  Then the Trainer's
train_batch_scene_policy against the fp64 PyTorch-CPU oracle and backprop_scene_policy on a dict of best_scene_actions.  The
cases' inputs are also run through the restatement alone by tests/test_cpu_scene_policy.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import orc
from map_harness import (assert_bit_identical, assert_train_batch_runs, bits, border_pixels, cached_engine, filled, gpu, HEAD,  # noqa: F401
                         make_trainer, s704_scene, stream)

import scene_policy_ref as ref
import scene_ref
import test_gpu_scene_objects as one_plane
import test_gpu_scene_sample as sample_side
import test_gpu_scene_softmax as softmax_side

pytestmark = pytest.mark.gpu

FILL = -7.0
BETA = 3.0
ROTS = (0, 3, 8, 13)
CENTRE, STRADDLE, OUTSIDE, ONE, WHOLE = range(5)
NAN = float("nan")


def flat(hm, pair, iy, ix):
    return (pair * hm + iy) * hm + ix


# The main layout: 8 pairs, rotations 0, 3, 8, 13 of 16 twice.  Group 0 = pairs 0, 2 (pair 0 selects by the UNION of two masks), its
# action in pair 2; group 1 = pairs 1, 3, no action, its w_nll a NaN that must be ignored; group 2 = pair 4, the single-pixel mask
# and no action: one candidate, pi = 1, v = mean, dq exactly 0; group 3 = pair 5 under a mask without a valid pixel: empty; group 4
# = pairs 6, 7 on every pixel with a NEGATIVE w_nll, its action in pair 7; group 5 has no pair.  Groups 0 and 1 are not contiguous.
MAIN = dict(mask_a=[CENTRE, STRADDLE, CENTRE, STRADDLE, -1, OUTSIDE, -1, -1], mask_b=[STRADDLE, -1, -1, -1, ONE, -1, -1, -1],
            groups=[0, 1, 0, 1, 2, 3, 4, 4], n_groups=6)
MAIN_WEIGHTS = [[1.0, 0.1], [NAN, -0.3], [2.0, 0.5], [1.0, 1.0], [-0.7, 0.2], [0.3, 0.3]]
MAIN_PIXEL = {240: (118, 117), 239: (118, 117), 320: (150, 160)}        # inside the centre rectangle, valid in every rotation
ACTING, EMPTY = [0, 4], [3, 5]


def main_case(hm, seed, beta=BETA, shift=0.0):
    side = scene_ref.geometry(hm)[2]
    q = (np.random.default_rng(seed).standard_normal((8, 1, side, side)) + shift).astype(np.float32)
    aff = np.stack([scene_ref.theta(ROTS[m % 4], 16) for m in range(8)])
    masks = sample_side.masks_for(hm) if hm == 239 else one_plane.rect_masks(hm)
    iy, ix = MAIN_PIXEL[hm]
    actions = [flat(hm, 2, iy, ix), -1, -1, -1, flat(hm, 7, iy + 3, ix - 5), -1]
    return dict(hm=hm, q=q, aff=aff, masks=masks, sel=MAIN, beta=beta, actions=actions, weights=MAIN_WEIGHTS, acting=ACTING, empty=EMPTY)


def border_case():
    """hm = 448 (S = 1280, 21 x 21 maps): in rotation 2 of 16 valid pixels lie on the image border, so element boxes are clipped by
    the heightmap edge.  Pair 0 (rotation 2, every pixel) and pair 1 (rotation 5, the band of the first 40 rows) are group 0 with
    the action at the centre of pair 0; pair 2 (rotation 2, the band) is group 1, its action the band's first candidate."""
    hm = 448
    q = np.random.default_rng(448).standard_normal((3, 1, 21, 21)).astype(np.float32)
    aff = np.stack([scene_ref.theta(r, 16) for r in (2, 5, 2)])
    masks = np.zeros((1, hm, hm))
    masks[0, :40] = 1.0
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    first = int(np.flatnonzero((scene_ref.map_coords(hm, aff[2], iy, ix)[2] & (masks[0] != 0)).ravel())[0])
    return dict(hm=hm, q=q, aff=aff, masks=masks, sel=dict(mask_a=[-1, 0, 0], mask_b=[-1, -1, -1], groups=[0, 0, 1], n_groups=2), beta=BETA,
                actions=[flat(hm, 0, 224, 220), 2 * hm * hm + first], weights=[[1.0, 0.05], [-0.4, 0.3]], acting=[0, 1], empty=[])


def boundary_case():
    """40 pairs at hm = 240 = launches of 32 + 8, pair m in rotation m % 16.  Group 0 = every pair but 1 and 33, split by the
    boundary, its action in pair 35; pair 1 is group 1 and pair 33, which carries pair 1's inputs, group 2, with the same action
    pixel and weights."""
    hm = 240
    q = np.random.default_rng(40).standard_normal((40, 1, 3, 3)).astype(np.float32)
    q[33] = q[1]
    aff = one_plane.affines()[np.arange(40) % 16]
    iy, ix = MAIN_PIXEL[hm]
    sel = dict(mask_a=[CENTRE if m % 2 else STRADDLE for m in range(40)], mask_b=[-1] * 40,
               groups=[1 if m == 1 else 2 if m == 33 else 0 for m in range(40)], n_groups=3)
    return dict(hm=hm, q=q, aff=aff, masks=one_plane.rect_masks(hm), sel=sel, beta=BETA,
                actions=[flat(hm, 35, iy, ix), flat(hm, 1, iy + 1, ix), flat(hm, 33, iy + 1, ix)],
                weights=[[1.0, 0.1], [0.8, -0.2], [0.8, -0.2]], acting=[0, 1, 2], empty=[])


# name -> the case: what tests/test_cpu_scene_policy.py runs through the restatement alone
CASES = {
    "hm 240": lambda: main_case(240, 1),
    "hm 320": lambda: main_case(320, 2),
    "hm 239": lambda: main_case(239, 3),
    "hm 448, clipped boxes": border_case,
    "40 pairs": boundary_case,
    "beta 0": lambda: main_case(240, 4, beta=0.0),
    "beta 1e4": lambda: main_case(240, 5, beta=1e4),
    "q + 1000": lambda: main_case(240, 6, shift=1000.0),
}


def run(eng, c, masks_dev=None, q=None, actions=None):
    """One smg_loss_scene_policy on prefilled outputs -> (loss [n_groups], dq [n, side, side], stats float64 [n_groups, 4]), host."""
    sel, n = c["sel"], len(c["aff"])
    q = torch.from_numpy(c["q"] if q is None else q).cuda()
    masks_dev = torch.from_numpy(c["masks"]).cuda() if masks_dev is None else masks_dev
    act = torch.tensor(c["actions"] if actions is None else actions, dtype=torch.int32, device="cuda")
    wgt = torch.tensor(c["weights"], dtype=torch.float64, device="cuda")
    loss, dq = filled((sel["n_groups"],), FILL), filled(q.shape, FILL)
    stats = torch.full((sel["n_groups"], 4), FILL, dtype=torch.float64, device="cuda")
    eng.loss_scene_policy(q.data_ptr(), c["aff"], c["hm"], n, masks_dev.data_ptr(), int(masks_dev.shape[0]), sel["mask_a"], sel["mask_b"],
                          sel["groups"], sel["n_groups"], c["beta"], act.data_ptr(), wgt.data_ptr(), stats.data_ptr(), loss.data_ptr(),
                          dq.data_ptr(), stream())
    return loss.cpu().numpy(), dq.cpu().numpy()[:, 0], stats.cpu().numpy()


def check(eng, c, what, masks_dev=None, q=None, actions=None):
    """The call against the restatement on the engine's own scene maps and against the softmax call; a second call bit-identical.
    Returns (loss, dq, stats, the restatement's dict)."""
    qh = c["q"] if q is None else q
    q_dev = torch.from_numpy(qh).cuda()
    masks_dev = torch.from_numpy(c["masks"]).cuda() if masks_dev is None else masks_dev
    loss, dq, stats = run(eng, c, masks_dev, q, actions)
    assert not (dq == FILL).any() and not (loss == FILL).any() and not (stats == FILL).any(), what      # every element written
    maps = one_plane.scene_maps(eng, q_dev, c["aff"], c["hm"])
    want = ref.policy(maps, c["aff"], c["hm"], c["masks"], beta=c["beta"], actions=c["actions"] if actions is None else actions,
                      weights=c["weights"], **c["sel"])
    worst = ref.gate_ratios(loss, dq, want)
    print("%s: beta %g, counts %s; largest error / gate: loss %.3g, dq %.3g" % (what, c["beta"], want["stats"][:, 0].astype(np.int64).tolist(), *worst))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (what, worst)
    rows = softmax_side.softmax(eng, q_dev, c["aff"], c["hm"], masks_dev, beta=c["beta"], **c["sel"])
    assert np.array_equal(stats.view(np.uint64), rows.view(np.uint64)), what          # smg_scene_softmax_objects' rows, bit for bit
    again = run(eng, c, masks_dev, q, actions)
    assert_bit_identical(loss, again[0])
    assert_bit_identical(dq, again[1])
    assert np.array_equal(stats.view(np.uint64), again[2].view(np.uint64))
    return loss, dq, stats, want


def assert_main_shape(c, loss, dq, stats, want):
    """What the main layout promises beyond the gates."""
    assert np.isfinite(loss).all() and np.isfinite(dq).all()
    assert (stats[c["acting"], 0] > 1).all() and stats[2, 0] == 1
    for g in c["empty"]:
        assert loss[g] == 0 and stats[g, 0] == 0 and np.isneginf(stats[g, 1:3]).all() and np.isnan(stats[g, 3])
    assert (dq[4] == 0).all() and (dq[5] == 0).all()            # one candidate without an action; no candidate
    assert not np.isnan(want["vact"][c["acting"]]).any()


@pytest.mark.parametrize("hm,S,side", ((240, 704, 3), (320, 928, 10)))
def test_policy_loss_against_the_restatement(gpu, hm, S, side):
    """The main layout: a union, two groups that are not contiguous, a group without an action whose w_nll is a NaN, a one-candidate
    group, an empty group, a group without a pair, a negative w_nll."""
    assert scene_ref.geometry(hm)[1:] == (S, side)
    c = CASES["hm %d" % hm]()
    out = check(cached_engine(S, 1), c, "hm %d" % hm)
    assert_main_shape(c, *out)
    if c["beta"] > 0:
        assert (np.abs(out[1][[0, 2, 6, 7]]).reshape(4, -1).max(1) > 0).all()


def test_policy_loss_with_masks_off_16_byte_alignment(gpu):
    """hm = 239 (57 121 pixels, no multiple of 4) with the masks tensor one double off 16-byte alignment."""
    c = CASES["hm 239"]()
    hm = c["hm"]
    buf = torch.zeros(c["masks"].size + 1, dtype=torch.float64, device="cuda")
    off = buf[1:].view(5, hm, hm)
    off.copy_(torch.from_numpy(c["masks"]))
    assert off.data_ptr() % 16 == 8 and hm * hm % 4 == 1
    assert_main_shape(c, *check(cached_engine(704, 1), c, "hm 239, masks 8 bytes off", masks_dev=off))


def test_policy_loss_where_the_heightmap_border_clips_the_boxes(gpu):
    c = CASES["hm 448, clipped boxes"]()
    maps_valid = scene_ref.map_coords(c["hm"], c["aff"][0], *np.meshgrid(np.arange(448), np.arange(448), indexing="ij"))[2]
    assert border_pixels(maps_valid) > 0
    loss, dq, stats, want = check(cached_engine(1280, 1), c, "hm 448")
    assert np.isfinite(loss).all() and np.isfinite(dq).all() and (stats[:, 0] > 0).all()
    assert (c["actions"][1] % (448 * 448)) // 448 == 0          # the second group's action lies on the image border


def test_policy_loss_across_the_launch_boundary(gpu):
    """40 pairs: group 0 split by the 32-pair boundary with its action in pair 35; pair 33 with pair 1's inputs in a group of its
    own gives pair 1's results bit for bit (the flattened action index differs, the pixel is the same)."""
    c = CASES["40 pairs"]()
    loss, dq, stats, want = check(cached_engine(704, 1, pairs=40), c, "40 pairs")
    assert np.isfinite(loss).all() and np.isfinite(dq).all()
    assert_bit_identical(loss[1:2], loss[2:3])
    assert_bit_identical(dq[1], dq[33])
    assert np.array_equal(stats[1].view(np.uint64), stats[2].view(np.uint64))
    assert (np.abs(dq[32:]).reshape(8, -1).max(1) > 0).all() and not np.array_equal(dq[1], dq[17])


@pytest.mark.parametrize("case", ("beta 0", "beta 1e4", "q + 1000"))
def test_policy_loss_limits(gpu, case):
    """beta = 0: dq exactly 0 and loss (w_nll - w_ent) log count; beta = 10^4 and q + 1000: nothing overflows, dq finite."""
    c = CASES[case]()
    loss, dq, stats, want = check(cached_engine(704, 1), c, case)
    assert_main_shape(c, loss, dq, stats, want)
    if case == "beta 0":
        assert (dq == 0).all()
        for g in c["acting"]:
            w = c["weights"][g]
            assert abs(loss[g] - (w[0] - w[1]) * np.log(stats[g, 0])) <= ref.GATE * (abs(w[0]) + abs(w[1])) * np.log(stats[g, 0])
    else:
        assert (np.abs(dq[[0, 2, 6, 7]]).reshape(4, -1).max(1) > 0).any()


def test_a_nan_in_one_pair(gpu):
    """A NaN map element in pair 0 (group 0): the loss of group 0 and every element of dq of pairs 0 and 2 are NaN; the other
    groups' losses, rows and dq keep their bits."""
    c = CASES["hm 240"]()
    eng = cached_engine(704, 1)
    base = run(eng, c)
    q = c["q"].copy()
    q[0, 0, 1, 1] = np.nan
    loss, dq, stats, want = check(eng, c, "a NaN element", q=q)
    assert np.isnan(loss[0]) and np.isnan(dq[[0, 2]]).all() and np.isnan(stats[0, 1:]).all()
    others = [1, 2, 3, 4, 5]
    assert_bit_identical(loss[others], base[0][others])
    assert_bit_identical(dq[[1, 3, 4, 5, 6, 7]], base[1][[1, 3, 4, 5, 6, 7]])
    assert np.array_equal(stats[others].view(np.uint64), base[2][others].view(np.uint64))


def test_an_action_that_is_no_candidate(gpu):
    """Group 0's action on a pixel its masks do not select (then: in a pair of another group, out of range): the loss of group 0 is
    NaN, the pi and entropy parts of its dq are written (the restatement's, at the gate), the other groups and all stats unchanged."""
    c = CASES["hm 240"]()
    eng = cached_engine(704, 1)
    base = run(eng, c)
    hm = c["hm"]
    assert c["masks"][CENTRE, 5, 5] == 0 and c["sel"]["groups"][7] != 0
    for what, bad in (("unselected", flat(hm, 2, 5, 5)), ("another group's pair", flat(hm, 7, *MAIN_PIXEL[hm])), ("out of range", 8 * hm * hm + 3),
                      ("below -1", -2)):
        actions = [bad] + c["actions"][1:]
        loss, dq, stats, want = check(eng, c, "action " + what, actions=actions)
        assert np.isfinite(dq).all() and (np.isnan(loss[0]) if bad >= 0 else np.isfinite(loss[0]))
        assert_bit_identical(loss[1:], base[0][1:])
        assert_bit_identical(dq[[1, 3, 4, 5, 6, 7]], base[1][[1, 3, 4, 5, 6, 7]])
        assert np.array_equal(stats.view(np.uint64), base[2].view(np.uint64))


def test_refusals(gpu):
    """-22, a message that starts with the function's name and names the cause, nothing launched: the outputs keep their fill.
    Every refusal of smg_scene_argmax_objects, head_out != 1, a NULL pointer, beta, the alignment of stats_out_dev and weight_dev."""
    import smg_hip
    L = smg_hip.lib()
    name = b"smg_loss_scene_policy"
    hm, side = 240, 3
    big = 37283                                            # 37 283 x 240^2 > 2^31 - 1
    aff = np.tile(scene_ref.theta(1, 16), (big, 1))
    shifted = aff[:16].copy()
    shifted[7, 5] = 0.25
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))         # noqa: E731
    ints = lambda v: (C.c_int * big)(*([v] * big))                 # noqa: E731
    zero, minus = ints(0), ints(-1)
    q = torch.zeros((16, 1, side, side), device="cuda")
    masks = torch.ones((2, hm, hm), dtype=torch.float64, device="cuda")
    rows = torch.full((3, 4), FILL, dtype=torch.float64, device="cuda")
    loss, dq = filled((3,), FILL), filled(q.shape, FILL)
    act = torch.tensor([flat(hm, 0, 120, 120), -1, -1], dtype=torch.int32, device="cuda")
    wgt = torch.ones((3, 2), dtype=torch.float64, device="cuda")
    eng, eng3, eng640 = cached_engine(704, 1), cached_engine(704, 3), cached_engine(640, 1)
    ok = dict(e=eng.h, q=q.data_ptr(), aff=ptr(aff), hm=hm, n=16, masks=masks.data_ptr(), n_masks=2, a=zero, b=minus, g=zero, n_groups=3, beta=BETA,
              act=act.data_ptr(), wgt=wgt.data_ptr(), rows=rows.data_ptr(), loss=loss.data_ptr(), dq=dq.data_ptr())

    def call(a):
        return L.smg_loss_scene_policy(a["e"], a["q"], a["aff"], a["hm"], a["n"], a["masks"], a["n_masks"], a["a"], a["b"], a["g"], a["n_groups"],
                                       a["beta"], a["act"], a["wgt"], a["rows"], a["loss"], a["dq"], None)

    def refused(word, **change):
        rc = call(dict(ok, **change))
        msg = L.smg_last_error()
        assert rc == -22 and msg.startswith(name + b":") and word in msg, (change.keys(), rc, msg)
    one_bad = lambda v: (C.c_int * 16)(*([0] * 15 + [v]))          # noqa: E731
    for key in ("q", "aff", "masks", "a", "b", "g", "act", "wgt", "rows", "loss", "dq"):
        refused(b"NULL", **{key: None})
    refused(b"head_out", e=eng3.h)
    refused(b"n_pairs < 1", n=0)
    refused(b"n_masks < 1", n_masks=0)
    refused(b"n_groups < 1", n_groups=0)
    for bad in (2, -2):
        refused(b"mask index", a=one_bad(bad))
        refused(b"mask index", b=one_bad(bad))
    for bad in (3, -1):
        refused(b"group outside", g=one_bad(bad))
    refused(b"int32", n=big)
    refused(b"does not pad", hm=320)
    refused(b"does not pad", hm=224)
    refused(b"1 x 1", e=eng640.h, hm=224)
    refused(b"translation", aff=ptr(shifted))
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        refused(b"beta", beta=bad)
    refused(b"stats_out_dev is not 8-byte aligned", rows=rows.data_ptr() + 4)
    refused(b"weight_dev is not 8-byte aligned", wgt=wgt.data_ptr() + 4)
    with pytest.raises(smg_hip.SmgError):
        eng.loss_scene_policy(q.data_ptr(), shifted, hm, 16, masks.data_ptr(), 2, [0] * 16, [-1] * 16, [0] * 16, 3, BETA, act.data_ptr(),
                              wgt.data_ptr(), rows.data_ptr(), loss.data_ptr(), dq.data_ptr(), stream())
    torch.cuda.synchronize()
    assert bool((rows == FILL).all()) and bool((loss == FILL).all()) and bool((dq == FILL).all())
    # and the accepted call writes every element: the constant map 0 with weights (1, 1), so the policy is uniform, lse = H = log count
    # and the loss is lse - beta 0 - H = 0; groups 1 and 2 have no pair
    assert call(ok) == 0
    r, l, d = rows.cpu().numpy(), loss.cpu().numpy(), dq.cpu().numpy()
    assert r[0, 0] > 0 and not (d == FILL).any() and not (l == FILL).any() and (l[1:] == 0).all() and np.isfinite(d).all()
    assert abs(l[0]) <= ref.GATE * 2 * np.log(r[0, 0]) and abs(r[0, 2] - np.log(r[0, 0])) <= softmax_side.ref.lse_gate(np.log(r[0, 0]))


# ---- the Trainer's methods ---------------------------------------------------------------------------------------------------------
def test_train_batch_scene_policy_vs_fp64_oracle_s704(gpu):
    """test_train_batch_scene_maps_vs_fp64_oracle_s704's scene: a 240^2 heightmap, two samples (rotations 1 and 6 of 16) that form
    ONE group selected by the 9 x 9 block mask, the action in the block, w_nll = 1, w_ent = 0.1, temperature 1 / 3.  The loss
    against the restatement over the product's own q (the kernel gate) and against the fp64 oracle, all 368 gradient tensors within
    3x the fp32 oracle's own error, the head's conv1 weight gradient identical between two runs.
    The oracle gate: the loss is a function of the candidates' values v_i, each a convex combination of its sample's q.  Its
    gradient is dloss/dv_i = pi_i (w_nll beta + w_ent beta^2 (v_i - mean)) - w_nll beta [i == act], so
        sum_i |dloss/dv_i| <= |w_nll| beta (sum pi + 1) + |w_ent| beta^2 sum_i pi_i |v_i - mean| <= 2 |w_nll| beta + |w_ent| beta^2 range(v)
    (sum pi = 1, |v_i - mean| <= max v - min v), and a relative error of 1e-3 of the largest |q| on every v_i moves the loss by at
    most 1e-3 scale (2 |w_nll| beta + |w_ent| beta^2 range of v)."""
    sc = s704_scene(1)
    hm, style, rots, block, aff, depth, md, x, mx, on, q64 = (sc[k] for k in ("hm", "style", "rots", "block", "aff", "depth", "md", "x", "mx", "on", "q64"))
    beta, w_nll, w_ent = 3.0, 1.0, 0.1
    mask = np.zeros((1, hm, hm))
    mask[0, block[:, 0], block[:, 1]] = 1.0
    k_act = 30                                                 # the action: sample 1, pixel block[30]
    action = (1, (int(block[k_act, 0]), int(block[k_act, 1])))

    def total(vs):
        v = torch.cat(vs)
        lse = torch.logsumexp(beta * v, 0)
        H = lse - beta * (torch.softmax(beta * v, 0) * v).sum()
        return w_nll * (lse - beta * v[81 + k_act]) - w_ent * H
    v64 = [scene_ref.scene_points(q64[j][0, 0], aff[j], hm, block) for j in range(2)]
    loss64 = total(v64)
    loss64.backward()
    g64 = {n: p.grad for n, p in sc["o64"].named_parameters() if p.grad is not None}
    on.zero_grad()
    qo = [orc.forward(on, x, mx, style, False, r) for r in rots]
    total([scene_ref.scene_points(qo[j][0, 0], aff[j], hm, block) for j in range(2)]).backward()

    tr = make_trainer('reinforcement', 1)
    runs = []
    for it in range(2):
        loss, q, stats = tr.train_batch_scene_policy(depth, md, style, rots, mask, [0, 0], [0, 0], [action], 1.0 / beta, [w_nll], [w_ent],
                                                     return_q=True, return_stats=True)
        assert tuple(q.shape) == (2, 1, 3, 3) and tuple(loss.shape) == (1,) and tuple(stats.shape) == (1, 4)
        runs.append(dict(tr.model.named_parameters())[HEAD + "conv1.weight"].grad.clone())
    qh = q.cpu().numpy()
    maps = scene_ref.scene_maps(qh[:, 0], aff, hm)[0].astype(np.float32)
    want = ref.policy(maps, aff, hm, mask, [0, 0], [-1, -1], [0, 0], 1, beta, [flat(hm, 1, *action[1])], [[w_nll, w_ent]])
    got = float(loss.cpu().numpy()[0])
    print("loss %.7f, restatement over the same q %.7f, |d| %.2e (gate %.2e); count %d" % (got, want["loss"][0], abs(got - want["loss"][0]),
                                                                                          ref.GATE * want["scale"][0], want["stats"][0, 0]))
    assert want["stats"][0, 0] == 162 and stats.cpu().numpy()[0, 0] == 162
    assert abs(got - want["loss"][0]) <= ref.GATE * want["scale"][0]
    scale = max(float(q64[j].detach().abs().max()) for j in range(2))
    v = torch.cat(v64).detach().numpy()
    gate = 1e-3 * scale * (2 * abs(w_nll) * beta + abs(w_ent) * beta * beta * float(v.max() - v.min()))
    loss64 = float(loss64.detach())
    print("fp64 oracle %.7f, |d| %.2e (gate %.2e)" % (loss64, abs(got - loss64), gate))
    assert abs(got - loss64) <= gate
    assert_train_batch_runs(tr, runs, on, g64, "S=704 scene policy")


def test_backprop_scene_policy(gpu, capsys):
    """backprop_scene_policy on best_scene_actions' dict at hm = 240 with two box objects: a finite loss and the reference's line;
    weight = 0 and entropy_weight = 0 leave every parameter gradient exactly zero; the loss of train_batch_scene_policy on the same
    16 rotations equals beta-weighted -log pi recomputed by the restatement from the returned q."""
    HM, R, T = sample_side.HM, sample_side.R, sample_side.TEMPERATURE_TR
    tr = make_trainer('reinforcement', 4, R=R)
    depth, obj = sample_side.scene()
    best = tr.best_scene_actions(depth, obj)
    for action in ("grasp", "suction", "grasp_then_suction"):
        loss = tr.backprop_scene_policy(depth, action, best, obj[..., None], T, weight=1.0, entropy_weight=0.05)
        line = capsys.readouterr().out.strip().splitlines()[-1]
        assert loss.shape == () and np.isfinite(loss) and line == 'Training loss: %f' % loss, (action, loss, line)
    tr.backprop_scene_policy(depth, "grasp", best, obj, T, weight=0.0, entropy_weight=0.0)
    assert all(float(p.grad.abs().max()) == 0 for p in tr.model.parameters() if p.grad is not None)
    assert any(p.grad is not None for p in tr.model.parameters())
    k, rot = best["bestg_id"]
    pixel = best["bestg_pixel"]
    loss, q, stats = tr.train_batch_scene_policy(depth, depth * obj[k], 0, list(range(R)), obj[k][None], [0] * R, [0] * R, [(rot, pixel)], T,
                                                 [1.0], [0.0], return_q=True, return_stats=True)
    aff = one_plane.affines(R)
    maps = scene_ref.scene_maps(q.cpu().numpy()[:, 0], aff, HM)[0].astype(np.float32)
    want = ref.policy(maps, aff, HM, obj[k][None], [0] * R, [-1] * R, [0] * R, 1, 1.0 / T, [flat(HM, rot, *pixel)], [[1.0, 0.0]])
    got, row = float(loss.cpu().numpy()[0]), stats.cpu().numpy()[0]
    nlogp = -((1.0 / T) * want["vact"][0] - row[2])             # -(beta v - lse), as _with_logp forms log pi
    print("backprop_scene_policy: loss %.7f, -log pi from the restatement %.7f, from the device's lse %.7f" % (got, want["loss"][0], nlogp))
    assert abs(got - want["loss"][0]) <= ref.GATE * want["scale"][0] and abs(got - nlogp) <= ref.GATE * want["scale"][0]
    assert got > 0 and row[0] == want["stats"][0, 0] > 1
