"""The loss of the Boltzmann policy in the scene frame without a GPU: include/smg_hip.h declares smg_loss_scene_policy and the
library exports it; tests/scene_policy_ref.py - the float64 restatement of loss and dq the GPU tests gate the kernels against - is
itself checked against torch fp64 autograd, its limits and a finite difference; the GPU cases' inputs go through the restatement
alone; the Trainer's methods refuse what they must before anything reaches the engine."""
import numpy as np
import pytest
import torch

from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_policy_ref as ref
import scene_ref
import test_gpu_scene_policy as gpu_side

ROTS = (0, 3, 8, 13)


def test_the_export_is_declared_exported_and_bound():
    hdr = assert_declared_exported_and_bound(
        "smg_loss_scene_policy",
        r"\bint\s+smg_loss_scene_policy\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*const float\*\s*affine_host,\s*int hm_size,\s*"
        r"int n_pairs,\s*const double\*\s*masks_dev,\s*int n_masks,\s*const int\*\s*pair_mask_a,\s*const int\*\s*pair_mask_b,\s*"
        r"const int\*\s*pair_group,\s*int n_groups,\s*double beta,\s*const int\*\s*action_dev,[\s\S]*?const double\*\s*weight_dev,[\s\S]*?"
        r"double\*\s*stats_out_dev,[\s\S]*?float\*\s*loss_dev,[\s\S]*?float\*\s*dq_dev,[\s\S]*?void\*\s*stream\);",
        18, "loss_scene_policy", ["train_batch_scene_policy", "backprop_scene_policy"])
    for word in ("loss_g = w_nll (lse_g - beta v_act) - w_ent H_g", "A = w_nll beta,  B = w_ent beta^2,  C = -w_nll beta", "treated as the identity",
                 "w_nll is ignored", "(0, -inf, -inf, NaN)", "No address is ever formed from the action", "not 8-byte aligned",
                 "negative, NaN or infinite", "fma(beta, v, -lse)", '"dense dq"'):
        assert word in hdr, word


def small_case(hm, seed=0):
    """Two groups over four pairs (rotations 0, 3, 8, 13 of 16): group 0 = pairs 0 and 2, pair 0 the union of two masks; group 1 =
    pairs 1 and 3.  Both groups act; the weights have mixed signs."""
    side = scene_ref.geometry(hm)[2]
    c = hm // 2
    q = np.random.default_rng(seed + hm).standard_normal((4, side, side))
    aff = np.stack([scene_ref.theta(r, 16) for r in ROTS])
    masks = np.zeros((3, hm, hm))
    masks[0, c - 6:c + 5, c - 4:c + 7] = 1.0
    masks[1, c - 20:c - 9, c - 10:c + 12] = 2.5
    masks[2, c + 3:c + 15, c - 12:c] = -1.0
    sel = dict(mask_a=[0, 2, 0, 2], mask_b=[1, -1, -1, -1], groups=[0, 1, 0, 1], n_groups=2)
    actions = [gpu_side.flat(hm, 2, c - 1, c + 2), gpu_side.flat(hm, 1, c + 5, c - 3)]
    return dict(hm=hm, q=q, aff=aff, masks=masks, sel=sel, beta=2.5, actions=actions, weights=[[1.0, 0.15], [-0.6, -0.2]])


def restate(c, round32=False, **change):
    c = dict(c, **change)
    values = scene_ref.scene_maps(c["q"].reshape(len(c["aff"]), c["q"].shape[-2], c["q"].shape[-1]), c["aff"], c["hm"])[0]
    return ref.policy(values, c["aff"], c["hm"], c["masks"], beta=c["beta"], actions=c["actions"], weights=c["weights"], round32=round32, **c["sel"])


@pytest.mark.parametrize("hm,side", ((240, 3), (320, 10)))
def test_restatement_against_torch_fp64_autograd(hm, side):
    """Loss and dq of the restatement on unrounded values against torch fp64 autograd of w_nll (logsumexp(beta v) - beta v_act) -
    w_ent H over scene_ref.scene_points: fp64 rounding, 1e-12 of max|dq|.  The sum of dq over a group's pairs is 0 (sum pi = 1,
    sum pi (v - mean) = 0, bilinear weights that sum to 1)."""
    assert scene_ref.geometry(hm)[2] == side
    c = small_case(hm)
    got = restate(c)
    loss, dq = ref.torch_policy(c["q"], c["aff"], hm, c["masks"], beta=c["beta"], actions=c["actions"], weights=c["weights"], **c["sel"])
    print("hm %d: counts %s, loss %s, max|dq| %.3g, max|d dq| %.3g" % (hm, got["stats"][:, 0].tolist(), got["loss"].tolist(), np.abs(dq).max(), np.abs(got["dq"] - dq).max()))
    assert (got["stats"][:, 0] > 100).all() and not np.isnan(got["vact"]).any()
    assert np.abs(got["loss"] - loss).max() <= 1e-12 * np.abs(loss).max()
    assert np.abs(got["dq"] - dq).max() <= 1e-12 * np.abs(dq).max() and np.abs(dq).max() > 1e-3
    for g in range(2):
        pairs = [j for j in range(4) if c["sel"]["groups"][j] == g]
        assert abs(got["dq"][pairs].sum()) <= 1e-12 * np.abs(got["dq"][pairs]).sum()
    # float32-rounded values move the result by rounding of that size only
    r32 = restate(c, round32=True)
    assert 0 < np.abs(r32["dq"] - got["dq"]).max() <= 1e-5 * np.abs(dq).max()


def test_limits_of_the_restatement():
    c = small_case(240)
    # beta = 0: the uniform policy - dq exactly 0, loss (w_nll - w_ent) log count
    z = restate(c, beta=0.0)
    assert (z["dq"] == 0).all()
    for g in range(2):
        w = c["weights"][g]
        assert abs(z["loss"][g] - (w[0] - w[1]) * np.log(z["stats"][g, 0])) <= 1e-13
    # act = -1: the NLL term and C are absent and w_nll is ignored, a NaN included
    plain = restate(c, actions=[-1, -1], weights=[[0.0, 0.15], [0.0, -0.2]])
    ignored = restate(c, actions=[-1, -1], weights=[[np.nan, 0.15], [123.0, -0.2]])
    assert np.array_equal(plain["loss"], ignored["loss"]) and np.array_equal(plain["dq"], ignored["dq"]) and np.isfinite(plain["dq"]).all()
    H = plain["stats"][:, 2] - c["beta"] * plain["stats"][:, 3]
    assert np.allclose(plain["loss"], -np.asarray([0.15, -0.2]) * H, rtol=1e-14, atol=0)
    # a negative w_nll: the loss and dq are linear in the weights
    a, b = restate(c, weights=[[1.0, 0.0], [1.0, 0.0]]), restate(c, weights=[[-2.0, 0.0], [-2.0, 0.0]])
    assert np.allclose(b["loss"], -2 * a["loss"], rtol=1e-14) and np.allclose(b["dq"], -2 * a["dq"], rtol=1e-13, atol=1e-18)
    # the loss is -(beta v - lse), the way _with_logp forms log pi
    assert np.array_equal(a["loss"], 1.0 * (a["stats"][:, 2] - c["beta"] * a["vact"])) and (a["loss"] > 0).all()
    logp = c["beta"] * np.float64(a["vact"]) - a["stats"][:, 2]
    assert np.allclose(a["loss"], -logp, rtol=1e-15, atol=0)
    # an action that is no candidate: NaN loss, the pi and entropy parts of dq stay
    hm = c["hm"]
    for bad in (gpu_side.flat(hm, 2, 3, 3), gpu_side.flat(hm, 1, 120, 120), 4 * hm * hm + 7, gpu_side.flat(hm, 2, 20, 120)):
        r = restate(c, actions=[bad, c["actions"][1]])
        assert np.isnan(r["loss"][0]) and np.isnan(r["vact"][0]) and np.isfinite(r["dq"]).all() and r["loss"][1] == restate(c)["loss"][1]
        only_pi = restate(c, actions=[-1, c["actions"][1]], weights=[[0.0, 0.15], c["weights"][1]])
        with_a = restate(c, actions=[-1, c["actions"][1]], weights=[[0.0, 0.0], c["weights"][1]])
        assert np.abs(r["dq"][[0, 2]]).max() > 0 and np.array_equal(with_a["dq"][[1, 3]], r["dq"][[1, 3]]) and np.isfinite(only_pi["dq"]).all()
    # an empty group (a mask without a pixel; a group without a pair): loss 0 without an action, NaN with one, dq exactly 0
    sel = dict(c["sel"], groups=[0, 1, 0, 2], n_groups=4)
    e = restate(c, masks=np.concatenate([c["masks"][:2], np.zeros((1, hm, hm))]), sel=sel, actions=[c["actions"][0], -1, -1, 5], weights=[[1, 1]] * 4)
    assert e["stats"][1, 0] == e["stats"][2, 0] == e["stats"][3, 0] == 0 and e["loss"][1] == e["loss"][2] == 0 and np.isnan(e["loss"][3])
    assert (e["dq"][[1, 3]] == 0).all() and np.isfinite(e["loss"][0])
    # a NaN candidate: its group's loss and every element of its pairs' dq NaN, the other group untouched
    q = c["q"].copy()
    q[0, 1, 1] = np.nan
    n, base = restate(c, q=q), restate(c)
    assert np.isnan(n["loss"][0]) and np.isnan(n["dq"][[0, 2]]).all() and n["loss"][1] == base["loss"][1] and np.array_equal(n["dq"][[1, 3]], base["dq"][[1, 3]])


def test_entropy_term_by_a_central_finite_difference():
    """d(-w_ent H)/dq on one map element against (loss(q + h) - loss(q - h)) / 2h of the restatement itself."""
    c = small_case(240, seed=3)
    c = dict(c, actions=[-1, -1], weights=[[0.0, 1.0], [0.0, -0.5]])
    base = restate(c)
    for j, el in ((0, (1, 1)), (3, (1, 1))):
        h = 1e-5
        up, dn = c["q"].copy(), c["q"].copy()
        up[(j,) + el] += h
        dn[(j,) + el] -= h
        fd = (restate(c, q=up)["loss"].sum() - restate(c, q=dn)["loss"].sum()) / (2 * h)
        print("pair %d element %s: dq %.9f, finite difference %.9f" % (j, el, base["dq"][(j,) + el], fd))
        assert abs(fd - base["dq"][(j,) + el]) <= 1e-7 * max(1.0, np.abs(base["dq"]).max()) and abs(fd) > 1e-4


@pytest.mark.parametrize("case", list(gpu_side.CASES))
def test_the_gpu_cases_through_the_restatement(case):
    """tests/test_gpu_scene_policy.py's cases on scene_ref.scene_maps of the same seeded maps, rounded to float32: every acting
    group has candidates and a candidate action, the empty groups none, everything that should be finite is, and every case has
    at least one non-empty group with an action."""
    c = gpu_side.CASES[case]()
    hm = c["hm"]
    assert len(c["aff"]) == len(c["q"]) == len(c["sel"]["groups"]) and c["q"].shape[1] == 1
    maps = scene_ref.scene_maps(c["q"][:, 0], c["aff"], hm)[0].astype(np.float32)
    r = ref.policy(maps, c["aff"], hm, c["masks"], beta=c["beta"], actions=c["actions"], weights=c["weights"], **c["sel"])
    print("%s: counts %s, loss %s" % (case, r["stats"][:, 0].tolist(), r["loss"].tolist()))
    assert len(c["acting"]) >= 1
    assert (r["stats"][c["acting"], 0] > 1).all() and not np.isnan(r["vact"][c["acting"]]).any() and all(c["actions"][g] >= 0 for g in c["acting"])
    assert (r["stats"][c["empty"], 0] == 0).all() and (r["loss"][c["empty"]] == 0).all()
    assert np.isfinite(r["loss"]).all() and np.isfinite(r["dq"]).all()
    if case == "beta 0":
        assert (r["dq"] == 0).all()
    elif case != "beta 1e4":
        acting_pairs = [j for j, g in enumerate(c["sel"]["groups"]) if g in c["acting"]]
        assert (np.abs(r["dq"][acting_pairs]).reshape(len(acting_pairs), -1).max(1) > 0).all()
    if case == "q + 1000":
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp(np.float64(c["beta"]) * r["stats"][0, 1]))          # a plain exp(beta v) overflows
    if case == "40 pairs":
        assert r["loss"][1] == r["loss"][2] and np.array_equal(r["dq"][1], r["dq"][33])


def test_trainer_methods_refuse_before_the_engine():
    # (on a CPU trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    hm = 240
    d = np.zeros((hm, hm))
    masks = np.zeros((2, hm, hm))
    masks[0, 110:130, 110:130] = 1.0
    masks[1, 0:10, 0:10] = 1.0
    rl, re = cpu_trainer('reinforcement'), cpu_trainer('reactive')
    ok = dict(depth_heightmap=d, m_depth_heightmap=d, style=0, rotations=[1, 6, 3], select_masks=masks, sample_masks=[0, 0, (0, 1)],
              sample_groups=[0, 0, 1], actions=[(1, (120, 121)), None], temperature=0.5)

    def refused(tr=rl, **change):
        with pytest.raises(ValueError):
            tr.train_batch_scene_policy(**dict(ok, **change))
    refused(tr=re)                                                              # reinforcement method only
    refused(depth_heightmap=np.zeros((224, 224)), m_depth_heightmap=np.zeros((224, 224)), select_masks=np.zeros((2, 224, 224)))   # a 1 x 1 map
    refused(actions=[(2, (120, 121)), None])                                    # the sample is in another group
    refused(actions=[(3, (120, 121)), None])                                    # no such sample
    refused(actions=[(1, (240, 121)), None])                                    # outside the heightmap
    refused(actions=[(1, (-1, 121)), None])
    refused(actions=[(1, (120.5, 121)), None])
    refused(actions=[None, (2, (5, 5))])                                        # selected by mask 1, but without a window in rotation 3
    refused(actions=[(1, (100, 121)), None])                                    # a window, but not selected
    for bad in (0.0, -1.0, float("nan"), (0.5,), [0.5, 1.0]):
        refused(temperature=bad)
    for bad in ([1.0, float("nan")], [float("inf"), 1.0], [1.0]):
        refused(nll_weights=bad)
        refused(entropy_weights=bad)
    refused(sample_masks=[0, 0, 2])
    refused(sample_masks=[0, 0])
    refused(sample_groups=[0, 0, 2])
    refused(select_masks=masks[:, :100])
    assert not rl.scene_to_map(hm, 3, 16, [[5, 5]])[2][0] and rl.scene_to_map(hm, 6, 16, [[100, 121]])[2][0]
    # legal arguments pass every check and reach the engine, which a CPU trainer does not have
    with pytest.raises(RuntimeError):
        rl.train_batch_scene_policy(**ok)
    with pytest.raises(RuntimeError):
        rl.train_batch_scene_policy(**dict(ok, nll_weights=[-0.5, 0.0], entropy_weights=[0.1, 0.2], temperature=float("inf")))
    # backprop_scene_policy: the method, the primitive and a dict without the action are refused first
    obj = np.zeros((2, hm, hm))
    obj[0, 112:128, 110:120] = 1.0
    obj[1, 114:126, 121:131] = 1.0
    best = dict(bestg_id=(0, 3), bestg_pixel=(120, 115), bestg_conf=1.0, bests_id=None, bests_pixel=None, bests_conf=-np.inf,
                bestgs_num=(0, 1), bestgs_pixel=(120, 125), bestgs_conf=0.5)
    with pytest.raises(ValueError):
        re.backprop_scene_policy(d, 'grasp', best, obj, 0.5)
    with pytest.raises(ValueError):
        rl.backprop_scene_policy(d, 'push', best, obj, 0.5)
    with pytest.raises(ValueError):
        rl.backprop_scene_policy(d, 'suction', best, obj, 0.5)
    with pytest.raises(ValueError):
        rl.backprop_scene_policy(d, 'grasp', best, obj, 0.0)
    with pytest.raises(ValueError):
        rl.backprop_scene_policy(d, 'grasp', dict(best, bestg_pixel=(5, 5)), obj, 0.5)      # not on the object
    with pytest.raises(ValueError):
        rl.backprop_scene_policy(d, 'grasp', best, obj, 0.5, weight=float("nan"))
    for action in ('grasp', 'grasp_then_suction'):
        with pytest.raises(RuntimeError):
            rl.backprop_scene_policy(d, action, best, obj[..., None], 0.5, weight=-0.3, entropy_weight=0.01)
