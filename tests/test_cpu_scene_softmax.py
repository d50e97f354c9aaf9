"""CPU-side checks of the Boltzmann normaliser (no GPU): the C ABI declares and exports smg_scene_softmax_objects and
smg_scene_class_softmax_objects and the binding carries them; tests/scene_softmax_ref.py's restatement agrees with a brute-force
loop and with torch.logsumexp in float64; the limits beta = 0 and beta large; the entropy against -sum p log p; arithmetic mean <=
mellowmax <= Boltzmann mean <= vmax; the header's streaming update and merge against the whole, within the gate; sum exp(beta v - lse) = 1;
Trainer.merge_policy_stats against the whole; the inputs of tests/test_gpu_scene_softmax.py through the restatement alone - every
group expected non-empty is, every shifted or steep case is finite -; and the Trainer methods refuse before they touch an engine."""
import math

import numpy as np
import pytest
import torch

from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_objects_ref
import scene_ref
import scene_softmax_ref as ref
import test_gpu_scene_softmax as gpu_side

TAIL = (r"const double\*\s*masks_dev,\s*int n_masks,\s*const int\*\s*map_mask_a,\s*const int\*\s*map_mask_b,\s*const int\*\s*map_group,\s*"
        r"int n_groups,\s*double beta,\s*double\*\s*stats_out_dev,\s*void\*\s*stream\)")


def test_both_exports_are_declared_exported_and_bound():
    hdr = assert_declared_exported_and_bound(
        "smg_scene_softmax_objects",
        r"\bint\s+smg_scene_softmax_objects\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int64_t map_stride,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*" + TAIL,
        15, "scene_softmax_objects", ["scene_policy_stats", "merge_policy_stats", "get_label_value_scene_soft"])
    assert_declared_exported_and_bound(
        "smg_scene_class_softmax_objects",
        r"\bint\s+smg_scene_class_softmax_objects\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*int cls,\s*" + TAIL,
        15, "scene_class_softmax_objects", ["scene_class_policy_stats"])
    for word in ("{count, vmax, lse, mean}", "fma(beta, M, log S)", "T / S", "(0, -inf, 0, 0)", "S = fma(S, r, 1)", "T = fma(T, r, v)",
                 "an empty side yields the other side unchanged", "(0, -inf, -inf, NaN)", "not 8-byte aligned", "negative, NaN or infinite"):
        assert word in hdr, word


def seeded(n, seed, scale=1.0, shift=0.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale + shift).astype(np.float32)


def test_restatement_against_a_brute_force_loop_and_torch():
    rng = np.random.default_rng(0)
    maps = rng.standard_normal((6, 9, 9)).astype(np.float32)
    maps[:, :2] = -np.inf                                  # invalid rows
    masks = (rng.random((3, 9, 9)) < 0.4).astype(np.float64)
    masks[2] = 0.0
    sel = dict(mask_a=[0, 1, 0, -1, 2, 1], mask_b=[-1, 0, -1, -1, -1, -1], groups=[0, 1, 0, 2, 3, 1], n_groups=5)
    for beta in (0.0, 0.5, 3.0, 40.0):
        got = ref.group_stats(maps, masks, beta=beta, **sel)
        for g in range(5):
            vals = []
            for m in range(6):
                if sel["groups"][m] != g:
                    continue
                see = scene_objects_ref.selected(masks, sel["mask_a"][m], sel["mask_b"][m])
                for iy in range(9):
                    for ix in range(9):
                        if see[iy, ix] and not np.isneginf(maps[m, iy, ix]):
                            vals.append(float(maps[m, iy, ix]))
            if not vals:
                assert g in (3, 4) and got[g, 0] == 0 and np.isneginf(got[g, 1:3]).all() and np.isnan(got[g, 3])
                continue
            z = sum(math.exp(beta * v) for v in vals)      # (small values: the plain sum does not overflow)
            lse, mean = math.log(z), sum(v * math.exp(beta * v) for v in vals) / z
            assert got[g, 0] == len(vals) and got[g, 1] == max(vals)
            assert abs(got[g, 2] - lse) <= ref.lse_gate(lse) and abs(got[g, 3] - mean) <= ref.mean_gate(max(abs(v) for v in vals))
            t = torch.tensor(vals, dtype=torch.float64)
            assert abs(got[g, 2] - float(torch.logsumexp(beta * t, 0))) <= ref.lse_gate(lse)
            assert abs(got[g, 3] - float((torch.softmax(beta * t, 0) * t).sum())) <= ref.mean_gate(max(abs(v) for v in vals))
    nan = maps.copy()
    nan[3, 5, 5] = np.nan
    got = ref.group_stats(nan, masks, beta=3.0, **sel)
    assert got[2, 0] == 63 and np.isnan(got[2, 1:]).all() and np.isfinite(got[[0, 1]]).all()


def test_limits_entropy_and_mellowmax():
    v = np.round(seeded(5000, 1) * 64) / np.float32(64)    # (multiples of 2^-6: the second largest value lies at least that far below)
    v[17] = v[40] = v[99] = v.max()                        # the maximum at least three times
    v64 = v.astype(np.float64)
    n, M, lse, mean = ref.stats_of(v, 0.0)
    assert (n, M) == (5000, v64.max()) and abs(lse - math.log(5000)) <= ref.lse_gate(lse) and abs(mean - math.fsum(v64) / 5000) <= ref.mean_gate(np.abs(v64).max())
    n, M, lse, mean = ref.stats_of(v, 1e6)
    assert abs((lse - 1e6 * M) - math.log(int((v == v.max()).sum()))) <= 1e-9 and abs(mean - M) <= ref.mean_gate(abs(M))
    for beta in (0.3, 3.0, 30.0):
        n, M, lse, mean = ref.stats_of(v, beta)
        p = np.exp(beta * v64 - lse)
        assert abs(math.fsum(p) - 1.0) <= ref.GATE                                  # sum exp(beta v - lse) = 1
        entropy = lse - beta * mean
        assert abs(entropy + math.fsum(p * np.log(p))) <= ref.GATE * max(1.0, beta * np.abs(v64).max())
        soft = (lse - math.log(n)) / beta
        assert math.fsum(v64) / n <= soft <= mean <= M and 0.0 <= entropy <= math.log(n)
    n, M, lse, mean = ref.stats_of(seeded(100, 2, shift=1000.0), 3.0)
    assert np.isfinite([lse, mean]).all() and lse > 3000.0


@pytest.mark.parametrize("beta", (0.0, 3.0, 1e4))
def test_streaming_update_and_merge_equal_the_whole(beta):
    """The header's ADD over every candidate, and MERGE over random splits (an empty part among them, each part streamed), against
    stats_of on the whole, within the gate; the count exact."""
    rng = np.random.default_rng(3)
    v = np.concatenate([seeded(700, 4), seeded(300, 5, shift=2.0), seeded(200, 6, shift=-50.0)])
    whole = ref.stats_of(v, beta)
    vmax = float(np.abs(v).max())

    def stream(part):
        st = ref.EMPTY
        for x in part:
            st = ref.add(st, x, beta)
        return st
    assert max(ref.gate_ratios(ref.finish(stream(v), beta), whole, vmax)) <= 1.0
    for _ in range(5):
        cuts = np.sort(rng.integers(0, len(v) + 1, size=6))
        cuts[3] = cuts[2]                                  # an empty part
        st = ref.EMPTY
        for part in np.split(v, cuts):
            st = ref.merge(st, stream(part), beta)
        r = ref.gate_ratios(ref.finish(st, beta), whole, vmax)
        assert max(r) <= 1.0, r
    assert ref.merge(ref.EMPTY, ref.EMPTY, beta) == ref.EMPTY and ref.finish(ref.EMPTY, beta)[:3] == (0.0, -np.inf, -np.inf)
    with_nan = ref.finish(ref.merge(stream(v[:10]), stream(np.asarray([1.0, np.nan, 2.0], dtype=np.float32)), beta), beta)
    assert with_nan[0] == 13 and np.isnan(with_nan[1:]).all()
    # the gate can fail: a float32 accumulator of S misses it
    if beta == 3.0:
        M = v.max()
        S32 = np.float32(0)
        for x in v:
            S32 += np.exp(np.float32(beta) * (x - M), dtype=np.float32)
        assert abs(beta * float(M) + math.log(float(S32)) - whole[2]) > ref.lse_gate(whole[2])


def test_merge_policy_stats_equals_the_whole():
    from trainer import Trainer
    parts = [seeded(400, 7), seeded(0, 8), seeded(250, 9, shift=1.5), seeded(30, 10, shift=-3.0)]
    for temps in (0.25, (0.25, 1.0, float("inf"))):
        seq = not np.isscalar(temps)
        betas = [1.0 / t for t in (temps if seq else [temps])]
        rows = np.array([[ref.stats_of(p, b) for p in parts] for b in betas])
        beta = np.asarray(betas).reshape(-1, 1) if seq else np.float64(betas[0])
        a = Trainer._policy_stats(rows[:, :2] if seq else rows[0, :2], beta)
        b = Trainer._policy_stats(rows[:, 2:] if seq else rows[0, 2:], beta)
        merged = Trainer.merge_policy_stats(a, b)
        assert merged["count"].shape == ((3, 1) if seq else (1,))
        for j, bt in enumerate(betas):
            whole = ref.stats_of(np.concatenate(parts), bt)
            got = [np.asarray(merged[f])[j, 0] if seq else merged[f][0] for f in ("count", "vmax", "lse", "mean")]
            assert max(ref.gate_ratios(got, whole, float(np.abs(np.concatenate(parts)).max()))) <= 1.0
            soft = np.asarray(merged["mellowmax"])[j, 0] if seq else merged["mellowmax"][0]
            arithmetic = float(np.concatenate(parts).astype(np.float64).mean())
            assert arithmetic - 1e-12 <= soft <= whole[3] + 1e-12 and whole[3] <= whole[1]
    empty = Trainer.merge_policy_stats(Trainer._policy_stats(np.array([ref.stats_of(parts[1], 4.0)]), np.float64(4.0)))
    assert empty["count"][0] == 0 and np.isneginf(empty["lse"][0]) and np.isnan(empty["mean"][0])
    with pytest.raises(ValueError):
        Trainer.merge_policy_stats()
    with pytest.raises(ValueError):
        Trainer.merge_policy_stats(Trainer._policy_stats(rows[0, :2], np.float64(4.0)), Trainer._policy_stats(rows[0, 2:], np.float64(2.0)))


@pytest.mark.parametrize("case", list(gpu_side.CASES))
def test_the_gpu_cases_through_the_restatement(case):
    """tests/test_gpu_scene_softmax.py's one-plane cases on scene_ref.scene_maps of the same seeded maps: the groups it expects to
    have candidates have them, the others none, every shifted or steep case is finite, and at beta = 10^4 the mean is vmax."""
    hm = 240
    qh, aff, sel, beta = gpu_side.CASES[case]()
    assert scene_ref.geometry(hm)[1:] == (gpu_side.S, gpu_side.SIDE) and len(aff) == len(qh) == len(sel["groups"])
    maps = scene_ref.scene_maps(qh, aff, hm)[0].astype(np.float32)
    rows = ref.group_stats(maps, gpu_side.masks_for(hm), beta=beta, **sel)
    print("%s: counts %s, lse %s" % (case, rows[:, 0].tolist(), rows[:, 2].tolist()))
    assert (rows[gpu_side.NONEMPTY, 0] > 0).all() and rows[3, 0] == len(qh) // 4 and (rows[gpu_side.EMPTY, 0] == 0).all()
    assert np.isfinite(rows[gpu_side.NONEMPTY]).all()
    if case in gpu_side.STEEP_OR_SHIFTED:
        assert np.isfinite(rows[gpu_side.NONEMPTY, 2:]).all()
    if case == "q + 1000":
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp(np.float64(beta) * rows[0, 1]))                  # a plain exp(beta v) overflows
    if case == "beta 1e4":
        for g in gpu_side.NONEMPTY:
            assert abs(rows[g, 3] - rows[g, 1]) <= ref.mean_gate(abs(rows[g, 1])), g


def test_trainer_methods_refuse_before_the_engine():
    # (on a CPU trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    d, m = np.zeros((240, 240)), np.ones((2, 240, 240))
    d224, m224 = np.zeros((224, 224)), np.ones((2, 224, 224))                   # S = 640: a 1 x 1 map has no extent
    rl, re = cpu_trainer('reinforcement'), cpu_trainer('reactive')
    with pytest.raises(ValueError):
        re.scene_policy_stats(d, m, 1.0)
    with pytest.raises(ValueError):
        rl.scene_class_policy_stats(d, m, 1.0)
    with pytest.raises(ValueError):
        rl.scene_policy_stats(d224, m224, 1.0)
    with pytest.raises(ValueError):
        re.scene_class_policy_stats(d224, m224, 1.0)
    with pytest.raises(ValueError):
        re.scene_class_policy_stats(d, m, 1.0, cls=3)
    for bad in (0.0, -0.5, float("nan"), float("-inf"), (1.0, 0.0), ()):
        with pytest.raises(ValueError):
            rl.scene_policy_stats(d, m, bad)
        with pytest.raises(ValueError):
            re.scene_class_policy_stats(d, m, bad)
    with pytest.raises(ValueError):
        re.get_label_value_scene_soft('grasp', 2, 0, 1, 0, d, m, 1.0, "expected")
    with pytest.raises(ValueError):
        rl.get_label_value_scene_soft('grasp', 2, 0, 1, 0, d, m, 1.0, "max")
    assert rl.get_label_value_scene_soft('grasp', 2, 0, 0, 0, d, m, 1.0, "mellowmax") == (0, 0)      # a zero-future case needs no forward
    # legal arguments pass every check and reach the engine, which a CPU trainer does not have
    with pytest.raises(RuntimeError):
        rl.scene_policy_stats(d, m, (0.5, float("inf")), joint=True)
    with pytest.raises(RuntimeError):
        re.scene_class_policy_stats(d, m, 0.01)
    with pytest.raises(RuntimeError):
        rl.sampled_scene_actions(d, m, 2, 1.0, 0, with_stats=True)
    with pytest.raises(RuntimeError):
        rl.get_label_value_scene_soft('grasp', 2, 0, 1, 0, d, m, 1.0, "expected")
    from trainer import Trainer
    assert Trainer._require_betas("t", 0.25) == ([4.0], False) and Trainer._require_betas("t", [float("inf"), 2.0]) == ([0.0, 0.5], True)
