"""numpy float64 restatement of smg_scene_softmax_objects' statistics (include/smg_hip.h), the reference of
tests/test_cpu_scene_softmax.py and tests/test_gpu_scene_softmax.py.  Plain helper module, no tests.

Like scene_objects_ref it starts from scene-frame maps that already exist - smg_scene_maps' output, a plane of
smg_scene_class_maps', or scene_ref.scene_maps' - and reuses scene_objects_ref.selected: selection and grouping are that module's,
what is restated here are the sums.  For the candidates v (float32, taken to float64) of a group and beta >= 0:
    count = len(v)        vmax = M = max(v)
    lse   = beta M + log(fsum(exp(beta (v - M))))
    mean  = fsum(v exp(beta (v - M))) / fsum(exp(beta (v - M)))
with math.fsum, the correctly rounded sum; a group without a candidate is (0, -inf, -inf, NaN), a NaN candidate makes vmax, lse and
mean NaN.  `add` and `merge` restate the header's streaming update and its merge rule on states (n, M, S, T).

The gate (`lse_gate`, `mean_gate`): |got - ref| <= 2^-36 max(1, |ref|) for lse and <= 2^-36 max(1, max|v|) for mean.  Derivation: the
device reaches S (and T) of a group through at most 32 sequential updates per thread (8 passes of 4 pixels), two 8-level trees (the
workgroup's and the grouped reduce's), a few slots per thread of the reduce and a carry per launch of 32 maps; every step is a few
roundings of 2^-53 relative, plus the argument error of exp - beta (v - M) is rounded once, and |beta (v - M)| is below 745 for
every term that is not 0, which exp turns into at most 745 2^-53 relative.  Crudely ~1000 2^-53 ~ 2^-43 relative on S and T; lse =
beta M + log S moves by that much absolutely plus one rounding of its own size, mean = T / S by that much of max|v|.  The factor 2^7
on top covers a device exp / log that is a few ulp rather than one.  The gate is still 4000 times below one float32 rounding
(2^-24), so a float accumulator, a missed rescale of the carried state or a wrong carry fails it.  No case is left out of any
comparison - there is no cap to state.  `count` is compared exactly: that is what catches a dropped or doubled candidate whose
weight lies below the gate."""
import math

import numpy as np

from scene_objects_ref import selected

GATE = 2.0 ** -36
EMPTY = (0, -np.inf, 0.0, 0.0)


def stats_of(v, beta):
    """(count, vmax, lse, mean) of the candidate values v (any float array) at beta, in float64 with math.fsum."""
    v = np.asarray(v, dtype=np.float64).ravel()
    if v.size == 0:
        return 0.0, -np.inf, -np.inf, np.nan
    if np.isnan(v).any():
        return float(v.size), np.nan, np.nan, np.nan
    M = float(v.max())
    e = np.exp(np.float64(beta) * (v - M))
    S = math.fsum(e)
    return float(v.size), M, float(beta) * M + math.log(S), math.fsum(v * e) / S


def candidates(maps, masks, mask_a, mask_b, groups, g):
    """float32 candidate values of group g in ascending flattened order (scene_objects_ref.group_argmax's candidates)."""
    vals = [maps[m][selected(masks, mask_a[m], mask_b[m]) & ~np.isneginf(maps[m])] for m in range(len(groups)) if groups[m] == g]
    return np.concatenate(vals) if vals else np.zeros(0, dtype=np.float32)


def group_stats(maps, masks, mask_a, mask_b, groups, n_groups, beta):
    """maps float32 [n_maps, hm, hm] (-inf = invalid), masks [n_masks, hm, hm], mask_a / mask_b / groups n_maps ints each -> float64
    [n_groups, 4] = {count, vmax, lse, mean} per group."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.ndim == 3 and beta >= 0 and np.isfinite(beta)
    assert len(mask_a) == len(mask_b) == len(groups) == maps.shape[0]
    return np.array([stats_of(candidates(maps, masks, mask_a, mask_b, groups, g), beta) for g in range(n_groups)], dtype=np.float64)


def add(state, v, beta):
    """The header's ADD: one candidate v into the state (n, M, S, T)."""
    n, M, S, T = state
    v = float(v)
    if n == 0:
        return 1, v, 1.0, v
    if v <= M or math.isnan(M):
        e = math.exp(beta * (v - M))
        return n + 1, M, S + e, T + v * e
    r = math.exp(beta * (M - v))
    return n + 1, v, S * r + 1.0, T * r + v


def merge(A, B, beta):
    """The header's MERGE of the states A (the earlier one) and B."""
    if B[0] == 0:
        return A
    if A[0] == 0:
        return B
    M = A[1] if A[1] > B[1] or math.isnan(A[1]) else B[1]
    if math.isnan(M):
        return A[0] + B[0], math.nan, math.nan, math.nan
    fa, fb = math.exp(beta * (A[1] - M)), math.exp(beta * (B[1] - M))
    return A[0] + B[0], M, A[2] * fa + B[2] * fb, A[3] * fa + B[3] * fb


def finish(state, beta):
    """The state as the output row (count, vmax, lse, mean)."""
    n, M, S, T = state
    if n == 0:
        return 0.0, -np.inf, -np.inf, np.nan
    if math.isnan(M):
        return float(n), np.nan, np.nan, np.nan
    return float(n), M, beta * M + math.log(S), T / S


def lse_gate(ref):
    return GATE * max(1.0, abs(ref))


def mean_gate(vabs_max):
    return GATE * max(1.0, vabs_max)


def gate_ratios(got, ref, vabs_max):
    """got / ref rows (count, vmax, lse, mean) of ONE group, vabs_max = max|v| of its candidates -> (lse ratio, mean ratio) =
    |got - ref| / gate, after the exact parts: count equal, vmax equal (both NaN counts as equal), NaN and -inf where the reference
    has them.  A ratio <= 1 passes."""
    assert got[0] == ref[0], ("count", got[0], ref[0])
    assert got[1] == ref[1] or (np.isnan(got[1]) and np.isnan(ref[1])), ("vmax", got[1], ref[1])
    if ref[0] == 0:
        assert np.isneginf(got[2]) and np.isnan(got[3]), got
        return 0.0, 0.0
    if np.isnan(ref[1]):
        assert np.isnan(got[2]) and np.isnan(got[3]), got
        return 0.0, 0.0
    assert np.isfinite(got[2]) and np.isfinite(got[3]), got
    return abs(got[2] - ref[2]) / lse_gate(ref[2]), abs(got[3] - ref[3]) / mean_gate(vabs_max)


def assert_rows(got, maps, masks, beta, what, **sel):
    """Device rows [n_groups, 4] against group_stats on the same float32 maps: every group through gate_ratios.  Prints and returns
    the largest (lse, mean) ratio."""
    ref = group_stats(maps, masks, beta=beta, **sel)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    worst = [0.0, 0.0]
    for g in range(ref.shape[0]):
        v = candidates(maps, masks, sel["mask_a"], sel["mask_b"], sel["groups"], g)
        finite = v[np.isfinite(v)]
        r = gate_ratios(got[g], ref[g], float(np.abs(finite).max()) if finite.size else 0.0)
        worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print("%s: beta %g, counts %s; largest error / gate: lse %.3g, mean %.3g" % (what, beta, ref[:, 0].astype(np.int64).tolist(), worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (what, worst)
    return worst
