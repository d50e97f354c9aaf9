"""numpy restatement of smg_scene_sample_objects' Boltzmann draw (include/smg_hip.h), the reference of
tests/test_cpu_scene_sample.py and tests/test_gpu_scene_sample.py.  Plain helper module, no tests.

Like scene_objects_ref it starts from scene-frame maps that already exist - smg_scene_maps' output, a plane of
smg_scene_class_maps', or scene_ref.scene_maps' - and reuses scene_objects_ref.selected: what is restated here is the noise and the
pick.  For a candidate with flattened index i into [n_maps, hm, hm], draw d and a 64-bit seed, all integers mod 2^64:
    x = seed + (d << 32) + i
    mix(x): x += 0x9E3779B97F4A7C15; z = x; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
            return z ^ z >> 31
    h = mix(mix(x));   u = ((h >> 12) + 0.5) * 2^-52;   G = -log(-log(u))
and the score is s = float32(beta * float64(v) + G); draw d of a group is np.argmax of the scores (the first NaN wins, the lowest
flattened index on ties) over the group's selected valid pixels.

Two places where this restatement and the kernel may differ in the last bit of a score, and the rule that covers them:
  - numpy's log and the device's need not agree in the last bit of G;
  - the kernel forms fma(beta, v, G), one rounding to double; numpy has no fma, so beta * v is rounded to double before G is added
    unless the product is exact (beta = 0, 3, 8 and a float32 v: it is) - at most one ulp of double, 2^-29 of a float32 step.
Each of two scores is off by at most one float32 rounding, which moves their difference by at most 2^-22 of the larger: a (group,
draw) is COMPARED when gap >= 2^-20 * max(|s1|, |s2|, 2^-100), gap = the difference of the two best float32 scores (`compared`)."""
import numpy as np

from scene_objects_ref import selected

GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def mix(x):
    """The splitmix64 finaliser on uint64 arrays (synthetic._splitmix64's arithmetic)."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=np.uint64) + GOLDEN
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def unit(h):
    """u of a hash h: ((h >> 12) + 0.5) * 2^-52, exact in float64 and strictly inside (0, 1)."""
    return ((np.asarray(h, dtype=np.uint64) >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52


def gumbel(seed, d, flat):
    """G float64 for the flattened indices `flat` (ints below 2^31) of draw d."""
    assert 0 <= int(seed) < 2 ** 64 and int(d) >= 0
    flat = np.asarray(flat, dtype=np.int64)
    assert ((flat >= 0) & (flat < 2 ** 31)).all()
    with np.errstate(over="ignore"):
        x = np.uint64((int(seed) + (int(d) << 32)) % 2 ** 64) + flat.astype(np.uint64)
    return -np.log(-np.log(unit(mix(mix(x)))))


def scores(v, beta, seed, d, flat):
    """float32 scores of the candidates with float32 values v at the flattened indices flat."""
    v = np.asarray(v)
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return (np.float64(beta) * v.astype(np.float64) + gumbel(seed, d, flat)).astype(np.float32)


def compared(gap, s1, s2):
    """Which (group, draw) the comparison rule of the module's docstring compares; a pick that hangs on no rounding (gap = inf: a
    NaN's win, a lone candidate, no candidate) always is."""
    with np.errstate(invalid="ignore"):
        return np.isposinf(gap) | (gap >= 2.0 ** -20 * np.maximum(np.maximum(np.abs(s1), np.abs(s2)), 2.0 ** -100))


def group_sample_scores(maps, masks, mask_a, mask_b, groups, n_groups, n_draws, beta, seed):
    """group_sample's (idx, val, gap) and the two best float32 scores (s1, s2) as float64 [n_groups, n_draws] (s2 = -inf with one
    candidate; both -inf with none)."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.ndim == 3 and n_draws >= 1 and beta >= 0 and np.isfinite(beta)
    n_maps, npix = maps.shape[0], maps.shape[1] * maps.shape[2]
    assert len(mask_a) == len(mask_b) == len(groups) == n_maps
    idx = np.full((n_groups, n_draws), -1, dtype=np.int64)
    val = np.full((n_groups, n_draws), -np.inf, dtype=np.float32)
    gap = np.full((n_groups, n_draws), np.inf)
    s1 = np.full((n_groups, n_draws), -np.inf)
    s2 = np.full((n_groups, n_draws), -np.inf)
    for g in range(n_groups):
        cand_i, cand_v = [], []
        for m in range(n_maps):
            if groups[m] != g:
                continue
            at = np.flatnonzero((selected(masks, mask_a[m], mask_b[m]) & ~np.isneginf(maps[m])).ravel())
            cand_i.append(m * npix + at)
            cand_v.append(maps[m].ravel()[at])
        if not cand_i or not sum(len(c) for c in cand_i):
            continue
        ci, cv = np.concatenate(cand_i), np.concatenate(cand_v)       # ascending flattened order: np.argmax takes the lowest on ties
        for d in range(n_draws):
            s = scores(cv, beta, seed, d, ci)
            k = int(np.argmax(s))                                      # (the first NaN wins)
            idx[g, d], val[g, d] = ci[k], cv[k]
            if np.isnan(s[k]) or len(s) == 1:                          # a NaN's win, or a lone candidate's, hangs on no rounding
                s1[g, d] = s[k]
                continue
            rest = np.delete(s, k)
            s1[g, d], s2[g, d] = s[k], rest.max()
            gap[g, d] = s1[g, d] - s2[g, d]
    return idx, val, gap, s1, s2


def group_sample(maps, masks, mask_a, mask_b, groups, n_groups, n_draws, beta, seed):
    """maps float32 [n_maps, hm, hm] (-inf = invalid), masks [n_masks, hm, hm], mask_a / mask_b / groups n_maps ints each ->
    (idx int64 [n_groups, n_draws], val float32 [n_groups, n_draws], gap float64 [n_groups, n_draws]): per group and draw the
    candidate with the best score as a flattened index into [n_maps, hm, hm] and the MAP value there, (-1, -inf) for a group with
    no map or no selected valid pixel; gap = the difference of the two best float32 scores of that (group, draw), inf where no
    second candidate competes."""
    return group_sample_scores(maps, masks, mask_a, mask_b, groups, n_groups, n_draws, beta, seed)[:3]


def chi_square(counts, probs):
    """Pearson's chi^2 of integer `counts` against probabilities `probs` (float64, sum 1) and its degrees of freedom: the bins are
    merged in ascending probability until each expects >= 5 (a last short bin joins the one before it)."""
    counts, probs = np.asarray(counts, dtype=np.float64), np.asarray(probs, dtype=np.float64)
    order = np.argsort(probs, kind="stable")
    exp, obs = probs[order] * counts.sum(), counts[order]
    be, bo, e_acc, o_acc = [], [], 0.0, 0.0
    for e, o in zip(exp, obs):
        e_acc += e
        o_acc += o
        if e_acc >= 5.0:
            be.append(e_acc)
            bo.append(o_acc)
            e_acc = o_acc = 0.0
    if e_acc > 0.0 or o_acc > 0.0:
        be[-1] += e_acc
        bo[-1] += o_acc
    be, bo = np.asarray(be), np.asarray(bo)
    return float(((bo - be) ** 2 / be).sum()), len(be) - 1


def chi_square_bound(df):
    """df + 4 sqrt(2 df): four standard deviations above the statistic's mean."""
    return df + 4.0 * np.sqrt(2.0 * df)
