"""numpy float64 restatement of smg_loss_scene_policy's loss and dq (include/smg_hip.h), the reference of
tests/test_cpu_scene_policy.py and tests/test_gpu_scene_policy.py.  Plain helper module, no tests.

It takes the candidates' VALUES as given - `values` [n_pairs, hm, hm]: smg_scene_maps' float32 output on the GPU side,
scene_ref.scene_maps' float64 on the CPU side - with the switch `round32`: True rounds every value to float32 first (what the
device's candidates are), False keeps the unrounded double (what torch fp64 autograd differentiates).  Geometry, corners and fractions are scene_ref's
(validity is the values': -inf marks an invalid pixel), the selection is scene_objects_ref.selected, lse and mean are
scene_softmax_ref.stats_of (math.fsum).
Per group g with candidates v_i (the selected valid pixels of its pairs), action act (a flattened index into [n_pairs, hm, hm] or
-1) and weights (w_nll, w_ent):
    pi_i = exp(beta v_i - lse)          H = lse - beta mean
    loss = w_nll (lse - beta v_act) - w_ent H                 (the w_nll term is absent, and w_nll not read, when act == -1)
    g_i  = pi_i (w_nll beta + w_ent beta^2 (v_i - mean)) - w_nll beta [i == act]
    dq[j][oy][ox] = sum over the candidates i of pair j of g_i * (bilinear weight of (oy, ox) at pixel i)
A group without a candidate: loss 0 with act == -1, else NaN; its pairs' dq 0.  An action that is no candidate of its group (out of
range, in a pair of another group, unselected, invalid): loss NaN, the pi and entropy parts of dq as usual.  A NaN candidate: loss
NaN and EVERY element of the group's pairs' dq NaN."""
import numpy as np

import scene_ref
from scene_objects_ref import selected
from scene_softmax_ref import stats_of

GATE = 2.0 ** -23


def policy(values, affines, hm, masks, mask_a, mask_b, groups, n_groups, beta, actions, weights, round32=True):
    """-> dict: loss float64 [n_groups], dq float64 [n_pairs, side, side], stats float64 [n_groups, 4] = {count, vmax, lse, mean},
    vact float64 [n_groups] (NaN where there is no candidate action), scale float64 [n_groups] = |w_nll| (|lse| + beta |v_act|) +
    |w_ent| (|lse| + beta |mean|), the size of the loss's terms (0 for an empty group)."""
    values = np.asarray(values)
    n, npix = values.shape[0], hm * hm
    side = scene_ref.geometry(hm)[2]
    assert values.shape == (n, hm, hm) and len(affines) == len(mask_a) == len(mask_b) == len(groups) == n
    actions = np.asarray(actions, dtype=np.int64).reshape(n_groups)
    weights = np.asarray(weights, dtype=np.float64).reshape(n_groups, 2)
    v_all = values.astype(np.float32).astype(np.float64) if round32 else values.astype(np.float64)
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    cand, geo = [], []
    for j in range(n):
        # validity is the VALUES' (-inf = invalid), as in scene_softmax_ref.candidates: a pixel within rounding of the validity
        # boundary is whatever the producer of the values decided (at hm = 239 a whole row and column of pixels lie exactly on it in
        # rotation 0); the float64 chain here may differ on such pixels only, and their corner is then clipped into the map (their
        # fraction is within rounding of 0 or 1)
        qy, qx, valid, margin = scene_ref.map_coords(hm, affines[j], iy, ix)
        held = ~np.isneginf(values[j])
        assert (margin[valid != held] < 1e-9).all(), "the values' -inf do not mark the invalid pixels of pair %d" % j
        see = held & selected(masks, mask_a[j], mask_b[j])
        cand.append(see)
        y0, x0, _, _ = scene_ref.corners(qy[see], qx[see], side)
        y0, x0 = np.clip(y0, 0, side - 2), np.clip(x0, 0, side - 2)
        geo.append((y0, x0, qy[see] - y0, qx[see] - x0))
    dq = np.zeros((n, side, side))
    loss, stats = np.zeros(n_groups), np.zeros((n_groups, 4))
    vact, scale = np.full(n_groups, np.nan), np.zeros(n_groups)
    for g in range(n_groups):
        pairs = [j for j in range(n) if groups[j] == g]
        v = [v_all[j][cand[j]] for j in pairs]
        count, vmax, lse, mean = stats[g] = stats_of(np.concatenate(v) if v else np.zeros(0), beta)
        act = int(actions[g])
        w_nll, w_ent = (weights[g, 0] if act >= 0 else 0.0), weights[g, 1]
        if count == 0:
            loss[g] = 0.0 if act < 0 else np.nan
            continue
        if 0 <= act < n * npix and groups[act // npix] == g and cand[act // npix].ravel()[act % npix]:
            vact[g] = v_all[act // npix].ravel()[act % npix]
        if np.isnan(lse):
            loss[g] = np.nan
            for j in pairs:
                dq[j] = np.nan
            continue
        loss[g] = -w_ent * (lse - beta * mean) + (w_nll * (lse - beta * vact[g]) if act >= 0 else 0.0)
        scale[g] = abs(w_nll) * (abs(lse) + beta * (abs(vact[g]) if act >= 0 and not np.isnan(vact[g]) else 0.0)) + abs(w_ent) * (abs(lse) + beta * abs(mean))
        for j, vj in zip(pairs, v):
            gi = np.exp(beta * vj - lse) * (w_nll * beta + w_ent * beta * beta * (vj - mean))
            if act >= 0 and act // npix == j and not np.isnan(vact[g]):
                gi[np.flatnonzero(np.flatnonzero(cand[j].ravel()) == act % npix)] -= w_nll * beta
            y0, x0, fy, fx = geo[j]
            for dy, dx, w in ((0, 0, (1 - fy) * (1 - fx)), (0, 1, (1 - fy) * fx), (1, 0, fy * (1 - fx)), (1, 1, fy * fx)):
                np.add.at(dq[j], (y0 + dy, x0 + dx), gi * w)
    return dict(loss=loss, dq=dq, stats=stats, vact=vact, scale=scale)


def torch_policy(q, affines, hm, masks, mask_a, mask_b, groups, n_groups, beta, actions, weights):
    """The same loss by torch fp64 autograd: q float64 [n_pairs, side, side]; per group w_nll (logsumexp(beta v) - beta v_act) -
    w_ent H over scene_ref.scene_points of the selected valid pixels, H = logsumexp(beta v) - beta sum softmax(beta v) v.  Every
    action must be a candidate.  -> (loss float64 [n_groups], dq float64 [n_pairs, side, side])."""
    import torch
    n, npix = len(affines), hm * hm
    qt = torch.tensor(np.asarray(q, dtype=np.float64), requires_grad=True)
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    losses = []
    for g in range(n_groups):
        vs, at = [], []
        for j in range(n):
            if groups[j] != g:
                continue
            see = scene_ref.map_coords(hm, affines[j], iy, ix)[2] & selected(masks, mask_a[j], mask_b[j])
            pix = np.stack([iy[see], ix[see]], axis=-1)
            vs.append(scene_ref.scene_points(qt[j], affines[j], hm, pix))
            at.append(j * npix + pix[:, 0] * hm + pix[:, 1])
        if not vs or not sum(len(a) for a in at):
            assert actions[g] < 0
            losses.append(torch.zeros((), dtype=torch.float64))
            continue
        v, at = torch.cat(vs), np.concatenate(at)
        lse = torch.logsumexp(beta * v, 0)
        H = lse - beta * (torch.softmax(beta * v, 0) * v).sum()
        loss = -weights[g][1] * H
        if actions[g] >= 0:
            k = np.flatnonzero(at == actions[g])
            assert len(k) == 1, "torch_policy: the action of group %d is no candidate" % g
            loss = loss + weights[g][0] * (lse - beta * v[int(k[0])])
        losses.append(loss)
    total = torch.stack(losses)
    total.sum().backward()
    return total.detach().numpy(), qt.grad.numpy()


def gate_ratios(loss, dq, ref):
    """Device loss [n_groups] and dq [n_pairs, side, side] against policy()'s dict -> (largest loss ratio, largest dq ratio) =
    |got - ref| / gate after the exact parts: NaN exactly where the reference has NaN; a pair whose reference dq is all zero exactly
    zero; a group whose terms have size 0 exactly the reference.  The gates: dq per pair 2^-23 max|reference dq of that pair|,
    loss per group 2^-23 scale.  A ratio <= 1 passes."""
    loss, dq = np.asarray(loss, dtype=np.float64), np.asarray(dq, dtype=np.float64)
    assert loss.shape == ref["loss"].shape and dq.shape == ref["dq"].shape, (loss.shape, dq.shape)
    worst_l = worst_d = 0.0
    for g in range(len(loss)):
        if np.isnan(ref["loss"][g]):
            assert np.isnan(loss[g]), ("loss", g, loss[g])
        elif ref["scale"][g] == 0:
            assert loss[g] == ref["loss"][g], ("loss", g, loss[g], ref["loss"][g])
        else:
            assert np.isfinite(loss[g]), ("loss", g, loss[g])
            worst_l = max(worst_l, abs(loss[g] - ref["loss"][g]) / (GATE * ref["scale"][g]))
    for j in range(len(dq)):
        r = ref["dq"][j]
        if np.isnan(r).any():
            assert np.isnan(r).all() and np.isnan(dq[j]).all(), ("dq", j)
            continue
        top = np.abs(r).max()
        if top == 0:
            assert (dq[j] == 0).all(), ("dq", j, dq[j])
        else:
            assert np.isfinite(dq[j]).all(), ("dq", j)
            worst_d = max(worst_d, np.abs(dq[j] - r).max() / (GATE * top))
    return worst_l, worst_d
