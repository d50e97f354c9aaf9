#!/usr/bin/env python3
"""Timing of smg_loss_scene_policy - loss and dq of the Boltzmann policy's log-likelihood and entropy per object - against the only
other device route to the same gradient: F.grid_sample with a prebuilt grid into [n_maps, hm, hm], torch.where, torch.logsumexp and
the loss in float64, then torch.autograd.grad back to q (grid_sample's backward scatters with floating-point atomics).

tools/scene_softmax_bench.py's geometry and protocol: a 640^2 heightmap (S = 1824, 38 x 38 Q maps), 8 box masks x 16 rotations =
128 pairs, object-major (pair = 16 object + rotation, group = object), --beta 3, one action per object (its best candidate,
found by smg_scene_argmax_objects), weights w_nll = 1, w_ent = 0.1; events on the launch stream around a window of --calls calls
(default 20), the sides alternating inside one process, 2 warm-ups of each, 7 repeats; median, range and spread per side, ms per call:

    timeout -k 10 300 python tools/scene_policy_bench.py > profiles/scene_policy.txt

Sides:
    policy             smg_loss_scene_policy: the normaliser (4 launches of 32 pairs + grouped reduces + finish), the gather per
                       (pair, map element), the losses
    grid_sample+grad   q.double() -> F.grid_sample(align_corners=True) on a prebuilt float64 grid [n_maps, hm, hm, 2] -> rounded to
                       float32 with a straight-through gradient (the header's "the rounding of v is the identity in the gradient") ->
                       torch.where(selected and valid, ., -inf) -> logsumexp, mean, entropy and loss in float64 ->
                       torch.autograd.grad(loss.sum(), q)
    softmax_objects    smg_scene_softmax_objects alone: `policy` minus this is the price of the gather and the losses
The gate before any time is printed: the two routes' dq against each other per pair at the GPU tests' gate, 2^-23 of the largest
|dq| of that pair, the losses at 2^-23 of their terms, and the fused call against tests/scene_policy_ref.py's restatement on
smg_scene_maps' own output; nothing is timed if it fails.  The maps are synthetic (seeded normal); the masks are the boxes of
synthetic.heightmap_scene, compact as real objects are.  No ratio is required of either side.
"""
import argparse
import functools
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from bench_sides import add_repo_paths, run_sides, side_stats, window

add_repo_paths()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--size", type=int, default=640, help="heightmap side (640 -> S = 1824)")
    ap.add_argument("--rotations", type=int, default=16)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--beta", type=float, default=3.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_policy_bench: no GPU visible (a timing needs the MI355X)")
    import models
    import scene_policy_ref
    import scene_ref
    import synthetic
    from trainer import Trainer

    hm, R, n, beta = args.size, args.rotations, args.objects, args.beta
    pad, S, side = Trainer._scene_geometry(hm)
    dev = torch.device("cuda:0")
    eng = models.get_engine(0, S, 1, 2, 1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n_maps = n * R
    aff = np.stack([models.rotation_theta(m % R, R) for m in range(n_maps)])
    mask_a, mask_b, groups = [m // R for m in range(n_maps)], [-1] * n_maps, [m // R for m in range(n_maps)]
    _, boxes = synthetic.heightmap_scene(8, size=hm, n_boxes=n)
    masks = torch.from_numpy(boxes).to(dev)                                  # float64 [n, hm, hm]: what the forward is given
    q = torch.from_numpy(np.random.default_rng(0).standard_normal((n_maps, 1, side, side)).astype(np.float32)).to(dev)
    weights_h = np.tile(np.asarray([[1.0, 0.1]]), (n, 1))
    weights = torch.from_numpy(weights_h).to(dev)
    rows = torch.empty((n, 4), dtype=torch.float64, device=dev)
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    dq = torch.empty_like(q)
    # one action per object: its best candidate
    act = torch.empty(n, dtype=torch.int32, device=dev)
    val = torch.empty(n, dtype=torch.float32, device=dev)
    eng.scene_argmax_objects(q.data_ptr(), side * side, n_maps, aff, hm, masks.data_ptr(), n, mask_a, mask_b, groups, n, act.data_ptr(), val.data_ptr(), stream)
    actions_h = act.cpu().numpy()
    if (actions_h < 0).any():
        sys.exit("scene_policy_bench: an object without a candidate")
    # the comparator's prebuilt inputs: the grid of every pair in grid_sample's normalised coordinates, float64, and which pixels are
    # candidates - selected by the object's mask and valid in the pair's rotation (validity as smg_scene_maps decides it)
    out = torch.empty((n_maps, hm, hm), dtype=torch.float32, device=dev)
    eng.scene_maps(q.data_ptr(), side * side, n_maps, aff, hm, out.data_ptr(), stream)
    maps_host = out.cpu().numpy()
    cand = (~torch.isinf(out)).view(n, R, hm, hm) & (masks != 0)[:, None]
    del out
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    grid_h = np.empty((n_maps, hm, hm, 2))
    for m in range(R):                                                      # (pair 16 k + r has rotation r)
        qy, qx, _, _ = scene_ref.map_coords(hm, aff[m], iy, ix)
        grid_h[m::R, ..., 0] = 2.0 * qx / (side - 1) - 1.0
        grid_h[m::R, ..., 1] = 2.0 * qy / (side - 1) - 1.0
    grid = torch.from_numpy(grid_h).to(dev)
    del grid_h
    act_long = act.long()
    zero, ninf = torch.zeros((), dtype=torch.float64, device=dev), torch.tensor(float("-inf"), dtype=torch.float64, device=dev)
    keep = {}
    print("# %d^2 heightmap, S = %d, %d objects x %d rotations = %d pairs of %d x %d; [%d, %d, %d] fp32 = %.1f MB never written by `policy` "
          "(the comparator holds them in float64, %.1f MB, beside a %.1f MB grid); masks %.1f MB float64; beta %g; %d calls between two events, ms per call"
          % (hm, S, n, R, n_maps, side, side, n_maps, hm, hm, n_maps * hm * hm * 4 / 1e6, n_maps * hm * hm * 8 / 1e6, grid.numel() * 8 / 1e6,
             masks.numel() * 8 / 1e6, beta, args.calls))

    def policy():
        eng.loss_scene_policy(q.data_ptr(), aff, hm, n_maps, masks.data_ptr(), n, mask_a, mask_b, groups, n, beta, act.data_ptr(),
                              weights.data_ptr(), rows.data_ptr(), loss.data_ptr(), dq.data_ptr(), stream)

    def grid_sample_grad():
        ql = q.detach().requires_grad_(True)
        v = F.grid_sample(ql.double(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        v = v + (v.float().double() - v).detach()                           # the float32 value, the gradient of the unrounded one
        vg = v.view(n, R, hm, hm)
        z = torch.where(cand, beta * vg, ninf).view(n, -1)
        lse = torch.logsumexp(z, dim=1)
        p = torch.exp(z - lse[:, None])
        mean = (p * torch.where(cand, vg, zero).view(n, -1)).sum(dim=1)
        total = weights[:, 0] * (lse - beta * v.view(-1)[act_long]) - weights[:, 1] * (lse - beta * mean)
        keep["loss"], keep["dq"] = total.detach(), torch.autograd.grad(total.sum(), ql)[0]

    def softmax_objects():
        eng.scene_softmax_objects(q.data_ptr(), side * side, n_maps, aff, hm, masks.data_ptr(), n, mask_a, mask_b, groups, n, beta,
                                  rows.data_ptr(), stream)

    # the gate: the two routes against each other and the fused call against the restatement, before anything is timed
    loss.fill_(-7.0)
    dq.fill_(-7.0)
    policy()
    got_loss, got_dq = loss.cpu().numpy().astype(np.float64), dq.cpu().numpy()[:, 0].astype(np.float64)
    grid_sample_grad()
    cmp_loss, cmp_dq = keep["loss"].cpu().numpy(), keep["dq"].cpu().numpy()[:, 0].astype(np.float64)
    want = scene_policy_ref.policy(maps_host, aff, hm, boxes, mask_a, mask_b, groups, n, beta, actions_h, weights_h)
    ratios = {}
    for name, other in (("comparator", dict(want, loss=cmp_loss, dq=cmp_dq)), ("restatement", want)):
        try:
            ratios[name] = [float(r) for r in scene_policy_ref.gate_ratios(got_loss, got_dq, other)]
        except AssertionError as err:
            sys.exit("scene_policy_bench: the fused call differs from the %s (%s): nothing timed" % (name, err))
    if max(ratios["comparator"] + ratios["restatement"]) > 1.0:
        sys.exit("scene_policy_bench: the two routes differ by more than the gate (error / gate, loss and dq: %s): nothing timed" % ratios)
    names = [("policy", policy), ("grid_sample+grad", grid_sample_grad), ("softmax_objects", softmax_objects)]
    sides = tuple((name, functools.partial(window, fn, args.calls, dev)) for name, fn in names)
    print("# the fused call is within the gate of the comparator and of the restatement (largest error / gate, loss and dq: %s); timing" % ratios)
    times = run_sides(sides, args.warmup, args.repeats, 17, line="repeat %d %-*s %.4f ms")
    summary = {"tool": "scene_policy_bench", "input_size": S, "heightmap": hm, "objects": n, "rotations": R, "pairs": n_maps, "map": [side, side],
               "beta": beta, "weights": [1.0, 0.1], "repeats": args.repeats, "calls_per_window": args.calls,
               "unwritten_mb": n_maps * hm * hm * 4 / 1e6, "candidates_per_object": [int(c) for c in want["stats"][:, 0]], "error_over_gate": ratios}
    for name, _ in sides:
        summary[name + "_ms"] = side_stats(times[name], spread=True)
    a, b, c = (summary[k + "_ms"] for k in ("policy", "grid_sample+grad", "softmax_objects"))
    summary["larger_spread_ms"] = max(a["spread"], b["spread"])
    summary["median_difference_ms"] = b["median"] - a["median"]
    summary["faster_side"] = "policy" if a["median"] < b["median"] else "grid_sample+grad"
    summary["difference_exceeds_larger_spread"] = bool(abs(b["median"] - a["median"]) > summary["larger_spread_ms"])
    summary["policy_minus_softmax_objects_ms"] = a["median"] - c["median"]
    summary["policy_minus_softmax_objects_exceeds_larger_spread"] = bool(abs(a["median"] - c["median"]) > max(a["spread"], c["spread"]))
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
