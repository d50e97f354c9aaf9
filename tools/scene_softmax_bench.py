#!/usr/bin/env python3
"""Timing of smg_scene_softmax_objects against the only other device route to the normaliser of the Boltzmann policy per object:
smg_scene_maps into [n_maps, hm, hm], torch.where(mask != 0, maps, -inf), then torch.logsumexp and the weighted mean per object.

tools/scene_sample_bench.py's geometry and protocol: a 640^2 heightmap (S = 1824, 38 x 38 Q maps), 8 box masks x 16 rotations =
128 maps, object-major (map = 16 object + rotation, group = object), --beta 3; events on the launch stream around a window of
--calls calls (default 20), the sides alternating inside one process, 2 warm-ups of each, 7 repeats; median, range and spread per
side, ms per call:

    timeout -k 10 300 python tools/scene_softmax_bench.py > profiles/scene_softmax.txt

Sides:
    softmax            smg_scene_softmax_objects: 4 launches of 32 maps, each followed by the grouped reduce, and the finish; a
                       candidate pays the geometry, the interpolation and one double exponential
    maps+logsumexp64   smg_scene_maps, torch.where(masks[object] != 0, maps, -inf) on [8, 16 hm^2], then in FLOAT64: z = beta v,
                       lse = torch.logsumexp(z), p = exp(z - lse), mean = sum(p v) with the -inf entries' products set to 0, count
                       and max - the comparator of equal accuracy
    maps+logsumexp32   the same in float32, for information: its lse is good to a float32 rounding, 4000 gates
    argmax_objects     smg_scene_argmax_objects: the same walk without the exponential; `softmax` minus this prices it
The gate before anything is timed: the fused call against the float64 comparator - count and vmax equal, lse and mean within the
gate of tests/scene_softmax_ref.py - and against that module's restatement on smg_scene_maps' own output; nothing is timed if it
fails.  The maps are synthetic (seeded normal); the masks are the boxes of synthetic.heightmap_scene, compact as real objects are.
No ratio is required of either side.
"""
import argparse
import functools
import json
import os
import sys

import numpy as np
import torch

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
        sys.exit("scene_softmax_bench: no GPU visible (a timing needs the MI355X)")
    import models
    import scene_softmax_ref
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
    q = torch.from_numpy(np.random.default_rng(0).standard_normal((n_maps, side, side)).astype(np.float32)).to(dev)
    out = torch.empty((n_maps, hm, hm), dtype=torch.float32, device=dev)
    ninf = torch.tensor(float("-inf"), device=dev)
    rows = torch.empty((n, 4), dtype=torch.float64, device=dev)
    idx1 = torch.empty(n, dtype=torch.int32, device=dev)
    val1 = torch.empty(n, dtype=torch.float32, device=dev)
    keep = {}
    print("# %d^2 heightmap, S = %d, %d objects x %d rotations = %d maps of %d x %d -> [%d, %d, %d] fp32 = %.1f MB never written by `softmax`; "
          "masks %.1f MB float64; beta %g; %d calls between two events, ms per call"
          % (hm, S, n, R, n_maps, side, side, n_maps, hm, hm, out.numel() * 4 / 1e6, masks.numel() * 8 / 1e6, beta, args.calls))

    def softmax():
        eng.scene_softmax_objects(q.data_ptr(), side * side, n_maps, aff, hm, masks.data_ptr(), n, mask_a, mask_b, groups, n, beta,
                                  rows.data_ptr(), stream)

    def maps_logsumexp(dtype, key):
        eng.scene_maps(q.data_ptr(), side * side, n_maps, aff, hm, out.data_ptr(), stream)
        v = torch.where((masks != 0)[:, None], out.view(n, R, hm, hm), ninf).view(n, -1).to(dtype)
        have = v != ninf
        z = beta * v
        lse = torch.logsumexp(z, dim=1)
        p = torch.exp(z - lse[:, None])
        mean = torch.where(have, p * v, torch.zeros((), dtype=dtype, device=dev)).sum(dim=1)
        keep[key] = torch.stack([have.sum(dim=1).to(dtype), v.max(dim=1).values, lse, mean], dim=1)

    def argmax_objects():
        eng.scene_argmax_objects(q.data_ptr(), side * side, n_maps, aff, hm, masks.data_ptr(), n, mask_a, mask_b, groups, n,
                                 idx1.data_ptr(), val1.data_ptr(), stream)

    # the gate: the fused call against the float64 comparator and against the restatement, before anything is timed
    rows.fill_(-5.0)
    softmax()
    got = rows.cpu().numpy()
    maps_logsumexp(torch.float64, "fp64")
    maps_logsumexp(torch.float32, "fp32")
    cmp64, cmp32 = keep["fp64"].cpu().numpy(), keep["fp32"].cpu().numpy().astype(np.float64)
    maps_host = out.cpu().numpy()
    want = scene_softmax_ref.group_stats(maps_host, boxes, mask_a, mask_b, groups, n, beta)
    ratios = {"comparator": [0.0, 0.0], "restatement": [0.0, 0.0], "fp32_comparator": [0.0, 0.0]}
    for g in range(n):
        v = scene_softmax_ref.candidates(maps_host, boxes, mask_a, mask_b, groups, g)
        vabs = float(np.abs(v).max()) if v.size else 0.0
        for name, other in (("comparator", cmp64), ("restatement", want)):
            try:
                r = scene_softmax_ref.gate_ratios(got[g], other[g], vabs)
            except AssertionError as err:
                sys.exit("scene_softmax_bench: object %d, the fused call differs from the %s (%s): nothing timed" % (g, name, err))
            ratios[name] = [max(a, b) for a, b in zip(ratios[name], r)]
        if want[g, 0] > 0:
            r32 = (abs(cmp32[g, 2] - want[g, 2]) / scene_softmax_ref.lse_gate(want[g, 2]), abs(cmp32[g, 3] - want[g, 3]) / scene_softmax_ref.mean_gate(vabs))
            ratios["fp32_comparator"] = [max(a, b) for a, b in zip(ratios["fp32_comparator"], r32)]
    if max(ratios["comparator"] + ratios["restatement"]) > 1.0:
        sys.exit("scene_softmax_bench: the fused call misses the gate (error / gate %s): nothing timed" % ratios)
    names = [("softmax", softmax), ("maps+logsumexp64", functools.partial(maps_logsumexp, torch.float64, "fp64")),
             ("maps+logsumexp32", functools.partial(maps_logsumexp, torch.float32, "fp32")), ("argmax_objects", argmax_objects)]
    sides = tuple((name, functools.partial(window, fn, args.calls, dev)) for name, fn in names)
    print("# the fused call is within the gate of the float64 comparator and of the restatement (largest error / gate, lse and mean: %s); timing" % ratios)
    times = run_sides(sides, args.warmup, args.repeats, 17, line="repeat %d %-*s %.4f ms")
    summary = {"tool": "scene_softmax_bench", "input_size": S, "heightmap": hm, "objects": n, "rotations": R, "maps": n_maps, "map": [side, side],
               "beta": beta, "repeats": args.repeats, "calls_per_window": args.calls, "unwritten_mb": out.numel() * 4 / 1e6,
               "mask_pixels_per_object": [int(c) for c in (boxes != 0).reshape(n, -1).sum(1)], "candidates_per_object": [int(c) for c in got[:, 0]],
               "error_over_gate": ratios}
    for name, _ in sides:
        summary[name + "_ms"] = side_stats(times[name], spread=True)
    a, b, b32, c = (summary[k + "_ms"] for k in ("softmax", "maps+logsumexp64", "maps+logsumexp32", "argmax_objects"))
    summary["larger_spread_ms"] = max(a["spread"], b["spread"])
    summary["median_difference_ms"] = b["median"] - a["median"]
    summary["faster_side"] = "softmax" if a["median"] < b["median"] else "maps+logsumexp64"
    summary["difference_exceeds_larger_spread"] = bool(abs(b["median"] - a["median"]) > summary["larger_spread_ms"])
    summary["fp32_median_difference_ms"] = b32["median"] - a["median"]
    summary["fp32_difference_exceeds_larger_spread"] = bool(abs(b32["median"] - a["median"]) > max(a["spread"], b32["spread"]))
    summary["softmax_minus_argmax_objects_ms"] = a["median"] - c["median"]
    summary["softmax_minus_argmax_objects_exceeds_larger_spread"] = bool(abs(a["median"] - c["median"]) > max(a["spread"], c["spread"]))
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
