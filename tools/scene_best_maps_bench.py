#!/usr/bin/env python3
"""Timing of smg_scene_best_maps - per object and heightmap pixel the best value over the rotations and the rotation that gives it -
against the only other device route to the same picture: smg_scene_maps into [n_maps, hm, hm], torch.where(mask != 0, maps, -inf)
and max(dim=1) over each object's rotations.

Config-5 geometry: a 640^2 heightmap (S = 1824, 38 x 38 Q maps), 8 box masks x 16 rotations = 128 maps, object-major as
Trainer.best_rotation_object_maps lays them out (map = 16 object + rotation, group = object): 128 x 640^2 fp32 = 210 MB of
scene-frame maps that the comparator writes and reads back and the fused call never forms.  Two rounds:
    on_object True   every map on its object's own pixels (the masks tensor, read before the geometry)
    on_object False  every pixel with a window, no masks tensor: every pixel pays the geometry of all 16 maps - the kernel's own
                     worst case; the comparator then needs no torch.where
The protocol is tools/scene_objects_bench.py's (bench_sides.py): events on the launch stream around a window of --calls calls
(default 20), the sides alternating inside one process, 2 warm-ups of each, 7 repeats; median and range per side, ms per call.
Sides:
    best_maps        smg_scene_best_maps (4 launches of 32 maps; the outputs carry the running best)
    maps+where+max   smg_scene_maps, torch.where(masks[object] != 0, maps, -inf) on [8, 16, hm, hm] (on_object True only), then
                     torch.max(dim=1) -> values and rotation indices [8, hm, hm] - the comparator
    argmax_objects   (on_object True, for orientation) smg_scene_argmax_objects on the same maps and masks: one pick per object
Before any time is printed the two routes are gated against each other: values bit for bit, rotations equal wherever a pixel has
a candidate, (-inf, -1) against -inf elsewhere; a mismatch ends the run.  The maps are synthetic (seeded normal): the kernels' time
does not depend on the values; the masks are the boxes of synthetic.heightmap_scene, compact as real objects are.  No ratio is
required of either side.

    python tools/scene_best_maps_bench.py [--repeats 7] [--warmup 2] > profiles/scene_best_maps.txt
"""
import argparse
import functools
import json
import sys

import numpy as np
import torch

from bench_sides import add_repo_paths, run_sides, side_stats, window

add_repo_paths()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--size", type=int, default=640, help="heightmap side (640 -> S = 1824)")
    ap.add_argument("--rotations", type=int, default=16)
    ap.add_argument("--objects", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_best_maps_bench: no GPU visible (a timing needs the MI355X)")
    import models
    import synthetic
    from trainer import Trainer

    hm, R, n = args.size, args.rotations, args.objects
    pad, S, side = Trainer._scene_geometry(hm)
    dev = torch.device("cuda:0")
    eng = models.get_engine(0, S, 1, 2, 1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n_maps = n * R
    aff = np.stack([models.rotation_theta(m % R, R) for m in range(n_maps)])
    groups, none = [m // R for m in range(n_maps)], [-1] * n_maps
    _, boxes = synthetic.heightmap_scene(8, size=hm, n_boxes=n)
    masks = torch.from_numpy(boxes).to(dev)                                  # float64 [n, hm, hm]: what the forward is given
    q = torch.from_numpy(np.random.default_rng(0).standard_normal((n_maps, side, side)).astype(np.float32)).to(dev)
    out = torch.empty((n_maps, hm, hm), dtype=torch.float32, device=dev)
    val = torch.empty((n, hm, hm), dtype=torch.float32, device=dev)
    arg = torch.empty((n, hm, hm), dtype=torch.int32, device=dev)
    idx1 = torch.empty(n, dtype=torch.int32, device=dev)
    val1 = torch.empty(n, dtype=torch.float32, device=dev)
    ninf = torch.tensor(float("-inf"), device=dev)
    keep = {}
    print("# %d^2 heightmap, S = %d, %d objects x %d rotations = %d maps of %d x %d -> [%d, %d, %d] fp32 = %.1f MB never written by `best_maps`; "
          "its outputs 2 x [%d, %d, %d] = %.1f MB; masks %.1f MB float64; %d calls between two events, ms per call"
          % (hm, S, n, R, n_maps, side, side, n_maps, hm, hm, out.numel() * 4 / 1e6, n, hm, hm, (val.numel() + arg.numel()) * 4 / 1e6,
             masks.numel() * 8 / 1e6, args.calls))

    for on_object in (True, False):
        def best_maps():
            if on_object:
                eng.scene_best_maps(q.data_ptr(), side * side, n_maps, aff, hm, masks.data_ptr(), n, groups, none, groups, n,
                                    val.data_ptr(), arg.data_ptr(), stream)
            else:
                eng.scene_best_maps(q.data_ptr(), side * side, n_maps, aff, hm, None, 0, none, none, groups, n, val.data_ptr(), arg.data_ptr(), stream)

        def maps_where_max():
            eng.scene_maps(q.data_ptr(), side * side, n_maps, aff, hm, out.data_ptr(), stream)
            sel = out.view(n, R, hm, hm)
            if on_object:
                sel = torch.where((masks != 0)[:, None], sel, ninf)
            keep["val"], keep["idx"] = sel.max(dim=1)

        def argmax_objects():
            eng.scene_argmax_objects(q.data_ptr(), side * side, n_maps, aff, hm, masks.data_ptr(), n, groups, none, groups, n,
                                     idx1.data_ptr(), val1.data_ptr(), stream)

        # the gate, before any time: the two routes give the same picture
        val.fill_(-5.0)
        arg.fill_(-5)
        best_maps()
        maps_where_max()
        v, a = val.cpu().numpy(), arg.cpu().numpy()
        cv, ci = keep["val"].cpu().numpy(), keep["idx"].cpu().numpy()
        has = a >= 0
        rot = a - (np.arange(n) * R)[:, None, None]
        gate = {"values_bit_equal": bool(np.array_equal(v.view(np.uint32), cv.view(np.uint32))),
                "indices_equal": bool(np.array_equal(rot[has], ci[has])) and bool(np.isneginf(cv[~has]).all()) and bool((a[~has] == -1).all())}
        if not all(gate.values()):
            sys.exit("scene_best_maps_bench: on_object %s: the two routes disagree: %s" % (on_object, gate))
        named = (("best_maps", best_maps), ("maps+where+max", maps_where_max)) + ((("argmax_objects", argmax_objects),) if on_object else ())
        sides = tuple((name, functools.partial(window, fn, args.calls, dev)) for name, fn in named)
        print("# on_object %s: %s" % (on_object, "every map on its object's pixels" if on_object else "every pixel with a window, no masks tensor"))
        times = run_sides(sides, args.warmup, args.repeats, 14)
        summary = {"tool": "scene_best_maps_bench", "on_object": on_object, "input_size": S, "heightmap": hm, "objects": n, "rotations": R,
                   "maps": n_maps, "map": [side, side], "repeats": args.repeats, "calls_per_window": args.calls,
                   "unwritten_mb": out.numel() * 4 / 1e6, "pixels_with_a_candidate_per_object": [int(c) for c in has.reshape(n, -1).sum(1)]}
        summary.update(gate)
        for name, _ in sides:
            summary[name + "_ms"] = side_stats(times[name], spread=True)
        a_, b_ = summary["best_maps_ms"], summary["maps+where+max_ms"]
        summary["larger_spread_ms"] = max(a_["spread"], b_["spread"])
        summary["median_difference_ms"] = b_["median"] - a_["median"]
        summary["difference_exceeds_larger_spread"] = bool(abs(b_["median"] - a_["median"]) > summary["larger_spread_ms"])
        print(json.dumps(summary))


if __name__ == "__main__":
    main()
