#!/usr/bin/env python3
"""Timing of smg_scene_class_argmax_objects against the only other device route to the same answer: smg_scene_class_maps(cls = 0)
into [n_maps, hm, hm], torch.where(mask != 0, maps, -inf) and an argmax per object.  tools/scene_objects_bench.py's twin for the
reactive net's three logit planes.

Config-5 geometry: a 640^2 heightmap (S = 1824, 38 x 38 logit maps in 3 planes), 8 box masks x 16 rotations = 128 maps,
object-major as Trainer.best_scene_class_actions lays them out (map = 16 object + rotation, group = object): 128 x 640^2 fp32 =
210 MB of scene-frame P(class 0) that the comparator writes and reads back and the fused call never forms.  The protocol is
tools/scene_objects_bench.py's: events on the launch stream around a window of --calls calls (default 20), the sides alternating
inside one process, 2 warm-ups of each, 7 repeats; median and range per side, ms per call.  Sides:
    class_objects         smg_scene_class_argmax_objects (4 launches of 32 maps, each followed by the grouped reduce); a selected
                          valid pixel pays the three interpolations and three double exponentials, every other pixel its mask load
    class_maps+where+max  smg_scene_class_maps(cls 0), torch.where(masks[object] != 0, maps, -inf) on [8, 16, hm, hm], then max and
                          argmax over each object's 16 x hm^2 values (torch.max(dim=1) on [8, 16 hm^2]) - the comparator
The logits are synthetic (seeded normal): the kernels' time does not depend on the values; the masks are the boxes of
synthetic.heightmap_scene, compact as real objects are.  Before any time is printed the two routes must agree - values bit for bit,
indices equal - or the tool exits.  No ratio is required of either side.

    python tools/scene_class_objects_bench.py [--repeats 7] [--warmup 2] > profiles/scene_class_objects.txt
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
    ap.add_argument("--cls", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_class_objects_bench: no GPU visible (a timing needs the MI355X)")
    import models
    import synthetic
    from trainer import Trainer

    hm, R, n, cls = args.size, args.rotations, args.objects, args.cls
    pad, S, side = Trainer._scene_geometry(hm)
    dev = torch.device("cuda:0")
    eng = models.get_engine(0, S, 3, 2, 1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n_maps = n * R
    aff = np.stack([models.rotation_theta(m % R, R) for m in range(n_maps)])
    mask_a, mask_b, groups = [m // R for m in range(n_maps)], [-1] * n_maps, [m // R for m in range(n_maps)]
    _, boxes = synthetic.heightmap_scene(8, size=hm, n_boxes=n)
    masks = torch.from_numpy(boxes).to(dev)                                  # float64 [n, hm, hm]: what the forward is given
    q = torch.from_numpy(np.random.default_rng(0).standard_normal((n_maps, 3, side, side)).astype(np.float32)).to(dev)
    out = torch.empty((n_maps, hm, hm), dtype=torch.float32, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    val = torch.empty(n, dtype=torch.float32, device=dev)
    ninf = torch.tensor(float("-inf"), device=dev)
    keep = {}

    def class_objects():
        eng.scene_class_argmax_objects(q.data_ptr(), n_maps, aff, hm, cls, masks.data_ptr(), n, mask_a, mask_b, groups, n,
                                       idx.data_ptr(), val.data_ptr(), stream)

    def class_maps_where_max():
        eng.scene_class_maps(q.data_ptr(), n_maps, aff, hm, cls, out.data_ptr(), stream)
        sel = torch.where((masks != 0)[:, None], out.view(n, R, hm, hm), ninf)
        keep["val"], keep["idx"] = sel.view(n, -1).max(dim=1)

    # the gate: the two routes agree - a value bit for bit wherever an object has a pixel, (-1, -inf) against -inf elsewhere
    class_objects()
    class_maps_where_max()
    i, v = idx.cpu().numpy(), val.cpu().numpy()
    ci, cv = keep["idx"].cpu().numpy(), keep["val"].cpu().numpy()
    has = i >= 0
    values_bit_equal = bool(np.array_equal(v.view(np.uint32), cv.view(np.uint32)))
    indices_equal = bool(np.array_equal(i[has] - np.arange(n)[has] * R * hm * hm, ci[has])) and bool(np.isneginf(cv[~has]).all())
    if not (values_bit_equal and indices_equal):
        sys.exit("scene_class_objects_bench: the two routes disagree (values bit-equal: %s, indices equal: %s); fused %s %s, comparator %s %s"
                 % (values_bit_equal, indices_equal, i.tolist(), v.tolist(), ci.tolist(), cv.tolist()))

    sides = tuple((name, functools.partial(window, fn, args.calls, dev)) for name, fn in (
        ("class_objects", class_objects), ("class_maps+where+max", class_maps_where_max)))
    print("# %d^2 heightmap, S = %d, %d objects x %d rotations = %d maps of 3 x %d x %d logits, cls %d -> [%d, %d, %d] fp32 = %.1f MB never "
          "written by `class_objects`; masks %.1f MB float64; %d calls between two events, ms per call"
          % (hm, S, n, R, n_maps, side, side, cls, n_maps, hm, hm, out.numel() * 4 / 1e6, masks.numel() * 8 / 1e6, args.calls))
    times = run_sides(sides, args.warmup, args.repeats, 20)
    summary = {"tool": "scene_class_objects_bench", "input_size": S, "heightmap": hm, "objects": n, "rotations": R, "maps": n_maps,
               "map": [3, side, side], "cls": cls, "repeats": args.repeats, "calls_per_window": args.calls, "unwritten_mb": out.numel() * 4 / 1e6,
               "mask_pixels_per_object": [int(c) for c in (boxes != 0).reshape(n, -1).sum(1)],
               "objects_with_a_pixel": int(has.sum()), "values_bit_equal": values_bit_equal, "indices_equal": indices_equal}
    for name, _ in sides:
        summary[name + "_ms"] = side_stats(times[name], spread=True)
    a, b = summary["class_objects_ms"], summary["class_maps+where+max_ms"]
    summary["larger_spread_ms"] = max(a["spread"], b["spread"])
    summary["median_difference_ms"] = b["median"] - a["median"]
    summary["difference_exceeds_larger_spread"] = bool(abs(b["median"] - a["median"]) > summary["larger_spread_ms"])
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
