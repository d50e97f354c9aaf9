#!/usr/bin/env python3
"""Timing of smg_scene_topk_objects against the only other device route to the same answer: smg_scene_maps into [n_maps, hm, hm],
torch.where(mask != 0, maps, -inf), then K rounds of a max per object and a disc fill.

tools/scene_objects_bench.py's geometry and protocol: a 640^2 heightmap (S = 1824, 38 x 38 Q maps), 8 box masks x 16 rotations =
128 maps, object-major (map = 16 object + rotation, group = object); events on the launch stream around a window of --calls calls
(default 20), the sides alternating inside one process, 2 warm-ups of each, 7 repeats; median, range and spread per side, ms per
call.  One run per K (--k, default 1 4 16) at --radius 8; give each K a process and a time limit of its own:

    for k in 1 4 16; do timeout -k 10 300 python tools/scene_topk_bench.py --k $k; done > profiles/scene_topk.txt

Sides:
    topk             smg_scene_topk_objects: K rounds of (4 launches of 32 maps, each followed by the grouped reduce); a round's
                     walk reads the earlier picks from the output itself
    maps+where+topk  smg_scene_maps, torch.where(masks[object] != 0, maps, -inf) on [8, 16, hm, hm], then K times: torch.max over
                     each object's 16 x hm^2 values, the pick decoded on the device, and -inf scattered over the (2 radius + 1)^2
                     window's pixels inside the disc, in all 16 rotations - the comparator; nothing comes back to the host
                     between rounds
    argmax_objects   (K = 1 only) smg_scene_argmax_objects: what the pick test and the staging of no picks add to one round
The two routes are compared first - indices equal, values bit for bit, (-1, -inf) where the comparator's maximum is -inf - and
nothing is timed if they differ.  The maps are synthetic (seeded normal): the kernels' time does not depend on the values; the
masks are the boxes of synthetic.heightmap_scene, compact as real objects are.  No ratio is required of either side.
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
    ap.add_argument("--k", type=int, nargs="+", default=[1, 4, 16], help="ranks per object, one run each")
    ap.add_argument("--radius", type=int, default=8, help="suppression radius in heightmap pixels")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_topk_bench: no GPU visible (a timing needs the MI355X)")
    import models
    import synthetic
    from trainer import Trainer

    hm, R, n, radius = args.size, args.rotations, args.objects, args.radius
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
    # the window of a disc: offsets (dy, dx) with dy^2 + dx^2 <= radius^2
    off = torch.arange(-radius, radius + 1, device=dev)
    dy, dx = torch.meshgrid(off, off, indexing="ij")
    inside = dy * dy + dx * dx <= radius * radius
    dy, dx = dy[inside], dx[inside]                                          # [D]
    obj = torch.arange(n, device=dev)[:, None].expand(n, dy.numel())
    print("# %d^2 heightmap, S = %d, %d objects x %d rotations = %d maps of %d x %d -> [%d, %d, %d] fp32 = %.1f MB never written by `topk`; "
          "masks %.1f MB float64; radius %d (%d pixels per disc); %d calls between two events, ms per call"
          % (hm, S, n, R, n_maps, side, side, n_maps, hm, hm, out.numel() * 4 / 1e6, masks.numel() * 8 / 1e6, radius, dy.numel(), args.calls))

    for K in args.k:
        idx = torch.empty((n, K), dtype=torch.int32, device=dev)
        val = torch.empty((n, K), dtype=torch.float32, device=dev)
        idx1 = torch.empty(n, dtype=torch.int32, device=dev)
        val1 = torch.empty(n, dtype=torch.float32, device=dev)
        keep = {}

        def topk():
            eng.scene_topk_objects(q.data_ptr(), side * side, n_maps, aff, hm, masks.data_ptr(), n, mask_a, mask_b, groups, n, K, radius,
                                   idx.data_ptr(), val.data_ptr(), stream)

        def maps_where_topk():
            eng.scene_maps(q.data_ptr(), side * side, n_maps, aff, hm, out.data_ptr(), stream)
            sel = torch.where((masks != 0)[:, None], out.view(n, R, hm, hm), ninf)
            flat = sel.view(n, -1)
            vals, idxs = [], []
            for _ in range(K):
                v, i = flat.max(dim=1)
                vals.append(v)
                idxs.append(i)
                pix = i % (hm * hm)
                py, px = (pix // hm)[:, None], (pix % hm)[:, None]
                ys, xs = py + dy[None], px + dx[None]                                           # [n, D]
                ok = (ys >= 0) & (ys < hm) & (xs >= 0) & (xs < hm)                              # (outside the image: the pick itself, again)
                sel[obj, :, torch.where(ok, ys, py), torch.where(ok, xs, px)] = ninf
            keep["val"], keep["idx"] = torch.stack(vals, 1), torch.stack(idxs, 1)

        def argmax_objects():
            eng.scene_argmax_objects(q.data_ptr(), side * side, n_maps, aff, hm, masks.data_ptr(), n, mask_a, mask_b, groups, n,
                                     idx1.data_ptr(), val1.data_ptr(), stream)

        # agreement of the two routes, before anything is timed
        topk()
        maps_where_topk()
        i, v = idx.cpu().numpy().astype(np.int64), val.cpu().numpy()
        ci, cv = keep["idx"].cpu().numpy(), keep["val"].cpu().numpy()
        has = i >= 0
        base = (np.arange(n) * R * hm * hm)[:, None]
        values_bit_equal = bool(np.array_equal(v.view(np.uint32), cv.view(np.uint32)))
        indices_equal = bool(np.array_equal((i - base)[has], ci[has])) and bool(np.isneginf(cv[~has]).all())
        if not (values_bit_equal and indices_equal):
            sys.exit("scene_topk_bench: K = %d, the two routes differ (values_bit_equal %s, indices_equal %s): nothing timed"
                     % (K, values_bit_equal, indices_equal))
        names = [("topk", topk), ("maps+where+topk", maps_where_topk)] + ([("argmax_objects", argmax_objects)] if K == 1 else [])
        sides = tuple((name, functools.partial(window, fn, args.calls, dev)) for name, fn in names)
        print("# K = %d: the two routes agree (%d of %d ranks filled); timing" % (K, int(has.sum()), has.size))
        times = run_sides(sides, args.warmup, args.repeats, 15, line="K %d " % K + "repeat %d %-*s %.4f ms")
        summary = {"tool": "scene_topk_bench", "input_size": S, "heightmap": hm, "objects": n, "rotations": R, "maps": n_maps, "map": [side, side],
                   "K": K, "radius": radius, "disc_pixels": int(dy.numel()), "repeats": args.repeats, "calls_per_window": args.calls,
                   "unwritten_mb": out.numel() * 4 / 1e6, "mask_pixels_per_object": [int(c) for c in (boxes != 0).reshape(n, -1).sum(1)],
                   "ranks_filled_per_object": [int(c) for c in has.sum(1)], "values_bit_equal": values_bit_equal, "indices_equal": indices_equal}
        for name, _ in sides:
            summary[name + "_ms"] = side_stats(times[name], spread=True)
        a, b = summary["topk_ms"], summary["maps+where+topk_ms"]
        summary["larger_spread_ms"] = max(a["spread"], b["spread"])
        summary["median_difference_ms"] = b["median"] - a["median"]
        summary["difference_exceeds_larger_spread"] = bool(abs(b["median"] - a["median"]) > summary["larger_spread_ms"])
        if K == 1:
            c = summary["argmax_objects_ms"]
            summary["topk_minus_argmax_objects_ms"] = a["median"] - c["median"]
            summary["topk_minus_argmax_objects_exceeds_larger_spread"] = bool(abs(a["median"] - c["median"]) > max(a["spread"], c["spread"]))
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
