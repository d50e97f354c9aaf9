#!/usr/bin/env python3
"""Timing of smg_scene_sample_objects against the only other device route to a Boltzmann draw per object: smg_scene_maps into
[n_maps, hm, hm], torch.where(mask != 0, maps, -inf), then per draw beta * maps - log(-log(rand)) from torch's generator and a max
per object.

tools/scene_topk_bench.py's geometry and protocol: a 640^2 heightmap (S = 1824, 38 x 38 Q maps), 8 box masks x 16 rotations =
128 maps, object-major (map = 16 object + rotation, group = object); events on the launch stream around a window of --calls calls
(default 20), the sides alternating inside one process, 2 warm-ups of each, 7 repeats; median, range and spread per side, ms per
call.  One run per n_draws (--draws, default 1 4 16) at --beta 3; give each a process and a time limit of its own:

    for k in 1 4 16; do timeout -k 10 300 python tools/scene_sample_bench.py --draws $k; done > profiles/scene_sample.txt

Sides:
    sample           smg_scene_sample_objects: n_draws rounds of (4 launches of 32 maps, each followed by the grouped reduce); a
                     candidate pays the geometry, the interpolation, a 64-bit hash and two double logarithms per round
    maps+where+gumbel  smg_scene_maps, torch.where(masks[object] != 0, maps, -inf) on [8, 16, hm, hm], then n_draws times:
                     torch.rand of that shape, beta * maps - log(-log(u)) and torch.max over each object's 16 x hm^2 scores - the
                     comparator; nothing comes back to the host between draws
    argmax_objects   smg_scene_argmax_objects: the same walk without the noise; `sample` at n_draws = 1 minus this is what the
                     hash and the logarithms cost
The comparator draws OTHER noise, so the two routes cannot be compared pick by pick.  The gate before anything is timed is the
fused call against tests/scene_sample_ref.py's group_sample on smg_scene_maps' own output (index equal wherever that module's rule
compares a draw, the value bit for bit the map at the pick); nothing is timed if it fails.  The maps are synthetic (seeded normal);
the masks are the boxes of synthetic.heightmap_scene, compact as real objects are.  No ratio is required of either side.
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
    ap.add_argument("--draws", type=int, nargs="+", default=[1, 4, 16], help="draws per object, one run each")
    ap.add_argument("--beta", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_sample_bench: no GPU visible (a timing needs the MI355X)")
    import models
    import scene_sample_ref
    import synthetic
    from trainer import Trainer

    hm, R, n, beta, seed = args.size, args.rotations, args.objects, args.beta, args.seed
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
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    print("# %d^2 heightmap, S = %d, %d objects x %d rotations = %d maps of %d x %d -> [%d, %d, %d] fp32 = %.1f MB never written by `sample`; "
          "masks %.1f MB float64; beta %g; %d calls between two events, ms per call"
          % (hm, S, n, R, n_maps, side, side, n_maps, hm, hm, out.numel() * 4 / 1e6, masks.numel() * 8 / 1e6, beta, args.calls))
    eng.scene_maps(q.data_ptr(), side * side, n_maps, aff, hm, out.data_ptr(), stream)
    maps_host = out.cpu().numpy()

    for K in args.draws:
        idx = torch.empty((n, K), dtype=torch.int32, device=dev)
        val = torch.empty((n, K), dtype=torch.float32, device=dev)
        idx1 = torch.empty(n, dtype=torch.int32, device=dev)
        val1 = torch.empty(n, dtype=torch.float32, device=dev)
        keep = {}

        def sample():
            eng.scene_sample_objects(q.data_ptr(), side * side, n_maps, aff, hm, masks.data_ptr(), n, mask_a, mask_b, groups, n, K, beta, seed,
                                     idx.data_ptr(), val.data_ptr(), stream)

        def maps_where_gumbel():
            eng.scene_maps(q.data_ptr(), side * side, n_maps, aff, hm, out.data_ptr(), stream)
            sel = torch.where((masks != 0)[:, None], out.view(n, R, hm, hm), ninf)
            flat = sel.view(n, -1)
            vals, idxs = [], []
            for _ in range(K):
                u = torch.rand(flat.shape, device=dev, generator=gen)
                score = beta * flat - torch.log(-torch.log(u))
                i = score.argmax(dim=1)
                idxs.append(i)
                vals.append(flat.gather(1, i[:, None])[:, 0])
            keep["val"], keep["idx"] = torch.stack(vals, 1), torch.stack(idxs, 1)

        def argmax_objects():
            eng.scene_argmax_objects(q.data_ptr(), side * side, n_maps, aff, hm, masks.data_ptr(), n, mask_a, mask_b, groups, n,
                                     idx1.data_ptr(), val1.data_ptr(), stream)

        # the gate: the fused call against the numpy restatement on the kernel's own maps, before anything is timed
        idx.fill_(-5)
        val.fill_(-5.0)
        sample()
        i, v = idx.cpu().numpy().astype(np.int64), val.cpu().numpy()
        ref_i, ref_v, gap, s1, s2 = scene_sample_ref.group_sample_scores(maps_host, boxes, mask_a, mask_b, groups, n, K, beta, seed)
        cmp = scene_sample_ref.compared(gap, s1, s2)
        has = i >= 0
        indices_equal = bool(np.array_equal(i[cmp], ref_i[cmp])) and bool(np.array_equal(has, ref_i >= 0))
        values_bit_equal = bool(np.array_equal(v[has].view(np.uint32), maps_host.ravel()[i[has]].view(np.uint32))) and bool(np.isneginf(v[~has]).all())
        skipped = int((~cmp).sum())
        if not (indices_equal and values_bit_equal and skipped * 1000 <= cmp.size):
            sys.exit("scene_sample_bench: n_draws = %d, the fused call differs from the restatement (indices_equal %s, values_bit_equal %s, "
                     "%d of %d draws not compared): nothing timed" % (K, indices_equal, values_bit_equal, skipped, cmp.size))
        maps_where_gumbel()
        ci = keep["idx"].cpu().numpy()
        comparator_inside = bool(((boxes.reshape(n, -1)[np.arange(n)[:, None], ci % (hm * hm)] != 0) | ~has).all())
        if not comparator_inside:
            sys.exit("scene_sample_bench: n_draws = %d, the comparator drew a pixel outside its object: nothing timed" % K)
        names = [("sample", sample), ("maps+where+gumbel", maps_where_gumbel), ("argmax_objects", argmax_objects)]
        sides = tuple((name, functools.partial(window, fn, args.calls, dev)) for name, fn in names)
        print("# n_draws = %d: the fused call equals the restatement (%d of %d draws filled, %d not compared); timing" % (K, int(has.sum()), has.size, skipped))
        times = run_sides(sides, args.warmup, args.repeats, 17, line="n_draws %d " % K + "repeat %d %-*s %.4f ms")
        summary = {"tool": "scene_sample_bench", "input_size": S, "heightmap": hm, "objects": n, "rotations": R, "maps": n_maps, "map": [side, side],
                   "n_draws": K, "beta": beta, "seed": seed, "repeats": args.repeats, "calls_per_window": args.calls,
                   "unwritten_mb": out.numel() * 4 / 1e6, "mask_pixels_per_object": [int(c) for c in (boxes != 0).reshape(n, -1).sum(1)],
                   "draws_filled_per_object": [int(c) for c in has.sum(1)], "draws_not_compared": skipped,
                   "values_bit_equal": values_bit_equal, "indices_equal": indices_equal}
        for name, _ in sides:
            summary[name + "_ms"] = side_stats(times[name], spread=True)
        a, b, c = summary["sample_ms"], summary["maps+where+gumbel_ms"], summary["argmax_objects_ms"]
        summary["larger_spread_ms"] = max(a["spread"], b["spread"])
        summary["median_difference_ms"] = b["median"] - a["median"]
        summary["difference_exceeds_larger_spread"] = bool(abs(b["median"] - a["median"]) > summary["larger_spread_ms"])
        summary["sample_minus_argmax_objects_ms"] = a["median"] - c["median"]
        summary["sample_per_draw_minus_argmax_objects_ms"] = a["median"] / K - c["median"]
        summary["sample_minus_argmax_objects_exceeds_larger_spread"] = bool(abs(a["median"] - c["median"]) > max(a["spread"], c["spread"]))
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
