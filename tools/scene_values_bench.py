#!/usr/bin/env python3
"""Timing of smg_scene_values against the only other device route to the same floats: smg_scene_maps into [n_maps, hm, hm] and
out[m, iy, ix] by advanced indexing on the device.

Config-5 geometry: a 640^2 heightmap (S = 1824, 38 x 38 Q maps), 8 objects x 16 rotations = 128 maps, object-major as
Trainer.scene_object_values lays them out: 128 x 640^2 fp32 = 210 MB of scene-frame maps that the comparator writes to read K
floats per map.  The protocol is tools/scene_objects_bench.py's: events on the launch stream around a window of --calls calls
(default 20), the sides alternating inside one process, 2 warm-ups of each, 7 repeats; median and range per side, ms per call.
One row per K = 1, 64 and 4096 seeded pixels per map (inside the heightmap: the comparator cannot index outside it).  Sides:
    values       smg_scene_values (4 launches of 32 maps x ceil(K / 256) workgroups, the corners read from global memory)
    maps+index   smg_scene_maps, then out[m, iy, ix] with index tensors that are built before the window - the comparator
The two sides are gated bit-equal for every K before any time is printed.  The maps are synthetic (seeded normal): the kernels'
time does not depend on the values.  No ratio is required of either side; the largest K records whether reading the corners from
global memory, without staging the map in LDS, holds up when a map's points fill sixteen workgroups.

    python tools/scene_values_bench.py [--repeats 7] [--warmup 2] > profiles/scene_values.txt
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
    ap.add_argument("--points", type=int, nargs="+", default=[1, 64, 4096], help="K, pixels per map: one row each")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_values_bench: no GPU visible (a timing needs the MI355X)")
    import models
    from trainer import Trainer

    hm, R, n = args.size, args.rotations, args.objects
    pad, S, side = Trainer._scene_geometry(hm)
    dev = torch.device("cuda:0")
    eng = models.get_engine(0, S, 1, 2, 1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n_maps = n * R
    aff = np.stack([models.rotation_theta(m % R, R) for m in range(n_maps)])
    q = torch.from_numpy(np.random.default_rng(0).standard_normal((n_maps, side, side)).astype(np.float32)).to(dev)
    out = torch.empty((n_maps, hm, hm), dtype=torch.float32, device=dev)
    rows, keep = [], {}
    for K in args.points:
        pix_h = np.random.default_rng(K).integers(0, hm, size=(n_maps, K, 2)).astype(np.int32)
        pix = torch.from_numpy(pix_h).to(dev)
        m_idx = torch.arange(n_maps, device=dev)[:, None].expand(n_maps, K).contiguous()
        iy, ix = pix[..., 0].long().contiguous(), pix[..., 1].long().contiguous()
        vals = torch.empty((n_maps, K), dtype=torch.float32, device=dev)

        def values(K=K, pix=pix, vals=vals):
            eng.scene_values(q.data_ptr(), side * side, n_maps, aff, hm, K, pix.data_ptr(), vals.data_ptr(), stream)

        def maps_index(m_idx=m_idx, iy=iy, ix=ix):
            eng.scene_maps(q.data_ptr(), side * side, n_maps, aff, hm, out.data_ptr(), stream)
            keep["vals"] = out[m_idx, iy, ix]
        # the gate: the same floats from both routes, before anything is timed
        vals.fill_(7.0)
        values()
        maps_index()
        a, b = vals.cpu().numpy(), keep["vals"].cpu().numpy()
        if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            sys.exit("scene_values_bench: K = %d: the two routes differ in %d of %d values; nothing timed" % (K, int((a.view(np.uint32) != b.view(np.uint32)).sum()), a.size))
        rows.append((K, values, maps_index, int(np.isfinite(a).sum())))
    print("# %d^2 heightmap, S = %d, %d objects x %d rotations = %d maps of %d x %d -> [%d, %d, %d] fp32 = %.1f MB never written by `values`; "
          "%d calls between two events, ms per call; the two sides bit-equal for K = %s"
          % (hm, S, n, R, n_maps, side, side, n_maps, hm, hm, out.numel() * 4 / 1e6, args.calls, ", ".join(str(r[0]) for r in rows)))
    for K, values, maps_index, finite in rows:
        sides = tuple((name, functools.partial(window, fn, args.calls, dev)) for name, fn in (("values", values), ("maps+index", maps_index)))
        times = run_sides(sides, args.warmup, args.repeats, 10, line="K %d " % K + "repeat %d %-*s %.4f ms")
        summary = {"tool": "scene_values_bench", "input_size": S, "heightmap": hm, "objects": n, "rotations": R, "maps": n_maps, "map": [side, side],
                   "K": K, "points_with_a_window": finite, "points": n_maps * K, "repeats": args.repeats, "calls_per_window": args.calls,
                   "unwritten_mb": out.numel() * 4 / 1e6, "values_bit_equal": True}
        for name, _ in sides:
            summary[name + "_ms"] = side_stats(times[name], spread=True)
        a, b = summary["values_ms"], summary["maps+index_ms"]
        summary["larger_spread_ms"] = max(a["spread"], b["spread"])
        summary["median_difference_ms"] = b["median"] - a["median"]
        summary["difference_exceeds_larger_spread"] = bool(abs(b["median"] - a["median"]) > summary["larger_spread_ms"])
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
