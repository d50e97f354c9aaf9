#!/usr/bin/env python3
"""Timing of the scene-frame Q map kernels against what a caller could do without them: the dense maps of
forward_dense(return_device=True) through torch's own F.grid_sample on the device, with the same sampling grid.

Config-5 geometry: a 640^2 heightmap (S = 1824, 38 x 38 Q maps), 32 rotations -> [32, 640, 640] scene-frame maps, 52 MB of fp32.
The protocol is tools/head_bwd_forms.py's: events on the launch stream around each call, the sides alternating inside one process,
2 warm-ups of each, 7 repeats; median and range per side.  The calls take tens of microseconds, so a timed window holds
--calls of them back to back (default 20) and the figures are per call.  Sides:
    scene_maps      smg_scene_maps (one launch)
    scene_argmax    smg_scene_argmax (the walk without the store + a one-workgroup reduce)
    maps+argmax     smg_scene_maps followed by smg_argmax over its output (the alternative to the fused argmax)
    grid_sample     F.grid_sample(q[:, None], grid, 'bilinear', 'border', align_corners=True) with a PREBUILT fp32 grid, then
                    torch.where(valid, ., -inf) with a prebuilt mask - the comparator (building grid and mask is not timed)
The maps are synthetic (seeded normal): the kernels' time does not depend on the values.

    python tools/scene_maps_bench.py [--repeats 7] [--warmup 2] > profiles/scene_maps.txt
"""
import argparse
import functools
import json
import sys

import numpy as np
import torch
import torch.nn.functional as F

from bench_sides import add_repo_paths, run_sides, side_stats, window

add_repo_paths()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--size", type=int, default=640, help="heightmap side (640 -> S = 1824)")
    ap.add_argument("--rotations", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_maps_bench: no GPU visible (a timing needs the MI355X)")
    import models
    import smg_hip
    from trainer import Trainer

    hm, R = args.size, args.rotations
    pad, S, side = Trainer._scene_geometry(hm)
    dev = torch.device("cuda:0")
    eng = models.get_engine(0, S, 1, 2, 1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    aff = np.stack([models.rotation_theta(r, R) for r in range(R)])
    q = torch.from_numpy(np.random.default_rng(0).standard_normal((R, side, side)).astype(np.float32)).to(dev)
    out = torch.empty((R, hm, hm), dtype=torch.float32, device=dev)
    idx = torch.empty(2, dtype=torch.int32, device=dev)
    val = torch.empty(2, dtype=torch.float32, device=dev)
    # the comparator's grid and mask, from the host restatement of the geometry
    pix = np.stack(np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij"), axis=-1)
    grid = np.empty((R, hm, hm, 2), dtype=np.float32)
    mask = np.empty((R, hm, hm), dtype=bool)
    for r in range(R):
        qy, qx, valid = Trainer.scene_to_map(hm, r, R, pix)
        grid[r, ..., 0], grid[r, ..., 1], mask[r] = 2 * qx / (side - 1) - 1, 2 * qy / (side - 1) - 1, valid
    grid_d, mask_d = torch.from_numpy(grid).to(dev), torch.from_numpy(mask).to(dev)
    ninf = torch.tensor(float("-inf"), device=dev)

    def scene_maps():
        eng.scene_maps(q.data_ptr(), side * side, R, aff, hm, out.data_ptr(), stream)

    def scene_argmax():
        eng.scene_argmax(q.data_ptr(), side * side, R, aff, hm, idx.data_ptr(), val.data_ptr(), stream)

    def maps_argmax():
        eng.scene_maps(q.data_ptr(), side * side, R, aff, hm, out.data_ptr(), stream)
        smg_hip.argmax(out.data_ptr(), out.numel(), idx[1:].data_ptr(), val[1:].data_ptr(), stream)

    def grid_sample():
        return torch.where(mask_d, F.grid_sample(q[:, None], grid_d, mode="bilinear", padding_mode="border", align_corners=True)[:, 0], ninf)

    sides = tuple((name, functools.partial(window, fn, args.calls, dev)) for name, fn in (
        ("scene_maps", scene_maps), ("scene_argmax", scene_argmax), ("maps+argmax", maps_argmax), ("grid_sample", grid_sample)))

    print("# %d^2 heightmap, S = %d, %d rotations, %d x %d maps -> [%d, %d, %d] fp32 = %.1f MB; %d calls between two events, ms per call"
          % (hm, S, R, side, side, R, hm, hm, out.numel() * 4 / 1e6, args.calls))
    times = run_sides(sides, args.warmup, args.repeats, 12)
    # agreement of the two sides (fp32 grid on the comparator's side: not bit-equal) and of the two argmax routes
    ref = grid_sample()
    both = torch.isfinite(ref) & torch.isfinite(out)
    i = idx.cpu().numpy()
    summary = {"tool": "scene_maps_bench", "input_size": S, "heightmap": hm, "rotations": R, "map": [side, side], "repeats": args.repeats, "calls_per_window": args.calls,
               "output_mb": out.numel() * 4 / 1e6,
               "max_abs_diff_vs_grid_sample": float((ref[both] - out[both]).abs().max()),
               "mask_mismatches_vs_grid_sample": int((torch.isfinite(ref) != torch.isfinite(out)).sum()),
               "argmax_routes_agree": bool(i[0] == i[1])}
    for name, _ in sides:
        summary[name + "_ms"] = side_stats(times[name])
    med = summary["scene_maps_ms"]["median"]
    summary["scene_maps_write_gb_per_s"] = out.numel() * 4 / 1e9 / (med * 1e-3)
    cmp_ = summary["grid_sample_ms"]
    summary["comparator_spread_ms"] = cmp_["max"] - cmp_["min"]
    summary["scene_maps_faster_than_comparator_beyond_its_spread"] = bool(cmp_["median"] - med > cmp_["max"] - cmp_["min"])
    summary["fused_argmax_faster_than_maps_plus_argmax"] = bool(summary["scene_argmax_ms"]["median"] < summary["maps+argmax_ms"]["median"])
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
