#!/usr/bin/env python3
"""Timing of the reactive net's scene-frame kernels against what a caller could do without them: the class logits of
forward_class_maps(logits=True, return_device=True) through torch's own F.grid_sample and softmax on the device.

Config-5 geometry: a 640^2 heightmap (S = 1824, 38 x 38 maps of three logits), 32 rotations -> [32, 640, 640] probabilities of one
class (52 MB of fp32) or [32, 3, 640, 640] of all three (157 MB).  The protocol is tools/scene_maps_bench.py's: events on the
launch stream around each call, the sides alternating inside one process, 2 warm-ups of each, 7 repeats; median and range per
side; a timed window holds --calls calls back to back (default 20) and the figures are per call.  Sides:
    class_maps_0    smg_scene_class_maps, cls 0 (one launch, one plane stored)
    class_maps_all  smg_scene_class_maps, cls -1 (one launch, three planes stored)
    class_argmax    smg_scene_class_argmax, cls 0 (the walk without the store + a one-workgroup reduce)
    maps+argmax     smg_scene_class_maps cls 0 followed by smg_argmax over its output (the alternative to the fused argmax)
    grid_sample     softmax(F.grid_sample(q, grid, 'bilinear', 'border', align_corners=True), dim=1) of the [32, 3, 38, 38] logits
                    with a PREBUILT fp32 grid, then torch.where(valid, ., -inf) with a prebuilt mask - the comparator of
                    class_maps_all (building grid and mask is not timed)
The logits are synthetic (seeded normal, std 2): the kernels' time does not depend on the values.

    python tools/scene_class_maps_bench.py [--repeats 7] [--warmup 2] > profiles/scene_class_maps.txt
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
        sys.exit("scene_class_maps_bench: no GPU visible (a timing needs the MI355X)")
    import models
    import smg_hip
    from trainer import Trainer

    hm, R = args.size, args.rotations
    pad, S, side = Trainer._scene_geometry(hm)
    dev = torch.device("cuda:0")
    eng = models.get_engine(0, S, 3, 2, 1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    aff = np.stack([models.rotation_theta(r, R) for r in range(R)])
    q = torch.from_numpy((2.0 * np.random.default_rng(0).standard_normal((R, 3, side, side))).astype(np.float32)).to(dev)
    out1 = torch.empty((R, hm, hm), dtype=torch.float32, device=dev)
    out3 = torch.empty((R, 3, hm, hm), dtype=torch.float32, device=dev)
    idx = torch.empty(2, dtype=torch.int32, device=dev)
    val = torch.empty(2, dtype=torch.float32, device=dev)
    # the comparator's grid and mask, from the host restatement of the geometry
    pix = np.stack(np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij"), axis=-1)
    grid = np.empty((R, hm, hm, 2), dtype=np.float32)
    mask = np.empty((R, 1, hm, hm), dtype=bool)
    for r in range(R):
        qy, qx, valid = Trainer.scene_to_map(hm, r, R, pix)
        grid[r, ..., 0], grid[r, ..., 1], mask[r, 0] = 2 * qx / (side - 1) - 1, 2 * qy / (side - 1) - 1, valid
    grid_d, mask_d = torch.from_numpy(grid).to(dev), torch.from_numpy(mask).to(dev)
    ninf = torch.tensor(float("-inf"), device=dev)

    def class_maps_0():
        eng.scene_class_maps(q.data_ptr(), R, aff, hm, 0, out1.data_ptr(), stream)

    def class_maps_all():
        eng.scene_class_maps(q.data_ptr(), R, aff, hm, -1, out3.data_ptr(), stream)

    def class_argmax():
        eng.scene_class_argmax(q.data_ptr(), R, aff, hm, 0, idx.data_ptr(), val.data_ptr(), stream)

    def maps_argmax():
        eng.scene_class_maps(q.data_ptr(), R, aff, hm, 0, out1.data_ptr(), stream)
        smg_hip.argmax(out1.data_ptr(), out1.numel(), idx[1:].data_ptr(), val[1:].data_ptr(), stream)

    def grid_sample():
        z = F.grid_sample(q, grid_d, mode="bilinear", padding_mode="border", align_corners=True)
        return torch.where(mask_d, torch.softmax(z, dim=1), ninf)

    sides = tuple((name, functools.partial(window, fn, args.calls, dev)) for name, fn in (
        ("class_maps_0", class_maps_0), ("class_maps_all", class_maps_all), ("class_argmax", class_argmax), ("maps+argmax", maps_argmax),
        ("grid_sample", grid_sample)))

    print("# %d^2 heightmap, S = %d, %d rotations, %d x %d x 3 logits -> [%d, %d, %d] fp32 = %.1f MB per class plane, %.1f MB for all three; "
          "%d calls between two events, ms per call" % (hm, S, R, side, side, R, hm, hm, out1.numel() * 4 / 1e6, out3.numel() * 4 / 1e6, args.calls))
    times = run_sides(sides, args.warmup, args.repeats, 14)
    # agreement of the two sides (fp32 grid and fp32 softmax on the comparator's side: not bit-equal) and of the two argmax routes
    ref = grid_sample()
    both = torch.isfinite(ref) & torch.isfinite(out3)
    i = idx.cpu().numpy()
    summary = {"tool": "scene_class_maps_bench", "input_size": S, "heightmap": hm, "rotations": R, "map": [3, side, side], "repeats": args.repeats,
               "calls_per_window": args.calls, "output_mb_one_class": out1.numel() * 4 / 1e6, "output_mb_all": out3.numel() * 4 / 1e6,
               "max_abs_diff_vs_grid_sample": float((ref[both] - out3[both]).abs().max()),
               "mask_mismatches_vs_grid_sample": int((torch.isfinite(ref) != torch.isfinite(out3)).sum()),
               "one_class_equals_its_plane_of_all": bool(torch.equal(out1.view(torch.int32), out3[:, 0].contiguous().view(torch.int32))),
               "argmax_routes_agree": bool(i[0] == i[1])}
    for name, _ in sides:
        summary[name + "_ms"] = side_stats(times[name])
    summary["class_maps_0_write_gb_per_s"] = out1.numel() * 4 / 1e9 / (summary["class_maps_0_ms"]["median"] * 1e-3)
    summary["class_maps_all_write_gb_per_s"] = out3.numel() * 4 / 1e9 / (summary["class_maps_all_ms"]["median"] * 1e-3)
    cmp_, all_ = summary["grid_sample_ms"], summary["class_maps_all_ms"]
    spread = max(cmp_["max"] - cmp_["min"], all_["max"] - all_["min"])
    summary["spread_ms"] = spread
    summary["class_maps_all_faster_than_comparator"] = bool(all_["median"] < cmp_["median"])
    summary["difference_beyond_the_spread"] = bool(abs(cmp_["median"] - all_["median"]) > spread)
    fused, two = summary["class_argmax_ms"], summary["maps+argmax_ms"]
    summary["fused_argmax_faster_than_maps_plus_argmax"] = bool(fused["median"] < two["median"])
    summary["argmax_difference_beyond_the_spread"] = bool(abs(two["median"] - fused["median"]) > max(fused["max"] - fused["min"], two["max"] - two["min"]))
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
