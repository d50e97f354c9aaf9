#!/usr/bin/env python3
"""Timing of smg_loss_scene_map (a whole label image per pair, parallel over the map) against the only other way to the same
loss: smg_loss_scene fed EVERY heightmap pixel as a list (serial in the pixels, one workgroup per pair).

Config-5 geometry: a 640^2 heightmap (S = 1824, 38 x 38 Q maps), 32 pairs = rotations 0 .. 31 of 32, seeded random q, full label
and weight images.  The protocol is tools/scene_maps_bench.py's: events on the launch stream around each window, the sides
alternating inside one process, 2 warm-ups of each, 7 repeats; median, range and spread (max - min) per side, ms per call.  Sides:
    label_map     smg_loss_scene_map on the [32, 640, 640] label and weight images (52.4 MB each)
    pixel_list    smg_loss_scene with K = 409 600 = every pixel, the (iy, ix) list, labels and weights PREBUILT on the device
                  (16 bytes per pixel: 210 MB for 32 pairs; building and uploading them is not timed) - the comparator
Before anything is timed the two sides' loss and dq must agree to 2^-22 of the loss and of max|dq| (each rounds an fp64 sum once).
A window holds --calls calls of label_map; one call of pixel_list is long, so its calls per window are lowered to what fits
--side-b-window-ms (at least 1) from the time of a first single call, and the count used is written out.

    python tools/scene_label_maps_bench.py --probe        # the agreement check and one timed call of pixel_list: sizes the timeout
    python tools/scene_label_maps_bench.py [--repeats 7] [--warmup 2] > profiles/scene_label_maps.txt
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
    ap.add_argument("--calls", type=int, default=20, help="calls of label_map per timed window (pixel_list: at most this many)")
    ap.add_argument("--side-b-window-ms", type=float, default=1000.0, help="longest pixel_list window: its calls per window are lowered to fit")
    ap.add_argument("--size", type=int, default=640, help="heightmap side (640 -> S = 1824)")
    ap.add_argument("--pairs", type=int, default=32, help="pairs = rotations 0 .. pairs - 1 of that many")
    ap.add_argument("--probe", action="store_true", help="check the agreement, time one call of pixel_list, print it and stop")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_label_maps_bench: no GPU visible (a timing needs the MI355X)")
    import models
    from trainer import Trainer

    hm, R = args.size, args.pairs
    pad, S, side = Trainer._scene_geometry(hm)
    dev = torch.device("cuda:0")
    eng = models.get_engine(0, S, 1, 2, R)
    stream = torch.cuda.current_stream(dev).cuda_stream
    aff = np.stack([models.rotation_theta(r, R) for r in range(R)])
    rng = np.random.default_rng(0)
    q = torch.from_numpy(rng.standard_normal((R, 1, side, side)).astype(np.float32)).to(dev)
    lab = torch.from_numpy((1.5 * rng.standard_normal((R, hm, hm))).astype(np.float32)).to(dev)        # |d| on both sides of 1
    wgt = torch.from_numpy(rng.uniform(0.2, 1.0, size=(R, hm, hm)).astype(np.float32)).to(dev)
    K = hm * hm
    iy, ix = torch.meshgrid(torch.arange(hm, dtype=torch.int32, device=dev), torch.arange(hm, dtype=torch.int32, device=dev), indexing="ij")
    pix = torch.stack((iy, ix), dim=-1).reshape(1, K, 2).expand(R, K, 2).contiguous()                  # every pixel, row-major, per pair
    lab_k, wgt_k = lab.reshape(R, K), wgt.reshape(R, K)
    loss_a, dq_a = torch.empty(R, device=dev), torch.empty_like(q)
    loss_b, dq_b = torch.empty(R, device=dev), torch.empty_like(q)

    def label_map():
        eng.loss_scene_map(q.data_ptr(), aff, hm, R, lab.data_ptr(), wgt.data_ptr(), loss_a.data_ptr(), dq_a.data_ptr(), stream)

    def pixel_list():
        eng.loss_scene(q.data_ptr(), aff, hm, R, K, pix.data_ptr(), lab_k.data_ptr(), wgt_k.data_ptr(), loss_b.data_ptr(), dq_b.data_ptr(), stream)

    print("# %d^2 heightmap, S = %d, %d pairs, %d x %d maps; label + weight images %.1f MB, pixel list + labels + weights %.1f MB; ms per call"
          % (hm, S, R, side, side, 2 * lab.numel() * 4 / 1e6, (pix.numel() + 2 * R * K) * 4 / 1e6))
    first_b = window(pixel_list, 1, dev)              # the first single call of the comparator (cold: an upper bound of a warm one)
    label_map()
    torch.cuda.synchronize(dev)
    la, lb = loss_a.double().cpu().numpy(), loss_b.double().cpu().numpy()
    da, db = dq_a.double().cpu().numpy(), dq_b.double().cpu().numpy()
    loss_err = float(np.max(np.abs(la - lb) / np.abs(lb)))
    dq_err = float(np.abs(da - db).max() / np.abs(db).max())
    print("agreement: max |loss_a - loss_b| / loss_b = %.3e, max |dq_a - dq_b| / max|dq_b| = %.3e (gate 2^-22 = %.3e); first single call of pixel_list %.3f ms"
          % (loss_err, dq_err, 2.0 ** -22, first_b), flush=True)
    if not (np.isfinite(la).all() and np.isfinite(da).all() and loss_err <= 2.0 ** -22 and dq_err <= 2.0 ** -22):
        sys.exit("scene_label_maps_bench: the two sides disagree; nothing timed")
    if args.probe:
        print(json.dumps({"tool": "scene_label_maps_bench", "probe_pixel_list_ms": first_b}))
        return
    calls_b = int(max(1, min(args.calls, args.side_b_window_ms // max(first_b, 1e-3))))
    sides = (("label_map", functools.partial(window, label_map, args.calls, dev)), ("pixel_list", functools.partial(window, pixel_list, calls_b, dev)))
    print("# calls per window: label_map %d, pixel_list %d" % (args.calls, calls_b))
    times = run_sides(sides, args.warmup, args.repeats, 10)
    summary = {"tool": "scene_label_maps_bench", "input_size": S, "heightmap": hm, "pairs": R, "map": [side, side], "repeats": args.repeats,
               "warmup": args.warmup, "calls_per_window": {"label_map": args.calls, "pixel_list": calls_b},
               "first_single_call_pixel_list_ms": first_b, "loss_rel_diff": loss_err, "dq_rel_diff": dq_err}
    for name, _ in sides:
        summary[name + "_ms"] = side_stats(times[name], spread=True)
    a, b = summary["label_map_ms"], summary["pixel_list_ms"]
    summary["larger_spread_ms"] = max(a["spread"], b["spread"])
    summary["label_map_below_pixel_list_by_more_than_the_larger_spread"] = bool(b["median"] - a["median"] > summary["larger_spread_ms"])
    summary["pixel_list_over_label_map"] = b["median"] / a["median"]
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
