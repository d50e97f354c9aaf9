"""The timing protocol of the side-by-side benches in this directory, once: events on the launch stream around a window of calls,
a warm-up of each side, then repeats in which the sides alternate their order inside one process; median and range per side."""
import os
import sys

import numpy as np
import torch


def add_repo_paths():
    """Puts the repository and its package directory on sys.path (the tools run from a checkout, not from an installed package)."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (repo, os.path.join(repo, "smg-multimodal-grasping_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


def window(fn, calls, dev):
    """ms per call of `calls` calls of fn back to back between two events, after a device synchronise."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / calls


def run_sides(sides, warmup, repeats, label_width, line="repeat %d %-*s %.4f ms"):
    """sides: (label, measure) pairs, measure() -> ms per call of one timed window (functools.partial(window, fn, calls, dev), each
    side with its own calls per window).  `warmup` untimed rounds, then `repeats` rounds, odd ones in reverse order, one printed
    line per window -> {label: [ms, ...]}."""
    times = {label: [] for label, _ in sides}
    for _ in range(warmup):
        for _, measure in sides:
            measure()
    for rep in range(repeats):
        for label, measure in (sides if rep % 2 == 0 else sides[::-1]):
            ms = measure()
            times[label].append(ms)
            print(line % (rep, label_width, label, ms), flush=True)
    return times


def side_stats(times, spread=False):
    stats = {"median": float(np.median(times)), "min": min(times), "max": max(times)}
    if spread:
        stats["spread"] = max(times) - min(times)
    return stats
