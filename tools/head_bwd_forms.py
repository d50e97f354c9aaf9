#!/usr/bin/env python3
"""A/B of the two forms of the head's value-convolution backward on a DENSE dq (engine option "head_bwd": 1 = the per-element
form with its fp32 atomics, 2 = the dense two-pass form).

Config-5 geometry: a 640^2 heightmap (S = 1824, 38 x 38 Q maps over 57^2 feature planes), 4 rotations of 32 as samples, full
weight maps.  Each repeat runs forward + smg_loss_map untimed, then times ONLY the smg_backward call between two events on the
launch stream; the forms alternate inside one process, after a warm-up of each.  Prints one line per repeat and a JSON summary:
median / min / max per form, the baseline's repeat-to-repeat spread and the ratio of the medians.
--classes 3: the same protocol on the 3-class head of a reactive trainer - label maps of classes 0 / 1 on every pixel, the dq of
smg_loss_map_ce.

    python tools/head_bwd_forms.py [--repeats 7] [--warmup 2] > profiles/head_bwd_forms.txt
    python tools/head_bwd_forms.py --classes 3 > profiles/head_bwd_forms_3class.txt
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
    ap.add_argument("--size", type=int, default=640, help="heightmap side (640 -> S = 1824)")
    ap.add_argument("--rotations", type=int, default=4)
    ap.add_argument("--classes", type=int, default=1, choices=(1, 3), help="1: reinforcement head + smg_loss_map; 3: reactive head + smg_loss_map_ce")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_bwd_forms: no GPU visible (a timing needs the MI355X)")
    import synthetic
    from oracle import affordance as orc
    from trainer import Trainer

    tr = Trainer('reinforcement' if args.classes == 1 else 'reactive', 0.5, False, None, False)
    sd = synthetic.make_state_dict(orc.state_layout(args.classes), 0)
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = tr.model
    model.gnum_rotations = model.snum_rotations = 32
    depth, masks = synthetic.heightmap_scene(4, size=args.size, n_boxes=8)
    hm, rots = tr._scenes_to_device(depth, depth * masks[0], list(range(5, 5 + args.rotations)))
    side, n = Trainer.dense_map_size(args.size), args.rotations
    dev = model._flat_params.device
    lab = torch.as_tensor(synthetic.uniform(5, "ab/lab", n * side * side, -1.5, 2.5).astype(np.float32), device=dev)
    wgt = torch.as_tensor(synthetic.uniform(5, "ab/w", n * side * side, 0.05, 1.0).astype(np.float32), device=dev)
    if args.classes == 3:      # every pixel labelled 0 or 1
        lab = torch.as_tensor(np.floor(synthetic.uniform(5, "ab/cls", n * side * side, 0.0, 2.0)).astype(np.float32), device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    head = "graspnet_val.grasp-val-conv1.weight"

    grads = {}

    def one(form):
        """forward + loss (untimed), then the timed backward; returns its ms and keeps the value convolution's weight gradient"""
        q = model.run(0, rots, 32, heightmaps=hm, mean=tr.image_mean, std=tr.image_std, keep_for_backward=True, update_bn=False)
        eng = model._saved[0]
        eng.set_option("head_bwd", form)
        dq = torch.empty_like(q)
        if args.classes == 1:
            eng.loss_map(q.data_ptr(), lab.data_ptr(), wgt.data_ptr(), n, loss.data_ptr(), dq.data_ptr(), stream)
        else:
            eng.loss_map_ce(q.data_ptr(), lab.data_ptr(), n, loss.data_ptr(), dq.data_ptr(), stream)
        model.flat_grads().zero_()
        net = model._net_struct(True)
        ms = window(lambda: eng.backward(net, dq.data_ptr(), stream), 1, dev)
        eng.set_option("head_bwd", 0)
        off, cnt = next((o, int(np.prod(s))) for nm, k, o, s in model._layout if nm == head and k == 0)
        grads[form] = model.flat_grads()[off:off + cnt].clone()
        return ms

    print("# %d^2 heightmap, %d rotations (%d streams), %d x %d maps, %s; the backward call only, ms"
          % (args.size, n, n + 1, side, side, "full weight maps" if args.classes == 1 else "3 classes, every pixel labelled 0 / 1"))
    sides = tuple(("head_bwd=%d backward" % form, functools.partial(one, form)) for form in (1, 2))
    times = run_sides(sides, args.warmup, args.repeats, 0, line="repeat %d %-*s %.3f ms")
    per_element, dense = (side_stats(times[label]) for label, _ in sides)
    eng = model._saved[0]
    d = float((grads[1].double() - grads[2].double()).norm() / grads[1].double().norm())
    print(json.dumps({
        "tool": "head_bwd_forms", **({} if args.classes == 1 else {"classes": args.classes}), "input_size": eng.S, "samples": n, "streams": n + 1, "map": [side, side], "repeats": args.repeats,
        "per_element_ms": per_element,
        "dense_ms": dense,
        "baseline_spread_ms": per_element["max"] - per_element["min"],
        "dense_over_per_element": dense["median"] / per_element["median"],
        "value_conv_wgrad_rel_distance": d,
    }))


if __name__ == "__main__":
    main()
