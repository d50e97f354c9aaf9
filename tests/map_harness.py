"""What the dense-map and scene-frame test modules (test_gpu_*maps.py, test_cpu_*maps.py) share, each once: the gpu fixture, seeded
trainers and engines, the fill / written / bit-identical idioms, the refusal table of the scene-frame label-map losses, the S = 704
scene of the train_batch tests with their common tail, and the CPU modules' "declared, exported and bound" check."""
import contextlib
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import gpu, grads_within_fp32_class, MEAN, STD, oracle_net, orc, REPO  # noqa: F401  (gpu: the fixture, for the map modules to import by name)

import scene_ref

HEAD = "graspnet_val.grasp-val-"        # style 0's head (oracle.affordance.STYLE_HEAD)
HEAD_OUT = {'reinforcement': 1, 'reactive': 3}


def make_trainer(method, seed, R=16):
    """A trainer of `method` with seeded weights, R rotations and a zero learning rate (reinforcement: the target net in sync)."""
    import synthetic
    from trainer import Trainer
    tr = Trainer(method, 0.5, False, None, False)
    sd = synthetic.make_state_dict(orc.state_layout(HEAD_OUT[method]), seed)
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    tr.model.gnum_rotations = tr.model.snum_rotations = R
    if method == 'reinforcement':
        tr.model_target.load_state_dict(tr.model.state_dict())
        tr.model_target.gnum_rotations = tr.model_target.snum_rotations = R
    tr.optimizer.lr = 0.0
    return tr


def cached_engine(S, out_ch, pairs=1):
    """The engine the suite caches per (device, S, head)."""
    import models
    return models.get_engine(0, S, out_ch, 2, pairs)


@contextlib.contextmanager
def own_engine(S, out_ch, pairs):
    """An engine of the test's own with ONE stream - a loss needs nothing of the network's workspace, only the engine's scratch -
    closed when the test is done: the engines the suite caches per (device, S, head) keep the memory they had."""
    import smg_hip
    eng = smg_hip.Engine(0, S, 1, pairs, out_ch)
    try:
        yield eng
    finally:
        torch.cuda.synchronize()
        eng.close()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


def filled(shape, value=-7.0):
    """A float32 device tensor no kernel has written yet: every element `value`."""
    return torch.full(tuple(shape), value, dtype=torch.float32, device="cuda")


def assert_written_and_finite(fill, *arrays):
    """Every element of the host arrays finite and none left at the fill."""
    for a in arrays:
        assert np.isfinite(a).all() and not (a == fill).any()


def assert_bit_identical(a, b):
    """Two float32 results (tensors or arrays), bit for bit: what a second identical call must give."""
    a, b = bits(a), bits(b)
    assert np.array_equal(a, b), "%s vs %s: %d elements differ" % (a.shape, b.shape, int((a != b).sum()) if a.shape == b.shape else -1)


def border_pixels(valid):
    """How many valid pixels of one [hm, hm] validity mask lie on the image border."""
    return int(valid[0].sum() + valid[-1].sum() + valid[1:-1, 0].sum() + valid[1:-1, -1].sum())


def assert_scene_loss_refusals(call, method, name, head_out, wrong_head_out, engine, loss, dq, name_leads):
    """The refusals of a scene-frame label-map loss at hm = 240, 4 pairs: -22, a message that names the function and the cause, and
    nothing launched - a head of the wrong width, a heightmap side that does not pad to the engine's S (twice), a 1 x 1 map,
    n_pairs < 1, an affine matrix with a translation - then SmgError from the Engine method on that matrix, and `loss` / `dq` still
    at their -7 fill.  call(eng, affine_ptr, hm, n) is the C entry point `name` and method(eng, affine, hm, n) the Engine's, both on
    the caller's buffers; engine(S, out_ch) is a context manager that yields an engine.  name_leads: the message must START with
    "<name>:" (otherwise it must hold the name)."""
    import smg_hip
    L = smg_hip.lib()
    hm = 240
    aff = np.stack([scene_ref.theta(r, 16) for r in range(4)])
    ap = aff.ctypes.data_as(C.POINTER(C.c_float))
    shifted = aff.copy()
    shifted[3, 5] = 0.25

    def refused(eng, affine, size, n, word):
        rc = call(eng, affine, size, n)
        msg = L.smg_last_error()
        assert rc == -22 and (msg.startswith(name + b":") if name_leads else name in msg) and word in msg, (rc, msg)
    with engine(704, head_out) as eng, engine(704, wrong_head_out) as eng_wrong, engine(640, head_out) as eng640:
        refused(eng_wrong, ap, hm, 4, b"head_out")
        refused(eng, ap, 320, 4, b"does not pad")
        refused(eng, ap, 224, 4, b"does not pad")
        refused(eng640, ap, 224, 4, b"1 x 1")
        refused(eng, ap, hm, 0, b"n_pairs < 1")
        refused(eng, shifted.ctypes.data_as(C.POINTER(C.c_float)), hm, 4, b"translation")
        with pytest.raises(smg_hip.SmgError):
            method(eng, shifted, hm, 4)
    torch.cuda.synchronize()
    assert bool((loss == -7.0).all()) and bool((dq == -7.0).all())


def s704_scene(out_ch, rots=(1, 6)):
    """The scene of the train_batch_scene_* tests: a 240^2 heightmap -> S = 704, 3 x 3 maps, style 0, one sample per rotation of 16.
    -> dict: hm, style, rots, block (the 81 pixels 116 .. 124 squared, row-major, all valid), aff (one matrix per sample), depth, md,
    x, mx (preprocessed), on (the fp32 oracle), o64 (its fp64 copy), q64 (o64's maps per sample, in the autograd graph)."""
    import synthetic
    hm, style, rots = 240, 0, list(rots)
    by, bx = np.meshgrid(np.arange(116, 125), np.arange(116, 125), indexing="ij")
    block = np.stack([by.ravel(), bx.ravel()], axis=-1)
    aff = [scene_ref.theta(r, 16) for r in rots]
    for a in aff:
        assert scene_ref.map_coords(hm, a, block[:, 0], block[:, 1])[2].all()
    depth, masks = synthetic.heightmap_scene(8, size=hm, n_boxes=8)
    md = depth * masks[0]
    x = orc.preprocess(depth, [MEAN] * 3, [STD] * 3)
    mx = orc.preprocess(md, [MEAN] * 3, [STD] * 3)
    assert x.shape[-1] == 704
    on = oracle_net(1, out_ch)
    o64 = copy.deepcopy(on).double()
    trunk, head = getattr(o64, orc.STYLE_TRUNK[style]).features, getattr(o64, orc.STYLE_HEAD[style])
    fm = trunk(mx.double())
    q64 = [head(torch.cat((trunk(orc.rotate(x, r, 16).double()), fm), 1)) for r in rots]
    assert tuple(q64[0].shape) == (1, out_ch, 3, 3)
    return dict(hm=hm, style=style, rots=rots, block=block, aff=aff, depth=depth, md=md, x=x, mx=mx, on=on, o64=o64, q64=q64)


def assert_train_batch_runs(tr, runs, on, g64, what, n_tensors=368):
    """The common tail of the train_batch tests: all `n_tensors` gradient tensors of `tr` - those of the fp64 oracle g64 - within 3x
    the fp32 oracle's own error against fp64 (three outliers below 5 % of their norm), and the head's conv1 weight gradient of the
    two `runs` not zero and bit for bit equal.  Returns how many tensors were compared."""
    rel_p, _, _ = grads_within_fp32_class(tr.model.named_parameters(), on.named_parameters(), g64, 3.0, what, max_outliers=3, outlier_cap=0.05)
    assert len(rel_p) == len(g64) == n_tensors, (len(rel_p), len(g64))
    assert float(runs[0].abs().max()) > 0
    assert_bit_identical(runs[0], runs[1])
    return len(rel_p)


def cpu_trainer(method):
    from trainer import Trainer
    tr = Trainer(method, 0.5, False, None, True)       # force_cpu: no engine can exist behind it
    tr.model.gnum_rotations = tr.model.snum_rotations = 16
    return tr


def assert_declared_exported_and_bound(symbol, header_regex, n_argtypes, engine_method, trainer_methods=()):
    """include/smg_hip.h declares `symbol` with the signature `header_regex` at the ABI version of the binding, the library exports
    it, smg_hip.py binds it with `n_argtypes` arguments behind Engine.<engine_method>, and the Trainer has `trainer_methods`.
    Returns the header's text."""
    import smg_hip
    from trainer import Trainer
    hdr = open(os.path.join(REPO, "include", "smg_hip.h")).read()
    assert re.search(header_regex, hdr)
    assert int(re.search(r"#define\s+SMG_ABI_VERSION\s+(\d+)", hdr).group(1)) == smg_hip.ABI_VERSION == 9
    assert hasattr(C.CDLL(smg_hip.LIB_PATH), symbol)
    assert symbol in smg_hip.EXPORTS
    assert smg_hip.lib().smg_version() == 9
    assert len(getattr(smg_hip.lib(), symbol).argtypes) == n_argtypes
    assert callable(getattr(smg_hip.Engine, engine_method))
    for m in trainer_methods:
        assert callable(getattr(Trainer, m))
    return hdr
