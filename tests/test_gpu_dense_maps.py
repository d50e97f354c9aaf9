"""Dense Q maps (heightmaps larger than 224^2) through the public interface, on the MI355X (run with -m gpu): whole-map
training (smg_loss_map + the dense form of the head's value-convolution backward) against the fp64 PyTorch-CPU oracle,
the one-pixel special case against train_batch, the config-5 geometry against an fp64 restatement of the head alone,
run-to-run determinism of the value-convolution weight gradient, forward_dense / best_dense_action against forward and
np.argmax, and the refusal of a 3-class head.

Yardsticks are the parity suite's own (helpers.q_close, helpers.grads_within_fp32_class: within 3x what fp32 costs
PyTorch-CPU itself against an fp64 evaluation)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import grads_within_fp32_class, MEAN, STD, oracle_net, orc, q_close
from map_harness import assert_bit_identical, cached_engine, filled, gpu, HEAD, make_trainer, stream  # noqa: F401

pytestmark = pytest.mark.gpu

def huber_map(q, lab, w):
    """sum over the map of w * Huber(q - label), code/trainer.py:345-348 per element (torch, any dtype)."""
    d = q - lab
    return (w * torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)).sum()


def rel_dist(a, b):
    a, b = a.double().cpu().numpy().ravel(), b.double().cpu().numpy().ravel()
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b * b).sum()), 1e-300))


def test_whole_map_training_vs_fp64_oracle_s928(gpu):
    """A 320^2 heightmap -> S = 928: 10 x 10 Q maps over ragged 29^2 feature planes.  One sample (style 0, rotation 3), labels
    U(-1.5, 2.5) - on the fp32 oracle Q spans -2.45 .. 3.08, 49 % of the elements sit in the linear Huber branch - and
    weights U(0, 1) with every seventh exactly 0.  Q by q_close, the loss to fp32 rounding of the same sum, all 368 gradient
    tensors within 3x the fp32 oracle's own error against fp64 (three outliers below 5 % of their norm, as
    test_g5_backward_gradients allows) - for the dense head backward ("head_bwd" = 2) and for the per-element one (= 1) on
    the same dq."""
    import synthetic
    style, rot = 0, 3
    depth, masks = synthetic.heightmap_scene(6, size=320)
    md = depth * masks[0]
    x = orc.preprocess(depth, [MEAN] * 3, [STD] * 3)
    mx = orc.preprocess(md, [MEAN] * 3, [STD] * 3)
    assert x.shape[-1] == 928
    lab = synthetic.uniform(3, "dense/lab", 100, -1.5, 2.5).astype(np.float32).reshape(1, 10, 10)
    wgt = synthetic.uniform(3, "dense/w", 100, 0.0, 1.0).astype(np.float32).reshape(1, 10, 10)
    wgt.reshape(-1)[::7] = 0.0
    lab_t, wgt_t = torch.from_numpy(lab).reshape(1, 1, 10, 10), torch.from_numpy(wgt).reshape(1, 1, 10, 10)

    on = oracle_net(1)
    rx = orc.rotate(x, rot, 16)
    o64 = copy.deepcopy(on).double()
    trunk, head = getattr(o64, orc.STYLE_TRUNK[style]).features, getattr(o64, orc.STYLE_HEAD[style])
    q64 = head(torch.cat((trunk(rx.double()), trunk(mx.double())), 1))
    assert tuple(q64.shape) == (1, 1, 10, 10)
    loss64 = huber_map(q64, lab_t.double(), wgt_t.double())
    loss64.backward()
    g64 = {n: p.grad for n, p in o64.named_parameters() if p.grad is not None}
    on.zero_grad()
    qo = orc.forward(on, x, mx, style, False, rot)
    d = (qo.detach() - lab_t).abs().numpy().ravel()
    print("fp32 oracle: Q %.2f .. %.2f, %.0f %% of the elements in the linear Huber branch, %d weights exactly 0"
          % (float(qo.detach().min()), float(qo.detach().max()), 100.0 * (d >= 1).mean(), int((wgt == 0).sum())))
    huber_map(qo, lab_t, wgt_t).backward()

    tr = make_trainer('reinforcement', 1)
    eng = cached_engine(928, 1)
    head_names = [HEAD + "conv1.weight", HEAD + "norm1.weight", HEAD + "norm1.bias"]
    got = {}
    try:
        for form in (2, 1):
            eng.set_option("head_bwd", form)
            loss, q = tr.train_batch_maps(depth, md, style, [rot], lab, wgt, return_q=True)
            assert tuple(q.shape) == (1, 1, 10, 10) and tuple(loss.shape) == (1,)
            qh = q.cpu().numpy().astype(np.float64)
            ok, worst = q_close(qh.ravel(), q64.detach().numpy().ravel(), what="S=928 head_bwd=%d" % form)
            assert ok, worst
            # the loss against the fp64 sum over the product's OWN q: what remains is the fp32 arithmetic of the loss kernel - three
            # roundings per term (difference, square or |.| - 0.5, weight), one add in the thread's strided sum (100 < 256 elements),
            # eight levels of the LDS tree: at most 12 units of 2^-24 of the sum of the terms' magnitudes; the gate is 16
            dd = qh.reshape(10, 10) - lab[0].astype(np.float64)
            terms = wgt[0].astype(np.float64) * np.where(np.abs(dd) < 1, 0.5 * dd * dd, np.abs(dd) - 0.5)
            err = abs(float(loss.cpu().numpy()[0]) - terms.sum())
            print("head_bwd=%d: loss %.7f, fp64 sum over the same q %.7f: |d| %.2e (gate %.2e); fp64 oracle loss %.7f"
                  % (form, float(loss[0]), terms.sum(), err, 16 * 2.0 ** -24 * np.abs(terms).sum(), float(loss64)))
            assert err <= 16 * 2.0 ** -24 * np.abs(terms).sum()
            rel_p, _, _ = grads_within_fp32_class(tr.model.named_parameters(), on.named_parameters(), g64, 3.0, "S=928 maps head_bwd=%d" % form,
                                                  max_outliers=3, outlier_cap=0.05)
            assert len(rel_p) == 368
            named = dict(tr.model.named_parameters())
            got[form] = {n: named[n].grad.clone() for n in head_names}
    finally:
        eng.set_option("head_bwd", 0)
    for n in head_names:
        print("dense vs per-element form, %-40s |d| / |g| = %.3e" % (n, rel_dist(got[2][n], got[1][n])))


def test_train_batch_pixels_at_origin_equals_train_batch(gpu):
    """One trained pixel per sample at (0, 0) is what train_batch trains (the Huber on element [0,0,0,0], code/trainer.py:345):
    loss and q bit-identical, and smg_loss_map's dq on the one-hot maps bit-identical to smg_loss's."""
    import synthetic
    tr = make_trainer('reinforcement', 2)
    depth, masks = synthetic.heightmap_scene(8, size=240, n_boxes=8)
    md = depth * masks[0]
    rots, labels = [5, 9], [0.4, 7.5]                 # one sample per Huber branch
    loss_a, q_a = tr.train_batch(depth, md, 0, rots, labels, return_q=True)
    loss_b, q_b = tr.train_batch_pixels(depth, md, 0, rots, [(0, 0), (0, 0)], labels, return_q=True)
    assert tuple(q_a.shape) == (2, 1, 3, 3)
    assert_bit_identical(q_a, q_b)
    assert_bit_identical(loss_a, loss_b)
    eng = cached_engine(704, 1)
    lab = torch.tensor(labels, dtype=torch.float32, device="cuda")
    lab_maps = torch.zeros_like(q_a)
    lab_maps[:, 0, 0, 0] = lab
    w_maps = torch.zeros_like(q_a)
    w_maps[:, 0, 0, 0] = 1.0
    out = []
    for use_map in (False, True):
        loss, dq = filled((2,), -1.0), filled(q_a.shape, -1.0)
        if use_map:
            eng.loss_map(q_a.data_ptr(), lab_maps.data_ptr(), w_maps.data_ptr(), 2, loss.data_ptr(), dq.data_ptr(), stream())
        else:
            eng.loss(0, q_a.data_ptr(), lab.data_ptr(), 2, loss.data_ptr(), dq.data_ptr(), stream())
        out.append((loss, dq))
    assert_bit_identical(out[0][1], out[1][1])
    assert_bit_identical(out[0][0], out[1][0])
    assert int((out[1][1] != 0).sum()) == 2
    # NULL weights: every element counts
    loss, dq = torch.empty(2, device="cuda"), torch.empty_like(q_a)
    eng.loss_map(q_a.data_ptr(), lab_maps.data_ptr(), None, 2, loss.data_ptr(), dq.data_ptr(), stream())
    ref = torch.stack([huber_map(q_a[k].double(), lab_maps[k].double(), 1.0) for k in range(2)])
    assert torch.allclose(loss.double(), ref, rtol=1e-6, atol=0)      # (nine positive terms: 3 roundings each + 4 tree levels = 7 x 2^-24)


def test_config5_geometry_head_alone_vs_fp64(gpu):
    """A 640^2 heightmap -> S = 1824: two rotations, 38 x 38 maps over 57^2 planes (3249 pixels in 3264 padded rows), full weight
    maps, the dense form.  Shapes and finiteness; then the head ALONE: from the engine's own h1 the chain BN(train) + ReLU ->
    20x20 convolution -> map loss is rebuilt with torch in fp64 (the truth) and in fp32, and the engine's dh1 and its gradients
    of conv1.weight, norm1.weight and norm1.bias must lie within 3x the fp32 evaluation's own error.  (The whole network at this
    size against the oracle is test_large_input_backward_config5_share's.)"""
    import synthetic
    tr = make_trainer('reinforcement', 0, R=32)
    depth, masks = synthetic.heightmap_scene(4, size=640, n_boxes=8)
    md = depth * masks[0]
    rots = [5, 6]
    n, side, HW, HWp = len(rots), 38, 57 * 57, 3264
    lab = synthetic.uniform(5, "dense5/lab", n * side * side, -1.5, 2.5).astype(np.float32).reshape(n, side, side)
    wgt = synthetic.uniform(5, "dense5/w", n * side * side, 0.05, 1.0).astype(np.float32).reshape(n, side, side)
    eng = cached_engine(1824, 1)
    eng.set_option("head_bwd", 2)
    try:
        loss, q = tr.train_batch_maps(depth, md, 0, rots, lab, wgt, return_q=True)
    finally:
        eng.set_option("head_bwd", 0)
    assert tuple(q.shape) == (n, 1, side, side) and tuple(loss.shape) == (n,)
    assert eng.HWp[5] == HWp and eng.H[5] == 57
    assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(loss).all())
    flat = tr.model.flat_grads()
    assert bool(torch.isfinite(flat).all())
    h1 = eng.debug_read("h1", count=n * HWp * 64).reshape(n, HWp, 64)[:, :HW].reshape(n, 57, 57, 64).transpose(0, 3, 1, 2).copy()
    dh1 = eng.debug_read("dh1", count=n * HWp * 64).reshape(n, HWp, 64)[:, :HW].reshape(n, 57, 57, 64).transpose(0, 3, 1, 2).copy()
    named = dict(tr.model.named_parameters())
    prm = {k: named[HEAD + k].detach().cpu() for k in ("conv1.weight", "norm1.weight", "norm1.bias")}
    grd = {k: named[HEAD + k].grad.detach().cpu().double() for k in prm}

    def head_tail(dtype):
        w = prm["conv1.weight"].to(dtype).requires_grad_(True)
        g = prm["norm1.weight"].to(dtype).requires_grad_(True)
        b = prm["norm1.bias"].to(dtype).requires_grad_(True)
        total, dys, qs = 0.0, [], []
        for j in range(n):          # the head runs once per pair: BatchNorm statistics per pair
            y = torch.nn.functional.batch_norm(torch.from_numpy(h1[j:j + 1]).to(dtype), None, None, g, b, True, 0.0, 1e-5)
            y.retain_grad()
            qj = torch.nn.functional.conv2d(torch.relu(y), w)
            total = total + huber_map(qj[0, 0], torch.from_numpy(lab[j]).to(dtype), torch.from_numpy(wgt[j]).to(dtype))
            dys.append(y)
            qs.append(qj.detach())
        total.backward()
        return {"dh1": torch.cat([y.grad for y in dys]).double(), "conv1.weight": w.grad.double(), "norm1.weight": g.grad.double(),
                "norm1.bias": b.grad.double()}, torch.cat(qs).double()

    t64, q64 = head_tail(torch.float64)
    t32, _ = head_tail(torch.float32)
    ok, worst = q_close(q.cpu().numpy().ravel(), q64.numpy().ravel(), what="S=1824 head alone")
    assert ok, worst
    mine = dict(grd, dh1=torch.from_numpy(dh1).double())
    bad = []
    for k in ("dh1", "conv1.weight", "norm1.weight", "norm1.bias"):
        nrm = float(t64[k].norm())
        e_p, e_o = float((mine[k] - t64[k]).norm()), float((t32[k] - t64[k]).norm())
        print("S=1824 head alone %-13s |err| %.3e  fp32-torch |err| %.3e  |g| %.3e  (%.2f of the 3x bound)" % (k, e_p, e_o, nrm, e_p / max(3 * e_o, 1e-300)))
        if not e_p <= 3.0 * e_o:
            bad.append(k)
    assert not bad, bad


def test_dense_head_backward_is_bit_reproducible(gpu):
    """Two identical train_batch_maps calls (zero learning rate, dense form): the value-convolution weight gradient - every element
    written by one thread, pairs in index order - bit for bit equal, dh1 too."""
    import synthetic
    tr = make_trainer('reinforcement', 3)
    depth, masks = synthetic.heightmap_scene(6, size=320)
    md = depth * masks[1]
    rots = [1, 6, 11]
    lab = synthetic.uniform(7, "det/lab", 300, -1.5, 2.5).reshape(3, 10, 10)
    eng = cached_engine(928, 1)
    HWp = eng.HWp[5]
    runs = []
    for it in range(2):
        tr.train_batch_maps(depth, md, 0, rots, lab)          # default "head_bwd" = 0: the mark selects the dense form
        g = dict(tr.model.named_parameters())[HEAD + "conv1.weight"].grad
        runs.append((g.clone(), eng.debug_read("dh1", count=3 * HWp * 64).copy()))
    assert float(runs[0][0].abs().max()) > 0
    assert_bit_identical(runs[0][0], runs[1][0])
    assert_bit_identical(runs[0][1], runs[1][1])


def test_forward_dense_and_best_dense_action(gpu):
    import synthetic
    tr = make_trainer('reinforcement', 4)
    depth, masks = synthetic.heightmap_scene(0)
    md = depth * masks[0]
    for kw in (dict(), dict(specific_rotation=7), dict(style=2), dict(style=1, is_target=True)):
        qd = tr.forward_dense(depth, md, **kw)
        qf = tr.forward(depth, md, is_volatile=True, **kw)
        assert qd.dtype == np.float64 and qd.shape == (len(qf), 1, 1)
        assert np.array_equal(qd[:, 0, 0], qf), kw
    assert tuple(tr.forward_dense(depth, md, return_device=True).shape) == (16, 1, 1)
    depth, masks = synthetic.heightmap_scene(8, size=240, n_boxes=8)
    md = depth * masks[0]
    with pytest.raises(NotImplementedError):
        tr.forward(depth, md, 0, True)                     # the scalar-per-rotation interface keeps its error
    for style in (0, 1):
        qd = tr.forward_dense(depth, md, style)
        assert qd.shape == (16, 3, 3)
        best = tr.best_dense_action(depth, md, style)
        r, oy, ox = np.unravel_index(np.argmax(qd), qd.shape)
        assert (best["rotation"], best["pixel"]) == (int(r), (int(oy), int(ox))), (best, r, oy, ox)
        assert best["conf"] == qd[r, oy, ox]
    one = tr.forward_dense(depth, md, 0, specific_rotation=4)
    assert one.shape == (1, 3, 3)
    ok, worst = q_close(one.ravel(), tr.forward_dense(depth, md, 0)[4].ravel(), what="S=704 rotation 4 alone vs in the sweep")
    assert ok, worst


def test_loss_map_refuses_a_three_class_head(gpu):
    """smg_loss_map on an engine with head_out == 3: -22, nothing launched (the outputs keep their fill)."""
    import smg_hip
    eng = cached_engine(640, 3)
    q = torch.zeros((1, 3, 1, 1), device="cuda")
    lab, loss, dq = torch.zeros((1, 1, 1, 1), device="cuda"), filled((1,)), filled((1, 3, 1, 1))
    rc = smg_hip.lib().smg_loss_map(eng.h, q.data_ptr(), lab.data_ptr(), None, 1, loss.data_ptr(), dq.data_ptr(), C.c_void_p(0))
    assert rc == -22
    assert b"head_out" in smg_hip.lib().smg_last_error()
    with pytest.raises(smg_hip.SmgError):
        eng.loss_map(q.data_ptr(), lab.data_ptr(), None, 1, loss.data_ptr(), dq.data_ptr(), None)
    torch.cuda.synchronize()
    assert float(loss[0]) == -7.0 and bool((dq == -7.0).all())
    with pytest.raises(smg_hip.SmgError):
        eng.set_option("head_bwd", 3)
