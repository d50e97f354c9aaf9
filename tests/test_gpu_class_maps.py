"""Dense class maps of the reactive method (heightmaps larger than 224^2) through the public interface, on the MI355X (run with
-m gpu): the whole-map cross entropy (smg_loss_map_ce) against torch's fp64 nll_loss on the same logits and against smg_loss
on a single labelled pixel, whole-map training with the dense and the per-element form of the 3-class head backward against the
fp64 PyTorch-CPU oracle, the config-5 geometry against an fp64 restatement of the head alone, run-to-run determinism,
train_batch_class_pixels against train_batch_class_maps, forward_class_maps / best_class_map_action against forward and
np.argmax, and the refusal of a one-channel head.

The reference criterion is CrossEntropyLoss2d (code/utils.py:306-313) with class weights {1, 1, 0} (code/trainer.py:38-60):
torch's weighted-mean nll_loss per sample.  Yardsticks are the parity suite's own (helpers.q_close,
helpers.grads_within_fp32_class: within 3x what fp32 costs PyTorch-CPU itself against an fp64 evaluation)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import grads_within_fp32_class, MEAN, STD, oracle_net, orc, q_close
from map_harness import assert_bit_identical, cached_engine, filled, gpu, HEAD, make_trainer, stream  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                          # one fp32 rounding, relative


def ce_map(q, y):
    """The reference criterion on a whole map: nll_loss(log_softmax(q, 1), y, weight = {1, 1, 0}), q [n, 3, H, W], y [n, H, W]."""
    w = torch.tensor([1.0, 1.0, 0.0], dtype=q.dtype)
    return F.nll_loss(F.log_softmax(q, dim=1), y, weight=w)


def loss_gate(q, y):
    """The fp32 gate of one pair's loss (see test_loss_map_ce_kernel_vs_torch_fp64): 32 x 2^-24 x (sum over the labelled pixels
    of B_p) / W with B_p = 2 max_c |q[c, p]| + log 3, which bounds every intermediate of the pixel.  q [3, H, W], y [H, W] numpy."""
    lab = y.reshape(-1) < 2
    B = 2.0 * np.abs(q.reshape(3, -1).astype(np.float64)).max(axis=0) + np.log(3.0)
    return 32 * U * B[lab].sum() / max(int(lab.sum()), 1)


def rel_dist(a, b):
    a, b = a.double().cpu().numpy().ravel(), b.double().cpu().numpy().ravel()
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b * b).sum()), 1e-300))


def test_loss_map_ce_kernel_vs_torch_fp64(gpu):
    """smg_loss_map_ce alone on an S = 928 engine (10 x 10 maps), three pairs of seeded logits N(0, std 2): pair 0 with mixed
    classes, pair 1 with one labelled pixel, pair 2 all class 2 - against torch's fp64 nll_loss(log_softmax) with weights
    {1, 1, 0} on the same logits, per pair.  Pair 2 gives loss 0 and dq 0 where torch gives 0/0 = NaN (the documented deviation:
    asserted, not compared).  Every class-2 pixel has dq exactly 0 in all three channels - also when its logits are inf.

    Gates, counted in fp32 roundings of 2^-24 (expf and logf are 1-ulp functions: two roundings each), not fitted to a result.
    Loss: q - max (1), expf (2), the sum of three exponentials (2), logf (2), + max (1), - q[y] (1), the thread's strided sum
    (1; with 100 < 256 pixels it adds to zero), eight levels of the LDS tree (8), the division by W (1): 19, gate 32.  Every
    intermediate of pixel p (q - max, log of the sum <= log 3, the log-sum-exp, q[y], the term itself) is at most
    B_p = 2 max_c |q[c, p]| + log 3 in magnitude, and a relative error u of an exponential moves the log of their sum by at most
    u <= u B_p; so |loss - truth| <= 32 x 2^-24 x sum_p B_p / W.
    dq: q - max and expf (3; the error of q - max moves an exponential e^-x by x e^-x u <= u / e), the sum (3 + 2 = 5), their
    quotient (3 + 5 + 1 = 9), - [c == y] (10), 1 / W (11), the product (12): gate 16 x 2^-24 / W per element (softmax and
    softmax - onehot are at most 1 in magnitude)."""
    eng = cached_engine(928, 3)
    assert (eng.OH, eng.OW) == (10, 10)
    g = torch.Generator().manual_seed(11)
    q = (2.0 * torch.randn((3, 3, 10, 10), generator=g)).float()
    y = torch.full((3, 10, 10), 2, dtype=torch.int64)
    y[0] = torch.randint(0, 3, (10, 10), generator=g)
    y[1, 6, 3] = 1
    assert sorted(np.unique(y[0].numpy())) == [0, 1, 2]

    def run(qh):
        qd, lab = qh.cuda(), y.float().reshape(3, 1, 10, 10).cuda()
        loss, dq = filled((3,)), filled(qd.shape)
        eng.loss_map_ce(qd.data_ptr(), lab.data_ptr(), 3, loss.data_ptr(), dq.data_ptr(), stream())
        torch.cuda.synchronize()
        return loss.cpu(), dq.cpu()

    loss, dq = run(q)
    for j in (0, 1):
        q64 = q[j:j + 1].double().requires_grad_(True)
        ref = ce_map(q64, y[j:j + 1])
        ref.backward()
        W = int((y[j] < 2).sum())
        gate = loss_gate(q[j].numpy(), y[j].numpy())
        err = abs(float(loss[j]) - float(ref.detach()))
        derr = float((dq[j].double() - q64.grad[0]).abs().max())
        print("pair %d: W %d, loss %.7f, fp64 %.7f: |d| %.2e (gate %.2e); max |d dq| %.2e (gate %.2e)"
              % (j, W, float(loss[j]), float(ref.detach()), err, gate, derr, 16 * U / W))
        assert err <= gate
        assert derr <= 16 * U / W
        masked = (y[j] == 2)[None].expand(3, 10, 10)
        assert bool((dq[j][masked] == 0).all()) and bool((dq[j][~masked] != 0).all())
    # no labelled pixel: torch's weighted mean is 0/0, the kernel gives loss 0 and no gradient
    assert bool(torch.isnan(ce_map(q[2:3].double(), y[2:3])))
    assert float(loss[2]) == 0.0 and bool((dq[2] == 0).all())
    # a class-2 pixel masks its logits whatever they hold
    q_inf = q.clone()
    p2 = torch.nonzero(y[0] == 2)[0]
    q_inf[0, 0, p2[0], p2[1]], q_inf[0, 1, p2[0], p2[1]], q_inf[0, 2, p2[0], p2[1]] = float("inf"), float("nan"), -float("inf")
    loss_i, dq_i = run(q_inf)
    assert_bit_identical(loss_i, loss)
    assert_bit_identical(dq_i, dq)


def test_one_weighted_pixel_equals_smg_loss_mode_1(gpu):
    """At S = 640 the map is one pixel: smg_loss_map_ce's loss and dq on labels 0 and 1 are bit-identical to smg_loss mode 1's
    (W = 1: x / 1 and 1 * x are exact, the per-pixel arithmetic is the same operation for operation)."""
    eng = cached_engine(640, 3)
    assert (eng.OH, eng.OW) == (1, 1)
    g = torch.Generator().manual_seed(12)
    q = (2.0 * torch.randn((2, 3, 1, 1), generator=g)).float().cuda()
    lab = torch.tensor([0.0, 1.0], device="cuda")
    out = []
    for use_map in (False, True):
        loss, dq = filled((2,), -1.0), filled(q.shape, -1.0)
        if use_map:
            eng.loss_map_ce(q.data_ptr(), lab.reshape(2, 1, 1, 1).data_ptr(), 2, loss.data_ptr(), dq.data_ptr(), stream())
        else:
            eng.loss(1, q.data_ptr(), lab.data_ptr(), 2, loss.data_ptr(), dq.data_ptr(), stream())
        out.append((loss, dq))
    assert_bit_identical(out[0][0], out[1][0])
    assert_bit_identical(out[0][1], out[1][1])
    assert bool((out[1][0] > 0).all()) and bool((out[1][1] != 0).all())


def test_whole_class_map_training_vs_fp64_oracle_s928(gpu):
    """A 320^2 heightmap -> S = 928: 10 x 10 class maps over ragged 29^2 feature planes.  One sample (style 0, rotation 3),
    labels floor(U(0, 3)): 32 / 38 / 30 pixels of class 0 / 1 / 2; on the fp32 oracle the logits span -2.71 .. 3.40 and the
    largest softmax probability is 0.983 (not saturated), the loss is 1.5990996 in fp32 and 1.5990991 in fp64.  Logits by
    q_close, the loss within the gate of test_loss_map_ce_kernel_vs_torch_fp64 of the fp64 criterion on the product's OWN
    logits, all 368 gradient tensors within 3x the fp32 oracle's own error against fp64 (three outliers below 5 % of their
    norm: the reference's own second fp32 evaluation with another thread count needs one, conv0.weight at 2.4 %) - for the
    dense head backward ("head_bwd" = 2) and for the per-element one (= 1) on the same dq."""
    import synthetic
    style, rot = 0, 3
    depth, masks = synthetic.heightmap_scene(6, size=320)
    md = depth * masks[0]
    x = orc.preprocess(depth, [MEAN] * 3, [STD] * 3)
    mx = orc.preprocess(md, [MEAN] * 3, [STD] * 3)
    assert x.shape[-1] == 928
    lab = np.minimum(np.floor(synthetic.uniform(3, "cls/lab", 100, 0, 3)), 2).astype(np.int64).reshape(1, 10, 10)
    assert [int((lab == c).sum()) for c in range(3)] == [32, 38, 30]
    y = torch.from_numpy(lab)

    on = oracle_net(1, 3)
    rx = orc.rotate(x, rot, 16)
    o64 = copy.deepcopy(on).double()
    trunk, head = getattr(o64, orc.STYLE_TRUNK[style]).features, getattr(o64, orc.STYLE_HEAD[style])
    q64 = head(torch.cat((trunk(rx.double()), trunk(mx.double())), 1))
    assert tuple(q64.shape) == (1, 3, 10, 10)
    loss64 = ce_map(q64, y)
    loss64.backward()
    g64 = {n: p.grad for n, p in o64.named_parameters() if p.grad is not None}
    on.zero_grad()
    qo = orc.forward(on, x, mx, style, False, rot)
    loss32 = ce_map(qo, y)
    print("fp32 oracle: logits %.2f .. %.2f, largest softmax probability %.3f, loss %.7f (fp64 %.7f)"
          % (float(qo.detach().min()), float(qo.detach().max()), float(torch.softmax(qo.detach(), 1).max()), float(loss32.detach()), float(loss64.detach())))
    loss32.backward()

    tr = make_trainer('reactive', 1)
    eng = cached_engine(928, 3)
    head_names = [HEAD + "conv1.weight", HEAD + "norm1.weight", HEAD + "norm1.bias"]
    got = {}
    try:
        for form in (2, 1):
            eng.set_option("head_bwd", form)
            loss, q = tr.train_batch_class_maps(depth, md, style, [rot], lab, return_q=True)
            assert tuple(q.shape) == (1, 3, 10, 10) and tuple(loss.shape) == (1,)
            qh = q.cpu()
            ok, worst = q_close(qh.numpy().astype(np.float64).ravel(), q64.detach().numpy().ravel(), what="S=928 classes head_bwd=%d" % form)
            assert ok, worst
            own = float(ce_map(qh.double(), y))
            gate = loss_gate(qh[0].numpy(), lab[0])
            err = abs(float(loss.cpu().numpy()[0]) - own)
            print("head_bwd=%d: loss %.7f, fp64 criterion on the same logits %.7f: |d| %.2e (gate %.2e); fp64 oracle loss %.7f"
                  % (form, float(loss[0]), own, err, gate, float(loss64)))
            assert err <= gate
            rel_p, _, _ = grads_within_fp32_class(tr.model.named_parameters(), on.named_parameters(), g64, 3.0, "S=928 class maps head_bwd=%d" % form,
                                                  max_outliers=3, outlier_cap=0.05)
            assert len(rel_p) == 368
            named = dict(tr.model.named_parameters())
            got[form] = {n: named[n].grad.clone() for n in head_names}
    finally:
        eng.set_option("head_bwd", 0)
    for n in head_names:
        print("dense vs per-element form, %-40s |d| / |g| = %.3e" % (n, rel_dist(got[2][n], got[1][n])))


def test_config5_geometry_three_class_head_alone_vs_fp64(gpu):
    """A 640^2 heightmap -> S = 1824: two rotations, 38 x 38 class maps over 57^2 planes (3249 pixels in 3264 padded rows), labels
    of all three classes, the dense form - the smallest shape whose data pass holds more than 64 KB of LDS (3 x 76 x 76 floats).
    Shapes and finiteness; then the head ALONE: from the engine's own h1 the chain BN(train) + ReLU -> 20x20 convolution 64 -> 3
    -> map cross entropy is rebuilt with torch in fp64 (the truth) and in fp32, and the engine's dh1 and its gradients of
    conv1.weight [3, 64, 20, 20], norm1.weight and norm1.bias must lie within 3x the fp32 evaluation's own error."""
    import synthetic
    tr = make_trainer('reactive', 0, R=32)
    depth, masks = synthetic.heightmap_scene(4, size=640, n_boxes=8)
    md = depth * masks[0]
    rots = [5, 6]
    n, side, HW, HWp = len(rots), 38, 57 * 57, 3264
    lab = np.minimum(np.floor(synthetic.uniform(5, "cls5/lab", n * side * side, 0, 3)), 2).astype(np.int64).reshape(n, side, side)
    assert all((lab[j] == c).any() for j in range(n) for c in range(3))
    eng = cached_engine(1824, 3)
    eng.set_option("head_bwd", 2)
    try:
        loss, q = tr.train_batch_class_maps(depth, md, 0, rots, lab, return_q=True)
    finally:
        eng.set_option("head_bwd", 0)
    assert tuple(q.shape) == (n, 3, side, side) and tuple(loss.shape) == (n,)
    assert eng.HWp[5] == HWp and eng.H[5] == 57
    assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(loss).all())
    flat = tr.model.flat_grads()
    assert bool(torch.isfinite(flat).all())
    h1 = eng.debug_read("h1", count=n * HWp * 64).reshape(n, HWp, 64)[:, :HW].reshape(n, 57, 57, 64).transpose(0, 3, 1, 2).copy()
    dh1 = eng.debug_read("dh1", count=n * HWp * 64).reshape(n, HWp, 64)[:, :HW].reshape(n, 57, 57, 64).transpose(0, 3, 1, 2).copy()
    named = dict(tr.model.named_parameters())
    prm = {k: named[HEAD + k].detach().cpu() for k in ("conv1.weight", "norm1.weight", "norm1.bias")}
    assert tuple(prm["conv1.weight"].shape) == (3, 64, 20, 20)
    grd = {k: named[HEAD + k].grad.detach().cpu().double() for k in prm}

    def head_tail(dtype):
        w = prm["conv1.weight"].to(dtype).requires_grad_(True)
        g = prm["norm1.weight"].to(dtype).requires_grad_(True)
        b = prm["norm1.bias"].to(dtype).requires_grad_(True)
        total, dys, qs = 0.0, [], []
        for j in range(n):          # the head runs once per pair: BatchNorm statistics per pair
            yj = F.batch_norm(torch.from_numpy(h1[j:j + 1]).to(dtype), None, None, g, b, True, 0.0, 1e-5)
            yj.retain_grad()
            qj = F.conv2d(torch.relu(yj), w)
            total = total + ce_map(qj, torch.from_numpy(lab[j:j + 1]))
            dys.append(yj)
            qs.append(qj.detach())
        total.backward()
        return {"dh1": torch.cat([v.grad for v in dys]).double(), "conv1.weight": w.grad.double(), "norm1.weight": g.grad.double(),
                "norm1.bias": b.grad.double()}, torch.cat(qs).double()

    t64, q64 = head_tail(torch.float64)
    t32, _ = head_tail(torch.float32)
    ok, worst = q_close(q.cpu().numpy().ravel(), q64.numpy().ravel(), what="S=1824 3-class head alone")
    assert ok, worst
    mine = dict(grd, dh1=torch.from_numpy(dh1).double())
    bad = []
    for k in ("dh1", "conv1.weight", "norm1.weight", "norm1.bias"):
        nrm = float(t64[k].norm())
        e_p, e_o = float((mine[k] - t64[k]).norm()), float((t32[k] - t64[k]).norm())
        print("S=1824 3-class head alone %-13s |err| %.3e  fp32-torch |err| %.3e  |g| %.3e  (%.2f of the 3x bound)" % (k, e_p, e_o, nrm, e_p / max(3 * e_o, 1e-300)))
        if not e_p <= 3.0 * e_o:
            bad.append(k)
    assert not bad, bad


def test_class_map_training_is_bit_reproducible(gpu):
    """Two identical train_batch_class_maps calls (zero learning rate, three rotations at S = 928, the default "head_bwd" = 0): the
    value-convolution weight gradient [3, 64, 20, 20] - every element written by one thread, pairs in index order - bit for bit
    equal and not zero, dh1 too."""
    import synthetic
    tr = make_trainer('reactive', 3)
    depth, masks = synthetic.heightmap_scene(6, size=320)
    md = depth * masks[1]
    rots = [1, 6, 11]
    lab = np.minimum(np.floor(synthetic.uniform(7, "clsdet/lab", 300, 0, 3)), 2).reshape(3, 10, 10)
    eng = cached_engine(928, 3)
    HWp = eng.HWp[5]
    runs = []
    for it in range(2):
        tr.train_batch_class_maps(depth, md, 0, rots, lab)
        g = dict(tr.model.named_parameters())[HEAD + "conv1.weight"].grad
        runs.append((g.clone(), eng.debug_read("dh1", count=3 * HWp * 64).copy()))
    assert tuple(runs[0][0].shape) == (3, 64, 20, 20)
    assert all(float(runs[0][0][o].abs().max()) > 0 for o in range(3))
    assert_bit_identical(runs[0][0], runs[1][0])
    assert_bit_identical(runs[0][1], runs[1][1])


def test_train_batch_class_pixels_equals_train_batch_class_maps(gpu):
    """One labelled pixel per sample is a label map of class 2 with that one entry: loss and logits bit-identical (240^2 heightmap,
    3 x 3 maps, two samples, one per class)."""
    import synthetic
    tr = make_trainer('reactive', 2)
    depth, masks = synthetic.heightmap_scene(8, size=240, n_boxes=8)
    md = depth * masks[0]
    rots, pixels, labels = [5, 9], [(2, 1), (0, 2)], [0, 1]
    maps = np.full((2, 3, 3), 2.0)
    for k, ((oy, ox), c) in enumerate(zip(pixels, labels)):
        maps[k, oy, ox] = c
    loss_a, q_a = tr.train_batch_class_maps(depth, md, 0, rots, maps, return_q=True)
    loss_b, q_b = tr.train_batch_class_pixels(depth, md, 0, rots, pixels, labels, return_q=True)
    assert tuple(q_a.shape) == (2, 3, 3, 3)
    assert_bit_identical(q_a, q_b)
    assert_bit_identical(loss_a, loss_b)
    assert bool((loss_a > 0).all())
    # ... and the value is the cross entropy of that one pixel
    for k, ((oy, ox), c) in enumerate(zip(pixels, labels)):
        ref = float(-torch.log_softmax(q_a[k, :, oy, ox].double().cpu(), 0)[c])
        assert abs(float(loss_a[k]) - ref) <= 32 * U * (2 * float(q_a[k, :, oy, ox].abs().max()) + np.log(3.0))


def test_forward_class_maps_and_best_class_map_action(gpu):
    import synthetic
    tr = make_trainer('reactive', 4)
    depth, masks = synthetic.heightmap_scene(0)
    md = depth * masks[0]
    p = tr.forward_class_maps(depth, md)
    assert p.dtype == np.float64 and p.shape == (16, 3, 1, 1)
    assert p[0, 0, 0, 0] == tr.forward(depth, md, 0, is_volatile=True)
    assert tuple(tr.forward_class_maps(depth, md, return_device=True).shape) == (16, 3, 1, 1)
    assert tr.forward_class_maps(depth, md, specific_rotation=7).shape == (1, 3, 1, 1)
    depth, masks = synthetic.heightmap_scene(8, size=240, n_boxes=8)
    md = depth * masks[0]
    for style in (0, 1):
        p = tr.forward_class_maps(depth, md, style)
        assert p.shape == (16, 3, 3, 3)
        assert float(np.abs(p.sum(axis=1) - 1.0).max()) <= 4 * U
        z = tr.forward_class_maps(depth, md, style, logits=True)
        assert z.shape == (16, 3, 3, 3)
        # (the device softmax in fp32 against an fp64 softmax of the same logits: 9 roundings up to the quotient, see the dq gate above)
        assert float(np.abs(torch.softmax(torch.from_numpy(z), 1).numpy() - p).max()) <= 16 * U
        best = tr.best_class_map_action(depth, md, style)
        r, oy, ox = np.unravel_index(np.argmax(p[:, 0]), p[:, 0].shape)
        assert (best["rotation"], best["pixel"]) == (int(r), (int(oy), int(ox))), (best, r, oy, ox)
        assert best["conf"] == p[r, 0, oy, ox]


def test_loss_map_ce_refuses_a_one_channel_head(gpu):
    """smg_loss_map_ce on an engine with head_out == 1: -22, nothing launched (the outputs keep their fill)."""
    import smg_hip
    eng = cached_engine(640, 1)
    q = torch.zeros((1, 1, 1, 1), device="cuda")
    lab, loss, dq = torch.zeros((1, 1, 1, 1), device="cuda"), filled((1,)), filled((1, 3, 1, 1))
    rc = smg_hip.lib().smg_loss_map_ce(eng.h, q.data_ptr(), lab.data_ptr(), 1, loss.data_ptr(), dq.data_ptr(), C.c_void_p(0))
    assert rc == -22
    assert b"head_out" in smg_hip.lib().smg_last_error()
    with pytest.raises(smg_hip.SmgError):
        eng.loss_map_ce(q.data_ptr(), lab.data_ptr(), 1, loss.data_ptr(), dq.data_ptr(), None)
    torch.cuda.synchronize()
    assert float(loss[0]) == -7.0 and bool((dq == -7.0).all())
