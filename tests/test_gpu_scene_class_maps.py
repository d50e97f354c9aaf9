"""The reactive net's class maps in the scene frame on the MI355X (run with -m gpu): smg_scene_class_maps / smg_scene_class_argmax /
smg_loss_scene_ce on an engine alone with synthetic logits N(0, std 2) against the fp64 restatement of tests/scene_class_ref.py
(probabilities to one fp32 rounding, the validity mask, np.argmax over the kernel's own maps, torch fp64 autograd for the loss),
their refusals, then train_batch_scene_class_pixels against the fp64 PyTorch-CPU oracle and forward_scene_class_maps /
best_scene_class_action against the trainer's own logits pushed through scene_class_ref."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import orc
from map_harness import assert_bit_identical, assert_train_batch_runs, cached_engine, filled, gpu, HEAD, make_trainer, s704_scene, stream  # noqa: F401

import scene_class_ref
import scene_ref

pytestmark = pytest.mark.gpu

SHAPES = ((240, 704, 3), (320, 928, 10))
FILL = 7.0


def affines(R=16, rots=None):
    return np.stack([scene_ref.theta(r, R) for r in (range(R) if rots is None else rots)])


def logits(seed, n, side):
    return (2.0 * np.random.default_rng(seed).standard_normal((n, 3, side, side))).astype(np.float32)


def gpu_class_maps(eng, q, aff, hm, cls):
    n = len(aff)
    out = filled((n, 3, hm, hm) if cls < 0 else (n, hm, hm), FILL)
    eng.scene_class_maps(q.data_ptr(), n, aff, hm, cls, out.data_ptr(), stream())
    return out.cpu().numpy()


def gpu_class_argmax(eng, q, aff, hm, cls):
    idx = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    val = filled((1,), -5.0)
    eng.scene_class_argmax(q.data_ptr(), len(aff), aff, hm, cls, idx.data_ptr(), val.data_ptr(), stream())
    return int(idx.cpu().numpy()[0]), val.cpu().numpy()[0]


def check_class_maps(got, q_host, aff, hm, what):
    """got [n, 3, hm, hm] against scene_class_ref: the validity mask on every pixel farther than 1e-6 from a boundary (at most 0.1 %
    excluded), -inf outside in all three planes, on valid pixels |gpu - ref| <= 2^-23 max(|ref|, 2^-126) - the single rounding of an
    fp64 result, check_maps' gate - and the three planes summing to 1 within 3 x 2^-24 (three roundings of 2^-24 P_c each)."""
    ref, valid, margin = scene_class_ref.scene_class_maps(q_host, aff, hm)
    sure = margin > 1e-6
    print("%s: %d of %d pixels within 1e-6 of a validity boundary; %d valid" % (what, int((~sure).sum()), sure.size, int(valid.sum())))
    assert (~sure).mean() <= 1e-3
    gv = ~np.isneginf(got)
    assert np.array_equal(gv[:, 0], gv[:, 1]) and np.array_equal(gv[:, 0], gv[:, 2])
    assert np.array_equal(gv[:, 0][sure], valid[sure])
    both = np.broadcast_to((gv[:, 0] & valid)[:, None], got.shape)
    err = np.abs(got[both].astype(np.float64) - ref[both])
    tol = 2.0 ** -23 * np.maximum(np.abs(ref[both]), 2.0 ** -126)
    print("%s: max |gpu - ref| / tol = %.3f" % (what, float((err / tol).max())))
    assert (err <= tol).all()
    total = np.moveaxis(got.astype(np.float64), 1, -1)[gv[:, 0]].sum(axis=1)
    print("%s: max |sum of the planes - 1| = %.3e (gate %.3e)" % (what, float(np.abs(total - 1.0).max()), 3 * 2.0 ** -24))
    assert (np.abs(total - 1.0) <= 3 * 2.0 ** -24).all()
    return ref, valid


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_scene_class_maps_against_fp64(gpu, hm, S, side):
    assert scene_ref.geometry(hm)[1:] == (S, side)
    eng = cached_engine(S, 3)
    aff = affines()
    qh = logits(S, 16, side)
    q = torch.from_numpy(qh).cuda()
    got = gpu_class_maps(eng, q, aff, hm, -1)
    check_class_maps(got, qh, aff, hm, "S=%d" % S)
    for cls in range(3):      # each single-cls output is its plane of the cls = -1 output, bit for bit
        one = gpu_class_maps(eng, q, aff, hm, cls)
        assert np.array_equal(one.view(np.uint32), got[:, cls].view(np.uint32)), cls


def test_scene_class_maps_with_an_odd_group_of_maps_and_an_unaligned_output(gpu):
    """More maps than one launch carries (33 > 32, the second launch starts at map 32) written to outputs that are 4 bytes off
    16-byte alignment: the guarded 4-byte stores instead of the 16-byte ones, the same values; the floats before and after stay."""
    hm, S, side = 240, 704, 3
    eng = cached_engine(S, 3)
    aff = affines(33)
    qh = logits(5, 33, side)
    q = torch.from_numpy(qh).cuda()
    n = 33 * 3 * hm * hm
    buf = filled((n + 2,), FILL)
    out = buf[1:1 + n]
    assert out.data_ptr() % 16 == 4
    eng.scene_class_maps(q.data_ptr(), 33, aff, hm, -1, out.data_ptr(), stream())
    got = out.cpu().numpy().reshape(33, 3, hm, hm)
    check_class_maps(got, qh, aff, hm, "33 maps, unaligned")
    assert float(buf[0]) == FILL and float(buf[-1]) == FILL
    buf1 = filled((n // 3 + 2,), FILL)
    out1 = buf1[1:1 + n // 3]
    assert out1.data_ptr() % 16 == 4
    eng.scene_class_maps(q.data_ptr(), 33, aff, hm, 1, out1.data_ptr(), stream())
    assert np.array_equal(out1.cpu().numpy().reshape(33, hm, hm).view(np.uint32), got[:, 1].view(np.uint32))
    assert float(buf1[0]) == FILL and float(buf1[-1]) == FILL


def loss_reference(qh, aff, hm, pix, lab):
    """fp64 autograd over scene_class_ref.scene_class_loss, per pair: (loss [n], dq [n, 3, OH, OW])."""
    losses, grads = [], []
    for j in range(len(qh)):
        qj = torch.from_numpy(qh[j]).double().requires_grad_(True)
        loss = scene_class_ref.scene_class_loss(qj, aff[j], hm, pix[j], lab[j])
        loss.backward()
        losses.append(float(loss.detach())); grads.append(qj.grad.numpy())
    return np.asarray(losses), np.stack(grads)


def gpu_loss(eng, qh, aff, hm, pix, lab):
    n, K = lab.shape
    q = torch.from_numpy(qh).cuda()
    pix_d, lab_d = torch.from_numpy(pix.astype(np.int32)).cuda(), torch.from_numpy(lab.astype(np.float32)).cuda()
    loss, dq = filled((n,), -FILL), filled(q.shape, -FILL)
    eng.loss_scene_ce(q.data_ptr(), aff, hm, n, K, pix_d.data_ptr(), lab_d.data_ptr(), loss.data_ptr(), dq.data_ptr(), stream())
    return loss.cpu().numpy(), dq.cpu().numpy()


def check_loss(got, ref, what):
    """Double arithmetic and one final rounding: loss within 2^-23 |ref loss|, every dq element within 2^-23 max|ref dq|, dq exactly 0
    where the reference is 0."""
    (loss, dq), (ref_loss, ref_dq) = got, ref
    print("%s: loss %s ref %s; max |d dq| %.2e, max |dq| %.2e" % (what, loss, ref_loss, np.abs(dq - ref_dq).max(), np.abs(ref_dq).max()))
    assert (np.abs(loss - ref_loss) <= 2.0 ** -23 * np.abs(ref_loss)).all()
    assert np.abs(dq - ref_dq).max() <= 2.0 ** -23 * np.abs(ref_dq).max()
    assert (dq[ref_dq == 0] == 0).all()


def draw_valid(rng, hm, aff, lo, hi, away_from=(), side=None):
    """A heightmap pixel in [lo, hi)^2 that is valid (margin > 1e-3) for `aff` and whose cell lies two or more from every cell in `away_from`."""
    while True:
        p = rng.integers(lo, hi, size=2)
        qy, qx, valid, margin = scene_ref.map_coords(hm, aff, p[0], p[1])
        if not valid or margin <= 1e-3:
            continue
        if side is not None:
            y0, x0 = (int(v) for v in scene_ref.corners(qy, qx, side)[:2])
            if any(max(abs(y0 - ya), abs(x0 - xa)) < 2 for ya, xa in away_from):
                continue
        return p


def cell_of(hm, aff, p, side):
    qy, qx = scene_ref.map_coords(hm, aff, p[0], p[1])[:2]
    return tuple(int(v) for v in scene_ref.corners(qy, qx, side)[:2])


def test_config5_geometry_maps_and_loss(gpu):
    """A 640^2 heightmap -> S = 1824, 38 x 38 maps, rotations 3 and 20 of 32: all three planes against the reference, and
    smg_loss_scene_ce with K = 300 points per pair (more than 256: the point loop runs twice; 38 x 38 is where three planes of
    double accumulators press on the LDS) - classes 0 / 1 / 2 mixed, duplicates, some points without a window."""
    hm, S, side = 640, 1824, 38
    assert scene_ref.geometry(hm)[1:] == (S, side)
    eng = cached_engine(S, 3)
    aff = affines(32, (3, 20))
    qh = logits(S, 2, side)
    got = gpu_class_maps(eng, torch.from_numpy(qh).cuda(), aff, hm, -1)
    check_class_maps(got, qh, aff, hm, "S=1824")
    rng = np.random.default_rng(17)
    K = 300
    pix = rng.integers(0, hm, size=(2, K, 2))
    lab = rng.integers(0, 3, size=(2, K))
    pix[:, 270:] = pix[:, 100:130]                       # duplicates across the two passes of the point loop, with labels of their own
    valid = np.stack([scene_ref.map_coords(hm, aff[j], pix[j, :, 0], pix[j, :, 1])[2] for j in range(2)])
    counted = valid & (lab < 2)
    print("S=1824 loss: %s points count per pair, %s lie outside every window" % (counted.sum(axis=1), (~valid).sum(axis=1)))
    assert (counted.sum(axis=1) > 100).all() and ((~valid) & (lab < 2)).any()
    ref = loss_reference(qh, aff, hm, pix, lab)
    assert int((ref[1] != 0).sum()) > 3 * 300
    runs = [gpu_loss(eng, qh, aff, hm, pix, lab) for _ in range(2)]
    check_loss(runs[0], ref, "S=1824 K=300")
    assert_bit_identical(runs[0][0], runs[1][0])
    assert_bit_identical(runs[0][1], runs[1][1])


def test_scene_class_argmax(gpu):
    """33 maps (the second launch group carries the first's result) at hm 240."""
    hm, S, side = 240, 704, 3
    eng = cached_engine(S, 3)
    aff = affines(33)
    qh = logits(S + 7, 33, side)
    q = torch.from_numpy(qh).cuda()
    for cls in (0, 2):
        flat = gpu_class_maps(eng, q, aff, hm, cls).ravel()
        i, v = gpu_class_argmax(eng, q, aff, hm, cls)
        assert i == int(np.argmax(flat)) and v.view(np.uint32) == flat[i].view(np.uint32), (cls, i, v)
        i2, v2 = gpu_class_argmax(eng, q, aff, hm, cls)      # two calls, one result
        assert i2 == i and v2.view(np.uint32) == v.view(np.uint32)
    # constant logits: every valid value ties at the float32 nearest 1/3, the lowest valid flattened index wins
    qc = torch.full((33, 3, side, side), 0.375, dtype=torch.float32, device="cuda")
    third = np.float32(1.0 / 3.0)
    flat = gpu_class_maps(eng, qc, aff, hm, 0).ravel()
    assert set(np.unique(flat).tolist()) == {-np.inf, float(third)}
    i, v = gpu_class_argmax(eng, qc, aff, hm, 0)
    assert i == int(np.flatnonzero(flat == third)[0]) == int(np.argmax(flat)) and v == third
    # a NaN logit in map 9 wins (the first NaN of the flattened maps), and it lies in map 9
    qn = q.clone()
    qn[9, 1, side // 2, side // 2] = float("nan")
    flat = gpu_class_maps(eng, qn, aff, hm, 0).ravel()
    assert np.isnan(flat).any()
    i, v = gpu_class_argmax(eng, qn, aff, hm, 0)
    assert i == int(np.argmax(flat)) == int(np.flatnonzero(np.isnan(flat))[0]) and np.isnan(v)
    assert i // (hm * hm) == 9


def test_loss_scene_ce_against_torch_fp64_autograd(gpu):
    """S = 928, 4 pairs (rotations 0, 3, 8, 13 of 16), K = 6: a class-0, a class-1 and a class-0/1 point around the centre, a
    duplicate of the second, a class-2 point, and a class-0 point at heightmap corner (0, 0), outside every window, which must
    neither contribute nor count (W = 4).  Then: a pair whose points are all class 2 gives loss 0 and dq 0; inf / NaN in the
    corner logits under a class-2 point change nothing, bit for bit."""
    hm, S, side = 320, 928, 10
    eng = cached_engine(S, 3)
    rots = [0, 3, 8, 13]
    aff = affines(16, rots)
    rng = np.random.default_rng(11)
    qh = logits(11, 4, side)
    K = 6
    pix = np.empty((4, K, 2), dtype=np.int64)
    lab = np.empty((4, K), dtype=np.int64)
    for j in range(4):
        for k in range(3):
            pix[j, k] = draw_valid(rng, hm, aff[j], 100, 220)
        pix[j, 3] = pix[j, 1]                                                                       # a duplicate
        pix[j, 4] = draw_valid(rng, hm, aff[j], 100, 220, [cell_of(hm, aff[j], p, side) for p in pix[j, :3]], side)      # class 2, corners of its own
        pix[j, 5] = (0, 0)
        assert not scene_ref.map_coords(hm, aff[j], 0, 0)[2]
        lab[j] = (0, 1, rng.integers(0, 2), 1, 2, 0)
    ref = loss_reference(qh, aff, hm, pix, lab)
    assert (ref[0] > 0).all() and all(0 < int((ref[1][j] != 0).sum()) <= 3 * 3 * 4 for j in range(4))
    # (W = 4, not 5: the corner point does not count.  With it counted the loss would be 4/5 of the reference.)
    runs = [gpu_loss(eng, qh, aff, hm, pix, lab) for _ in range(2)]
    check_loss(runs[0], ref, "S=928 K=6")
    assert_bit_identical(runs[0][0], runs[1][0])
    assert_bit_identical(runs[0][1], runs[1][1])
    # pair 2 all class 2: loss 0, dq 0; the other pairs as before
    lab2 = lab.copy()
    lab2[2] = 2
    loss2, dq2 = gpu_loss(eng, qh, aff, hm, pix, lab2)
    assert loss2[2] == 0.0 and (dq2[2] == 0).all()
    keep = [0, 1, 3]
    assert np.array_equal(loss2[keep].view(np.uint32), runs[0][0][keep].view(np.uint32)) and np.array_equal(dq2[keep].view(np.uint32), runs[0][1][keep].view(np.uint32))
    # non-finite logits under the class-2 point only
    qi = qh.copy()
    for j in range(4):
        y0, x0 = cell_of(hm, aff[j], pix[j, 4], side)
        qi[j, 0, y0, x0], qi[j, 1, y0, x0 + 1], qi[j, 2, y0 + 1, x0], qi[j, 0, y0 + 1, x0 + 1] = np.inf, np.nan, -np.inf, np.nan
    loss_i, dq_i = gpu_loss(eng, qi, aff, hm, pix, lab)
    assert np.array_equal(loss_i.view(np.uint32), runs[0][0].view(np.uint32)) and np.array_equal(dq_i.view(np.uint32), runs[0][1].view(np.uint32))


def test_scene_class_entry_points_refuse(gpu):
    """-22 and nothing launched (the outputs keep their fill): a one-channel engine (the message names head_out), a heightmap side
    that does not pad to the engine's S, a 1 x 1 map, n_maps < 1, K < 1, cls out of range (-1 included for the argmax), an affine
    matrix with a translation."""
    import smg_hip
    L = smg_hip.lib()
    aff = affines()
    ap = aff.ctypes.data_as(C.POINTER(C.c_float))
    q = torch.zeros((16, 3, 3, 3), device="cuda")
    out = filled((16, 3, 240, 240), FILL)
    idx, val = torch.full((1,), -5, dtype=torch.int32, device="cuda"), filled((1,), -5.0)
    pix = torch.full((1, 1, 2), 120, dtype=torch.int32, device="cuda")
    lab, loss, dq = torch.zeros((1, 1), device="cuda"), filled((1,), -FILL), filled((1, 3, 3, 3), -FILL)

    def maps(e, n, a, hm, cls):
        return L.smg_scene_class_maps(e.h, q.data_ptr(), n, a, hm, cls, out.data_ptr(), None)

    def argmax(e, n, a, hm, cls):
        return L.smg_scene_class_argmax(e.h, q.data_ptr(), n, a, hm, cls, idx.data_ptr(), val.data_ptr(), None)

    def ce(e, a, hm, n, K):
        return L.smg_loss_scene_ce(e.h, q.data_ptr(), a, hm, n, K, pix.data_ptr(), lab.data_ptr(), loss.data_ptr(), dq.data_ptr(), None)

    eng1 = cached_engine(704, 1)
    for rc in (maps(eng1, 16, ap, 240, 0), argmax(eng1, 16, ap, 240, 0), ce(eng1, ap, 240, 1, 1)):
        assert rc == -22 and b"head_out" in L.smg_last_error()
    eng = cached_engine(704, 3)
    assert maps(eng, 16, ap, 240, 0) == 0 and argmax(eng, 16, ap, 240, 0) == 0 and ce(eng, ap, 240, 1, 1) == 0      # (the calls are well-formed)
    torch.cuda.synchronize()
    out.fill_(FILL); idx.fill_(-5); val.fill_(-5.0); loss.fill_(-FILL); dq.fill_(-FILL)
    for rc in (maps(eng, 16, ap, 320, 0), argmax(eng, 16, ap, 320, 0), ce(eng, ap, 320, 1, 1),          # hm 320 pads to 928, not 704
               maps(eng, 0, ap, 240, 0), argmax(eng, 0, ap, 240, 0), ce(eng, ap, 240, 0, 1), ce(eng, ap, 240, 1, 0),
               maps(eng, 16, ap, 240, 3), maps(eng, 16, ap, 240, -2), argmax(eng, 16, ap, 240, 3), argmax(eng, 16, ap, 240, -1)):
        assert rc == -22
    shifted = aff.copy()
    shifted[15, 2] = 0.25
    sp = shifted.ctypes.data_as(C.POINTER(C.c_float))
    assert maps(eng, 16, sp, 240, -1) == -22 and argmax(eng, 16, sp, 240, 0) == -22
    shifted0 = aff.copy()
    shifted0[0, 5] = -0.5
    assert ce(eng, shifted0.ctypes.data_as(C.POINTER(C.c_float)), 240, 1, 1) == -22
    eng640 = cached_engine(640, 3)
    for rc in (maps(eng640, 16, ap, 224, 0), argmax(eng640, 16, ap, 224, 0), ce(eng640, ap, 224, 1, 1)):
        assert rc == -22
    with pytest.raises(smg_hip.SmgError):
        eng640.scene_class_argmax(q.data_ptr(), 16, aff, 224, 0, idx.data_ptr(), val.data_ptr(), None)
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and int(idx[0]) == -5 and float(val[0]) == -5.0 and float(loss[0]) == -FILL and bool((dq == -FILL).all())


def test_train_batch_scene_class_pixels_vs_fp64_oracle_s704(gpu):
    """A 240^2 heightmap -> S = 704, 3 x 3 maps: two samples (style 0, rotations 1 and 6 of 16), K = 3: one class-0 and one class-1
    scene pixel and a class-2 padding point at heightmap pixel (0, 0), where no window is centred.  Per sample the loss against
    the fp64 criterion over the product's OWN logits (one fp32 rounding: 2^-23 of the terms, over W).  Summed over the samples
    against the fp64 oracle: q_close bounds each logit error by 1e-3 scale (scale = the oracle's largest |logit|), an interpolated
    logit is a convex combination of logits, logsumexp minus one logit is 2-Lipschitz in the max norm and a sample's loss is a
    mean over its points: 2 x 1e-3 x scale per sample.  All 368 gradient tensors within 3x the fp32 oracle's own error against
    fp64 (test_train_batch_scene_pixels_vs_fp64_oracle_s704's yardstick), and - the head backward took its dense form - the value
    convolution's weight gradient identical between two runs."""
    sc = s704_scene(3)
    hm, style, rots, aff, depth, md, x, mx, on, q64 = (sc[k] for k in ("hm", "style", "rots", "aff", "depth", "md", "x", "mx", "on", "q64"))
    pix = np.asarray([[(118, 123), (124, 116), (0, 0)], [(121, 119), (115, 126), (0, 0)]])
    lab = np.asarray([[0, 1, 2], [1, 0, 2]])
    for j in range(2):
        assert scene_ref.map_coords(hm, aff[j], pix[j, :, 0], pix[j, :, 1])[2].tolist() == [True, True, False]

    def total(qs):
        return sum(scene_class_ref.scene_class_loss(qs[j][0], aff[j], hm, pix[j], lab[j]) for j in range(2))
    loss64 = total(q64)
    loss64.backward()
    g64 = {n: p.grad for n, p in sc["o64"].named_parameters() if p.grad is not None}
    on.zero_grad()
    total([orc.forward(on, x, mx, style, False, r) for r in rots]).backward()

    tr = make_trainer('reactive', 1)
    runs = []
    for it in range(2):
        loss, q = tr.train_batch_scene_class_pixels(depth, md, style, rots, pix, lab, return_q=True)
        assert tuple(q.shape) == (2, 3, 3, 3) and tuple(loss.shape) == (2,)
        runs.append(dict(tr.model.named_parameters())[HEAD + "conv1.weight"].grad.clone())
    qh = q.cpu().numpy().astype(np.float64)
    scale = 0.0
    for j in range(2):
        keep = lab[j] < 2
        z = scene_class_ref.scene_class_points(torch.from_numpy(qh[j]), aff[j], hm, pix[j][keep])
        terms = scene_class_ref.nll_terms(z, torch.from_numpy(lab[j][keep]))[0].numpy()
        W = int(keep.sum())
        own, gate = terms.sum() / W, 2.0 ** -23 * np.abs(terms).sum() / W
        print("sample %d: loss %.7f, fp64 over the same logits %.7f, |d| %.2e (gate %.2e)" % (j, float(loss[j]), own, abs(float(loss[j]) - own), gate))
        assert abs(float(loss[j]) - own) <= gate
        scale = max(scale, float(q64[j].detach().abs().max()))
    gate = 2 * 1e-3 * scale * 2
    print("loss sum %.7f, fp64 oracle %.7f, |d| %.2e (gate %.2e)" % (float(loss.double().sum()), float(loss64.detach()), abs(float(loss.double().sum()) - float(loss64.detach())), gate))
    assert abs(float(loss.double().sum()) - float(loss64.detach())) <= gate
    n_compared = assert_train_batch_runs(tr, runs, on, g64, "S=704 scene class pixels")
    print("%d gradient tensors compared, %d in the fp64 oracle" % (n_compared, len(g64)))


def test_forward_scene_class_maps_and_best_scene_class_action(gpu):
    import synthetic
    from trainer import Trainer
    hm, side = 240, 3
    tr = make_trainer('reactive', 4)
    depth, masks = synthetic.heightmap_scene(8, size=hm, n_boxes=8)
    md = depth * masks[0]
    aff = affines()
    eng = cached_engine(704, 3)
    for style in (0, 1):
        ps = tr.forward_scene_class_maps(depth, md, style)
        qd = tr._last_q.cpu().numpy()                        # the logits of that very call
        assert ps.dtype == np.float64 and ps.shape == (16, 3, hm, hm)
        ref, valid = check_class_maps(ps.astype(np.float32), qd, aff, hm, "forward_scene_class_maps style %d" % style)
        assert np.isneginf(ps[:, 0][~valid]).all() and (~valid).any() and valid.any()
        best = tr.best_scene_class_action(depth, md, style)
        ref2, valid2, _ = scene_class_ref.scene_class_maps(tr._last_q.cpu().numpy(), aff, hm)
        r, (iy, ix) = best["rotation"], best["pixel"]
        assert valid2[r, iy, ix]
        assert abs(best["conf"] - ref2[r, 0, iy, ix]) <= 2.0 ** -23 * abs(ref2[r, 0, iy, ix])
        top = ref2[:, 0][valid2].max()
        assert best["conf"] >= np.float32(top) - 2.0 ** -23 * abs(top)
        qy, qx, ok = Trainer.scene_to_map(hm, r, 16, (iy, ix))
        assert ok and best["map_pixel"] == (float(qy), float(qx))
    one = tr.forward_scene_class_maps(depth, md, 0, cls=0)
    assert one.shape == (16, hm, hm)
    ref0, valid0, margin0 = scene_class_ref.scene_class_maps(tr._last_q.cpu().numpy(), aff, hm)
    assert np.array_equal((~np.isneginf(one))[margin0 > 1e-6], valid0[margin0 > 1e-6])
    both = valid0 & ~np.isneginf(one)
    assert (np.abs(one[both] - ref0[:, 0][both]) <= 2.0 ** -23 * np.abs(ref0[:, 0][both])).all()
    dev = tr.forward_scene_class_maps(depth, md, 0, return_device=True)
    assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (16, 3, hm, hm)
    # logits=True: the three planes through smg_scene_maps with map_stride = 3 OH OW, bit for bit
    z = tr.forward_scene_class_maps(depth, md, 0, logits=True, return_device=True)
    assert tuple(z.shape) == (16, 3, hm, hm)
    q = tr._last_q
    for c in range(3):
        out = filled((16, hm, hm), FILL)
        eng.scene_maps(q[:, c].data_ptr(), 3 * side * side, 16, aff, hm, out.data_ptr(), stream())
        assert torch.equal(out.view(torch.int32), z[:, c].contiguous().view(torch.int32)), c
    z1 = tr.forward_scene_class_maps(depth, md, 0, cls=1, logits=True)
    assert z1.shape == (16, hm, hm) and np.array_equal(z1, z[:, 1].cpu().numpy().astype(np.float64))
    one = tr.forward_scene_class_maps(depth, md, 0, specific_rotation=5)
    assert one.shape == (1, 3, hm, hm)
    check_class_maps(one.astype(np.float32), tr._last_q.cpu().numpy(), aff[5:6], hm, "rotation 5 alone")
    gs = tr.forward_scene_class_maps(depth, md, 2)
    assert gs.shape == (1, 3, hm, hm)
    check_class_maps(gs.astype(np.float32), tr._last_q.cpu().numpy(), aff[0:1], hm, "style 2 = rotation 0")
