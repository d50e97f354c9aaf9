"""Scene-frame Q maps on the MI355X (run with -m gpu): smg_scene_maps / smg_scene_argmax / smg_loss_scene on an engine alone with
synthetic maps against the fp64 restatement of tests/scene_ref.py (values to one fp32 rounding, the validity mask, the sense of
the rotation, np.argmax over the kernel's own maps, torch fp64 autograd for the loss), then train_batch_scene_pixels against the
fp64 PyTorch-CPU oracle and forward_scene / best_scene_action against forward_dense pushed through scene_ref."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import orc
from map_harness import assert_bit_identical, assert_train_batch_runs, cached_engine, filled, gpu, HEAD, make_trainer, s704_scene, stream  # noqa: F401

import scene_ref

pytestmark = pytest.mark.gpu

SHAPES = ((240, 704, 3), (320, 928, 10))


def affines(R=16):
    return np.stack([scene_ref.theta(r, R) for r in range(R)])


def gpu_scene_maps(eng, q, aff, hm, map_stride=None):
    n = len(aff)
    out = filled((n, hm, hm), 7.0)
    eng.scene_maps(q.data_ptr(), q[0].numel() if map_stride is None else map_stride, n, aff, hm, out.data_ptr(), stream())
    return out.cpu().numpy()


def gpu_scene_argmax(eng, q, aff, hm):
    idx = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    val = filled((1,), -5.0)
    eng.scene_argmax(q.data_ptr(), q[0].numel(), len(aff), aff, hm, idx.data_ptr(), val.data_ptr(), stream())
    return int(idx.cpu().numpy()[0]), val.cpu().numpy()[0]


def check_maps(got, q_host, aff, hm, what):
    """The validity mask on every pixel farther than 1e-6 from a boundary (at most 0.1 % excluded), -inf outside, and on valid pixels
    |gpu - ref| <= 2^-23 max(|ref|, 2^-126): the single rounding of an fp64 result."""
    ref, valid, margin = scene_ref.scene_maps(q_host, aff, hm)
    sure = margin > 1e-6
    print("%s: %d of %d pixels within 1e-6 of a validity boundary; %d valid" % (what, int((~sure).sum()), sure.size, int(valid.sum())))
    assert (~sure).mean() <= 1e-3
    gv = ~np.isneginf(got)
    assert np.array_equal(gv[sure], valid[sure])
    both = gv & valid
    err = np.abs(got[both].astype(np.float64) - ref[both])
    tol = 2.0 ** -23 * np.maximum(np.abs(ref[both]), 2.0 ** -126)
    print("%s: max |gpu - ref| / tol = %.3f" % (what, float((err / tol).max())))
    assert (err <= tol).all()
    return ref, valid


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_scene_maps_against_fp64(gpu, hm, S, side):
    assert scene_ref.geometry(hm)[1:] == (S, side)
    eng = cached_engine(S, 1)
    aff = affines()
    q = torch.from_numpy(np.random.default_rng(S).standard_normal((16, side, side)).astype(np.float32)).cuda()
    got = gpu_scene_maps(eng, q, aff, hm)
    check_maps(got, q.cpu().numpy(), aff, hm, "S=%d" % S)
    # one class plane of a [R, 3, OH, OW] tensor: map_stride = 3 OH OW
    q3 = torch.from_numpy(np.random.default_rng(S + 1).standard_normal((16, 3, side, side)).astype(np.float32)).cuda()
    got = gpu_scene_maps(eng, q3[:, 1], aff, hm, map_stride=3 * side * side)
    check_maps(got, q3[:, 1].cpu().numpy(), aff, hm, "S=%d, plane 1 of 3" % S)


def test_scene_maps_with_an_odd_group_of_maps_and_an_unaligned_output(gpu):
    """More maps than one launch carries (33 > 32, the second launch starts at map 32) written to an output that is 4 bytes off
    16-byte alignment: the guarded 4-byte stores instead of the 16-byte ones, the same values."""
    hm, S, side = 240, 704, 3
    eng = cached_engine(S, 1)
    aff = np.stack([scene_ref.theta(r, 33) for r in range(33)])
    q = torch.from_numpy(np.random.default_rng(5).standard_normal((33, side, side)).astype(np.float32)).cuda()
    buf = filled((33 * hm * hm + 2,), 7.0)
    out = buf[1:1 + 33 * hm * hm]
    assert out.data_ptr() % 16 == 4
    eng.scene_maps(q.data_ptr(), side * side, 33, aff, hm, out.data_ptr(), stream())
    check_maps(out.cpu().numpy().reshape(33, hm, hm), q.cpu().numpy(), aff, hm, "33 maps, unaligned")
    assert float(buf[0]) == 7.0 and float(buf[-1]) == 7.0
    i, v = gpu_scene_argmax(eng, q, aff, hm)
    flat = out.cpu().numpy()
    assert i == int(np.argmax(flat)) and v.view(np.uint32) == flat[i].view(np.uint32)


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_rotation_sense_on_a_plane_of_scene_coordinates(gpu, hm, S, side):
    """Q_r = f(u) = 0.7 u_x - 1.3 u_y + 0.2 at the SCENE coordinates u = A p of each window centre p: bilinear interpolation
    reproduces a plane, so every rotation's scene-frame map must be f at the heightmap pixels, to 2^-23 max|f| (fp32 map elements
    and output) + 2^-22 (0.7 + 1.3) (A is fp32: A^T A != I)."""
    eng = cached_engine(S, 1)
    aff = affines()
    c = 2.0 * (32.0 * np.arange(side) + 319.5) / (S - 1) - 1.0         # window centres, normalised, rotated frame
    py, px = np.meshgrid(c, c, indexing="ij")
    q = np.empty((16, side, side))
    for r in range(16):
        a = aff[r].astype(np.float64)
        q[r] = 0.7 * (a[0] * px + a[1] * py) - 1.3 * (a[3] * px + a[4] * py) + 0.2
    got = gpu_scene_maps(eng, torch.from_numpy(q.astype(np.float32)).cuda(), aff, hm)
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    ux, uy = scene_ref.scene_u(hm, iy, ix)
    f = 0.7 * ux - 1.3 * uy + 0.2
    tol = 2.0 ** -23 * np.abs(q).max() + 2.0 ** -22 * (0.7 + 1.3)
    for r in range(16):
        v = ~np.isneginf(got[r])
        assert v.sum() >= 1000
        err = float(np.abs(got[r][v] - f[v]).max())
        print("S=%d rotation %2d: max |map - f| %.2e (tol %.2e) on %d pixels" % (S, r, err, tol, int(v.sum())))
        assert err <= tol, (r, err, tol)


@pytest.mark.parametrize("hm,S,side", SHAPES)
def test_scene_argmax(gpu, hm, S, side):
    eng = cached_engine(S, 1)
    aff = affines()
    qh = np.random.default_rng(S + 7).standard_normal((16, side, side)).astype(np.float32)
    q = torch.from_numpy(qh).cuda()
    flat = gpu_scene_maps(eng, q, aff, hm).ravel()
    i, v = gpu_scene_argmax(eng, q, aff, hm)
    assert i == int(np.argmax(flat)) and v.view(np.uint32) == flat[i].view(np.uint32)
    i2, v2 = gpu_scene_argmax(eng, q, aff, hm)               # two calls, one result
    assert i2 == i and v2.view(np.uint32) == v.view(np.uint32)
    # a constant map: every valid value ties, the lowest valid flattened index wins
    qc = torch.full((16, side, side), 0.375, dtype=torch.float32, device="cuda")
    flat = gpu_scene_maps(eng, qc, aff, hm).ravel()
    assert set(np.unique(flat).tolist()) == {-np.inf, 0.375}
    i, v = gpu_scene_argmax(eng, qc, aff, hm)
    assert i == int(np.flatnonzero(flat == 0.375)[0]) == int(np.argmax(flat)) and v == np.float32(0.375)
    # a NaN in one map element wins (the first NaN of the flattened maps)
    qn = q.clone()
    qn[9, side // 2, side // 2] = float("nan")
    flat = gpu_scene_maps(eng, qn, aff, hm).ravel()
    assert np.isnan(flat).any()
    i, v = gpu_scene_argmax(eng, qn, aff, hm)
    assert i == int(np.argmax(flat)) == int(np.flatnonzero(np.isnan(flat))[0]) and np.isnan(v)
    assert i // (hm * hm) == 9


def test_loss_scene_against_torch_fp64_autograd(gpu):
    """S = 928, 4 pairs (rotations 0, 3, 8, 13 of 16), K = 5 points each: one duplicated, one of weight exactly 0, labels that put
    points on both Huber branches.  Loss within 2^-23 |loss|, every dq element within 2^-23 max|reference dq|, exactly 0 away from
    the touched corners, two calls bit-identical."""
    import smg_hip
    hm, S, side = 320, 928, 10
    eng = cached_engine(S, 1)
    rots = [0, 3, 8, 13]
    aff = np.stack([scene_ref.theta(r, 16) for r in rots])
    rng = np.random.default_rng(11)
    qh = rng.standard_normal((4, 1, side, side)).astype(np.float32)
    pix = np.empty((4, 5, 2), dtype=np.int32)
    for j in range(4):      # valid points: drawn around the centre, where every rotation has windows
        k = 0
        while k < 4:
            p = rng.integers(100, 220, size=2)
            if scene_ref.map_coords(hm, aff[j], p[0], p[1])[3] > 1e-3 and scene_ref.map_coords(hm, aff[j], p[0], p[1])[2]:
                pix[j, k] = p
                k += 1
        pix[j, 4] = pix[j, 1]                                   # a duplicate
    wgt = rng.uniform(0.2, 1.0, size=(4, 5)).astype(np.float32)
    wgt[:, 2] = 0.0                                             # a masked point
    lab = np.empty((4, 5), dtype=np.float32)
    ref_loss, ref_dq, branches = [], [], []
    v0 = [scene_ref.scene_points(torch.from_numpy(qh[j, 0]).double(), aff[j], hm, pix[j]).numpy() for j in range(4)]
    for j in range(4):      # |d| = 0.3 (quadratic) and 1.7 (linear), alternating, both signs
        lab[j] = (v0[j] + np.asarray([0.3, -1.7, 0.5, 1.7, -0.3])).astype(np.float32)
    for j in range(4):
        qj = torch.from_numpy(qh[j, 0]).double().requires_grad_(True)
        d = scene_ref.scene_points(qj, aff[j], hm, pix[j]) - torch.from_numpy(lab[j]).double()
        loss = (torch.from_numpy(wgt[j]).double() * scene_ref.huber(d)).sum()
        loss.backward()
        ref_loss.append(float(loss.detach())); ref_dq.append(qj.grad.numpy()); branches += (d.abs() < 1).tolist()
    assert any(branches) and not all(branches)
    ref_loss, ref_dq = np.asarray(ref_loss), np.stack(ref_dq)
    q = torch.from_numpy(qh).cuda()
    pix_d, lab_d, wgt_d = torch.from_numpy(pix).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(wgt).cuda()
    runs = []
    for _ in range(2):
        loss, dq = filled((4,)), filled(q.shape)
        eng.loss_scene(q.data_ptr(), aff, hm, 4, 5, pix_d.data_ptr(), lab_d.data_ptr(), wgt_d.data_ptr(), loss.data_ptr(), dq.data_ptr(), stream())
        runs.append((loss.cpu().numpy(), dq.cpu().numpy()[:, 0]))
    loss, dq = runs[0]
    print("loss", loss, "ref", ref_loss, "max |ddq| %.2e, max |dq| %.2e" % (np.abs(dq - ref_dq).max(), np.abs(ref_dq).max()))
    assert (np.abs(loss - ref_loss) <= 2.0 ** -23 * np.abs(ref_loss)).all()
    assert np.abs(dq - ref_dq).max() <= 2.0 ** -23 * np.abs(ref_dq).max()
    assert (dq[ref_dq == 0] == 0).all() and int((ref_dq != 0).sum()) <= 4 * 4 * 4
    assert_bit_identical(runs[0][0], runs[1][0])
    assert_bit_identical(runs[0][1], runs[1][1])
    # NULL weights = all ones
    loss1, dq1 = torch.empty(4, device="cuda"), torch.empty_like(q)
    eng.loss_scene(q.data_ptr(), aff, hm, 4, 5, pix_d.data_ptr(), lab_d.data_ptr(), None, loss1.data_ptr(), dq1.data_ptr(), stream())
    ones = []
    for j in range(4):
        d = scene_ref.scene_points(torch.from_numpy(qh[j, 0]).double(), aff[j], hm, pix[j]) - torch.from_numpy(lab[j]).double()
        ones.append(float(scene_ref.huber(d).sum()))
    assert (np.abs(loss1.cpu().numpy() - np.asarray(ones)) <= 2.0 ** -23 * np.abs(ones)).all()
    # a 3-class engine refuses: -22, nothing launched
    eng3 = cached_engine(704, 3)
    loss3, dq3 = filled((1,)), filled((1, 3, 3, 3))
    rc = smg_hip.lib().smg_loss_scene(eng3.h, dq3.data_ptr(), aff.ctypes.data_as(C.POINTER(C.c_float)), 240, 1, 5, pix_d.data_ptr(), lab_d.data_ptr(), None,
                                      loss3.data_ptr(), dq3.data_ptr(), C.c_void_p(0))
    assert rc == -22 and b"head_out" in smg_hip.lib().smg_last_error()
    torch.cuda.synchronize()
    assert float(loss3[0]) == -7.0 and bool((dq3 == -7.0).all())


def test_scene_entry_points_refuse_bad_geometry(gpu):
    """-22 and nothing launched: a heightmap side that does not pad to the engine's S, a 1 x 1 map, n_maps < 1, K < 1, an affine
    matrix with a translation (the chain is p = A^T u: rotations about the centre)."""
    import smg_hip
    L = smg_hip.lib()
    eng = cached_engine(704, 1)
    aff = affines()
    ap = aff.ctypes.data_as(C.POINTER(C.c_float))
    q = torch.zeros((16, 3, 3), device="cuda")
    out = filled((16, 240, 240), 7.0)
    idx, val = torch.full((1,), -5, dtype=torch.int32, device="cuda"), filled((1,), -5.0)
    pix = torch.full((1, 1, 2), 120, dtype=torch.int32, device="cuda")
    lab, loss, dq = torch.zeros((1, 1), device="cuda"), filled((1,)), filled((1, 1, 3, 3))
    assert L.smg_scene_maps(eng.h, q.data_ptr(), 9, 16, ap, 320, out.data_ptr(), None) == -22
    assert L.smg_scene_maps(eng.h, q.data_ptr(), 9, 0, ap, 240, out.data_ptr(), None) == -22
    assert L.smg_scene_argmax(eng.h, q.data_ptr(), 9, 16, ap, 224, idx.data_ptr(), val.data_ptr(), None) == -22
    assert L.smg_scene_argmax(eng.h, q.data_ptr(), 9, -1, ap, 240, idx.data_ptr(), val.data_ptr(), None) == -22
    assert L.smg_loss_scene(eng.h, q.data_ptr(), ap, 240, 1, 0, pix.data_ptr(), lab.data_ptr(), None, loss.data_ptr(), dq.data_ptr(), None) == -22
    assert L.smg_loss_scene(eng.h, q.data_ptr(), ap, 260, 1, 1, pix.data_ptr(), lab.data_ptr(), None, loss.data_ptr(), dq.data_ptr(), None) == -22
    shifted = aff.copy()
    shifted[15, 2] = 0.25
    assert L.smg_scene_maps(eng.h, q.data_ptr(), 9, 16, shifted.ctypes.data_as(C.POINTER(C.c_float)), 240, out.data_ptr(), None) == -22
    eng640 = cached_engine(640, 1)
    assert L.smg_scene_maps(eng640.h, q.data_ptr(), 1, 16, ap, 224, out.data_ptr(), None) == -22
    with pytest.raises(smg_hip.SmgError):
        eng640.scene_argmax(q.data_ptr(), 1, 16, aff, 224, idx.data_ptr(), val.data_ptr(), None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(idx[0]) == -5 and float(val[0]) == -5.0 and float(loss[0]) == -7.0 and bool((dq == -7.0).all())


def test_train_batch_scene_pixels_vs_fp64_oracle_s704(gpu):
    """A 240^2 heightmap -> S = 704, 3 x 3 maps: two samples (style 0, rotations 1 and 6 of 16), K = 2 valid scene pixels each, one
    per Huber branch.  The loss against the fp64 sum over the product's OWN q pushed through scene_ref (what remains is one fp32
    rounding: 2^-23 of the terms) and against the fp64 oracle's (|dv| <= max|dq|: q_close's 1e-3 of the map's scale per point),
    all 368 gradient tensors within 3x the fp32 oracle's own error against fp64 (test_whole_map_training_vs_fp64_oracle_s928's
    yardstick), and - the head backward took its dense form - the value convolution's weight gradient identical between two runs."""
    sc = s704_scene(1)
    hm, style, rots, aff, depth, md, x, mx, on, q64 = (sc[k] for k in ("hm", "style", "rots", "aff", "depth", "md", "x", "mx", "on", "q64"))
    pix = np.asarray([[(118, 123), (124, 116)], [(121, 119), (115, 126)]])
    for j in range(2):
        assert scene_ref.map_coords(hm, aff[j], pix[j, :, 0], pix[j, :, 1])[2].all()
    v64 = [scene_ref.scene_points(q64[j][0, 0], aff[j], hm, pix[j]) for j in range(2)]
    lab = np.stack([v.detach().numpy() + np.asarray([0.4, -1.6]) for v in v64]).astype(np.float32)       # |d| = 0.4 and 1.6
    wgt = np.asarray([[1.0, 0.5], [0.75, 1.0]], dtype=np.float32)

    def total(vs, dtype):
        return sum((torch.from_numpy(wgt[j]).to(dtype) * scene_ref.huber(vs[j] - torch.from_numpy(lab[j]).to(dtype))).sum() for j in range(2))
    loss64 = total(v64, torch.float64)
    loss64.backward()
    g64 = {n: p.grad for n, p in sc["o64"].named_parameters() if p.grad is not None}
    on.zero_grad()
    qo = [orc.forward(on, x, mx, style, False, r) for r in rots]
    total([scene_ref.scene_points(qo[j][0, 0], aff[j], hm, pix[j]) for j in range(2)], torch.float32).backward()

    tr = make_trainer('reinforcement', 1)
    runs = []
    for it in range(2):
        loss, q = tr.train_batch_scene_pixels(depth, md, style, rots, pix, lab, wgt, return_q=True)
        assert tuple(q.shape) == (2, 1, 3, 3) and tuple(loss.shape) == (2,)
        runs.append(dict(tr.model.named_parameters())[HEAD + "conv1.weight"].grad.clone())
    qh = q.cpu().numpy().astype(np.float64)
    own, scale = 0.0, 0.0
    for j in range(2):
        d = scene_ref.scene_points(torch.from_numpy(qh[j, 0]), aff[j], hm, pix[j]) - torch.from_numpy(lab[j]).double()
        terms = (torch.from_numpy(wgt[j]).double() * scene_ref.huber(d)).numpy()
        err = abs(float(loss[j]) - terms.sum())
        print("sample %d: loss %.7f, fp64 over the same q %.7f, |d| %.2e (gate %.2e)" % (j, float(loss[j]), terms.sum(), err, 2.0 ** -23 * np.abs(terms).sum()))
        assert err <= 2.0 ** -23 * np.abs(terms).sum()
        own += terms.sum()
        scale = max(scale, float(q64[j].detach().abs().max()))
    gate = 1e-3 * scale * float(wgt.sum())       # huber' <= 1, each v a convex combination of q: |d loss| <= sum_k w_k max|dq|
    print("loss sum %.7f, fp64 oracle %.7f, |d| %.2e (gate %.2e)" % (own, float(loss64), abs(own - float(loss64)), gate))
    assert abs(float(loss.double().sum()) - float(loss64)) <= gate
    assert_train_batch_runs(tr, runs, on, g64, "S=704 scene pixels")


def test_forward_scene_and_best_scene_action(gpu):
    import synthetic
    from trainer import Trainer
    hm = 240
    tr = make_trainer('reinforcement', 4)
    depth, masks = synthetic.heightmap_scene(8, size=hm, n_boxes=8)
    md = depth * masks[0]
    aff = affines()
    for style in (0, 1):
        qs = tr.forward_scene(depth, md, style)
        qd = tr._last_q.cpu().numpy()[:, 0]                  # forward_dense's own output of that very call
        assert qs.dtype == np.float64 and qs.shape == (16, hm, hm)
        ref, valid = check_maps(qs.astype(np.float32), qd, aff, hm, "forward_scene style %d" % style)
        assert np.isneginf(qs[~valid]).all() and (~valid).any() and valid.any()
        best = tr.best_scene_action(depth, md, style)
        qd2 = tr._last_q.cpu().numpy()[:, 0]
        r, (iy, ix) = best["rotation"], best["pixel"]
        ref2, valid2, _ = scene_ref.scene_maps(qd2, aff, hm)
        assert valid2[r, iy, ix]
        assert abs(best["conf"] - ref2[r, iy, ix]) <= 2.0 ** -23 * abs(ref2[r, iy, ix])
        assert best["conf"] >= np.float32(ref2[valid2].max()) - 2.0 ** -23 * abs(ref2[valid2].max())
        qy, qx, ok = Trainer.scene_to_map(hm, r, 16, (iy, ix))
        assert ok and best["map_pixel"] == (float(qy), float(qx))
    dev = tr.forward_scene(depth, md, 0, return_device=True)
    assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (16, hm, hm)
    one = tr.forward_scene(depth, md, 0, specific_rotation=5)
    assert one.shape == (1, hm, hm)
    check_maps(one.astype(np.float32), tr._last_q.cpu().numpy()[:, 0], aff[5:6], hm, "rotation 5 alone")
    gs = tr.forward_scene(depth, md, 2, is_target=True)
    assert gs.shape == (1, hm, hm)
    check_maps(gs.astype(np.float32), tr._last_q.cpu().numpy()[:, 0], aff[0:1], hm, "style 2 = rotation 0")
