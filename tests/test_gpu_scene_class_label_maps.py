"""Scene-frame class-label maps on the MI355X (run with -m gpu): smg_loss_scene_map_ce on an engine alone with synthetic logits
against torch fp64 autograd through tests/scene_class_ref.py (tests/scene_class_label_ref.py builds the cases), against
smg_loss_scene_ce fed the counted pixels as a list, its masks, groups of more than 32 pairs, a map beyond 45 x 45 and the refusals,
then train_batch_scene_class_maps against the fp64 PyTorch-CPU oracle and against train_batch_scene_class_pixels."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import orc
from map_harness import (assert_bit_identical, assert_scene_loss_refusals, assert_train_batch_runs, assert_written_and_finite, bits,  # noqa: F401
                         border_pixels, filled, gpu, HEAD, make_trainer, own_engine, s704_scene, stream)

import scene_class_label_ref
import scene_class_ref
import scene_label_ref
import scene_ref

pytestmark = pytest.mark.gpu

ROTS = (0, 3, 8, 13)
_CASES = {}


def case(hm, rots=ROTS):
    """One reference per shape, shared by the tests and never modified."""
    key = (hm, tuple(rots))
    if key not in _CASES:
        _CASES[key] = scene_class_label_ref.make_case(hm, rots, 16, seed=hm)
    return _CASES[key]


def run(eng, q, aff, hm, label):
    """One smg_loss_scene_map_ce call on device tensors, outputs pre-filled with -7 -> (loss [n], dq [n, 3, side, side]) on the host."""
    n = q.shape[0]
    loss, dq = filled((n,)), filled(q.shape)
    eng.loss_scene_map_ce(q.data_ptr(), aff, hm, n, label.data_ptr(), loss.data_ptr(), dq.data_ptr(), stream())
    return loss.cpu().numpy(), dq.cpu().numpy()


def assert_fp64_gates(loss, dq, ref_loss, ref_dq, what):
    """Double arithmetic, one division, one rounding: |loss - ref| <= 2^-23 |ref| and per pair max|dq - ref| <= 2^-23 max|ref dq|
    (2^-24 is the rounding; the rest covers the device's double exp / log against torch's, orders below); everything finite and
    written over the -7 fill."""
    for j in range(len(loss)):
        print("%s pair %d: loss %.7f ref %.7f |d| %.2e (gate %.2e); max |ddq| %.2e (gate %.2e)" % (
            what, j, loss[j], ref_loss[j], abs(loss[j] - ref_loss[j]), 2.0 ** -23 * abs(ref_loss[j]),
            np.abs(dq[j] - ref_dq[j]).max(), 2.0 ** -23 * np.abs(ref_dq[j]).max()))
    assert_written_and_finite(-7.0, loss, dq)
    assert (np.abs(loss - ref_loss) <= 2.0 ** -23 * np.abs(ref_loss)).all()
    for j in range(len(loss)):
        assert np.abs(dq[j] - ref_dq[j]).max() <= 2.0 ** -23 * np.abs(ref_dq[j]).max()


def check_against_fp64(c, what):
    q, lab = torch.from_numpy(c["q"]).cuda(), torch.from_numpy(c["label"]).cuda()
    with own_engine(c["S"], 3, 4) as eng:
        loss, dq = run(eng, q, c["aff"], c["hm"], lab)
        loss2, dq2 = run(eng, q, c["aff"], c["hm"], lab)        # a second call: bit-identical
    assert_fp64_gates(loss, dq, c["loss"], c["dq"], what)
    assert_bit_identical(loss, loss2)
    assert_bit_identical(dq, dq2)
    return loss, dq


def assert_case_mix(c):
    """The recipe's conditions: 0.6 <= W / valid <= 0.8, each class at least 300 points per pair, NaN labels at invalid pixels."""
    for j in range(len(c["W"])):
        nvalid = int(c["valid"][j].sum())
        assert 0.6 <= c["W"][j] / nvalid <= 0.8, (j, c["W"][j], nvalid)
        assert c["n0"][j] >= 300 and c["n1"][j] >= 300
    assert np.isnan(c["label"][~c["valid"]]).all()


@pytest.mark.parametrize("hm,S,side", ((240, 704, 3), (320, 928, 10)))
def test_loss_scene_map_ce_against_torch_fp64_autograd(gpu, hm, S, side):
    """4 pairs (rotations 0, 3, 8, 13 of 16), full label images of the recipe's mix (0, 1, 2, NaN, 7, -1, 0.5; NaN at every invalid
    pixel).  Loss within 2^-23 |ref|, dq within 2^-23 max|reference dq| per pair, every output written and finite, two calls
    bit-identical."""
    c = case(hm)
    assert (c["S"], c["side"]) == (S, side)
    assert_case_mix(c)
    check_against_fp64(c, "hm=%d" % hm)


def test_loss_scene_map_ce_where_the_heightmap_border_clips_the_boxes(gpu):
    """hm = 448 (S = 1280, 21 x 21 maps): in rotation 2 of 16 valid pixels lie on the image border, so an element's pixel box is cut
    by the heightmap edge (at 240 and 320 the valid area stays inside).  Same gates."""
    c = case(448, (2, 5))
    assert (c["S"], c["side"]) == (1280, 21)
    assert_case_mix(c)
    border = border_pixels(c["valid"][0])
    print("rotation 2: %d valid pixels on the image border" % border)
    assert border > 0
    check_against_fp64(c, "hm=448")


def test_loss_scene_map_ce_groups_of_pairs(gpu):
    """33 pairs at hm = 240 (the second launch group carries pair 32 alone), pair 32 with pair 0's inputs: bit-equal results across
    the group boundary, pair 31 differs, one pair of the first group against fp64."""
    hm, S, side = 240, 704, 3
    rng = np.random.default_rng(33)
    rots = list(range(32)) + [0]
    aff = np.stack([scene_ref.theta(r, 32) for r in rots])
    q = rng.standard_normal((33, 3, side, side)).astype(np.float32)
    lab = rng.choice(np.asarray(scene_class_label_ref.LABEL_VALUES), size=(33, hm, hm), p=scene_class_label_ref.LABEL_SHARES).astype(np.float32)
    q[32], lab[32] = q[0], lab[0]
    with own_engine(S, 3, 33) as eng:
        loss, dq = run(eng, torch.from_numpy(q).cuda(), aff, hm, torch.from_numpy(lab).cuda())
    assert_written_and_finite(-7.0, loss, dq)
    assert loss[0] > 0 and np.abs(dq[0]).max() > 0
    assert_bit_identical(loss[32:33], loss[0:1])
    assert_bit_identical(dq[32], dq[0])
    assert not np.array_equal(dq[31], dq[0]) and loss[31] != loss[0]
    l0, g0, terms, W = scene_class_label_ref.autograd(q[5], aff[5], hm, lab[5])
    assert W > 600
    assert_fp64_gates(loss[5:6], dq[5:6], np.asarray([l0]), g0[None], "33 pairs, pair 5")


def test_loss_scene_map_ce_with_matrices_that_are_no_rotation(gpu):
    """scene_point asks for no rotation, so neither does this call: a sheared and stretched 2x2 part, one shrunk to half (boxes twice
    as wide) and the zero matrix (no inverse: every workgroup walks the whole heightmap, every labelled pixel lands on the map's
    centre) against torch fp64 autograd with the gates above."""
    hm, S, side = 240, 704, 3
    aff = scene_label_ref.odd_affines()
    n = len(aff)
    rng = np.random.default_rng(77)
    q = rng.standard_normal((n, 3, side, side)).astype(np.float32)
    lab = rng.choice(np.asarray(scene_class_label_ref.LABEL_VALUES), size=(n, hm, hm), p=scene_class_label_ref.LABEL_SHARES).astype(np.float32)
    with own_engine(S, 3, 4) as eng:
        loss, dq = run(eng, torch.from_numpy(q).cuda(), aff, hm, torch.from_numpy(lab).cuda())
    ref = [scene_class_label_ref.autograd(q[j], aff[j], hm, lab[j]) for j in range(n)]
    print("points per 2x2 part: %s" % [r[3] for r in ref])
    assert all(r[3] > 500 for r in ref)
    assert_fp64_gates(loss, dq, np.asarray([r[0] for r in ref]), np.stack([r[1] for r in ref]), "2x2 part")
    for c in range(3):                       # the zero matrix: all of it on the centre element of each plane
        assert int((dq[2, c] != 0).sum()) == 1 and dq[2, c, 1, 1] != 0


def test_loss_scene_map_ce_against_loss_scene_ce_on_the_same_pixels(gpu):
    """smg_loss_scene_ce fed exactly the counted pixels of the 320^2 case as a list (pair by pair: K differs): both kernels round
    an fp64 sum of the same terms, divided by the same W, once, so the loss agrees to 2^-22 of the list's loss and dq to 2^-22 of
    the list's max|dq|."""
    c = case(320)
    hm = c["hm"]
    with own_engine(c["S"], 3, 4) as eng:
        q, lab = torch.from_numpy(c["q"]).cuda(), torch.from_numpy(c["label"]).cuda()
        loss, dq = run(eng, q, c["aff"], hm, lab)
        for j in range(4):
            pix, y, keep = scene_class_label_ref.counted(hm, c["aff"][j], c["label"][j])
            K = int(keep.sum())
            assert K == c["W"][j] > 10000
            pix_d = torch.from_numpy(np.ascontiguousarray(pix[keep], dtype=np.int32)).cuda()
            lab_d = torch.from_numpy(y[keep].astype(np.float32)).cuda()
            lj, dj = filled((1,)), filled((1, 3, c["side"], c["side"]))
            eng.loss_scene_ce(q[j:j + 1].data_ptr(), c["aff"][j:j + 1], hm, 1, K, pix_d.data_ptr(), lab_d.data_ptr(), lj.data_ptr(), dj.data_ptr(), stream())
            lj, dj = float(lj.cpu()[0]), dj.cpu().numpy()[0]
            print("pair %d: K %d, loss %.7f vs %.7f, max |ddq| %.2e of %.2e" % (j, K, loss[j], lj, np.abs(dq[j] - dj).max(), np.abs(dj).max()))
            assert lj > 0 and abs(loss[j] - lj) <= 2.0 ** -22 * abs(lj)
            assert np.abs(dq[j] - dj).max() <= 2.0 ** -22 * np.abs(dj).max()


def test_loss_scene_map_ce_masks(gpu):
    """An image of class 2, NaN and 7 only: loss and dq bitwise zero, whatever the logits hold (a NaN among them).  An image labelled
    only in the interior of one 2 x 2-cell: dq bitwise zero at every element but that cell's four corners, in all three planes."""
    c = case(320)
    hm, side = c["hm"], c["side"]
    with own_engine(c["S"], 3, 4) as eng:
        qn = c["q"].copy()
        qn[:, 1, side // 2, side // 2] = np.nan
        none = np.asarray([2.0, np.nan, 7.0], dtype=np.float32)[np.arange(4 * hm * hm).reshape(4, hm, hm) % 3]
        loss, dq = run(eng, torch.from_numpy(qn).cuda(), c["aff"], hm, torch.from_numpy(none).cuda())
        assert np.array_equal(bits(loss), np.zeros(4, dtype=np.uint32)) and np.array_equal(bits(dq), np.zeros(dq.shape, dtype=np.uint32))
        # pixels whose home cell is (4, 5), at least 0.05 map units inside it, labelled 0 / 1 alternately; class 2 elsewhere
        iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
        lab = np.full((4, hm, hm), 2.0, dtype=np.float32)
        for j in range(4):
            qy, qx, valid, _ = scene_ref.map_coords(hm, c["aff"][j], iy, ix)
            inside = valid & (qy > 4.05) & (qy < 4.95) & (qx > 5.05) & (qx < 5.95)
            assert inside.sum() > 100
            lab[j][inside] = (np.arange(int(inside.sum())) % 2).astype(np.float32)
        loss, dq = run(eng, torch.from_numpy(c["q"]).cuda(), c["aff"], hm, torch.from_numpy(lab).cuda())
        corners = np.zeros((side, side), dtype=bool)
        corners[4:6, 5:7] = True
        assert (loss > 0).all()
        assert (dq[:, :, corners] != 0).all()
        assert np.array_equal(bits(dq[:, :, ~corners]), np.zeros((4, 3, side * side - 4), dtype=np.uint32))


def test_loss_scene_map_ce_on_a_map_beyond_45_x_45(gpu):
    """hm = 800 -> S = 2272, 52 x 52 maps, one pair, rotation 3 of 16, labels of the recipe's mix on a 64 x 64 block (class 2
    elsewhere: the fp64 reference stays cheap).  smg_loss_scene_ce refuses this size (its accumulators live in LDS); the label-map
    call returns 0 and meets the fp64 gates: the limit of 45 x 45 is gone."""
    import smg_hip
    hm, S, side = 800, 2272, 52
    assert scene_ref.geometry(hm)[1:] == (S, side)
    with own_engine(S, 3, 1) as eng:
        aff = scene_ref.theta(3, 16)[None]
        rng = np.random.default_rng(800)
        q = rng.standard_normal((1, 3, side, side)).astype(np.float32)
        lab = np.full((1, hm, hm), 2.0, dtype=np.float32)
        lab[0, 368:432, 368:432] = rng.choice(np.asarray(scene_class_label_ref.LABEL_VALUES), size=(64, 64), p=scene_class_label_ref.LABEL_SHARES)
        l0, g0, terms, W = scene_class_label_ref.autograd(q[0], aff[0], hm, lab[0])
        print("hm=800: W = %d, %d map elements with a gradient" % (W, int((g0 != 0).any(axis=0).sum())))
        assert W > 2500 and int((g0 != 0).any(axis=0).sum()) >= 16
        qd, labd = torch.from_numpy(q).cuda(), torch.from_numpy(lab).cuda()
        L = smg_hip.lib()
        pix = torch.full((1, 1, 2), 400, dtype=torch.int32, device="cuda")
        one = torch.zeros((1, 1), device="cuda")
        loss, dq = filled((1,)), filled(qd.shape)
        rc = L.smg_loss_scene_ce(eng.h, qd.data_ptr(), aff.ctypes.data_as(C.POINTER(C.c_float)), hm, 1, 1, pix.data_ptr(), one.data_ptr(),
                                 loss.data_ptr(), dq.data_ptr(), None)
        assert rc == -22 and b"LDS" in L.smg_last_error()
        loss, dq = run(eng, qd, aff, hm, labd)
        assert_fp64_gates(loss, dq, np.asarray([l0]), g0[None], "hm=800")
        assert (dq[0][g0 == 0] == 0).all()
        loss2, dq2 = run(eng, qd, aff, hm, labd)
        assert_bit_identical(loss, loss2)
        assert_bit_identical(dq, dq2)


def test_loss_scene_map_ce_refusals(gpu):
    """-22, a message that names the function and the cause, and nothing launched: a one-channel head, a heightmap side that does not
    pad to the engine's S, a 1 x 1 map, n_pairs < 1, an affine matrix with a translation."""
    import smg_hip
    L = smg_hip.lib()
    q = torch.zeros((4, 3, 3, 3), device="cuda")
    lab = torch.zeros((4, 320, 320), device="cuda")
    loss, dq = filled((4,)), filled((4, 3, 3, 3))

    def call(eng, affine, size, n):
        return L.smg_loss_scene_map_ce(eng.h, q.data_ptr(), affine, size, n, lab.data_ptr(), loss.data_ptr(), dq.data_ptr(), None)

    def method(eng, affine, size, n):
        eng.loss_scene_map_ce(q.data_ptr(), affine, size, n, lab.data_ptr(), loss.data_ptr(), dq.data_ptr(), None)
    assert_scene_loss_refusals(call, method, b"smg_loss_scene_map_ce", 3, 1, lambda S, out_ch: own_engine(S, out_ch, 4), loss, dq, name_leads=True)


def test_train_batch_scene_class_maps_vs_fp64_oracle_s704(gpu):
    """test_train_batch_scene_class_pixels_vs_fp64_oracle_s704's recipe with label IMAGES: a 240^2 heightmap, two samples (style 0,
    rotations 1 and 6 of 16), classes 0 / 1 on the 9 x 9 block around the centre (pixels 116 - 124) with four class-2 holes, class 2
    elsewhere, and a class-0 label at heightmap pixel (0, 0), where no window is centred: it must neither raise nor count (W = 77).
    Per sample the loss against the fp64 criterion over the product's OWN logits (2^-23 of the terms, over W); summed over the
    samples against the fp64 oracle with that test's gate (2 x 1e-3 x scale per sample); all 368 gradient tensors within 3x the
    fp32 oracle's own error against fp64; the head's conv1 weight gradient identical between two runs; and
    train_batch_scene_class_pixels on the same 77 labelled pixels gives the same losses to 2^-22."""
    sc = s704_scene(3)
    hm, style, rots, block, aff, depth, md, x, mx, on, q64 = (sc[k] for k in ("hm", "style", "rots", "block", "aff", "depth", "md", "x", "mx", "on", "q64"))
    for j in range(2):
        assert not scene_ref.map_coords(hm, aff[j], 0, 0)[2]
    yk = np.random.default_rng(3).integers(0, 2, size=(2, 81))
    yk[:, [7, 30, 31, 66]] = 2                                                 # four holes inside the block
    assert all((yk[j] == cls).sum() > 20 for j in range(2) for cls in (0, 1))
    lab = np.full((2, hm, hm), 2.0, dtype=np.float32)
    for j in range(2):
        lab[j, block[:, 0], block[:, 1]] = yk[j]
    lab[:, 0, 0] = 0.0
    pix0 = np.concatenate([block, [[0, 0]]])                                   # the oracle's criterion sees pixel (0, 0) too, and drops it

    def total(qs):
        return sum(scene_class_ref.scene_class_loss(qs[j][0], aff[j], hm, pix0, np.concatenate([yk[j], [0]])) for j in range(2))
    loss64 = total(q64)
    loss64.backward()
    g64 = {n: p.grad for n, p in sc["o64"].named_parameters() if p.grad is not None}
    on.zero_grad()
    total([orc.forward(on, x, mx, style, False, r) for r in rots]).backward()

    tr = make_trainer('reactive', 1)
    runs = []
    for it in range(2):
        loss, q = tr.train_batch_scene_class_maps(depth, md, style, rots, lab, return_q=True)
        assert tuple(q.shape) == (2, 3, 3, 3) and tuple(loss.shape) == (2,)
        runs.append(dict(tr.model.named_parameters())[HEAD + "conv1.weight"].grad.clone())
    qh = q.cpu().numpy().astype(np.float64)
    scale = 0.0
    for j in range(2):
        l0, _, terms, W = scene_class_label_ref.autograd(qh[j], aff[j], hm, lab[j])
        assert W == 77 == len(terms)
        own, gate = terms.sum() / W, 2.0 ** -23 * np.abs(terms).sum() / W
        print("sample %d: loss %.7f, fp64 over the same logits %.7f, |d| %.2e (gate %.2e)" % (j, float(loss[j]), own, abs(float(loss[j]) - own), gate))
        assert abs(float(loss[j]) - own) <= gate
        scale = max(scale, float(q64[j].detach().abs().max()))
    gate = 2 * 1e-3 * scale * 2
    print("loss sum %.7f, fp64 oracle %.7f, |d| %.2e (gate %.2e)" % (float(loss.double().sum()), float(loss64.detach()), abs(float(loss.double().sum()) - float(loss64.detach())), gate))
    assert abs(float(loss.double().sum()) - float(loss64.detach())) <= gate
    assert_train_batch_runs(tr, runs, on, g64, "S=704 scene class label maps")
    # the same 77 labelled pixels as a list (the four holes ride along as class-2 padding; pixel (0, 0) would raise there)
    loss_p = tr.train_batch_scene_class_pixels(depth, md, style, rots, np.stack([block, block]), yk)
    a, b = loss.cpu().numpy().astype(np.float64), loss_p.cpu().numpy().astype(np.float64)
    print("label maps", a, "pixel list", b)
    assert (np.abs(a - b) <= 2.0 ** -22 * np.abs(b)).all()
