"""Scene-frame label maps on the MI355X (run with -m gpu): smg_loss_scene_map on an engine alone with synthetic maps against torch
fp64 autograd through tests/scene_ref.py (tests/scene_label_ref.py builds the cases), against smg_loss_scene fed the same pixels
as a list, its masks, groups of more than 32 pairs and refusals, then train_batch_scene_maps against the fp64 PyTorch-CPU oracle
and against train_batch_scene_pixels."""
import contextlib

import numpy as np
import pytest
import torch

from helpers import orc
from map_harness import (assert_bit_identical, assert_scene_loss_refusals, assert_train_batch_runs, assert_written_and_finite, bits,  # noqa: F401
                         border_pixels, cached_engine, filled, gpu, HEAD, make_trainer, s704_scene, stream)

import scene_label_ref
import scene_ref

pytestmark = pytest.mark.gpu

ROTS = (0, 3, 8, 13)
_CASES = {}


def case(hm, rots=ROTS):
    """One reference per shape, shared by the tests and never modified."""
    key = (hm, tuple(rots))
    if key not in _CASES:
        _CASES[key] = scene_label_ref.make_case(hm, rots, 16, seed=hm)
    return _CASES[key]


def run(eng, q, aff, hm, label, weight):
    """One smg_loss_scene_map call on device tensors, outputs pre-filled with -7 -> (loss [n], dq [n, side, side]) on the host."""
    n = q.shape[0]
    loss, dq = filled((n,)), filled(q.shape)
    eng.loss_scene_map(q.data_ptr(), aff, hm, n, label.data_ptr(), None if weight is None else weight.data_ptr(), loss.data_ptr(),
                       dq.data_ptr(), stream())
    return loss.cpu().numpy(), dq.cpu().numpy()[:, 0]


def check_against_fp64(c, what):
    eng = cached_engine(c["S"], 1)
    q, lab, wgt = (torch.from_numpy(c[k]).cuda() for k in ("q", "label", "weight"))
    loss, dq = run(eng, q, c["aff"], c["hm"], lab, wgt)
    for j in range(len(loss)):
        print("%s pair %d: loss %.7f ref %.7f |d| %.2e (gate %.2e); max |ddq| %.2e (gate %.2e); quadratic share %.2f" % (
            what, j, loss[j], c["loss"][j], abs(loss[j] - c["loss"][j]), 2.0 ** -23 * c["abs_terms"][j],
            np.abs(dq[j] - c["dq"][j]).max(), 2.0 ** -23 * np.abs(c["dq"][j]).max(), c["quad"]))
    assert_written_and_finite(-7.0, loss, dq)
    assert (np.abs(loss - c["loss"]) <= 2.0 ** -23 * c["abs_terms"]).all()
    for j in range(len(loss)):
        assert np.abs(dq[j] - c["dq"][j]).max() <= 2.0 ** -23 * np.abs(c["dq"][j]).max()
    loss2, dq2 = run(eng, q, c["aff"], c["hm"], lab, wgt)            # a second call: bit-identical
    assert_bit_identical(loss, loss2)
    assert_bit_identical(dq, dq2)
    return loss, dq


@pytest.mark.parametrize("hm,S,side", ((240, 704, 3), (320, 928, 10)))
def test_loss_scene_map_against_torch_fp64_autograd(gpu, hm, S, side):
    """4 pairs (rotations 0, 3, 8, 13 of 16), full label and weight images: labels on both Huber branches, NaN labels at invalid pixels
    and under the zero weights (every 7th pixel).  Loss within 2^-23 sum|terms|, dq within 2^-23 max|reference dq|, every output
    written and finite, two calls bit-identical."""
    c = case(hm)
    assert (c["S"], c["side"]) == (S, side)
    assert 0.3 <= c["quad"] <= 0.7
    assert np.isnan(c["label"][~c["valid"]]).all() and (c["weight"] == 0).mean() > 0.14
    check_against_fp64(c, "hm=%d" % hm)


def test_loss_scene_map_where_the_heightmap_border_clips_the_boxes(gpu):
    """hm = 448 (S = 1280, 21 x 21 maps): in rotation 2 of 16 valid pixels lie on the image border, so an element's pixel box is cut
    by the heightmap edge (at 240 and 320 the valid area stays inside).  Same gates."""
    c = case(448, (2, 5))
    assert (c["S"], c["side"]) == (1280, 21)
    border = border_pixels(c["valid"][0])
    print("rotation 2: %d valid pixels on the image border" % border)
    assert border > 0
    check_against_fp64(c, "hm=448")


def test_loss_scene_map_groups_of_pairs(gpu):
    """33 pairs at hm = 240 (the second launch carries pair 32 alone), pair 32 with pair 0's inputs: bit-equal results."""
    hm, S, side = 240, 704, 3
    eng = cached_engine(S, 1, pairs=33)
    rng = np.random.default_rng(33)
    rots = list(range(32)) + [0]
    aff = np.stack([scene_ref.theta(r, 32) for r in rots])
    q = rng.standard_normal((33, 1, side, side)).astype(np.float32)
    lab = rng.standard_normal((33, hm, hm)).astype(np.float32) * 1.5
    wgt = rng.uniform(0.2, 1.0, size=(33, hm, hm)).astype(np.float32)
    q[32], lab[32], wgt[32] = q[0], lab[0], wgt[0]
    loss, dq = run(eng, torch.from_numpy(q).cuda(), aff, hm, torch.from_numpy(lab).cuda(), torch.from_numpy(wgt).cuda())
    assert_written_and_finite(-7.0, loss, dq)
    assert loss[0] > 0 and np.abs(dq[0]).max() > 0
    assert_bit_identical(loss[32:33], loss[0:1])
    assert_bit_identical(dq[32], dq[0])
    assert not np.array_equal(dq[31], dq[0])
    l0, g0, terms, _ = scene_label_ref.autograd(q[5, 0], aff[5], hm, lab[5], wgt[5])           # one pair of the first launch against fp64
    assert abs(loss[5] - l0) <= 2.0 ** -23 * np.abs(terms).sum() and np.abs(dq[5] - g0).max() <= 2.0 ** -23 * np.abs(g0).max()


def test_loss_scene_map_with_matrices_that_are_no_rotation(gpu):
    """scene_point asks for no rotation, so neither does this call: a sheared and stretched 2x2 part, one shrunk to half (boxes twice
    as wide) and the zero matrix (no inverse: every workgroup walks the whole heightmap, every pixel lands on the map's centre)
    against torch fp64 autograd with the gates above."""
    hm, S, side = 240, 704, 3
    eng = cached_engine(S, 1)
    aff = scene_label_ref.odd_affines()
    n = len(aff)
    rng = np.random.default_rng(77)
    q = rng.standard_normal((n, 1, side, side)).astype(np.float32)
    lab = (rng.standard_normal((n, hm, hm)) * 1.5).astype(np.float32)
    wgt = rng.uniform(0.2, 1.0, size=(n, hm, hm)).astype(np.float32)
    loss, dq = run(eng, torch.from_numpy(q).cuda(), aff, hm, torch.from_numpy(lab).cuda(), torch.from_numpy(wgt).cuda())
    for j in range(n):
        l0, g0, terms, _ = scene_label_ref.autograd(q[j, 0], aff[j], hm, lab[j], wgt[j])
        print("2x2 part %d: %d pixels, loss %.6f ref %.6f (gate %.2e), max |ddq| %.2e (gate %.2e)" % (
            j, len(terms), loss[j], l0, 2.0 ** -23 * np.abs(terms).sum(), np.abs(dq[j] - g0).max(), 2.0 ** -23 * np.abs(g0).max()))
        assert len(terms) > 700
        assert abs(loss[j] - l0) <= 2.0 ** -23 * np.abs(terms).sum()
        assert np.abs(dq[j] - g0).max() <= 2.0 ** -23 * np.abs(g0).max()
    assert int((dq[2] != 0).sum()) == 1 and dq[2][1, 1] != 0          # the zero matrix: all of it on the centre element


def test_loss_scene_map_against_loss_scene_on_the_same_pixels(gpu):
    """smg_loss_scene fed exactly the valid, weighted pixels of the 320^2 case as a list (pair by pair: K differs): both kernels
    round an fp64 sum of the same terms once, so loss and dq agree to 2^-22 of sum|terms| and max|dq|."""
    c = case(320)
    hm = c["hm"]
    eng = cached_engine(c["S"], 1)
    q, lab, wgt = (torch.from_numpy(c[k]).cuda() for k in ("q", "label", "weight"))
    loss, dq = run(eng, q, c["aff"], hm, lab, wgt)
    for j in range(4):
        pix, keep = scene_label_ref.contributing(hm, c["aff"][j], c["weight"][j])
        K = len(pix)
        assert K > 10000
        pix_d = torch.from_numpy(np.ascontiguousarray(pix, dtype=np.int32)).cuda()
        lab_d, wgt_d = torch.from_numpy(c["label"][j][keep]).cuda(), torch.from_numpy(c["weight"][j][keep]).cuda()
        lj, dj = filled((1,)), filled((1, 1, c["side"], c["side"]))
        eng.loss_scene(q[j:j + 1].data_ptr(), c["aff"][j:j + 1], hm, 1, K, pix_d.data_ptr(), lab_d.data_ptr(), wgt_d.data_ptr(), lj.data_ptr(),
                       dj.data_ptr(), stream())
        lj, dj = float(lj.cpu()[0]), dj.cpu().numpy()[0, 0]
        print("pair %d: K %d, loss %.7f vs %.7f, max |ddq| %.2e of %.2e" % (j, K, loss[j], lj, np.abs(dq[j] - dj).max(), np.abs(dj).max()))
        assert abs(loss[j] - lj) <= 2.0 ** -22 * c["abs_terms"][j]
        assert np.abs(dq[j] - dj).max() <= 2.0 ** -22 * np.abs(dj).max()


def test_loss_scene_map_masks(gpu):
    """All-zero weights: loss 0 and dq exactly 0 everywhere, whatever the labels hold.  NULL weights = explicit ones, bit for bit."""
    c = case(240)
    hm = c["hm"]
    eng = cached_engine(c["S"], 1)
    q = torch.from_numpy(c["q"]).cuda()
    nan_lab = torch.full((4, hm, hm), float("nan"), device="cuda")
    loss, dq = run(eng, q, c["aff"], hm, nan_lab, torch.zeros((4, hm, hm), device="cuda"))
    assert np.array_equal(bits(loss), np.zeros(4, dtype=np.uint32)) and np.array_equal(bits(dq), np.zeros(dq.shape, dtype=np.uint32))
    lab = torch.from_numpy(np.nan_to_num(c["label"], nan=0.25)).cuda()
    loss_null, dq_null = run(eng, q, c["aff"], hm, lab, None)
    loss_ones, dq_ones = run(eng, q, c["aff"], hm, lab, torch.ones((4, hm, hm), device="cuda"))
    assert (loss_null > 0).all() and np.abs(dq_null).max() > 0
    assert_bit_identical(loss_null, loss_ones)
    assert_bit_identical(dq_null, dq_ones)


def test_loss_scene_map_refusals(gpu):
    """-22, a message that names the cause and nothing launched: a 3-class head, a heightmap side that does not pad to the engine's S,
    a 1 x 1 map, n_pairs < 1, an affine matrix with a translation."""
    import smg_hip
    L = smg_hip.lib()
    q = torch.zeros((4, 1, 3, 3), device="cuda")
    lab = torch.zeros((4, 320, 320), device="cuda")
    loss, dq = filled((4,)), filled((4, 3, 3, 3))

    def call(eng, affine, size, n):
        return L.smg_loss_scene_map(eng.h, q.data_ptr(), affine, size, n, lab.data_ptr(), None, loss.data_ptr(), dq.data_ptr(), None)

    def method(eng, affine, size, n):
        eng.loss_scene_map(q.data_ptr(), affine, size, n, lab.data_ptr(), None, loss.data_ptr(), dq.data_ptr(), None)
    assert_scene_loss_refusals(call, method, b"smg_loss_scene_map", 1, 3, lambda S, out_ch: contextlib.nullcontext(cached_engine(S, out_ch)),
                               loss, dq, name_leads=False)


def test_train_batch_scene_maps_vs_fp64_oracle_s704(gpu):
    """test_train_batch_scene_pixels_vs_fp64_oracle_s704's recipe with label IMAGES: a 240^2 heightmap, two samples (rotations 1 and 6
    of 16), weights non-zero on the 9 x 9 block around the centre with four zeros inside, NaN labels wherever the weight is 0, both
    Huber branches.  The loss against fp64 over the product's own q (2^-23 of the terms) and against the fp64 oracle (that test's
    gate), all 368 gradient tensors within 3x the fp32 oracle's own error, the head's conv1 weight gradient identical between two
    runs, and train_batch_scene_pixels on the same 81 pixels gives the same losses to 2^-22."""
    sc = s704_scene(1)
    hm, style, rots, block, aff, depth, md, x, mx, on, q64 = (sc[k] for k in ("hm", "style", "rots", "block", "aff", "depth", "md", "x", "mx", "on", "q64"))
    v64 = [scene_ref.scene_points(q64[j][0, 0], aff[j], hm, block) for j in range(2)]
    rng = np.random.default_rng(3)
    wk = rng.uniform(0.25, 1.0, size=(2, 81)).astype(np.float32)
    wk[:, [7, 30, 31, 66]] = 0.0                                               # a few zeros inside the block
    off = np.tile(np.asarray([0.4, -1.6, 1.6, -0.4]), 21)[:81]                 # |d| = 0.4 (quadratic) and 1.6 (linear)
    lk = np.stack([v.detach().numpy() + off for v in v64]).astype(np.float32)
    lab = np.full((2, hm, hm), np.nan, dtype=np.float32)
    wgt = np.zeros((2, hm, hm), dtype=np.float32)
    for j in range(2):
        lab[j, block[:, 0], block[:, 1]] = np.where(wk[j] != 0, lk[j], np.nan)
        wgt[j, block[:, 0], block[:, 1]] = wk[j]

    def total(vs, dtype):
        return sum((torch.from_numpy(wk[j]).to(dtype) * scene_ref.huber(vs[j] - torch.from_numpy(lk[j]).to(dtype))).sum() for j in range(2))
    loss64 = total(v64, torch.float64)
    loss64.backward()
    g64 = {n: p.grad for n, p in sc["o64"].named_parameters() if p.grad is not None}
    on.zero_grad()
    qo = [orc.forward(on, x, mx, style, False, r) for r in rots]
    total([scene_ref.scene_points(qo[j][0, 0], aff[j], hm, block) for j in range(2)], torch.float32).backward()

    tr = make_trainer('reinforcement', 1)
    runs = []
    for it in range(2):
        loss, q = tr.train_batch_scene_maps(depth, md, style, rots, lab, wgt, return_q=True)
        assert tuple(q.shape) == (2, 1, 3, 3) and tuple(loss.shape) == (2,)
        runs.append(dict(tr.model.named_parameters())[HEAD + "conv1.weight"].grad.clone())
    qh = q.cpu().numpy().astype(np.float64)
    own, scale, branches = 0.0, 0.0, []
    for j in range(2):
        d = scene_ref.scene_points(torch.from_numpy(qh[j, 0]), aff[j], hm, block) - torch.from_numpy(lk[j]).double()
        terms = (torch.from_numpy(wk[j]).double() * scene_ref.huber(d)).numpy()
        branches += (d.abs() < 1)[torch.from_numpy(wk[j] != 0)].tolist()
        err = abs(float(loss[j]) - terms.sum())
        print("sample %d: loss %.7f, fp64 over the same q %.7f, |d| %.2e (gate %.2e)" % (j, float(loss[j]), terms.sum(), err, 2.0 ** -23 * np.abs(terms).sum()))
        assert err <= 2.0 ** -23 * np.abs(terms).sum()
        own += terms.sum()
        scale = max(scale, float(q64[j].detach().abs().max()))
    assert any(branches) and not all(branches)
    gate = 1e-3 * scale * float(wk.sum())       # huber' <= 1, each v a convex combination of q: |d loss| <= sum_k w_k max|dq|
    print("loss sum %.7f, fp64 oracle %.7f, |d| %.2e (gate %.2e)" % (own, float(loss64), abs(own - float(loss64)), gate))
    assert abs(float(loss.double().sum()) - float(loss64)) <= gate
    assert_train_batch_runs(tr, runs, on, g64, "S=704 scene label maps")
    # the same 81 pixels as a list
    loss_p = tr.train_batch_scene_pixels(depth, md, style, rots, np.stack([block, block]), np.nan_to_num(lk), wk)
    a, b = loss.cpu().numpy().astype(np.float64), loss_p.cpu().numpy().astype(np.float64)
    print("label maps", a, "pixel list", b)
    assert (np.abs(a - b) <= 2.0 ** -22 * np.abs(b)).all()
