"""CPU-side checks of the reactive net's scene-frame interface (no GPU): the C ABI declares and exports smg_scene_class_maps /
smg_scene_class_argmax / smg_loss_scene_ce (ABI version 8), the fp64 restatement (tests/scene_class_ref.py) agrees with a softmax
over torch's own bilinear grid_sample of the logits, its point form is torch's weighted nll_loss, and the Python entry points
refuse - a reinforcement trainer, a 224^2 heightmap, bad labels, shapes and pixels - before they touch the engine, while the
reinforcement scene-frame entry points keep refusing a reactive trainer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_class_ref
import scene_ref


def test_scene_class_entry_points_are_declared_exported_and_bound():
    assert_declared_exported_and_bound(
        "smg_scene_class_maps", r"\bint\s+smg_scene_class_maps\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int n_maps,\s*const float\*\s*affine_host,\s*"
        r"int hm_size,\s*int cls,\s*float\*\s*out_dev,\s*void\*\s*stream\)", 8, "scene_class_maps")
    assert_declared_exported_and_bound(
        "smg_scene_class_argmax", r"\bint\s+smg_scene_class_argmax\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int n_maps,\s*const float\*\s*affine_host,\s*"
        r"int hm_size,\s*int cls,\s*int\*\s*idx_out_dev,\s*float\*\s*val_out_dev,\s*void\*\s*stream\)", 9, "scene_class_argmax")
    assert_declared_exported_and_bound(
        "smg_loss_scene_ce", r"\bint\s+smg_loss_scene_ce\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*const float\*\s*affine_host,\s*int hm_size,\s*"
        r"int n_pairs,\s*int K,\s*const int\*\s*pixels_dev,\s*const float\*\s*label_dev,\s*float\*\s*loss_dev,\s*float\*\s*dq_dev,\s*"
        r"void\*\s*stream\)", 11, "loss_scene_ce")


@pytest.mark.parametrize("hm,R", [(240, 16), (320, 16)])
def test_scene_class_ref_agrees_with_softmax_of_grid_sample_fp64(hm, R):
    """The map form against softmax(F.grid_sample(logits, bilinear, border, align_corners=True), dim=1) in fp64 on a grid built
    from the map coordinates themselves, on every valid pixel, to 1e-12 (test_scene_ref_agrees_with_grid_sample_fp64's tolerance
    on the logits; a softmax - 1-Lipschitz, values in [0, 1] - of logits that close adds nothing of that order)."""
    _, S, side = scene_ref.geometry(hm)
    rng = np.random.default_rng(hm + 3)
    q = 2.0 * rng.standard_normal((R, 3, side, side))
    aff = [scene_ref.theta(r, R) for r in range(R)]
    out, valid, _ = scene_class_ref.scene_class_maps(q, aff, hm)
    assert out.shape == (R, 3, hm, hm) and valid.shape == (R, hm, hm)
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    worst = 0.0
    for r in range(R):
        qy, qx, v, _ = scene_ref.map_coords(hm, aff[r], iy, ix)
        assert np.array_equal(v, valid[r]) and v.sum() >= 1000
        grid = torch.from_numpy(np.stack([2 * qx / (side - 1) - 1, 2 * qy / (side - 1) - 1], axis=-1))[None]
        gs = F.grid_sample(torch.from_numpy(q[r])[None], grid, mode="bilinear", padding_mode="border", align_corners=True)
        p = torch.softmax(gs, dim=1)[0].numpy()
        worst = max(worst, float(np.abs(p[:, v] - out[r][:, v]).max()))
        assert np.isneginf(out[r][:, ~v]).all()
        assert float(np.abs(out[r][:, v].sum(axis=0) - 1.0).max()) <= 1e-15 * 4
    print("hm %d: max |scene_class_ref - softmax(grid_sample)| %.2e on valid pixels" % (hm, worst))
    assert worst <= 1e-12


def test_scene_class_ref_point_form_is_the_weighted_nll_loss():
    """scene_class_loss on valid labelled points equals F.nll_loss(F.log_softmax(z), y, weight = {1, 1, 0}) of the interpolated
    logits (fp64, 1e-14: the same arithmetic in another order), ignores an invalid point and a class-2 point over non-finite
    logits, and gives 0 with a zero gradient when nothing is labelled."""
    hm = 320
    side = scene_ref.geometry(hm)[2]
    aff = scene_ref.theta(3, 16)
    q = (2.0 * torch.randn((3, side, side), generator=torch.Generator().manual_seed(5))).double()
    pix = np.asarray([(150, 160), (171, 144), (120, 200), (150, 160)])
    y = np.asarray([0, 1, 2, 1])
    assert scene_ref.map_coords(hm, aff, pix[:, 0], pix[:, 1])[2].all() and not scene_ref.map_coords(hm, aff, 0, 0)[2]
    z = scene_class_ref.scene_class_points(q, aff, hm, pix)
    want = F.nll_loss(F.log_softmax(z, dim=1), torch.from_numpy(y), weight=torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64))
    got = scene_class_ref.scene_class_loss(q, aff, hm, pix, y)
    assert abs(float(got) - float(want)) <= 1e-14 * abs(float(want))
    with_corner = scene_class_ref.scene_class_loss(q, aff, hm, np.concatenate([pix, [(0, 0)]]), np.concatenate([y, [0]]))
    assert float(with_corner) == float(got)
    qn = q.clone()

    def cell(p):
        qy, qx = scene_ref.map_coords(hm, aff, p[0], p[1])[:2]
        return [int(v) for v in scene_ref.corners(qy, qx, side)[:2]]

    (y0, x0), (ya, xa) = cell(pix[2]), cell(pix[0])
    assert max(abs(y0 - ya), abs(x0 - xa)) >= 2                 # the class-2 point shares no corner with point 0
    qn[0, y0, x0], qn[1, y0 + 1, x0 + 1] = float("inf"), float("nan")
    pts = [0, 2]
    assert float(scene_class_ref.scene_class_loss(qn, aff, hm, pix[pts], y[pts])) == float(scene_class_ref.scene_class_loss(q, aff, hm, pix[pts], y[pts]))
    qg = q.clone().requires_grad_(True)
    none = scene_class_ref.scene_class_loss(qg, aff, hm, pix[2:3], y[2:3])
    none.backward()
    assert float(none.detach()) == 0.0 and bool((qg.grad == 0).all())


def test_scene_class_entry_points_have_no_cpu_fallback():
    tr = cpu_trainer('reactive')
    d = np.zeros((240, 240))
    with pytest.raises(RuntimeError):
        tr.forward_scene_class_maps(d, d, 0)
    with pytest.raises(RuntimeError):
        tr.forward_scene_class_maps(d, d, 0, cls=1, logits=True)
    with pytest.raises(RuntimeError):
        tr.best_scene_class_action(d, d, 0)
    with pytest.raises(RuntimeError):
        tr.train_batch_scene_class_pixels(d, d, 0, [1, 2], [[(120, 120), (118, 121)], [(119, 119), (120, 122)]], [[0, 1], [1, 2]])
    with pytest.raises(RuntimeError):
        tr.train_batch_scene_class_pixels(d, d, 0, [1, 2], [(120, 120), (119, 119)], [0, 1])         # K = 1 form
    with pytest.raises(RuntimeError):                   # a class-2 padding point needs no window: (0, 0) passes the checks
        tr.train_batch_scene_class_pixels(d, d, 0, [1], [[(120, 120), (0, 0)]], [[1, 2]])


def test_scene_class_entry_points_are_for_the_reactive_method():
    tr = cpu_trainer('reinforcement')
    d = np.zeros((240, 240))
    with pytest.raises(ValueError):
        tr.forward_scene_class_maps(d, d, 0)
    with pytest.raises(ValueError):
        tr.best_scene_class_action(d, d, 0)
    with pytest.raises(ValueError):
        tr.train_batch_scene_class_pixels(d, d, 0, [1], [(120, 120)], [0])


def test_reinforcement_scene_entry_points_still_refuse_a_reactive_trainer():
    tr = cpu_trainer('reactive')
    d = np.zeros((240, 240))
    with pytest.raises(ValueError):
        tr.forward_scene(d, d, 0)
    with pytest.raises(ValueError):
        tr.best_scene_action(d, d, 0)
    with pytest.raises(ValueError):
        tr.train_batch_scene_pixels(d, d, 0, [1], [(120, 120)], [0.5])


def test_scene_class_entry_points_refuse_before_the_engine():
    tr = cpu_trainer('reactive')
    d = np.zeros((240, 240))                 # S = 704: 3 x 3 maps, valid pixels around the centre only
    # (on this trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    from trainer import Trainer
    assert not Trainer.scene_to_map(240, 1, 16, (0, 0))[2] and Trainer.scene_to_map(240, 1, 16, (120, 120))[2]
    train = tr.train_batch_scene_class_pixels
    with pytest.raises(ValueError):
        train(d, d, 0, [1], [(120, 120)], [3])                                              # a label outside {0, 1, 2}
    with pytest.raises(ValueError):
        train(d, d, 0, [1], [(120, 120)], [0.5])
    with pytest.raises(ValueError):
        train(d, d, 0, [1], [(0, 0)], [0])                                                  # a class-0 pixel without a window
    with pytest.raises(ValueError):
        train(d, d, 0, [1, 2], [[(120, 120), (0, 0)], [(120, 120), (119, 119)]], [[0, 1], [1, 0]])
    with pytest.raises(ValueError):
        train(d, d, 0, [1], [(120, 240)], [0])                                              # outside the heightmap
    with pytest.raises(ValueError):
        train(d, d, 0, [1], [[(120, 120), (-1, 5)]], [[0, 2]])                              # padding must lie in the heightmap too
    with pytest.raises(ValueError):
        train(d, d, 0, [1], [(120.5, 120)], [0])                                            # not an integer pixel
    with pytest.raises(ValueError):
        train(d, d, 0, [1, 2], [(120, 120)], [0, 1])                                        # one sample's pixels missing
    with pytest.raises(ValueError):
        train(d, d, 0, [1, 2], np.zeros((2, 2, 3)) + 120, np.zeros((2, 2)))                 # not (iy, ix) pairs
    with pytest.raises(ValueError):
        train(d, d, 0, [1, 2], np.zeros((2, 2, 2)) + 120, np.zeros((2, 3)))                 # labels of another K
    with pytest.raises(ValueError):
        tr.forward_scene_class_maps(d, d, 0, cls=3)
    d224 = np.zeros((224, 224))              # S = 640: a 1 x 1 map has no extent
    with pytest.raises(ValueError):
        tr.forward_scene_class_maps(d224, d224, 0)
    with pytest.raises(ValueError):
        tr.best_scene_class_action(d224, d224, 0)
    with pytest.raises(ValueError):
        train(d224, d224, 0, [1], [(112, 112)], [0])
