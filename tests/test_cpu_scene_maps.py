"""CPU-side checks of the scene-frame Q map interface (no GPU): the C ABI declares and exports smg_scene_maps / smg_scene_argmax /
smg_loss_scene, the fp64 restatement of the geometry (tests/scene_ref.py) agrees with torch's own bilinear grid_sample and with
Trainer.scene_to_map, known answers pin the window geometry and the rotation, and the Python entry points refuse - without a
GPU, for a reactive trainer, for invalid pixels, wrong shapes and a 224^2 heightmap - before they touch the engine."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_ref


def test_scene_entry_points_are_declared_exported_and_bound():
    assert_declared_exported_and_bound(
        "smg_scene_maps", r"\bint\s+smg_scene_maps\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int64_t map_stride,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*float\*\s*out_dev,\s*void\*\s*stream\)", 8, "scene_maps")
    assert_declared_exported_and_bound(
        "smg_scene_argmax", r"\bint\s+smg_scene_argmax\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*int64_t map_stride,\s*int n_maps,\s*"
        r"const float\*\s*affine_host,\s*int hm_size,\s*int\*\s*idx_out_dev,\s*float\*\s*val_out_dev,\s*void\*\s*stream\)", 9, "scene_argmax")
    assert_declared_exported_and_bound(
        "smg_loss_scene", r"\bint\s+smg_loss_scene\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*const float\*\s*affine_host,\s*int hm_size,\s*"
        r"int n_pairs,\s*int K,\s*const int\*\s*pixels_dev,\s*const float\*\s*label_dev,\s*const float\*\s*weight_dev,\s*"
        r"float\*\s*loss_dev,\s*float\*\s*dq_dev,\s*void\*\s*stream\)", 12, "loss_scene")


@pytest.mark.parametrize("hm,R", [(240, 16), (320, 16)])
def test_scene_ref_agrees_with_grid_sample_fp64(hm, R):
    """The map form against F.grid_sample(bilinear, border, align_corners=True) in fp64 on a grid built from the map coordinates
    themselves (no affine_grid): the interpolation and the clamp of the last cell, on every valid pixel, to 1e-12."""
    _, S, side = scene_ref.geometry(hm)
    rng = np.random.default_rng(hm)
    q = rng.standard_normal((R, side, side))
    aff = [scene_ref.theta(r, R) for r in range(R)]
    out, valid, _ = scene_ref.scene_maps(q, aff, hm)
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    worst, fewest = 0.0, hm * hm
    for r in range(R):
        qy, qx, v, _ = scene_ref.map_coords(hm, aff[r], iy, ix)
        assert np.array_equal(v, valid[r])
        grid = torch.from_numpy(np.stack([2 * qx / (side - 1) - 1, 2 * qy / (side - 1) - 1], axis=-1))[None]
        gs = F.grid_sample(torch.from_numpy(q[r])[None, None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0, 0].numpy()
        worst = max(worst, float(np.abs(gs[v] - out[r][v]).max()))
        fewest = min(fewest, int(v.sum()))
        assert np.isneginf(out[r][~v]).all()
    print("hm %d: max |scene_ref - grid_sample| %.2e on valid pixels; smallest valid area per rotation %d pixels" % (hm, worst, fewest))
    assert worst <= 1e-12
    assert fewest >= 1000


def test_trainer_scene_to_map_equals_scene_ref():
    from trainer import Trainer
    for hm, R in ((240, 16), (320, 16), (640, 32)):
        rng = np.random.default_rng(hm)
        pix = rng.integers(0, hm, size=(5, 40, 2))
        for r in (0, 1, R // 2, R - 3):
            qy, qx, valid = Trainer.scene_to_map(hm, r, R, pix)
            ry, rx, rv, _ = scene_ref.map_coords(hm, scene_ref.theta(r, R), pix[..., 0], pix[..., 1])
            assert qy.shape == (5, 40) and valid.dtype == bool
            assert np.array_equal(qy, ry) and np.array_equal(qx, rx) and np.array_equal(valid, rv)
        # one rotation per sample, as train_batch_scene_pixels asks
        rots = np.asarray([0, 3, 8, 13, 5]).reshape(5, 1)
        qy, qx, valid = Trainer.scene_to_map(hm, rots, R, pix)
        for j in range(5):
            ry, rx, rv, _ = scene_ref.map_coords(hm, scene_ref.theta(int(rots[j, 0]), R), pix[j, :, 0], pix[j, :, 1])
            assert np.array_equal(qy[j], ry) and np.array_equal(qx[j], rx) and np.array_equal(valid[j], rv)


def test_known_answer_window_centres_at_rotation_zero():
    """hm = 320: pad 144, S = 928, 10 x 10 windows.  Window ox is centred on input pixel 32 ox + 319.5, heightmap pixel ix on
    2 ix + 144.5: ix = 16 ox + 87.5, so the nearest pixels 16 ox + 87 / + 88 sit 1/32 of a cell to either side (one input pixel) - and read a one-hot
    map at that element as (1 - 1/32)^2."""
    hm = 320
    assert scene_ref.geometry(hm) == (144, 928, 10)
    th = scene_ref.theta(0, 16)
    assert th.tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    for oy, ox in ((0, 0), (3, 7), (9, 9), (9, 0)):
        for dy, dx in ((87, 87), (88, 88), (87, 88)):
            iy, ix = 16 * oy + dy, 16 * ox + dx
            qy, qx, valid, _ = scene_ref.map_coords(hm, th, iy, ix)
            assert valid == (qy >= 0 and qx >= 0 and qy <= 9 and qx <= 9)
            assert abs(qy - (oy + (-1 if dy == 87 else 1) / 32)) <= 1e-12 and abs(qx - (ox + (-1 if dx == 87 else 1) / 32)) <= 1e-12
            if valid:
                q = np.zeros((1, 10, 10))
                q[0, oy, ox] = 1.0
                out, _, _ = scene_ref.scene_maps(q, [th], hm)
                assert abs(out[0, iy, ix] - (1 - 1 / 32) ** 2) <= 1e-12
    # the outermost valid pixels: the first / last window centres, nothing beyond them
    _, _, valid, _ = scene_ref.map_coords(hm, th, np.arange(hm), np.arange(hm))
    assert np.flatnonzero(valid)[[0, -1]].tolist() == [88, 16 * 9 + 87]


def test_known_answer_half_turn_mirrors_the_scene():
    """Rotation 8 of 16 is a half turn: heightmap pixel (iy, ix) lies on its map where the mirrored pixel (hm-1-iy, hm-1-ix) lies
    on rotation 0's (cos(pi) is exactly -1 in float32, sin(pi) rounds to 1.2e-16: the tolerance is for that)."""
    hm = 320
    rng = np.random.default_rng(1)
    pix = rng.integers(0, hm, size=(200, 2))
    qy8, qx8, v8, _ = scene_ref.map_coords(hm, scene_ref.theta(8, 16), pix[:, 0], pix[:, 1])
    qy0, qx0, v0, _ = scene_ref.map_coords(hm, scene_ref.theta(0, 16), hm - 1 - pix[:, 0], hm - 1 - pix[:, 1])
    assert np.abs(qy8 - qy0).max() <= 1e-9 and np.abs(qx8 - qx0).max() <= 1e-9
    assert np.array_equal(v8, v0) and v8.any() and not v8.all()
    # and a quarter turn (4 of 16) is NOT its own mirror: the sense of the rotation matters
    qy4, qx4, _, _ = scene_ref.map_coords(hm, scene_ref.theta(4, 16), pix[:, 0], pix[:, 1])
    qym, qxm, _, _ = scene_ref.map_coords(hm, scene_ref.theta(12, 16), pix[:, 0], pix[:, 1])
    assert np.abs(qy4 - qym).max() > 1.0


def test_rotation_sense_against_the_forward_own_rotation():
    """The anchor of the rotation's sense: the oracle's own rotate (F.affine_grid + F.grid_sample nearest, code/models.py:378-382)
    moves the 2x2 input block of a heightmap pixel to where the chain says that pixel is seen - (px, py) = 32 q + 319.5 - to within
    the nearest-neighbour sampling (the block's copies lie within 1.5 input pixels of its rotated centre).  A transposed or
    sign-flipped rotation misses by tens of pixels at every rotation but 0 and 8."""
    from helpers import orc
    hm = 240
    pad, S, _ = scene_ref.geometry(hm)
    for r in (1, 5, 11, 14):
        for iy, ix in ((120, 120), (60, 150), (200, 101), (95, 33)):
            img = torch.zeros((1, 1, S, S))
            img[0, 0, 2 * iy + pad:2 * iy + pad + 2, 2 * ix + pad:2 * ix + pad + 2] = 1.0
            rot = orc.rotate(img, r, 16)[0, 0].numpy()
            ys, xs = np.nonzero(rot)
            assert len(ys) >= 1, (r, iy, ix)
            qy, qx, _, _ = scene_ref.map_coords(hm, scene_ref.theta(r, 16), iy, ix)
            px, py = 32.0 * qx + 319.5, 32.0 * qy + 319.5
            assert np.abs(xs - px).max() <= 1.5 and np.abs(ys - py).max() <= 1.5, (r, iy, ix, px, py, xs, ys)


def test_scene_entry_points_have_no_cpu_fallback():
    tr = cpu_trainer('reinforcement')
    d = np.zeros((240, 240))
    with pytest.raises(RuntimeError):
        tr.forward_scene(d, d, 0)
    with pytest.raises(RuntimeError):
        tr.best_scene_action(d, d, 0)
    with pytest.raises(RuntimeError):
        tr.train_batch_scene_pixels(d, d, 0, [1, 2], [[(120, 120), (118, 121)], [(119, 119), (120, 122)]], [[0.5, 1.5], [0.1, 0.2]])
    with pytest.raises(RuntimeError):
        tr.train_batch_scene_pixels(d, d, 0, [1, 2], [(120, 120), (119, 119)], [0.5, 1.5])          # K = 1 form


def test_scene_entry_points_are_for_the_reinforcement_method():
    tr = cpu_trainer('reactive')
    d = np.zeros((240, 240))
    with pytest.raises(ValueError):
        tr.forward_scene(d, d, 0)
    with pytest.raises(ValueError):
        tr.best_scene_action(d, d, 0)
    with pytest.raises(ValueError):
        tr.train_batch_scene_pixels(d, d, 0, [1], [(120, 120)], [0.5])


def test_train_batch_scene_pixels_refuses_before_the_engine():
    tr = cpu_trainer('reinforcement')
    d = np.zeros((240, 240))                 # S = 704: 3 x 3 maps, valid pixels around the centre only
    # (on this trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    from trainer import Trainer
    assert not Trainer.scene_to_map(240, 1, 16, (0, 0))[2] and Trainer.scene_to_map(240, 1, 16, (120, 120))[2]
    with pytest.raises(ValueError):
        tr.train_batch_scene_pixels(d, d, 0, [1], [(0, 0)], [0.5])                                   # no window is centred on a corner
    with pytest.raises(ValueError):
        tr.train_batch_scene_pixels(d, d, 0, [1, 2], [[(120, 120), (0, 0)], [(120, 120), (119, 119)]], np.zeros((2, 2)))
    with pytest.raises(ValueError):
        tr.train_batch_scene_pixels(d, d, 0, [1], [(120, 240)], [0.5])                               # outside the heightmap
    with pytest.raises(ValueError):
        tr.train_batch_scene_pixels(d, d, 0, [1, 2], [(120, 120)], [0.5, 0.1])                       # one sample's pixels missing
    with pytest.raises(ValueError):
        tr.train_batch_scene_pixels(d, d, 0, [1, 2], np.zeros((2, 2, 3)) + 120, np.zeros((2, 2)))    # not (iy, ix) pairs
    with pytest.raises(ValueError):
        tr.train_batch_scene_pixels(d, d, 0, [1, 2], np.zeros((2, 2, 2)) + 120, np.zeros((2, 3)))    # labels of another K
    with pytest.raises(ValueError):
        tr.train_batch_scene_pixels(d, d, 0, [1, 2], np.zeros((2, 2, 2)) + 120, np.zeros((2, 2)), np.ones((2, 1)))
    d224 = np.zeros((224, 224))              # S = 640: a 1 x 1 map has no extent
    with pytest.raises(ValueError):
        tr.forward_scene(d224, d224, 0)
    with pytest.raises(ValueError):
        tr.best_scene_action(d224, d224, 0)
    with pytest.raises(ValueError):
        tr.train_batch_scene_pixels(d224, d224, 0, [1], [(112, 112)], [0.5])
    with pytest.raises(ValueError):
        Trainer.scene_to_map(224, 0, 16, (112, 112))
