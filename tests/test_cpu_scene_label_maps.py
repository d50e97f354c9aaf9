"""CPU-side checks of the scene-frame label-map interface (no GPU): the C ABI declares and exports smg_loss_scene_map and the
binding carries it, the fp64 restatement of tests/scene_label_ref.py - map form and gather by map element - agrees with
scene_ref.scene_points + torch autograd, and Trainer.train_batch_scene_maps refuses before it touches the engine."""
import numpy as np
import pytest

from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_label_ref
import scene_ref


def test_loss_scene_map_is_declared_exported_and_bound():
    assert_declared_exported_and_bound(
        "smg_loss_scene_map", r"\bint\s+smg_loss_scene_map\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*const float\*\s*affine_host,\s*int hm_size,\s*"
        r"int n_pairs,\s*const float\*\s*label_dev,\s*const float\*\s*weight_dev,\s*float\*\s*loss_dev,\s*float\*\s*dq_dev,\s*"
        r"void\*\s*stream\)", 10, "loss_scene_map", ["train_batch_scene_maps"])


@pytest.mark.parametrize("hm", [240, 320])
def test_label_map_restatement_against_autograd_fp64(hm):
    """(Validates the REFERENCE, tests/scene_label_ref.py, not the product: it needs no library and passes without the feature.)
    Full label and weight images (both Huber branches, NaN labels at invalid pixels and under the zero weights), 4 rotations:
    the map form's loss against the point form's to 1e-12 relative, the gather by map element - the heightmap box of each
    element's 2x2-cell square, as the kernel walks it - against the autograd dq to 1e-12, and no box misses a pixel."""
    c = scene_label_ref.make_case(hm, (0, 3, 8, 13), 16, seed=hm)
    assert 0.3 <= c["quad"] <= 0.7
    for j in range(4):
        q, aff, lab, wgt = c["q"][j, 0], c["aff"][j], c["label"][j], c["weight"][j]
        lm, terms = scene_label_ref.map_form(q, aff, hm, lab, wgt)
        assert np.isfinite(lm) and abs(lm - c["loss"][j]) <= 1e-12 * c["abs_terms"][j]
        assert abs(np.abs(terms).sum() - c["abs_terms"][j]) <= 1e-12 * c["abs_terms"][j]
        lg, dq, st = scene_label_ref.gather(q, aff, hm, lab, wgt)
        err = float(np.abs(dq - c["dq"][j]).max())
        print("hm %d rotation %2d: gather loss |d| %.2e, max |ddq| %.2e of %.2e; boxes up to %d, at most %d pixels touch one element"
              % (hm, (0, 3, 8, 13)[j], abs(lg - c["loss"][j]), err, np.abs(c["dq"][j]).max(), st["max_box"], st["max_touch"]))
        assert st["touch"] == st["touch_all"]
        assert err <= 1e-12
        assert abs(lg - c["loss"][j]) <= 1e-12 * c["abs_terms"][j]
        # NULL weights: every valid pixel with a finite label
        full = np.nan_to_num(lab, nan=0.5)
        l1, g1, t1, _ = scene_label_ref.autograd(q, aff, hm, full, None)
        l2, g2, st2 = scene_label_ref.gather(q, aff, hm, full, None)
        assert abs(l1 - l2) <= 1e-12 * np.abs(t1).sum() and np.abs(g1 - g2).max() <= 1e-12 * max(1.0, np.abs(g1).max())
        assert len(t1) == int(c["valid"][j].sum())


def test_boxes_hold_every_touching_pixel_where_the_border_clips_them():
    """(Validates the reference's box construction, not the product.)  hm = 448, rotation 2 of 16: valid pixels on the image
    border, boxes cut by the heightmap edge."""
    hm = 448
    aff = scene_ref.theta(2, 16)
    _, _, side = scene_ref.geometry(hm)
    rng = np.random.default_rng(448)
    q = rng.standard_normal((side, side))
    lab = rng.standard_normal((hm, hm)) * 1.5
    l1, g1, t1, _ = scene_label_ref.autograd(q, aff, hm, lab, None)
    l2, g2, st = scene_label_ref.gather(q, aff, hm, lab, None)
    assert st["touch"] == st["touch_all"]
    assert abs(l1 - l2) <= 1e-12 * np.abs(t1).sum() and np.abs(g1 - g2).max() <= 1e-12 * np.abs(g1).max()


def test_boxes_hold_every_touching_pixel_for_matrices_that_are_no_rotation():
    """(Validates the reference's box construction, not the product.)  The box comes from the inverse of A^T, so a sheared,
    stretched or shrunk 2x2 part loses no pixel; a matrix without an inverse walks the whole heightmap."""
    hm = 240
    _, _, side = scene_ref.geometry(hm)
    rng = np.random.default_rng(7)
    q = rng.standard_normal((side, side))
    lab = rng.standard_normal((hm, hm)) * 1.5
    wgt = rng.uniform(0.2, 1.0, size=(hm, hm))
    for aff in scene_label_ref.odd_affines():
        l1, g1, t1, _ = scene_label_ref.autograd(q, aff, hm, lab, wgt)
        l2, g2, st = scene_label_ref.gather(q, aff, hm, lab, wgt)
        print("2x2 part %s: %d contributing pixels, boxes up to %d" % (aff[[0, 1, 3, 4]].tolist(), len(t1), st["max_box"]))
        assert len(t1) > 700 and st["touch"] == st["touch_all"]
        assert abs(l1 - l2) <= 1e-12 * np.abs(t1).sum() and np.abs(g1 - g2).max() <= 1e-12 * np.abs(g1).max()
    assert scene_label_ref.element_box(hm, scene_label_ref.odd_affines()[2], 1, 1) == (0, hm - 1, 0, hm - 1)


def test_train_batch_scene_maps_has_no_cpu_fallback():
    """Whole images with invalid pixels under them pass every check (nothing is raised for pixels without a window) and reach the
    engine, which a CPU trainer does not have."""
    tr = cpu_trainer('reinforcement')
    d = np.zeros((240, 240))
    with pytest.raises(RuntimeError):
        tr.train_batch_scene_maps(d, d, 0, [1, 2], np.zeros((2, 240, 240)), np.ones((2, 240, 240)))
    with pytest.raises(RuntimeError):
        tr.train_batch_scene_maps(d, d, 0, [1], np.zeros((1, 240, 240)))


def test_train_batch_scene_maps_refuses_before_the_engine():
    # (on a CPU trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    d = np.zeros((240, 240))
    with pytest.raises(ValueError):
        cpu_trainer('reactive').train_batch_scene_maps(d, d, 0, [1], np.zeros((1, 240, 240)))
    tr = cpu_trainer('reinforcement')
    d224 = np.zeros((224, 224))              # S = 640: a 1 x 1 map has no extent
    with pytest.raises(ValueError):
        tr.train_batch_scene_maps(d224, d224, 0, [1], np.zeros((1, 224, 224)))
    with pytest.raises(ValueError):
        tr.train_batch_scene_maps(d, d, 0, [1], None)                                                # labels are not optional
    with pytest.raises(ValueError):
        tr.train_batch_scene_maps(d, d, 0, [1, 2], np.zeros((1, 240, 240)))                          # one sample's image missing
    with pytest.raises(ValueError):
        tr.train_batch_scene_maps(d, d, 0, [1], np.zeros((1, 3, 3)))                                 # a map-frame label map
    with pytest.raises(ValueError):
        tr.train_batch_scene_maps(d, d, 0, [1], np.zeros((240, 240)))                                # no sample axis
    with pytest.raises(ValueError):
        tr.train_batch_scene_maps(d, d, 0, [1], np.zeros((1, 240, 240)), np.ones((1, 240, 239)))     # weights of another shape
    with pytest.raises(ValueError):
        tr.train_batch_scene_maps(np.zeros((2, 240, 240)), np.zeros((2, 240, 240)), 0, [[1], [2, 3]], np.zeros((2, 240, 240)))
