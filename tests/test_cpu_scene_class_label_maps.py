"""CPU-side checks of the scene-frame class-label-map interface (no GPU): the C ABI declares and exports smg_loss_scene_map_ce and
the binding carries it, the fp64 restatement of tests/scene_class_label_ref.py - autograd over every pixel and the gather by map
element - agree with each other and with scene_class_ref.scene_class_loss, and Trainer.train_batch_scene_class_maps refuses
before it touches the engine."""
import ctypes

import numpy as np
import pytest
import torch

from map_harness import assert_declared_exported_and_bound, cpu_trainer

import scene_class_label_ref
import scene_class_ref
import scene_ref
import smg_hip

ROTS = (0, 3, 8, 13)


def test_loss_scene_map_ce_is_declared_exported_and_bound():
    assert_declared_exported_and_bound(
        "smg_loss_scene_map_ce", r"\bint\s+smg_loss_scene_map_ce\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*const float\*\s*affine_host,\s*int hm_size,\s*"
        r"int n_pairs,\s*const float\*\s*label_dev,\s*float\*\s*loss_dev,\s*float\*\s*dq_dev,\s*void\*\s*stream\)", 9, "loss_scene_map_ce",
        ["train_batch_scene_class_maps"])


def test_a_library_without_the_symbol_is_reported_as_a_stale_build(monkeypatch):
    """The export was added without a version step, so a version-9 library built before it passes the version check: lib() must
    name it a stale build (SmgError, "rebuild it"), not fail with an AttributeError at first use."""
    real = ctypes.CDLL(smg_hip.LIB_PATH)

    class Stale(object):
        def __getattr__(self, name):
            if name == "smg_loss_scene_map_ce":
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(smg_hip, "_lib", None)
    monkeypatch.setattr(smg_hip.C, "CDLL", lambda path: Stale())
    with pytest.raises(smg_hip.SmgError, match="smg_loss_scene_map_ce.*rebuild it"):
        smg_hip.lib()


@pytest.mark.parametrize("hm", [240, 320])
def test_class_label_map_restatement_against_autograd_fp64(hm):
    """(Validates the REFERENCE, tests/scene_class_label_ref.py, not the product: it needs no library and passes without the
    feature.)  Full label images of the recipe's class mix, 4 rotations: the gather by map element - the heightmap box of each
    element's 2x2-cell square, as the kernel walks it, loss and W counted at the home element - against the autograd form: loss to
    1e-12 of sum|terms| / W, dq to 1e-12, W equal, and no box misses a pixel."""
    c = scene_class_label_ref.make_case(hm, ROTS, 16, seed=hm)
    for j in range(4):
        nvalid = int(c["valid"][j].sum())
        print("hm %d rotation %2d: W %d of %d valid, class 0 / 1: %d / %d" % (hm, ROTS[j], c["W"][j], nvalid, c["n0"][j], c["n1"][j]))
        assert 0.6 <= c["W"][j] / nvalid <= 0.8
        assert c["n0"][j] >= 300 and c["n1"][j] >= 300 and c["n0"][j] + c["n1"][j] == c["W"][j]
        assert np.isnan(c["label"][j][~c["valid"][j]]).all()
        lg, dq, st = scene_class_label_ref.gather(c["q"][j], c["aff"][j], hm, c["label"][j])
        err = float(np.abs(dq - c["dq"][j]).max())
        print("    gather loss |d| %.2e, max |ddq| %.2e of %.2e; boxes up to %d, at most %d pixels touch one element"
              % (abs(lg - c["loss"][j]), err, np.abs(c["dq"][j]).max(), st["max_box"], st["max_touch"]))
        assert st["touch"] == st["touch_all"]
        assert st["W"] == c["W"][j]
        assert err <= 1e-12
        assert abs(lg - c["loss"][j]) <= 1e-12 * c["abs_terms"][j] / c["W"][j]


def test_one_point_image_against_the_point_form():
    """(Validates the reference.)  An image with one labelled pixel is scene_class_ref.scene_class_loss on that point."""
    hm = 240
    aff = scene_ref.theta(3, 16)
    _, _, side = scene_ref.geometry(hm)
    q = np.random.default_rng(1).standard_normal((3, side, side))
    assert scene_ref.map_coords(hm, aff, 118, 123)[2]
    for cls in (0, 1):
        lab = np.full((hm, hm), 2.0, dtype=np.float32)
        lab[118, 123] = cls
        qt = torch.from_numpy(q).requires_grad_(True)
        ref = scene_class_ref.scene_class_loss(qt, aff, hm, [(118, 123)], [cls])
        ref.backward()
        l1, g1, terms, W = scene_class_label_ref.autograd(q, aff, hm, lab)
        l2, g2, st = scene_class_label_ref.gather(q, aff, hm, lab)
        assert W == st["W"] == 1 and len(terms) == 1 and float(ref.detach()) > 0
        assert abs(l1 - float(ref.detach())) <= 1e-12 and abs(l2 - float(ref.detach())) <= 1e-12
        assert np.abs(g1 - qt.grad.numpy()).max() <= 1e-12 and np.abs(g2 - qt.grad.numpy()).max() <= 1e-12
        assert int((g2 != 0).sum()) == 12


def test_an_image_without_a_labelled_pixel_gives_zero():
    """(Validates the reference.)  All class 2 - and NaN, and 7 - : loss 0, dq 0, W 0."""
    hm = 240
    aff = scene_ref.theta(3, 16)
    _, _, side = scene_ref.geometry(hm)
    q = np.random.default_rng(2).standard_normal((3, side, side))
    for lab in (np.full((hm, hm), 2.0), np.where(np.arange(hm * hm).reshape(hm, hm) % 2 == 0, np.nan, 7.0)):
        l1, g1, terms, W = scene_class_label_ref.autograd(q, aff, hm, lab)
        l2, g2, st = scene_class_label_ref.gather(q, aff, hm, lab)
        assert l1 == 0.0 and l2 == 0.0 and W == 0 and st["W"] == 0 and len(terms) == 0
        assert not g1.any() and not g2.any()


def test_train_batch_scene_class_maps_has_no_cpu_fallback():
    """A whole image - labelled pixels without a window among them: nothing is raised for those - passes every check and reaches
    the engine, which a CPU trainer does not have."""
    tr = cpu_trainer('reactive')
    d = np.zeros((240, 240))
    lab = np.full((2, 240, 240), 2.0)
    lab[:, 118:123, 118:123] = 1.0
    lab[:, 0, 0] = 0.0                      # no window is centred on heightmap pixel (0, 0)
    with pytest.raises(RuntimeError):
        tr.train_batch_scene_class_maps(d, d, 0, [1, 2], lab)
    with pytest.raises(RuntimeError):
        tr.train_batch_scene_class_maps(np.zeros((2, 240, 240)), np.zeros((2, 240, 240)), 0, [[1], [2]], lab)


def test_train_batch_scene_class_maps_refuses_before_the_engine():
    # (on a CPU trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    d = np.zeros((240, 240))
    ok = np.full((1, 240, 240), 2.0)
    with pytest.raises(ValueError):
        cpu_trainer('reinforcement').train_batch_scene_class_maps(d, d, 0, [1], ok)
    tr = cpu_trainer('reactive')
    d224 = np.zeros((224, 224))              # S = 640: a 1 x 1 map has no extent
    with pytest.raises(ValueError):
        tr.train_batch_scene_class_maps(d224, d224, 0, [1], np.full((1, 224, 224), 2.0))
    with pytest.raises(ValueError):
        tr.train_batch_scene_class_maps(d, d, 0, [1], None)                                          # a missing image
    with pytest.raises(ValueError):
        tr.train_batch_scene_class_maps(d, d, 0, [1, 2], ok)                                         # one sample's image missing
    with pytest.raises(ValueError):
        tr.train_batch_scene_class_maps(d, d, 0, [1], np.full((1, 3, 3), 2.0))                       # a map-frame label map
    with pytest.raises(ValueError):
        tr.train_batch_scene_class_maps(d, d, 0, [1], np.full((240, 240), 2.0))                      # no sample axis
    with pytest.raises(ValueError):
        tr.train_batch_scene_class_maps(np.zeros((2, 240, 240)), np.zeros((2, 240, 240)), 0, [[1], [2, 3]], np.full((2, 240, 240), 2.0))
    for bad in (3.0, -1.0, 0.5, np.nan):
        lab = ok.copy()
        lab[0, 7, 9] = bad
        with pytest.raises(ValueError):
            tr.train_batch_scene_class_maps(d, d, 0, [1], lab)
    # the reinforcement counterpart keeps refusing a reactive trainer
    with pytest.raises(ValueError):
        tr.train_batch_scene_maps(d, d, 0, [1], np.zeros((1, 240, 240)))
