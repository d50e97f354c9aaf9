"""CPU-side checks of the dense class-map interface of the reactive method (no GPU): the C ABI declares and exports
smg_loss_map_ce, the four Trainer entry points exist, refuse a reinforcement trainer, refuse to run without the GPU instead of
falling back to anything, and reject wrong shapes, class indices and pixels before they touch the engine."""
import numpy as np
import pytest

from map_harness import assert_declared_exported_and_bound, cpu_trainer


def test_loss_map_ce_is_declared_exported_and_bound():
    assert_declared_exported_and_bound(
        "smg_loss_map_ce", r"\bint\s+smg_loss_map_ce\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*const float\*\s*label_dev,\s*"
        r"int n_pairs,\s*float\*\s*loss_dev,\s*float\*\s*dq_dev,\s*void\*\s*stream\)", 7, "loss_map_ce")


def test_class_map_entry_points_have_no_cpu_fallback():
    tr = cpu_trainer('reactive')
    d = np.zeros((240, 240))
    with pytest.raises(RuntimeError):
        tr.forward_class_maps(d, d, 0)
    with pytest.raises(RuntimeError):
        tr.best_class_map_action(d, d, 0)
    with pytest.raises(RuntimeError):
        tr.train_batch_class_maps(d, d, 0, [1, 2], np.zeros((2, 3, 3)))
    with pytest.raises(RuntimeError):
        tr.train_batch_class_pixels(d, d, 0, [1, 2], [(0, 0), (2, 1)], [0, 1])


def test_class_map_entry_points_are_for_the_reactive_method():
    tr = cpu_trainer('reinforcement')
    d = np.zeros((240, 240))
    with pytest.raises(ValueError):
        tr.forward_class_maps(d, d, 0)
    with pytest.raises(ValueError):
        tr.best_class_map_action(d, d, 0)
    with pytest.raises(ValueError):
        tr.train_batch_class_maps(d, d, 0, [1], np.zeros((1, 3, 3)))
    with pytest.raises(ValueError):
        tr.train_batch_class_pixels(d, d, 0, [1], [(0, 0)], [1])


def test_train_batch_class_maps_rejects_bad_input_before_the_engine():
    from trainer import Trainer
    assert Trainer.dense_map_size(240) == 3
    tr = cpu_trainer('reactive')
    d = np.zeros((240, 240))                 # S = 704: 3 x 3 maps
    # (on this trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    with pytest.raises(ValueError):
        tr.train_batch_class_maps(d, d, 0, [1, 2], np.zeros((2, 1, 1)))                  # the S = 640 shape
    with pytest.raises(ValueError):
        tr.train_batch_class_maps(d, d, 0, [1, 2], np.zeros((3, 3, 3)))                  # one map too many
    with pytest.raises(ValueError):
        tr.train_batch_class_maps(d, d, 0, [1, 2], np.zeros((2, 3, 3, 3)))               # one map per class is not a label map
    with pytest.raises(ValueError):
        tr.train_batch_class_maps(np.zeros((2, 240, 240)), np.zeros((2, 240, 240)), 0, [[1], [2, 3]], np.zeros((2, 3, 3)))   # 3 samples in 2 scenes
    bad = np.zeros((2, 3, 3))
    bad[1, 2, 0] = 3
    with pytest.raises(ValueError):
        tr.train_batch_class_maps(d, d, 0, [1, 2], bad)                                  # a class index torch's nll_loss would refuse
    with pytest.raises(ValueError):
        tr.train_batch_class_pixels(d, d, 0, [1, 2], [(0, 0), (1, 1)], [0, 3])           # the same through the pixel form
    with pytest.raises(ValueError):
        tr.train_batch_class_pixels(d, d, 0, [1], [(3, 0)], [1])                         # outside the 3 x 3 map
    with pytest.raises(ValueError):
        tr.train_batch_class_pixels(d, d, 0, [1, 2], [(0, 0)], [0, 1])                   # one pixel, two labels
    with pytest.raises(RuntimeError):
        tr.train_batch_class_maps(d, d, 0, [1, 2], np.full((2, 3, 3), 2.0))              # well-formed: only the engine is missing
