"""CPU-side checks of the dense-Q-map interface (no GPU): the C ABI declares and exports smg_loss_map, the Python entry
points exist and - like every other entry point - refuse to run without the GPU instead of falling back to anything, and
train_batch_maps rejects label / weight maps of the wrong shape before it touches the engine."""
import numpy as np
import pytest

from map_harness import assert_declared_exported_and_bound, cpu_trainer


def test_loss_map_is_declared_exported_and_bound():
    hdr = assert_declared_exported_and_bound(
        "smg_loss_map", r"\bint\s+smg_loss_map\s*\(\s*smg_engine\*\s*e,\s*const float\*\s*q_dev,\s*const float\*\s*label_dev,\s*"
        r"const float\*\s*weight_dev,\s*int n_pairs,\s*float\*\s*loss_dev,\s*float\*\s*dq_dev,\s*void\*\s*stream\)", 8, "loss_map")
    assert '"head_bwd"' in hdr


def test_dense_map_size_follows_the_network_strides():
    from trainer import Trainer
    # heightmap side -> padded input S -> S / 32 feature rows -> 20x20 valid convolution
    assert [Trainer.dense_map_size(h) for h in (224, 240, 320, 640)] == [1, 3, 10, 38]


def test_dense_entry_points_have_no_cpu_fallback():
    tr = cpu_trainer('reinforcement')
    d = np.zeros((240, 240))
    with pytest.raises(RuntimeError):
        tr.forward_dense(d, d, 0)
    with pytest.raises(RuntimeError):
        tr.best_dense_action(d, d, 0)
    with pytest.raises(RuntimeError):
        tr.train_batch_maps(d, d, 0, [1, 2], np.zeros((2, 3, 3)), np.ones((2, 3, 3)))
    with pytest.raises(RuntimeError):
        tr.train_batch_pixels(d, d, 0, [1, 2], [(0, 0), (2, 1)], [0.5, 1.5])


def test_train_batch_maps_rejects_wrong_shapes_before_the_engine():
    tr = cpu_trainer('reinforcement')
    d = np.zeros((240, 240))                 # S = 704: 3 x 3 maps
    # (on this trainer anything that reaches the engine raises RuntimeError: a ValueError proves the check came first)
    with pytest.raises(ValueError):
        tr.train_batch_maps(d, d, 0, [1, 2], np.zeros((2, 1, 1)))                        # the S = 640 shape
    with pytest.raises(ValueError):
        tr.train_batch_maps(d, d, 0, [1, 2], np.zeros((3, 3, 3)))                        # one map too many
    with pytest.raises(ValueError):
        tr.train_batch_maps(d, d, 0, [1, 2], np.zeros((2, 3, 3)), np.ones((2, 3, 4)))    # weight map of another shape
    with pytest.raises(ValueError):
        tr.train_batch_maps(np.zeros((2, 240, 240)), np.zeros((2, 240, 240)), 0, [[1], [2, 3]], np.zeros((2, 3, 3)))   # 3 samples in 2 scenes
    with pytest.raises(ValueError):
        tr.train_batch_pixels(d, d, 0, [1], [(3, 0)], [0.5])                             # outside the 3 x 3 map
    with pytest.raises(ValueError):
        tr.train_batch_pixels(d, d, 0, [1, 2], [(0, 0)], [0.5, 0.1])


def test_dense_training_is_for_the_reinforcement_method():
    tr = cpu_trainer('reactive')
    d = np.zeros((240, 240))
    with pytest.raises(ValueError):
        tr.train_batch_maps(d, d, 0, [1], np.zeros((1, 3, 3)))
    with pytest.raises(ValueError):
        tr.forward_dense(d, d, 0)
