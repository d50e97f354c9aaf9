"""The value of scene-frame maps at LISTED heightmap pixels (include/smg_hip.h, smg_scene_values / smg_scene_class_values), the
reference of tests/test_cpu_scene_values.py and tests/test_gpu_scene_values.py.  Plain helper module, no tests.

A value at a pixel is the map form's value there and nothing else, so the reference is a gather: from the fp64 maps of
tests/scene_ref.py / tests/scene_class_ref.py, or - for the bit-for-bit checks - from the float32 maps smg_scene_maps /
smg_scene_class_maps wrote for the same q.  A point outside the heightmap is -inf."""
import numpy as np

import scene_class_ref
import scene_ref


def gather(maps, pixels):
    """maps [n, hm, hm] or [n, C, hm, hm] (any float dtype, kept), pixels int [n, K, 2] = (iy, ix), any integers ->
    [n, K] or [n, C, K]: maps[m, ..., iy, ix], -inf for a point outside [0, hm)^2."""
    maps = np.asarray(maps)
    pix = np.asarray(pixels).astype(np.int64)
    n, hm = maps.shape[0], maps.shape[-1]
    assert pix.ndim == 3 and pix.shape[0] == n and pix.shape[2] == 2 and maps.shape[-2] == hm
    inside = ((pix >= 0) & (pix < hm)).all(axis=2)                     # [n, K]
    iy, ix = np.where(inside, pix[..., 0], 0), np.where(inside, pix[..., 1], 0)
    m = np.arange(n)[:, None]
    if maps.ndim == 3:
        return np.where(inside, maps[m, iy, ix], maps.dtype.type(-np.inf))
    got = np.moveaxis(maps[m, :, iy, ix], -1, 1)                       # [n, K, C] -> [n, C, K]
    return np.where(inside[:, None, :], got, maps.dtype.type(-np.inf))


def values(q, affines, hm, pixels):
    """q [n, OH, OW], affines [n, 6], pixels [n, K, 2] -> float64 [n, K]: scene_ref.scene_maps gathered."""
    return gather(scene_ref.scene_maps(q, affines, hm)[0], pixels)


def class_values(q, affines, hm, pixels):
    """q [n, 3, OH, OW] -> float64 [n, 3, K]: scene_class_ref.scene_class_maps gathered (-inf in all three planes where invalid)."""
    return gather(scene_class_ref.scene_class_maps(q, affines, hm)[0], pixels)
