"""fp64 restatement of the scene-frame geometry of dense Q maps (include/smg_hip.h, "dense Q maps in the scene frame"), the
reference of tests/test_cpu_scene_maps.py and tests/test_gpu_scene_maps.py.  Plain helper module, no tests.

Map form (numpy): every heightmap pixel of every map.  Point form (torch): the interpolated value at given heightmap pixels as a
differentiable function of the map, so autograd gives dq.

Coordinates are (x = column, y = row).  For a heightmap of side hm:
    pad = int((ceil(2 hm sqrt(2) / 32) * 32 - 2 hm) / 2),  S = 2 hm + 2 pad,  OH = OW = S / 32 - 19
    x = 2 ix + 0.5 + pad                 centre of the pixel's 2x2 block of the padded input
    u = 2 (x, y) / (S - 1) - 1           align_corners=True
    p = A^T u                            A = 2x2 part of the sample's float32 theta; the forward computed rotated[p] = image[A p]
    (px, py) = (p + 1) / 2 * (S - 1)
    qx = (px - 319.5) / 32               map element ox = the 20x20 window over input pixels 32 ox .. 32 ox + 639
valid: 0 <= qx <= OW - 1 and 0 <= qy <= OH - 1; value: bilinear at (qy, qx) with x0 = min(floor(qx), OW - 2)."""
import numpy as np
import torch


def geometry(hm):
    """(pad, S, side) of a hm^2 heightmap."""
    hm = int(hm)
    pad = int((np.ceil(float(2 * hm) * np.sqrt(2) / 32) * 32 - 2 * hm) / 2)
    S = 2 * hm + 2 * pad
    return pad, S, S // 32 - 19


def theta(rotation, num_rotations):
    """The six float32 numbers of code/models.py:372-376 (float64 trig, then .float()), restated here independently."""
    t = np.radians(rotation * (360 / num_rotations))
    return np.asarray([np.cos(-t), np.sin(-t), 0, -np.sin(-t), np.cos(-t), 0]).astype(np.float32)


def scene_u(hm, iy, ix):
    """Normalised scene coordinates (ux, uy) of heightmap pixels."""
    pad, S, _ = geometry(hm)
    x = 2.0 * np.asarray(ix, dtype=np.float64) + 0.5 + pad
    y = 2.0 * np.asarray(iy, dtype=np.float64) + 0.5 + pad
    return 2.0 * x / (S - 1) - 1.0, 2.0 * y / (S - 1) - 1.0


def map_coords(hm, affine, iy, ix):
    """(qy, qx, valid, margin) of heightmap pixels on the map of the sample with `affine` (6 float32); margin = distance to the
    nearest validity boundary in map units."""
    _, S, side = geometry(hm)
    a = np.asarray(affine, dtype=np.float32).astype(np.float64).reshape(6)
    ux, uy = scene_u(hm, iy, ix)
    pxn = a[0] * ux + a[3] * uy          # A^T u
    pyn = a[1] * ux + a[4] * uy
    px, py = (pxn + 1.0) / 2.0 * (S - 1), (pyn + 1.0) / 2.0 * (S - 1)
    qx, qy = (px - 319.5) / 32.0, (py - 319.5) / 32.0
    valid = (qx >= 0) & (qx <= side - 1) & (qy >= 0) & (qy <= side - 1)
    margin = np.minimum(np.minimum(np.abs(qx), np.abs(qx - (side - 1))), np.minimum(np.abs(qy), np.abs(qy - (side - 1))))
    return qy, qx, valid, margin


def corners(qy, qx, side):
    """(y0, x0, fy, fx) of valid map coordinates."""
    x0 = np.minimum(np.floor(qx), side - 2).astype(np.int64)
    y0 = np.minimum(np.floor(qy), side - 2).astype(np.int64)
    return y0, x0, qy - y0, qx - x0


def scene_maps(q, affines, hm):
    """Map form: q [n, OH, OW] (any float dtype, widened to float64), affines [n, 6] -> (values float64 [n, hm, hm] with -inf at
    invalid pixels, valid bool [n, hm, hm], margin float64 [n, hm, hm])."""
    q = np.asarray(q).astype(np.float64)
    n, side = q.shape[0], q.shape[-1]
    assert geometry(hm)[2] == side == q.shape[1]
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    out = np.full((n, hm, hm), -np.inf)
    val = np.zeros((n, hm, hm), dtype=bool)
    mar = np.zeros((n, hm, hm))
    for m in range(n):
        qy, qx, valid, margin = map_coords(hm, affines[m], iy, ix)
        y0, x0, fy, fx = corners(qy[valid], qx[valid], side)
        Q = q[m]
        out[m][valid] = (1 - fy) * ((1 - fx) * Q[y0, x0] + fx * Q[y0, x0 + 1]) + fy * ((1 - fx) * Q[y0 + 1, x0] + fx * Q[y0 + 1, x0 + 1])
        val[m], mar[m] = valid, margin
    return out, val, mar


def scene_points(q, affine, hm, pixels):
    """Point form: q torch [OH, OW] (any float dtype, may require grad), pixels [K, 2] = (iy, ix), all valid -> v torch [K] in q's
    dtype.  The corner indices and weights come from the float64 chain; the interpolation itself is torch, so autograd gives dq."""
    side = q.shape[-1]
    pix = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
    qy, qx, valid, _ = map_coords(hm, affine, pix[:, 0], pix[:, 1])
    assert valid.all(), "scene_points: an invalid pixel"
    y0, x0, fy, fx = corners(qy, qx, side)
    y0, x0 = torch.from_numpy(y0), torch.from_numpy(x0)
    fy, fx = torch.from_numpy(fy).to(q.dtype), torch.from_numpy(fx).to(q.dtype)
    return (1 - fy) * ((1 - fx) * q[y0, x0] + fx * q[y0, x0 + 1]) + fy * ((1 - fx) * q[y0 + 1, x0] + fx * q[y0 + 1, x0 + 1])


def huber(d):
    """code/trainer.py:345-348 per element (torch, any dtype)."""
    return torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
