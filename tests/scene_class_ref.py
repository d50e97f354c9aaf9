"""fp64 restatement of the reactive net's class maps in the scene frame (include/smg_hip.h, "the reactive net's class maps in the
scene frame"), the reference of tests/test_cpu_scene_class_maps.py and tests/test_gpu_scene_class_maps.py.  Plain helper module,
no tests; the geometry is tests/scene_ref.py's.

The three LOGIT planes are interpolated at the scene point (same corners, same fractions) and the softmax is taken there.
Map form (numpy): every heightmap pixel of every map.  Point form (torch): the weighted-mean cross entropy (class weights
{1, 1, 0}) of the interpolated logits at given heightmap pixels as a differentiable function of the maps, so autograd gives dq."""
import numpy as np
import torch

import scene_ref


def scene_class_logits(q, affines, hm):
    """q [n, 3, OH, OW] -> (interpolated logits float64 [n, 3, hm, hm] with -inf at invalid pixels, valid bool [n, hm, hm], margin)."""
    q = np.asarray(q).astype(np.float64)
    planes = [scene_ref.scene_maps(q[:, c], affines, hm) for c in range(3)]
    return np.stack([p[0] for p in planes], axis=1), planes[0][1], planes[0][2]


def scene_class_maps(q, affines, hm):
    """Map form: q [n, 3, OH, OW] (any float dtype, widened to float64), affines [n, 6] -> (P float64 [n, 3, hm, hm] = softmax
    over axis 1 of the interpolated logits, -inf in all three planes at invalid pixels; valid bool [n, hm, hm]; margin)."""
    z, valid, margin = scene_class_logits(q, affines, hm)
    out = np.full(z.shape, -np.inf)
    v = np.broadcast_to(valid[:, None], z.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        zv = np.moveaxis(z, 1, -1)[valid]                        # [pixels, 3]
        e = np.exp(zv - zv.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
    np.moveaxis(out, 1, -1)[valid] = p
    assert np.isneginf(out[~v]).all()
    return out, valid, margin


def scene_class_points(q, affine, hm, pixels):
    """q torch [3, OH, OW] (any float dtype, may require grad), pixels [K, 2] = (iy, ix), all valid -> the interpolated logits
    z torch [K, 3] in q's dtype (scene_ref.scene_points per plane)."""
    return torch.stack([scene_ref.scene_points(q[c], affine, hm, pixels) for c in range(3)], dim=1)


def nll_terms(z, y):
    """Per point: weight_y * (logsumexp(z) - z[y]) with class weights {1, 1, 0} and the weights themselves; z [K, 3], y int64 [K]."""
    w = torch.tensor([1.0, 1.0, 0.0], dtype=z.dtype)[y]
    nll = torch.logsumexp(z, dim=1) - z.gather(1, y[:, None])[:, 0]
    return w * nll, w


def scene_class_loss(q, affine, hm, pixels, labels):
    """Point form: the loss of one pair - F.nll_loss(F.log_softmax(z, 1), y, weight = {1, 1, 0}) on the interpolated logits, with
    the interface's two deviations from torch spelled out: a point that is outside the heightmap or has no window in this rotation
    contributes nothing and does not count in W, and W == 0 gives 0 (with a zero gradient), not 0/0.  Class-2 points are dropped
    before any logit is read.  q torch [3, OH, OW]; pixels [K, 2]; labels [K] in {0, 1, 2}.  Returns a 0-d tensor in q's dtype."""
    pix = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    inside = (pix >= 0).all(axis=1) & (pix < hm).all(axis=1)
    valid = scene_ref.map_coords(hm, affine, pix[:, 0], pix[:, 1])[2]
    keep = inside & valid & (y < 2)
    if not keep.any():
        return (q * 0).sum()
    terms, w = nll_terms(scene_class_points(q, affine, hm, pix[keep]), torch.from_numpy(y[keep]))
    return terms.sum() / w.sum()
