"""fp64 restatement of the scene-frame label-map Huber (include/smg_hip.h, smg_loss_scene_map) on top of tests/scene_ref.py, the
reference of tests/test_cpu_scene_label_maps.py and tests/test_gpu_scene_label_maps.py.  Plain helper module, no tests.

    loss      = sum over the pixels that are valid in the pair's rotation and whose weight is not 0 of  w huber(v - label)
    dq[oy,ox] = sum over the same pixels of  w huber'(v - label) * (bilinear weight of (oy, ox) at that pixel)

Three forms: `autograd` (scene_ref.scene_points on the contributing pixels + torch autograd: the reference), `map_form` (numpy,
from scene_ref.scene_maps' values: the loss and its terms) and `gather` (numpy, by map element over the heightmap bounding box of
the element's 2x2-cell square, as the kernel walks it)."""
import numpy as np
import torch

import scene_ref


def contributing(hm, affine, weight):
    """(pixels [K, 2] = (iy, ix) in row-major order, flat bool mask [hm, hm]) of the pixels that count: valid and w != 0."""
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    valid = scene_ref.map_coords(hm, affine, iy, ix)[2]
    keep = valid if weight is None else valid & (np.asarray(weight) != 0)
    return np.stack([iy[keep], ix[keep]], axis=-1), keep


def autograd(q, affine, hm, label, weight):
    """q [side, side] (any float dtype; widened to float64) -> (loss float, dq float64 [side, side], terms float64 [K], d float64 [K])
    by torch fp64 autograd through scene_ref.scene_points on the contributing pixels only."""
    qt = torch.from_numpy(np.asarray(q).astype(np.float64)).requires_grad_(True)
    pix, keep = contributing(hm, affine, weight)
    if len(pix) == 0:
        return 0.0, np.zeros(qt.shape), np.zeros(0), np.zeros(0)
    w = torch.ones(len(pix), dtype=torch.float64) if weight is None else torch.from_numpy(np.asarray(weight)[keep].astype(np.float64))
    d = scene_ref.scene_points(qt, affine, hm, pix) - torch.from_numpy(np.asarray(label)[keep].astype(np.float64))
    terms = w * scene_ref.huber(d)
    loss = terms.sum()
    loss.backward()
    return float(loss.detach()), qt.grad.numpy(), terms.detach().numpy(), d.detach().numpy()


def map_form(q, affine, hm, label, weight):
    """The loss from the MAP form of the geometry (scene_ref.scene_maps): (loss, terms [K]) in numpy float64."""
    v, valid, _ = scene_ref.scene_maps(np.asarray(q)[None], [affine], hm)
    keep = valid[0] if weight is None else valid[0] & (np.asarray(weight) != 0)
    w = np.ones(int(keep.sum())) if weight is None else np.asarray(weight)[keep].astype(np.float64)
    d = v[0][keep] - np.asarray(label)[keep].astype(np.float64)
    terms = w * np.where(np.abs(d) < 1, 0.5 * d * d, np.abs(d) - 0.5)
    return float(terms.sum()), terms


def element_box(hm, affine, oy, ox):
    """Heightmap bounding box (by0, by1, bx0, bx1), inclusive, of the map square [ox - 1, ox + 1] x [oy - 1, oy + 1] (clipped to the
    map) pushed back through u = A^-T p, widened by one pixel per side and clipped to the heightmap; the whole heightmap for a
    matrix without a usable inverse (|det| <= 1e-6 of the squared norm, or not finite)."""
    pad, S, side = scene_ref.geometry(hm)
    a = np.asarray(affine, dtype=np.float32).astype(np.float64).reshape(6)
    qx = np.asarray([max(ox - 1, 0), min(ox + 1, side - 1)] * 2, dtype=np.float64)
    qy = np.asarray([max(oy - 1, 0)] * 2 + [min(oy + 1, side - 1)] * 2, dtype=np.float64)
    pxn, pyn = 2.0 * (32.0 * qx + 319.5) / (S - 1) - 1.0, 2.0 * (32.0 * qy + 319.5) / (S - 1) - 1.0
    det = a[0] * a[4] - a[3] * a[1]                                    # of A^T = [a0 a3; a1 a4]
    if not (abs(det) > 1e-6 * (a[0] ** 2 + a[1] ** 2 + a[3] ** 2 + a[4] ** 2) and np.isfinite(det)):
        return 0, hm - 1, 0, hm - 1
    ux, uy = (a[4] * pxn - a[3] * pyn) / det, (a[0] * pyn - a[1] * pxn) / det          # A^-T p
    fx, fy = ((ux + 1.0) / 2.0 * (S - 1) - 0.5 - pad) / 2.0, ((uy + 1.0) / 2.0 * (S - 1) - 0.5 - pad) / 2.0
    bx0, bx1 = max(int(np.floor(fx.min())) - 1, 0), min(int(np.ceil(fx.max())) + 1, hm - 1)
    by0, by1 = max(int(np.floor(fy.min())) - 1, 0), min(int(np.ceil(fy.max())) + 1, hm - 1)
    return by0, by1, bx0, bx1


def gather(q, affine, hm, label, weight):
    """By map element: (loss, dq float64 [side, side], stats) with stats = {"touch": pixel-element incidences found in the boxes,
    "touch_all": the same counted over the whole heightmap (equal when no box missed a pixel), "max_box": largest box side,
    "max_touch": most pixels touching one element, "clipped": elements whose unclipped box would leave the heightmap}."""
    Q = np.asarray(q).astype(np.float64)
    side = Q.shape[-1]
    lab = np.asarray(label)
    iy_all, ix_all = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    qy, qx, valid, _ = scene_ref.map_coords(hm, affine, iy_all, ix_all)
    touch_all = 4 * int(valid.sum())           # a valid pixel touches the four corners of its cell
    dq = np.zeros((side, side))
    loss, touch, max_box, max_touch = 0.0, 0, 0, 0
    for oy in range(side):
        for ox in range(side):
            by0, by1, bx0, bx1 = element_box(hm, affine, oy, ox)
            if by1 < by0 or bx1 < bx0:
                continue
            max_box = max(max_box, by1 - by0 + 1, bx1 - bx0 + 1)
            iy, ix = np.meshgrid(np.arange(by0, by1 + 1), np.arange(bx0, bx1 + 1), indexing="ij")
            iy, ix = iy.ravel(), ix.ravel()
            py, px, v, _ = scene_ref.map_coords(hm, affine, iy, ix)
            iy, ix, py, px = iy[v], ix[v], py[v], px[v]
            y0, x0, fy, fx = scene_ref.corners(py, px, side)
            dy, dx = oy - y0, ox - x0
            t = (dy >= 0) & (dy <= 1) & (dx >= 0) & (dx <= 1)
            touch += int(t.sum())
            max_touch = max(max_touch, int(t.sum()))
            w = np.ones(len(iy)) if weight is None else np.asarray(weight)[iy, ix].astype(np.float64)
            t &= w != 0
            iy, ix, y0, x0, fy, fx, dy, dx, w = (z[t] for z in (iy, ix, y0, x0, fy, fx, dy, dx, w))
            val = (1 - fy) * ((1 - fx) * Q[y0, x0] + fx * Q[y0, x0 + 1]) + fy * ((1 - fx) * Q[y0 + 1, x0] + fx * Q[y0 + 1, x0 + 1])
            d = val - lab[iy, ix].astype(np.float64)
            quad = np.abs(d) < 1
            home = (dy == 0) & (dx == 0)
            loss += float((w * np.where(quad, 0.5 * d * d, np.abs(d) - 0.5))[home].sum())
            g = w * np.where(quad, d, np.sign(d))
            dq[oy, ox] = float((g * np.where(dy == 1, fy, 1 - fy) * np.where(dx == 1, fx, 1 - fx)).sum())
    return loss, dq, {"touch": touch, "touch_all": touch_all, "max_box": max_box, "max_touch": max_touch}


def odd_affines():
    """2x2 parts that are no rotation (scene_point asks for none): a sheared and stretched turn (determinant 1.32: the valid area of a 3 x 3 map shrinks from 1024 heightmap pixels to about 776), a turn shrunk to half (the valid
    area and the boxes are twice as wide), and the zero matrix (no inverse: every pixel lands on the centre of the map)."""
    c, s = np.cos(np.radians(30.0)), np.sin(np.radians(30.0))
    return np.asarray([[1.1 * c, 1.1 * s + 0.2, 0, -1.1 * s, 1.1 * c, 0],
                       [0.5 * c, -0.5 * s, 0, 0.5 * s, 0.5 * c, 0],
                       [0, 0, 0, 0, 0, 0]], dtype=np.float32)


def make_case(hm, rotations, num_rotations, seed):
    """The inputs of one label-map case and their fp64 reference.  q float32 [n, 1, side, side] seeded normal; labels = the fp64
    value of the pixel + one of (0.3, -1.7, 1.7, -0.3) (both Huber branches, both signs), NaN at every pixel that is invalid in the
    pair's rotation; weights U(0.2, 1) with every 7th pixel (row-major) exactly 0 and a NaN label under each of those zeros.
    Returns a dict: q, aff [n, 6], label, weight (float32 [n, hm, hm]), loss [n], dq [n, side, side], abs_terms [n] = sum |terms|,
    quad = fraction of contributing pixels on the quadratic branch."""
    _, S, side = scene_ref.geometry(hm)
    rng = np.random.default_rng(seed)
    n = len(rotations)
    q = rng.standard_normal((n, 1, side, side)).astype(np.float32)
    aff = np.stack([scene_ref.theta(r, num_rotations) for r in rotations])
    v, valid, _ = scene_ref.scene_maps(q[:, 0], aff, hm)
    off = np.asarray([0.3, -1.7, 1.7, -0.3])[rng.integers(0, 4, size=(n, hm, hm))]
    label = np.where(valid, v + off, np.nan).astype(np.float32)
    weight = rng.uniform(0.2, 1.0, size=(n, hm, hm)).astype(np.float32)
    zero = (np.arange(hm * hm) % 7 == 0).reshape(hm, hm)
    weight[:, zero] = 0.0
    label[:, zero] = np.nan
    loss, dq, abs_terms, quad, cnt = [], [], [], 0, 0
    for j in range(n):
        l, g, terms, d = autograd(q[j, 0], aff[j], hm, label[j], weight[j])
        assert np.isfinite(l) and np.isfinite(g).all()
        loss.append(l); dq.append(g); abs_terms.append(float(np.abs(terms).sum()))
        quad += int((np.abs(d) < 1).sum()); cnt += len(d)
    return {"hm": hm, "S": S, "side": side, "q": q, "aff": aff, "label": label, "weight": weight, "valid": valid,
            "loss": np.asarray(loss), "dq": np.stack(dq), "abs_terms": np.asarray(abs_terms), "quad": quad / max(cnt, 1)}
