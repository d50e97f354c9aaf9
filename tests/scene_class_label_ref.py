"""fp64 restatement of the scene-frame class-label-map cross entropy (include/smg_hip.h, smg_loss_scene_map_ce) on top of
tests/scene_class_ref.py and tests/scene_label_ref.py, the reference of tests/test_cpu_scene_class_label_maps.py and
tests/test_gpu_scene_class_label_maps.py.  Plain helper module, no tests.

A heightmap pixel is a POINT when it is valid in the pair's rotation and its label is exactly 0 or 1; W = the number of points;
every other pixel (class 2, NaN, any other value) is "no loss".  With z the three interpolated logits of a point:
    loss         = (sum over the points of logsumexp(z) - z[y]) / W                      (0 when W == 0)
    dq[c,oy,ox]  = (1 / W) sum over the points of (softmax(z)[c] - [c == y]) * (bilinear weight of (oy, ox) at the pixel)

Two forms: `autograd` (scene_class_ref.scene_class_loss fed every heightmap pixel + torch autograd: the reference) and `gather`
(numpy, by map element over scene_label_ref.element_box, as the kernel walks it)."""
import numpy as np
import torch

import scene_class_ref
import scene_label_ref
import scene_ref

LABEL_VALUES = (0, 1, 2, np.nan, 7, -1, 0.5)                  # make_case's label mix: 0 and 1 count, all the others are "no loss"
LABEL_SHARES = (.35, .35, .1, .05, .05, .05, .05)


def classes(label):
    """int64 class per pixel: the label where it is exactly 0 or 1, else 2."""
    lab = np.asarray(label)
    return np.where((lab == 0) | (lab == 1), lab, 2).astype(np.int64)


def counted(hm, affine, label):
    """(pixels [hm * hm, 2] = every (iy, ix) in row-major order, y int64 [hm * hm], keep bool [hm * hm] = valid and class 0 / 1)."""
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    pix = np.stack([iy.ravel(), ix.ravel()], axis=-1)
    y = classes(label).ravel()
    valid = scene_ref.map_coords(hm, affine, pix[:, 0], pix[:, 1])[2]
    return pix, y, valid & (y < 2)


def autograd(q, affine, hm, label):
    """q [3, side, side] (any float dtype; widened to float64) -> (loss float, dq float64 [3, side, side], terms float64 [W] = the
    nll of every point in row-major order, W) by torch fp64 autograd through scene_class_ref.scene_class_loss fed EVERY heightmap
    pixel in row-major order with y = label where the label is 0 or 1, else 2."""
    qt = torch.from_numpy(np.asarray(q).astype(np.float64)).requires_grad_(True)
    pix, y, keep = counted(hm, affine, label)
    loss = scene_class_ref.scene_class_loss(qt, affine, hm, pix, y)
    loss.backward()
    W = int(keep.sum())
    if W == 0:
        return float(loss.detach()), qt.grad.numpy(), np.zeros(0), 0
    with torch.no_grad():
        terms = scene_class_ref.nll_terms(scene_class_ref.scene_class_points(qt.detach(), affine, hm, pix[keep]), torch.from_numpy(y[keep]))[0]
    return float(loss.detach()), qt.grad.numpy(), terms.numpy(), W


def gather(q, affine, hm, label):
    """By map element: (loss, dq float64 [3, side, side], stats) with stats = {"W": points counted at their home elements, "touch":
    pixel-element incidences of valid pixels found in the boxes, "touch_all": the same counted over the whole heightmap (equal when
    no box missed a pixel), "max_box": largest box side, "max_touch": most pixels touching one element}."""
    Q = np.asarray(q).astype(np.float64)
    side = Q.shape[-1]
    y_all = classes(label)
    iy_all, ix_all = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    valid = scene_ref.map_coords(hm, affine, iy_all, ix_all)[2]
    touch_all = 4 * int(valid.sum())           # a valid pixel touches the four corners of its cell
    dq = np.zeros((3, side, side))
    lsum, W, touch, max_box, max_touch = 0.0, 0, 0, 0, 0
    for oy in range(side):
        for ox in range(side):
            by0, by1, bx0, bx1 = scene_label_ref.element_box(hm, affine, oy, ox)
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
            y = y_all[iy, ix]
            t &= y < 2
            y, y0, x0, fy, fx, dy, dx = (z[t] for z in (y, y0, x0, fy, fx, dy, dx))
            z = (1 - fy) * ((1 - fx) * Q[:, y0, x0] + fx * Q[:, y0, x0 + 1]) + fy * ((1 - fx) * Q[:, y0 + 1, x0] + fx * Q[:, y0 + 1, x0 + 1])      # [3, k]
            m = z.max(axis=0)
            e = np.exp(z - m)
            s = e.sum(axis=0)
            home = (dy == 0) & (dx == 0)
            lsum += float(((np.log(s) + m) - z[y, np.arange(len(y))])[home].sum())
            W += int(home.sum())
            g = e / s - (np.arange(3)[:, None] == y[None, :])
            dq[:, oy, ox] = (g * (np.where(dy == 1, fy, 1 - fy) * np.where(dx == 1, fx, 1 - fx))).sum(axis=1)
    if W == 0:
        return 0.0, np.zeros((3, side, side)), {"W": 0, "touch": touch, "touch_all": touch_all, "max_box": max_box, "max_touch": max_touch}
    return lsum / W, dq / W, {"W": W, "touch": touch, "touch_all": touch_all, "max_box": max_box, "max_touch": max_touch}


def make_case(hm, rotations, num_rotations, seed):
    """The inputs of one class-label-map case and their fp64 reference.  q float32 [n, 3, side, side] seeded normal; labels drawn
    from LABEL_VALUES with LABEL_SHARES (0 and 1 count; 2, NaN, 7, -1 and 0.5 are "no loss"), then NaN at every pixel that is
    invalid in the pair's rotation.  Returns a dict: q, aff [n, 6], label (float32 [n, hm, hm]), valid, loss [n],
    dq [n, 3, side, side], abs_terms [n] = sum |nll|, W [n], n0 / n1 [n] = counted points of class 0 / 1."""
    _, S, side = scene_ref.geometry(hm)
    rng = np.random.default_rng(seed)
    n = len(rotations)
    q = rng.standard_normal((n, 3, side, side)).astype(np.float32)
    aff = np.stack([scene_ref.theta(r, num_rotations) for r in rotations])
    label = rng.choice(np.asarray(LABEL_VALUES, dtype=np.float64), size=(n, hm, hm), p=LABEL_SHARES).astype(np.float32)
    iy, ix = np.meshgrid(np.arange(hm), np.arange(hm), indexing="ij")
    valid = np.stack([scene_ref.map_coords(hm, aff[j], iy, ix)[2] for j in range(n)])
    label[~valid] = np.nan
    loss, dq, abs_terms, W = [], [], [], []
    for j in range(n):
        l, g, terms, w = autograd(q[j], aff[j], hm, label[j])
        assert np.isfinite(l) and np.isfinite(g).all()
        loss.append(l); dq.append(g); abs_terms.append(float(np.abs(terms).sum())); W.append(w)
    return {"hm": hm, "S": S, "side": side, "q": q, "aff": aff, "label": label, "valid": valid, "loss": np.asarray(loss),
            "dq": np.stack(dq), "abs_terms": np.asarray(abs_terms), "W": np.asarray(W),
            "n0": np.asarray([int((label[j] == 0).sum()) for j in range(n)]), "n1": np.asarray([int((label[j] == 1).sum()) for j in range(n)])}
