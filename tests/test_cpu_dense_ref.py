"""The fp64 restatement of one dense layer (tests/dense_ref.py) against torch modules and autograd in fp64 on a tiny dense block - 2
streams, planes 5 x 5 and 6 x 7 (HW % 64 != 0), 6 layers of growth 4 over 8 input channels, so that the two-layer group (layers 0-1)
and the four-layer group (layers 2-5) of the 1x1 data gradient both occur, consumed by a final BatchNorm like norm5.  The backward is
walked the way csrc/backward.hip walks it (G' form, per-layer and grouped segments from dense_ref.dgrad1_segments); every
intermediate the GPU gates read - GS, D2, the two weight gradients, norm2's affine gradients - and the block input's gradient at the
end equal autograd's.

Then the REFERENCE is perturbed the way a subtly wrong kernel would be, and the error the gate would take is printed as a ratio to
the gate (all > 1): tests/test_gpu_dense_gates.py would fail on each.  Measured (-s prints every one): on the tiny block a lost
segment of the four-layer group at 1.9e6 - 2.5e6 x the gate, another layer's norm1 at 3.1e6 - 3.8e6, statistics counted over HWp at
1.4e6 - 4.7e6, a stream's partial tile missing from a weight gradient at 1.3e6 - 1.8e6; on the oracle's block-4 planes (20^2, 21^2) a
dropped last 64-row tile at 2.8e5 - 5.3e5 and a lost bottom / right tap on the ragged tile at 2.3e5 - 3.8e5.  The keep-masks leave out
at most 0.0024 % of any plane (rule: 1 %).  And on the fp64 oracle's planes of the two scenes the GPU gates
run: the restatement reproduces the oracle's own layers, and every keep-mask of the gates leaves out at most 1 % of its elements."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_ref as dr
import stage_ref as sr
from helpers import _WGRAD_BLK, _WGRAD_GATE, _fp32_chain
from test_cpu_stage_ref import _bn, _close, _nchw, _oracle_planes, _plane, _tp

PLANES = [(5, 5), (6, 7)]
NS, L, CIN0, GROWTH, BOTT = 2, 6, 8, 4, 8
CTOT = CIN0 + L * GROWTH
_WALKS = {}


def test_groups_of_the_1x1_data_gradient():
    """g_lo / g_hi for the four block lengths: groups of kGroup = 4 counted from the top, the remainder at the bottom; every column of
    every layer's input is covered exactly once by the segments"""
    assert [dr.group_of(6, i) for i in range(6)] == [(0, 1), (0, 1), (2, 5), (2, 5), (2, 5), (2, 5)]
    assert [dr.group_of(12, i)[0] for i in range(12)] == [0] * 4 + [4] * 4 + [8] * 4
    assert {dr.group_of(24, i) for i in range(24)} == {(4 * k, 4 * k + 3) for k in range(6)}
    assert {dr.group_of(16, i) for i in range(16)} == {(4 * k, 4 * k + 3) for k in range(4)}
    for Lb, cin0 in zip(dr.LAYERS, dr.CIN0):
        cover = np.zeros((Lb, cin0 + 32 * Lb), dtype=int)
        for i in range(Lb):
            for layers, c0, c1 in dr.dgrad1_segments(Lb, i, cin0):
                for l in layers:
                    assert c1 <= cin0 + 32 * l
                    cover[l, c0:c1] += 1
        for l in range(Lb):
            assert (cover[l, :cin0 + 32 * l] == 1).all() and (cover[l, cin0 + 32 * l:] == 0).all()


class _W:
    pass


def _walk(H, W):
    """the tiny block forward and backward, in torch (autograd) and in numpy (dense_ref), once per plane"""
    if (H, W) in _WALKS:
        return _WALKS[(H, W)]
    r = np.random.default_rng(100 + H * W)
    HW = H * W
    o = _W()
    o.H, o.W, o.HW = H, W, HW
    o.prm = []
    for i in range(L):
        cin = CIN0 + GROWTH * i
        o.prm.append(dict(g1=r.standard_normal(cin), b1=0.5 * r.standard_normal(cin), w1=r.standard_normal((BOTT, cin)) / np.sqrt(cin),
                          g2=r.standard_normal(BOTT), b2=0.5 * r.standard_normal(BOTT), w2=r.standard_normal((GROWTH, BOTT, 3, 3)) / np.sqrt(9 * BOTT)))
    g5, b5 = r.standard_normal(CTOT), r.standard_normal(CTOT)
    x0 = [r.standard_normal((HW, CIN0)) * (1 + s) + 0.3 * s for s in range(NS)]
    R = [r.standard_normal((HW, CTOT)) for _ in range(NS)]
    # torch
    tp = [{k: torch.from_numpy(v).requires_grad_(True) for k, v in p.items()} for p in o.prm]
    loss, o.t_x0, o.t_bt, o.t_y = 0.0, [], [], []
    for s in range(NS):
        xt = _nchw(x0[s], H, W).requires_grad_(True)
        feats, bts, ys = [xt], [], []
        for p in tp:
            bt = F.conv2d(F.relu(_bn(torch.cat(feats, 1), p["g1"], p["b1"])), p["w1"][:, :, None, None])
            bt.retain_grad()
            y = F.conv2d(F.relu(_bn(bt, p["g2"], p["b2"])), p["w2"], padding=1)
            y.retain_grad()
            feats.append(y); bts.append(bt); ys.append(y)
        loss = loss + (_bn(torch.cat(feats, 1), g5, b5) * _nchw(R[s], H, W)).sum()
        o.t_x0.append(xt); o.t_bt.append(bts); o.t_y.append(ys)
    loss.backward()
    o.tp = tp
    # numpy, forward
    o.X = [np.zeros((HW, CTOT)) for _ in range(NS)]
    o.BT = [[None] * L for _ in range(NS)]
    for s in range(NS):
        o.X[s][:, :CIN0] = x0[s]
        for i, p in enumerate(o.prm):
            cin = CIN0 + GROWTH * i
            o.BT[s][i] = dr.conv1_fwd(o.X[s][:, :cin], p["g1"], p["b1"], p["w1"])[0]
            o.X[s][:, cin:cin + GROWTH] = dr.conv2_fwd(o.BT[s][i], H, W, p["g2"], p["b2"], p["w2"])[0]
    # numpy, backward in the order of the engine's walk
    o.G = [g5 * R[s] for s in range(NS)]
    o.G0 = [[None] * L for _ in range(NS)]           # G' in front of layer i's 1x1 data gradients
    o.GS, o.DY, o.D2 = ([[None] * L for _ in range(NS)] for _ in range(3))
    o.dW1, o.dW2, o.aff = [None] * L, [None] * L, [None] * L
    cols = np.arange(9 * BOTT)
    for i in reversed(range(L)):
        p = o.prm[i]
        cin = CIN0 + GROWTH * i
        for s in range(NS):
            o.GS[s][i] = sr.bn_bwd(o.G[s][:, cin:cin + GROWTH], o.X[s][:, cin:cin + GROWTH])
            o.DY[s][i] = (sr.bn_pre(o.BT[s][i], p["g2"], p["b2"]) > 0) * dr.conv2_dgrad(o.GS[s][i], H, W, p["w2"])[0]
            o.D2[s][i] = dr.norm2_bwd(o.DY[s][i], o.BT[s][i], p["g2"])
            o.G0[s][i] = o.G[s].copy()
        o.aff[i] = dr.norm2_affine([o.DY[s][i] for s in range(NS)], [o.BT[s][i] for s in range(NS)])
        Gs, A64, _ = dr.conv2_wgrad_ops([o.GS[s][i] for s in range(NS)], [o.BT[s][i] for s in range(NS)], H, W, p["g2"], p["b2"], cols)
        o.dW2[i] = np.concatenate([o.GS[s][i] for s in range(NS)]).T @ A64
        _, A64, _ = dr.conv1_wgrad_ops([o.D2[s][i] for s in range(NS)], [o.X[s] for s in range(NS)], p["g1"], p["b1"], np.arange(BOTT), np.arange(cin))
        o.dW1[i] = np.concatenate([o.D2[s][i] for s in range(NS)]).T @ A64
        for layers, c0, c1 in dr.dgrad1_segments(L, i, CIN0, GROWTH):
            for s in range(NS):
                o.G[s][:, c0:c1] = _seg(o, s, i, layers, c0, c1)[0]
    _WALKS[(H, W)] = o
    return o


def _seg(o, s, i, layers, c0, c1, params=None, G0=None):
    params = [(o.prm[l]["g1"], o.prm[l]["b1"], o.prm[l]["w1"]) for l in layers] if params is None else params
    return dr.conv1_dgrad(o.G[s] if G0 is None else G0, o.X[s], params, [o.D2[s][l] for l in layers], c0, c1)


@pytest.mark.parametrize("H,W", PLANES)
def test_dense_layer_forward_and_backward_equal_torch(H, W):
    o = _walk(H, W)
    for s in range(NS):
        for i in range(L):
            cin = CIN0 + GROWTH * i
            _close(o.BT[s][i], _plane(o.t_bt[s][i]), "conv1 forward")
            _close(o.X[s][:, cin:cin + GROWTH], _plane(o.t_y[s][i]), "conv2 forward")
            _close(o.GS[s][i], _plane(o.t_y[s][i].grad), "GS = bn_bwd(G' slice, x slice), layer %d" % i)
            _close(o.D2[s][i], _plane(o.t_bt[s][i].grad), "D2, affine form")
            assert dr.unit_form_error(o.D2[s][i], o.D2[s][i]) == 0.0
        _close(sr.bn_bwd(o.G[s][:, :CIN0], o.X[s][:, :CIN0]), _plane(o.t_x0[s].grad), "block input gradient: every segment landed once")
    for i in range(L):
        t = o.tp[i]
        _close(o.dW1[i], t["w1"].grad.numpy(), "conv1 weight gradient")
        _close(dr.w2_grad_mat(t["w2"].grad.numpy()), o.dW2[i], "conv2 weight gradient")
        _close(o.aff[i]["db"], t["b2"].grad.numpy(), "norm2 dbeta")
        _close(o.aff[i]["dg"], t["g2"].grad.numpy(), "norm2 dgamma")
        assert (o.aff[i]["dbm"] >= np.abs(o.aff[i]["db"]) - 1e-12).all() and (o.aff[i]["dgm"] >= np.abs(o.aff[i]["dg"]) - 1e-12).all()


@pytest.mark.parametrize("H,W", PLANES)
def test_im2col_forms_agree(H, W):
    """the whole-plane tap-by-tap product, the materialised im2col, its pixel and column samples, forward and flipped"""
    r = np.random.default_rng(7)
    a, w2 = r.standard_normal((H * W, BOTT)), r.standard_normal((GROWTH, BOTT, 3, 3))
    full = dr.im2col(a, H, W)
    _close(full @ dr.w2_fwd_mat(w2).T, dr.conv3x3(a, H, W, dr.w2_fwd_mat(w2))[0], "conv3x3")
    pix, cols = np.asarray([0, W - 1, H * W - 1, H * W // 2]), np.arange(0, 9 * BOTT, 5)
    assert np.array_equal(dr.im2col(a, H, W, pix=pix), full[pix]) and np.array_equal(dr.im2col(a, H, W, cols=cols), full[:, cols])
    g = r.standard_normal((H * W, GROWTH))
    _close(dr.im2col(g, H, W, flip=True) @ dr.w2_bwd_mat(w2).T, dr.conv2_dgrad(g, H, W, w2)[0], "flipped gather")
    ref = _plane(F.conv_transpose2d(_nchw(g, H, W), torch.from_numpy(w2), padding=1))
    _close(dr.conv2_dgrad(g, H, W, w2)[0], ref, "conv2 data gradient = transposed convolution")


def _report(what, e_pert, gate):
    print("perturbation: %-78s error %.3e = %.3g x the gate (%.3e)" % (what, e_pert, e_pert / gate, gate))
    assert e_pert > gate, (what, e_pert, gate)


@pytest.mark.parametrize("H,W", PLANES)
def test_what_the_data_gradient_gates_catch(H, W):
    """at the bottom of the four-layer group (layer 2: grouped form on [0, 16), layers 2-5) - one segment lost, another layer's norm1
    mask - against the 2x fp32-chain gate of the conv1 data gradient"""
    o = _walk(H, W)
    i = 2
    (layers, c0, c1), = [sg for sg in dr.dgrad1_segments(L, i, CIN0, GROWTH) if sg[1] == 0]
    assert layers == [2, 3, 4, 5] and (c0, c1) == (0, 16)
    for s in range(NS):
        ref, mag, ch, keep = _seg(o, s, i, layers, c0, c1, G0=o.G0[s][i])
        assert 1 - keep.mean() <= 0.01
        gate = 2.0 * dr.rms(ch, ref, mag, keep)
        lost = _seg(o, s, i, layers[:-1], c0, c1, G0=o.G0[s][i])[0]
        _report("%dx%d stream %d: segment of layer 5 lost from the four-layer group" % (H, W, s), dr.rms(lost, ref, mag, keep), gate)
        prm = [(o.prm[l]["g1"], o.prm[l]["b1"], o.prm[l]["w1"]) for l in layers]
        prm[1] = (o.prm[2]["g1"], o.prm[2]["b1"], o.prm[3]["w1"])          # (the segment's columns [0, 16) exist in both layers)
        other = _seg(o, s, i, layers, c0, c1, params=prm, G0=o.G0[s][i])[0]
        _report("%dx%d stream %d: layer 3's segment masked and scaled with layer 2's norm1" % (H, W, s), dr.rms(other, ref, mag, keep), gate)


@pytest.mark.parametrize("H,W", PLANES)
def test_what_the_forward_and_weight_gradient_gates_catch(H, W):
    """statistics counted over HWp instead of HW (conv1 forward, 2x chain); one stream's last partial tile missing from the conv1
    weight gradient (_WGRAD_GATE x the blocked reduction)"""
    o = _walk(H, W)
    i = 3
    p, cin = o.prm[i], CIN0 + GROWTH * i
    HWp = -(-o.HW // 64) * 64
    for s in range(NS):
        x = o.X[s][:, :cin].astype(np.float32)
        ref, mag = dr.conv1_fwd(x, p["g1"], p["b1"], p["w1"])
        gate = 2.0 * dr.rms(dr.conv1_chain(x, p["g1"], p["b1"], p["w1"].astype(np.float32), np.arange(o.HW)), ref, mag)
        mean = x.astype(np.float64).sum(0) / HWp
        inv = 1.0 / np.sqrt((x.astype(np.float64) ** 2).sum(0) / HWp - mean ** 2 + sr.EPS)
        bad = np.maximum((x - mean) * inv * p["g1"] + p["b1"], 0.0) @ p["w1"].T
        _report("%dx%d stream %d: statistics counted over HWp = %d instead of HW = %d" % (H, W, s, HWp, o.HW), dr.rms(bad, ref, mag), gate)
    D2 = [o.D2[s][i].astype(np.float32) for s in range(NS)]
    X = [o.X[s].astype(np.float32) for s in range(NS)]
    D, A64, A32 = dr.conv1_wgrad_ops(D2, X, p["g1"].astype(np.float32), p["b1"].astype(np.float32), np.arange(BOTT), np.arange(cin))
    _, e_blk, ref, mag = dr.wgrad_errors(np.zeros((BOTT, cin)), D, A64, A32, blks=(_WGRAD_BLK,))
    tail = slice(NS * o.HW - min(16, o.HW), NS * o.HW)          # the last stream's last (partial) tile of 16 rows
    bad = ref - D[tail].astype(np.float64).T @ A64[tail]
    _report("%dx%d: the last stream's partial tile missing from the conv1 weight gradient" % (H, W), dr.rms(bad, ref, mag), _WGRAD_GATE * e_blk[_WGRAD_BLK])


# ---- on the oracle's planes of the two scenes: block 4's padded, ragged plane; the keep-masks ------------------------------------------------
BACKWARD_LAYERS = {"S640": [(1, 3), (1, 6), (2, 5), (2, 6), (2, 9), (2, 12), (3, 21), (3, 24), (4, 1), (4, 13), (4, 14), (4, 16)],      # cases A, C, D
                   "S672": [(1, 3), (1, 6), (2, 9), (3, 21), (3, 24), (4, 13), (4, 16)]}                                                # case B


def _lp(sd, block, layer, name):
    return _tp(sd, "denseblock%d.denselayer%d.%s" % (block, layer, name))


@pytest.mark.parametrize("case", sorted(BACKWARD_LAYERS))
def test_restatement_reproduces_the_oracle_and_sees_a_dropped_tile_and_a_lost_tap(case):
    """Block 4, layer 8 on the oracle's plane (20^2: 448 rows for 400 pixels, 2.5 tiles of 8 per side; 21^2: 448 for 441, 2.6 tiles):
    the restated layer equals the oracle's own output; a conv1 that drops the last 64-row tile of the padded plane and a conv2 that
    loses the bottom (right) tap on the ragged last tile row (column) are past the 2x chain gates."""
    P = _oracle_planes(case)
    sd, H = P["sd"], P["S"] // 32
    HW, cin = H * H, dr.cin_of(4, 8)
    g1, b1, w1 = _lp(sd, 4, 8, "norm1.weight"), _lp(sd, 4, 8, "norm1.bias"), _lp(sd, 4, 8, "conv1.weight").reshape(128, cin)
    g2, b2, w2 = _lp(sd, 4, 8, "norm2.weight"), _lp(sd, 4, 8, "norm2.bias"), _lp(sd, 4, 8, "conv2.weight")
    for s in range(2):
        X = P["x"][3][s]
        bt, mag1 = dr.conv1_fwd(X[:, :cin], g1, b1, w1)
        out, mag2 = dr.conv2_fwd(bt.astype(np.float32), H, H, g2, b2, w2)
        assert np.abs(out - X[:, cin:cin + 32]).max() <= 1e-5 * np.abs(out).max()          # (the oracle's planes are kept in fp32)
        gate1 = 2.0 * dr.rms(dr.conv1_chain(X[:, :cin], g1, b1, w1, np.arange(HW)), bt, mag1)
        bad = bt.copy()
        bad[(HW // 64) * 64:] = 0
        _report("%s stream %d: conv1 drops the last 64-row tile (rows %d..%d)" % (case, s, (HW // 64) * 64, HW - 1), dr.rms(bad, bt, mag1), gate1)
        bt32 = bt.astype(np.float32)
        gate2 = 2.0 * dr.rms(dr.conv2_chain(bt32, H, H, g2, b2, w2, np.arange(HW)), out, mag2)
        a = dr.act64(bt32, g2, b2)
        edge = (H // 8) * 8                                                                    # first row / column of the ragged tile
        for name, t0, rowsel in (("bottom", 6, np.arange(HW) // H >= edge), ("right", 2, np.arange(HW) % H >= edge)):
            wm = dr.w2_fwd_mat(w2).astype(np.float64)
            taps = [6, 7, 8] if name == "bottom" else [2, 5, 8]
            lost = sum(dr.im2col(a, H, H)[:, t * 128:(t + 1) * 128] @ wm[:, t * 128:(t + 1) * 128].T for t in taps)
            bad = out - rowsel[:, None] * lost
            _report("%s stream %d: conv2 loses the %s taps on the ragged tile (from %d)" % (case, s, name, edge), dr.rms(bad, out, mag2), gate2)


@pytest.mark.parametrize("case", sorted(BACKWARD_LAYERS))
def test_keep_masks_leave_out_at_most_one_percent(case):
    """the borderline-ReLU rule of the dense gates on the oracle's planes: norm2's mask of every gated layer (conv2 data gradient) and
    the combined norm1 masks of every segment of its conv1 data gradient (up to four layers' masks at once)"""
    P = _oracle_planes(case)
    sd = P["sd"]
    worst = 0.0
    for block, layer in BACKWARD_LAYERS[case]:
        cin, Lb = dr.cin_of(block, layer), dr.LAYERS[block - 1]
        for s in range(2):
            X = P["x"][block - 1][s]
            bt = dr.conv1_fwd(X[:, :cin], _lp(sd, block, layer, "norm1.weight"), _lp(sd, block, layer, "norm1.bias"),
                              _lp(sd, block, layer, "conv1.weight").reshape(128, cin))[0].astype(np.float32)
            sh2 = dr.excluded_share(*dr.relu_sides(bt, _lp(sd, block, layer, "norm2.weight"), _lp(sd, block, layer, "norm2.bias")))
            sh1 = 0.0
            for layers, c0, c1 in dr.dgrad1_segments(Lb, layer - 1, dr.CIN0[block - 1]):
                keep = np.ones((len(X), c1 - c0), dtype=bool)
                for l in layers:
                    on, off = dr.relu_sides(X[:, c0:c1], _lp(sd, block, l + 1, "norm1.weight")[c0:c1], _lp(sd, block, l + 1, "norm1.bias")[c0:c1])
                    keep &= on | off
                sh1 = max(sh1, 1 - keep.mean())
            print("%s block %d layer %2d stream %d: excluded %.4f %% (norm2 mask), %.4f %% (norm1 masks of a segment, worst)" % (case, block, layer, s, 100 * sh2, 100 * sh1))
            worst = max(worst, sh1, sh2)
    assert worst <= 0.01, worst
