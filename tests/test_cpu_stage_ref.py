"""The fp64 restatements of tests/stage_ref.py against torch modules and autograd in fp64, at tiny shapes (planes 12^2 -> 6^2 and
10^2 -> 5^2, 8 - 16 channels, 2 - 4 streams, a shared stream with several users), and - on the planes of the fp64 oracle's forward of
the two scenes the GPU gates run (tests/test_gpu_stage_gates.py) - the yardsticks of those gates themselves: the same element-wise
formulas evaluated in numpy fp32 stay within the rounding counts K_* of stage_ref.py, and the borderline-ReLU rule drops at most
1 % of any plane it is applied to."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stage_ref as sr
from helpers import _fp32_chain, MEAN, STD, oracle_net, orc

TOL = 1e-12
PLANES = [(12, 12), (10, 10)]


def _rng(seed):
    return np.random.default_rng(seed)


def _nchw(a, H, W):
    """[HW][C] -> torch [1][C][H][W]"""
    return torch.from_numpy(np.ascontiguousarray(a.reshape(H, W, -1).transpose(2, 0, 1)))[None]


def _plane(t):
    """torch [1][C][H][W] -> [HW][C]"""
    a = t.detach().numpy()[0]
    return np.ascontiguousarray(a.transpose(1, 2, 0).reshape(-1, a.shape[0]))


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert err <= TOL, (what, err)


def _bn(x, g, b):
    return F.batch_norm(x, None, None, torch.from_numpy(g) if isinstance(g, np.ndarray) else g, torch.from_numpy(b) if isinstance(b, np.ndarray) else b,
                        training=True, eps=sr.EPS)


# ---- forward restatements ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(24, 24), (20, 20)])
def test_stem_conv_is_conv2d_7x7_stride2_pad3(H, W):
    r = _rng(1)
    img, w = r.standard_normal((H, W, 3)), r.standard_normal((8, 3, 7, 7))
    ref = _plane(F.conv2d(_nchw(img.reshape(H * W, 3), H, W), torch.from_numpy(w), stride=2, padding=3))
    got, mag = sr.stem_conv(img, w, np.arange(H // 2))
    _close(got, ref, "stem, image form")
    assert (mag >= np.abs(got) - 1e-12).all()
    # rows picked from the two edges only
    rows = np.asarray([0, 1, H // 2 - 1])
    _close(sr.stem_conv(img, w, rows)[0], ref.reshape(H // 2, W // 2, 8)[rows].reshape(-1, 8), "stem, rows")
    # heightmap form: one channel presented three times = the weights summed over the input channels, 49 taps
    one = img[:, :, :1]
    ref1 = _plane(F.conv2d(_nchw(np.repeat(one, 3, axis=2).reshape(H * W, 3), H, W), torch.from_numpy(w), stride=2, padding=3))
    _close(sr.stem_conv(one, w.sum(1, keepdims=True), np.arange(H // 2))[0], ref1, "stem, heightmap form")
    # ... and two channels' weights are NOT the same thing (what a stem that dropped one would compute)
    two = sr.stem_conv(one, w[:, :2].sum(1, keepdims=True), np.arange(H // 2))[0]
    assert np.abs(two - ref1).max() > 1e-2 * np.abs(ref1).max()


@pytest.mark.parametrize("H,W", PLANES)
def test_pool0_is_bn_relu_maxpool(H, W):
    r = _rng(2)
    x, g, b = r.standard_normal((H * W, 8)) * 3 + 1, r.standard_normal(8), r.standard_normal(8)
    ref = _plane(F.max_pool2d(F.relu(_bn(_nchw(x, H, W), g, b)), 3, 2, 1))
    got, mag = sr.pool0(x, H, W, g, b)
    _close(got, ref, "pool0")
    assert (mag >= got).all()
    win = sr.pool_windows(np.maximum(sr.bn_pre(x, g, b), 0.0), H, W, -np.inf)
    assert win.shape == (9, (H // 2) * (W // 2), 8) and np.array_equal(win.max(0), got)


@pytest.mark.parametrize("H,W", PLANES)
def test_transition_forward_both_orders(H, W):
    r = _rng(3)
    x, g, b, w = r.standard_normal((H * W, 16)), r.standard_normal(16), r.standard_normal(16), r.standard_normal((8, 16))
    ref = _plane(F.avg_pool2d(F.conv2d(F.relu(_bn(_nchw(x, H, W), g, b)), torch.from_numpy(w)[:, :, None, None]), 2))
    _close(sr.transition_fwd(x, H, W, g, b, w), ref, "transition, conv then pool")
    _close(sr.pooled_act(x, H, W, g, b) @ w.T, ref, "transition, pool then conv")
    # a transition that dropped the last row of pooled pixels is visible in the rms the gate takes
    bad = ref.copy()
    bad[-(W // 2):] = 0
    assert np.sqrt((((bad - ref) / (sr.pooled_act(x, H, W, g, b) @ np.abs(w).T + 1e-30)) ** 2).mean()) > 1e-3


def _tiny_head(r, HW, C, n_rot):
    x4 = [r.standard_normal((HW, C)) * (1 + s) + 0.3 * s for s in range(n_rot + 1)]
    pa, pb = list(range(n_rot)), [n_rot] * n_rot
    p = dict(g5=r.standard_normal(C), b5=r.standard_normal(C), g0=r.standard_normal(2 * C), b0=r.standard_normal(2 * C),
             w0=r.standard_normal((6, 2 * C)), g1=r.standard_normal(6), b1=r.standard_normal(6))
    return x4, pa, pb, p


@pytest.mark.parametrize("H,W", [(6, 6), (5, 5)])
def test_feat_and_head_conv0(H, W):
    r = _rng(4)
    x4, pa, pb, p = _tiny_head(r, H * W, 8, 2)
    Fm, M = sr.feat(x4, p["g5"], p["b5"], pa, pb)
    assert (M >= np.abs(Fm) - 1e-12).all()
    for j in range(2):
        f = torch.cat((_bn(_nchw(x4[pa[j]], H, W), p["g5"], p["b5"]), _bn(_nchw(x4[pb[j]], H, W), p["g5"], p["b5"])), 1)
        _close(Fm[j], _plane(f), "feat")
        h = F.conv2d(F.relu(_bn(f, p["g0"], p["b0"])), torch.from_numpy(p["w0"])[:, :, None, None])
        _close(sr.head_conv0(Fm[j], p["g0"], p["b0"], p["w0"])[0], _plane(h), "head conv0")
    # Statistics of ANOTHER row (pair 1's for pair 0 - what indexing the [pair][2048] sums by stream would read).  Every half of F is a
    # BatchNorm output, so the rows differ only through eps / var of norm5's input: parts in 10^5 - 10^6.  The gate still sees it: the
    # error it takes (rms of err / sum |a||w|) rises far past twice the fp32 chain's.
    h_pair, a64 = sr.head_conv0(Fm[0], p["g0"], p["b0"], p["w0"])
    mean1, inv1 = sr.bn_stats(Fm[1])
    h_other = np.maximum((Fm[0] - mean1) * inv1 * p["g0"] + p["b0"], 0.0) @ p["w0"].T
    mag = a64 @ np.abs(p["w0"]).T
    a32 = sr.bn32(Fm[0].astype(np.float32), p["g0"], p["b0"])
    e_chain = np.sqrt((((_fp32_chain(a32, p["w0"].astype(np.float32)).astype(np.float64) - sr.head_conv0(Fm[0].astype(np.float32), p["g0"], p["b0"], p["w0"].astype(np.float32))[0]) / mag) ** 2).mean())
    e_other = np.sqrt((((h_other - h_pair) / mag) ** 2).mean())
    assert e_other > 10 * 2.0 * e_chain, (e_other, e_chain)


# ---- backward restatements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", PLANES)
def test_g_prime_identity(H, W):
    """x consumed by three BatchNorm + ReLU with different gamma / beta: bn_bwd(G', x) is autograd's gradient of x"""
    r = _rng(5)
    C = 8
    x = r.standard_normal((H * W, C)) * 2 + 0.5
    xt = _nchw(x, H, W).requires_grad_(True)
    loss, Gp = 0.0, np.zeros((H * W, C))
    for j in range(3):
        g, b, R = r.standard_normal(C), r.standard_normal(C), r.standard_normal((H * W, C))
        loss = loss + (F.relu(_bn(xt, g, b)) * _nchw(R, H, W)).sum()
        Gp += g * (sr.bn_pre(x, g, b) > 0) * R
    loss.backward()
    _close(sr.bn_bwd(Gp, x), _plane(xt.grad), "G' identity")
    assert (sr.bn_bwd_mag(Gp, x) >= np.abs(sr.bn_bwd(Gp, x)) - 1e-12).all()
    assert (sr.bn_bwd_sum_mag(Gp, x) >= sr.bn_bwd_mag(Gp, x) - 1e-12).all()
    # the two fp32 evaluations: exact sums, and sums formed tile by tile in fp32 (16-term chains: <= 18 roundings of the summed magnitudes)
    for tile in (False, True):
        e = np.abs(sr.bn_bwd32(Gp, x, tile_sums=tile).astype(np.float64) - sr.bn_bwd(Gp, x))
        assert (e <= (8 + 2 * 18 * tile) * sr.U * sr.bn_bwd_sum_mag(Gp, x)).all(), tile
    assert np.abs(sr.tile_sum32(Gp) - Gp.astype(np.float32).astype(np.float64).sum(0)).max() <= 18 * sr.U * np.abs(Gp).sum(0).max()


@pytest.mark.parametrize("H,W", PLANES)
def test_transition_backward(H, W):
    """data gradient in the G' form and weight gradient against autograd of avg_pool2d(conv2d(relu(bn(x)))), two streams sharing the
    weights, the transition's output consumed by two BatchNorm + ReLU (its G')"""
    r = _rng(6)
    Cp, C0 = 16, 8
    g, b, w = r.standard_normal(Cp), r.standard_normal(Cp), r.standard_normal((C0, Cp))
    gt, bt, wt = (torch.from_numpy(v).requires_grad_(True) for v in (g, b, w))
    cons = [(r.standard_normal(C0), r.standard_normal(C0)) for _ in range(2)]
    xs, dXs, loss, checks = [], [], 0.0, []
    for s in range(2):
        x = r.standard_normal((H * W, Cp)) * (1 + s)
        xt = _nchw(x, H, W).requires_grad_(True)
        y = F.avg_pool2d(F.conv2d(F.relu(_bn(xt, gt, bt)), wt[:, :, None, None]), 2)
        xn = _plane(y)
        Gn = np.zeros_like(xn)
        for gj, bj in cons:
            R = r.standard_normal(xn.shape)
            loss = loss + (F.relu(_bn(y, gj, bj)) * _nchw(R, H // 2, W // 2)).sum()
            Gn += gj * (sr.bn_pre(xn, gj, bj) > 0) * R
        Gx, dX, on = sr.transition_bwd(x, H, W, g, b, w, xn, Gn)
        xs.append(x); dXs.append(dX); checks.append((Gx, x, xt))
    loss.backward()
    for Gx, x, xt in checks:
        _close(sr.bn_bwd(Gx, x), _plane(xt.grad), "transition data gradient")
    _close(sr.transition_wgrad(xs, H, W, g, b, dXs), wt.grad.numpy(), "transition weight gradient")


@pytest.mark.parametrize("H,W", [(6, 6), (5, 5)])
def test_norm5_concat_head_backward_with_a_shared_stream(H, W):
    """3 rotation streams + the masked stream all pairs share (3 users): G'_4, norm5's affine gradients, dF and the head conv0
    weight gradient against autograd.  Dropping the last user of the shared stream is visible."""
    r = _rng(7)
    C, n_rot = 8, 3
    x4, pa, pb, p = _tiny_head(r, H * W, C, n_rot)
    t = {k: torch.from_numpy(v).requires_grad_(True) for k, v in p.items()}
    xt = [_nchw(x, H, W).requires_grad_(True) for x in x4]
    n5 = [_bn(x, t["g5"], t["b5"]) for x in xt]
    Fm, _ = sr.feat(x4, p["g5"], p["b5"], pa, pb)
    loss, DF, dW, z0s = 0.0, [], 0.0, []
    for j in range(n_rot):
        z0 = _bn(torch.cat((n5[pa[j]], n5[pb[j]]), 1), t["g0"], t["b0"])
        z0.retain_grad()
        h1 = F.conv2d(F.relu(z0), t["w0"][:, :, None, None])
        y1 = F.relu(_bn(h1, t["g1"], t["b1"]))
        R = r.standard_normal((H * W, 6))
        loss = loss + (y1 * _nchw(R, H, W)).sum()
        h1n = _plane(h1)
        dh1 = (sr.bn_pre(h1n, p["g1"], p["b1"]) > 0) * R          # what the engine keeps in DH1: the gradient behind relu1
        df, A, on, wsum = sr.head_conv0_bwd(h1n, dh1, Fm[j], p["g1"], p["g0"], p["b0"], p["w0"])
        DF.append(df); dW = dW + wsum; z0s.append(z0)
    loss.backward()
    for j in range(n_rot):
        _close(DF[j], _plane(z0s[j].grad), "dF")
    _close(dW, t["w0"].grad.numpy(), "head conv0 weight gradient")
    G4, dy5, mag, db, dg, dbm, dgm = sr.norm5_bwd(x4, Fm, np.stack(DF), p["g0"], p["g5"], pa, pb)
    for s in range(n_rot + 1):
        _close(sr.bn_bwd(G4[s], x4[s]), _plane(xt[s].grad), "norm5 backward, stream %d" % s)
    # norm5 feeds a BatchNorm directly (no ReLU in between): its bias gradient is zero in exact arithmetic and its weight gradient is
    # what eps leaves of it - both sums cancel to rounding noise, so they are compared on the scale of their sum |term|
    assert (np.abs(db - t["b5"].grad.numpy()) <= TOL * dbm).all() and (np.abs(dg - t["g5"].grad.numpy()) <= TOL * dgm).all()
    assert (np.abs(db) <= 1e-10 * dbm).all()
    assert (mag >= np.abs(dy5) - 1e-12).all() and (dbm >= np.abs(db) - 1e-12).all() and (dgm >= np.abs(dg) - 1e-12).all()
    lost = sr.norm5_bwd(x4, Fm[:-1], np.stack(DF[:-1]), p["g0"], p["g5"], pa[:-1], pb[:-1])
    worst = (np.abs(lost[0][n_rot] - G4[n_rot]) / (np.abs(p["g5"]) * mag[n_rot] + 1e-300)).max()
    assert worst > 1e-3, worst                                      # against k_g4 * 2^-24 = 1e-5


# ---- the GPU gates' yardsticks on the oracle's planes of the two scenes ----------------------------------------------------------------------
SCENES = {"S640": dict(seed=0, size=224, rot=3, S=640, dq=[[[1.0]]]),
          "S672": dict(seed=8, size=236, rot=2, S=672, dq=[[[1.0, -0.5], [0.25, -2.0]]])}
_ORACLE = {}


def _oracle_planes(case):
    """fp64 oracle forward of one rotation + the masked stream; every stage's plane as the engine would hold it (fp32, [HW][C])"""
    if case in _ORACLE:
        return _ORACLE[case]
    import synthetic
    c = SCENES[case]
    depth, masks = synthetic.heightmap_scene(c["seed"], size=c["size"], n_boxes=8)
    x = orc.preprocess(depth, [MEAN] * 3, [STD] * 3)
    mx = orc.preprocess(depth * masks[0], [MEAN] * 3, [STD] * 3)
    assert x.shape[-1] == c["S"]
    net = copy.deepcopy(oracle_net(0)).double()
    feats = getattr(net, orc.STYLE_TRUNK[0]).features
    head = getattr(net, orc.STYLE_HEAD[0])
    out = {}
    hooks = [getattr(feats, n).register_forward_hook(lambda m, i, o, n=n: out.setdefault(n, []).append(_plane(o).astype(np.float32)))
             for n in ("conv0", "denseblock1", "denseblock2", "denseblock3", "denseblock4")]
    with torch.no_grad():
        f = torch.cat((feats(orc.rotate(x, c["rot"], 16).double()), feats(mx.double())), 1)
    for h in hooks:
        h.remove()
    sd = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    P = {"stem": out["conv0"], "x": [out["denseblock%d" % b] for b in (1, 2, 3, 4)], "sd": sd, "S": c["S"]}
    P["feat"] = _plane(f).astype(np.float32)[None]
    # the head behind conv0, with autograd for DH1 (the gradient behind relu1) from a fixed dq
    h1 = head[2](F.relu(head[0](f))).detach().requires_grad_(True)
    y1 = F.relu(head[3](h1))
    y1.retain_grad()
    q = head[5](y1)
    q.backward(torch.tensor(c["dq"], dtype=torch.float64)[None])
    P["h1"] = _plane(h1).astype(np.float32)[None]
    P["dh1"] = (_plane(y1.grad) * (_plane(y1) > 0)).astype(np.float32)[None]
    _ORACLE[case] = P
    return P


def _hp(sd, name):
    return sd["graspnet_val.grasp-val-" + name]


def _tp(sd, name):
    return sd["grasp_depth_trunk.features." + name]


@pytest.mark.parametrize("case", sorted(SCENES))
def test_fp32_evaluation_of_the_elementwise_stages_stays_within_the_rounding_counts(case):
    """The check of the YARDSTICK (not of a kernel): pool0, feat, the norm5 backward and its two sums evaluated in numpy fp32 from
    the oracle's planes against the fp64 restatement, within k * 2^-24 * mag with the counts K_BN, k_g4, k_sums5 of stage_ref.py."""
    P = _oracle_planes(case)
    sd, S = P["sd"], P["S"]
    Hs, H4 = S // 2, S // 32
    g0, b0 = _tp(sd, "norm0.weight"), _tp(sd, "norm0.bias")
    for s in range(2):
        ref, mag = sr.pool0(P["stem"][s], Hs, Hs, g0, b0)
        r = (np.abs(sr.pool0_32(P["stem"][s], Hs, Hs, g0, b0).astype(np.float64) - ref) / mag).max() / sr.U
        print("%s pool0 stream %d: numpy fp32 at %.2f roundings of %d" % (case, s, r, sr.K_BN))
        assert r <= sr.K_BN
    x4 = [P["x"][3][s] for s in range(2)]
    g5, b5 = _tp(sd, "norm5.weight"), _tp(sd, "norm5.bias")
    ref, mag = sr.feat(x4, g5, b5, [0], [1])
    r = (np.abs(sr.feat32(x4, g5, b5, [0], [1]).astype(np.float64) - ref) / mag).max() / sr.U
    print("%s feat: numpy fp32 at %.2f roundings of %d" % (case, r, sr.K_BN))
    assert r <= sr.K_BN
    assert np.abs(ref - P["feat"]).max() <= 1e-5 * np.abs(ref).max()          # the restatement agrees with the oracle's own features
    hn0, hn1 = _hp(sd, "norm0.weight"), _hp(sd, "norm1.weight")
    df = sr.head_conv0_bwd(P["h1"][0], P["dh1"][0], P["feat"][0], hn1, hn0, _hp(sd, "norm0.bias"), _hp(sd, "conv0.weight").reshape(64, 2048))[0]
    DF = df.astype(np.float32)[None]
    G4, dy5, mag, db, dg, dbm, dgm = sr.norm5_bwd(x4, P["feat"], DF, hn0, g5, [0], [1])
    G32, db32, dg32 = sr.norm5_bwd32(x4, P["feat"], DF, hn0, g5, [0], [1])
    r = (np.abs(G32.astype(np.float64) - G4) / (np.abs(g5) * mag + 1e-300)).max() / sr.U
    kb = sr.k_sums5(H4 * H4, 2, False)
    rb, rg = (np.abs(db32 - db) / dbm).max() / sr.U, (np.abs(dg32 - dg) / dgm).max() / sr.U
    print("%s norm5 backward: numpy fp32 at %.2f roundings of %d; dbeta5 %.2f, dgamma5 %.2f of %d" % (case, r, sr.k_g4(1), rb, rg, kb))
    assert r <= sr.k_g4(1) and rb <= kb and rg <= kb


@pytest.mark.parametrize("case", sorted(SCENES))
def test_borderline_relu_rule_drops_at_most_one_percent(case):
    """the `keep` rule of the data-gradient gates on the planes it is applied to: the three transition norms and the head's norm0"""
    P = _oracle_planes(case)
    sd = P["sd"]
    for s in range(2):
        for t in (1, 2, 3):
            keep = sr.bn_keep(P["x"][t - 1][s], _tp(sd, "transition%d.norm.weight" % t), _tp(sd, "transition%d.norm.bias" % t))
            print("%s transition %d stream %d: %.4f %% borderline" % (case, t, s, 100 * (1 - keep.mean())))
            assert 1 - keep.mean() <= 0.01
    keep = sr.bn_keep(P["feat"][0], _hp(sd, "norm0.weight"), _hp(sd, "norm0.bias"))
    print("%s head norm0: %.4f %% borderline" % (case, 100 * (1 - keep.mean())))
    assert 1 - keep.mean() <= 0.01
