"""Operator-level gates on the stages AROUND the dense layers (the dense layers have theirs in test_gpu_dense_gates.py; what the gate
modules share is tests/gate_harness.py): every stage's
input and output are read back from the engine and the stage is recomputed in fp64 from its OWN input buffer with its own fp64
batch statistics over [:HW] of each stream or pair (tests/stage_ref.py, proved against torch in tests/test_cpu_stage_ref.py).

Forward: stem conv0 in the heightmap form (F_STEM1, 49 taps) and the image form (F_STEM, 147), norm0 + ReLU + pool0 with the raw stem
value at the argmax, the three transitions (F_POOL), norm5 + concat (feat_kernel), the head's norm0 + ReLU + conv0.
Backward (one debug_stop each, inputs and outputs read after that ONE stop): at 350 the head conv0 data and weight gradients,
norm5_bwd_kernel on every single-user stream and on the shared masked stream, norm5's affine gradients; at 250 / 150 / 50 transition
3 / 2 / 1's E_UNPOOL data gradient and W_POOL weight gradient.

Two geometries, for the tile variants and padded rows they select (asserted from eng.H / eng.HWp, gate_harness.GEOMETRY):
  S = 640: planes 320^2, 160^2 (128-row, no padding), 80^2 (128-row), 40^2 (64-row), 20^2 (448 rows for 400 pixels); 6 streams, 5 pairs:
           the masked stream has 5 users, more than norm5_bwd_kernel's 4 phases; sample 3 enters with dq = 1e-6, 20 binades low.
  S = 672: planes 336^2, 168^2 (28288 rows for 28224), 84^2 (64-row, 7104 for 7056), 42^2 (128-row, 1792 for 1764), 21^2 (448 for 441,
           Q 2 x 2, a partial 64-pixel chunk in feat_kernel); 3 streams, 2 pairs.

Yardsticks - the project's own (helpers.py): matrix products and data gradients within 2x the error of a plain fp32 multiply-add
chain over the same operands (rms of err / sum |a||w|), weight gradients within 3x the blocked fp32 reduction over ALL streams x
pixels; element-wise stages within k * 2^-24 * mag of fp64, k = the fp32 roundings on the kernel's path (stage_ref.K_*, counted from
the kernel source).  The fp32 chain runs on a sample of each stream's pixels (the plane's first and last rows - the last tile of a
padded plane - and pixels strided through it); the kernel's error is taken on that sample AND on the whole plane of every stream,
both against the sample's chain error: one wrong tile row anywhere raises the whole-plane rms by orders of magnitude.

Two roundings the kernels legitimately make are modelled in the yardsticks, not covered by a wider factor (both found by these
gates, both traced to the kernel source; the figures stand at the assertions):
  * the forward statistics of planes written by whole tiles of the implicit-GEMM forward are fp32 strip sums (stage_ref.strip_sum_slack):
    pool0 and feat_kernel inherit a mean / invstd that is off by more than one rounding where a channel's mean is small against its spread;
  * the backward statistics mean(G') and mean(G' * xhat) are sums of fp32 tile sums (stage_ref.tile_sum32): the transitions' weight
    gradient adds their deviation coherently over every pixel.

What each gate would catch (reasoned from the restatements; tests/test_cpu_stage_ref.py perturbs the REFERENCE accordingly):
  * a transition that drops the last tile row of a padded plane: test_transition_forward at S = 672 - the whole-plane rms runs over every
    pixel of 84^2 / 42^2 / 21^2 (7104 / 1792 / 448 rows for 7056 / 1764 / 441 pixels); 64 rows that are zero instead of the product put
    err / sum |a||w| near 1 on 1 - 15 % of the plane: an rms of 0.1 - 0.4 against a gate of 6e-8;
  * a head conv0 that takes statistics by stream instead of by pair: test_head_conv0_forward - F is a BatchNorm output, so another row's
    statistics differ by eps / var only, parts in 10^5 - 10^6 of the operand: still ten times the gate and more (the CPU file measures it);
  * a norm5_bwd that loses the fifth user of the masked stream: test_head_conv0_and_norm5_backward at S = 640 - g4 of stream 5 misses one
    of five terms of the size of mag, against a bound of 150 * 2^-24 = 9e-6 of mag;
  * a heightmap-form stem that sums two of the three channel weights: test_stem_conv0_heightmap_form - the reference multiplies the plane
    by the fp64 sum of all three; a third of sum |a||w| is missing from every element.

Out of scope: the transition norms' weight / bias gradients leave through db_flush_kernel at the END of the walk - they are not final
at a stop and stay with the end-to-end gradient tests; so do input sizes that are no multiple of 32 (zero_uncovered_kernel)."""
import numpy as np
import pytest
import torch

import dense_ref as dr
import stage_ref as sr
from gate_harness import CT, HEAD, SCENES, TRUNK, GateCtx, elementwise, gate, gpu, wgrad_gate  # noqa: F401  (gpu: the fixture)
from helpers import _fp32_blocked, _fp32_chain, product_net

pytestmark = pytest.mark.gpu

CASES = {"S640": SCENES["S640x6"], "S672": SCENES["S672x3"]}
_NETS, _FWD = {}, {}


def _ctx(gpu, case):
    """net, heightmaps and stream / pair layout of one geometry (built once per module)"""
    if case not in _NETS:
        net = product_net(0)
        _NETS[case] = GateCtx(net, {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}, CASES[case], gpu)
    return _NETS[case]


def _fwd(gpu, case):
    """ONE heightmap-form forward per geometry; every buffer the forward gates compare is read after that one run"""
    if case not in _FWD:
        x = _ctx(gpu, case)
        x.forward()
        B = {"img": x.eng.debug_read("img").reshape(-1, x.HWp[0], 4)[:x.NS, :x.S * x.S, 0].copy(),
             "stem": x.rd("stem", x.NS, 1, 64), "stemv": x.rd("dy0", x.NS, 2, 64),
             "feat": x.rd("feat", x.NP, 5, 2048), "h1": x.rd("h1", x.NP, 5, 64)}
        for b in range(4):
            B["x%d" % (b + 1)] = x.rd("x%d" % (b + 1), x.NS, 2 + b, CT[b])
        _FWD[case] = B
    return _ctx(gpu, case), _FWD[case]


# ---- forward -----------------------------------------------------------------------------------------------------------------------------
def _stem_rows(Hs):
    return np.concatenate([np.arange(24), np.arange(Hs - 24, Hs)])          # 48 rows: both padded edges of the 7x7 window


@pytest.mark.parametrize("case", sorted(CASES))
def test_stem_conv0_heightmap_form(gpu, case):
    """F_STEM1: K = 49 taps on the one-channel plane.  Reference: the three channels' weights summed in fp64 (= the 3-channel
    convolution of three equal channels); yardstick: the fp32 chain over 49 taps with that sum rounded ONCE to fp32, which is what
    pack_weights_kernel stores (PK_STEM1).  sum |a||w| is taken over all 147 products."""
    x, B = _fwd(gpu, case)
    S, Hs = x.S, x.H[1]
    w = x.tp("conv0.weight")
    w1 = w.astype(np.float64).sum(1, keepdims=True)
    rows = _stem_rows(Hs)
    pix = (rows[:, None] * Hs + np.arange(Hs)[None, :]).ravel()
    for n in range(x.NS):
        img = B["img"][n].reshape(S, S, 1)
        ref, _ = sr.stem_conv(img, w1, rows)
        mag = np.abs(sr.stem_cols(img.astype(np.float64), rows)) @ sr.stem_wmat(np.abs(w.astype(np.float64)).sum(1, keepdims=True)).T + 1e-300
        chain = _fp32_chain(sr.stem_cols(img, rows), sr.stem_wmat(w1.astype(np.float32)))
        gate("%s stem conv0, heightmap form, stream %d" % (case, n), dr.rms(B["stem"][n][pix], ref, mag), dr.rms(chain, ref, mag), 2.0, n=ref.size)


def test_stem_conv0_image_form(gpu):
    """F_STEM: the 3-channel image (net.forward), K = 147, S = 640, both streams"""
    import models
    from helpers import scene_tensors
    net = _ctx(gpu, "S640").net
    xi, mx = scene_tensors(0, [0])
    net.forward(xi, mx, 0, True, 3)
    torch.cuda.synchronize()
    eng = models._ENGINES[(0, 640, net.HEAD_OUT)]
    assert eng.H[1] == 320 and eng.HWp[1] == 102400
    img = eng.debug_read("img").reshape(-1, eng.HWp[0], 4)[:2, :640 * 640, :]
    stem = eng.debug_read("stem", count=2 * eng.HWp[1] * 64).reshape(2, eng.HWp[1], 64)[:, :320 * 320]
    assert (img[..., 3] == 0).all() and not (img[0, :, 0] == img[1, :, 0]).all()
    w = net.state_dict()[TRUNK + "conv0.weight"].detach().cpu().numpy()
    rows = _stem_rows(320)
    pix = (rows[:, None] * 320 + np.arange(320)[None, :]).ravel()
    for n in range(2):
        im = img[n, :, :3].reshape(640, 640, 3)
        ref, mag = sr.stem_conv(im, w, rows)
        chain = _fp32_chain(sr.stem_cols(im, rows), sr.stem_wmat(w))
        gate("S640 stem conv0, image form, stream %d" % n, dr.rms(stem[n][pix], ref, mag + 1e-300), dr.rms(chain, ref, mag + 1e-300), 2.0, n=ref.size)


@pytest.mark.parametrize("case", sorted(CASES))
def test_pool0_and_raw_stem_value_at_the_argmax(gpu, case):
    """pool0_kernel on whole planes: x1[:, :64] against the window maximum of the fp64 relu(bn(stem)), within K_BN roundings of bn_mag
    (mean, invstd, gamma * invstd, x - mean, the fused multiply-add: stage_ref.K_BN).  And the raw stem value the kernel keeps for the
    pooled stem tail's backward (DY0 aliases it after the forward): bit-equal to one of the <= 9 raw values of its window, and its fp64
    BN + ReLU equals the window's fp64 maximum within the same bound."""
    x, B = _fwd(gpu, case)
    Hs = x.H[1]
    g, b = x.tp("norm0.weight"), x.tp("norm0.bias")
    for n in range(x.NS):
        stem = B["stem"][n]
        ref, mag = sr.pool0(stem, Hs, Hs, g, b)
        # the stem plane's statistics come from whole 128-row tiles (fp32 strip sums): their error moves mean and invstd by more than a
        # rounding of either where a channel's mean is small against its spread (measured without the term: 20.7 roundings of mag on the
        # masked stream of S = 640, 2.5 - 3.5 on the others)
        slack = sr.maxpool3s2(sr.bn_stat_slack(stem, g, (Hs * Hs // 128) * 128), Hs, Hs)
        elementwise("%s pool0 stream %d" % (case, n), B["x1"][n][:, :64], ref, mag, sr.K_BN, slack)
        sv = B["stemv"][n]
        win = sr.pool_windows(stem, Hs, Hs, np.float32(np.nan))
        assert (win == sv[None]).any(0).all(), "a kept stem value is none of its window's"
        mean, inv = sr.bn_stats(stem)
        elementwise("%s BN + ReLU of the kept raw stem value, stream %d" % (case, n),
                    np.maximum((sv.astype(np.float64) - mean) * (inv * g) + b, 0.0), ref, mag, sr.K_BN)      # (fp64 on both sides: 0)


@pytest.mark.parametrize("t", [1, 2, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_transition_forward(gpu, case, t):
    """F_POOL: x{t} (all channels) -> x{t+1}[:, :C/2].  Reference in the reference's order (conv, then pool), yardstick in the
    kernel's (the 2 x 2 average of relu(bn(x)) formed in fp32, then the fp32 chain over the channels)."""
    x, B = _fwd(gpu, case)
    H, Cp = x.H[1 + t], CT[t - 1]
    C0 = Cp // 2
    g, b = x.tp("transition%d.norm.weight" % t), x.tp("transition%d.norm.bias" % t)
    w = x.tp("transition%d.conv.weight" % t).reshape(C0, Cp)
    pix = dr.sample((H // 2) ** 2)
    cols = np.arange(0, C0, max(1, C0 // 128))
    for n in range(x.NS):
        X = B["x%d" % t][n]
        got = B["x%d" % (t + 1)][n][:, :C0]
        ref = sr.transition_fwd(X, H, H, g, b, w)
        mag = sr.pooled_act(X, H, H, g, b) @ np.abs(w.astype(np.float64)).T + 1e-300
        a32 = sr.pooled_act32(X, H, H, g, b)[pix]
        chain = _fp32_chain(a32, np.ascontiguousarray(w[cols]))
        sel = np.ix_(pix, cols)
        gate("%s transition %d stream %d" % (case, t, n), dr.rms(got[sel], ref[sel], mag[sel]), dr.rms(chain, ref[sel], mag[sel]), 2.0,
             e_whole=dr.rms(got, ref, mag), n=chain.size)


@pytest.mark.parametrize("case", sorted(CASES))
def test_norm5_concat(gpu, case):
    """feat_kernel: F[pair] = norm5(x4[rotation stream]) | norm5(x4[masked stream]), no ReLU; K_BN roundings of bn_mag, whole planes"""
    x, B = _fwd(gpu, case)
    g5 = x.tp("norm5.weight")
    ref, mag = sr.feat(list(B["x4"]), g5, x.tp("norm5.bias"), x.pa, x.pb)
    # x4's first 512 channels leave transition 3 through 64-row tiles: the whole ones (384 of the 400 / 441 pixels) sum their statistics
    # in fp32 strips, the last one and the 3x3 kernels' channels per element in fp64 (measured without the term: 9.5 / 8.0 roundings)
    HW = x.H[5] ** 2
    sl = [np.concatenate([sr.bn_stat_slack(v[:, :512], g5[:512], (HW // 64) * 64), np.zeros((HW, 512))], axis=1) for v in B["x4"]]
    for j in range(x.NP):
        for half, name, s in ((slice(0, 1024), "rotation", x.pa[j]), (slice(1024, 2048), "masked", x.pb[j])):
            elementwise("%s feat pair %d, %s half" % (case, j, name), B["feat"][j][:, half], ref[j][:, half], mag[j][:, half], sr.K_BN, sl[s])


@pytest.mark.parametrize("case", sorted(CASES))
def test_head_conv0_forward(gpu, case):
    """head norm0 + ReLU + conv0 (2048 -> 64): statistics PER PAIR, K = 2048, every pixel of every pair"""
    x, B = _fwd(gpu, case)
    g, b, w = x.hp("norm0.weight"), x.hp("norm0.bias"), x.hp("conv0.weight").reshape(64, 2048)
    for j in range(x.NP):
        ref, a64 = sr.head_conv0(B["feat"][j], g, b, w)
        mag = a64 @ np.abs(w.astype(np.float64)).T + 1e-300
        chain = _fp32_chain(sr.bn32(B["feat"][j], g, b), w)
        gate("%s head conv0 pair %d" % (case, j), dr.rms(B["h1"][j], ref, mag), dr.rms(chain, ref, mag), 2.0, n=ref.size)


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
def _wgrad_gate(what, got, a64, w64, a32, w32):
    """the project's weight-gradient gate against the blocked fp32 reduction, its 512-term form printed beside the gated 64-term one"""
    a32, w32 = np.ascontiguousarray(a32), np.ascontiguousarray(w32)
    wgrad_gate(what, got, a64, w64, lambda blk: _fp32_blocked(a32, w32, blk), (64, 512))


@pytest.mark.parametrize("case", sorted(CASES))
def test_head_conv0_and_norm5_backward(gpu, case):
    """Stop 350: the head and norm5_bwd_kernel are done, nothing of block 4 yet.
      * head conv0 data gradient: df = relu'(bn0(feat)) * (A @ W0), A = the BN-corrected dh1 (gamma = head norm1), K = 64: 2x chain;
      * head conv0 weight gradient: sum over pairs and pixels of A^T relu(bn0(feat)): 3x blocked, every 8th row / column;
      * norm5 backward: g4 = gamma5 * sum over the stream's users of the BN-corrected df of that user's half - every single-user
        rotation stream and the shared masked stream (5 users at S = 640: the fifth shares phase 0 with the first; 2 at S = 672);
      * norm5.bias / norm5.weight: the sums of dy5 and dy5 * xhat5 over all streams (final here: the kernel adds them itself).
        norm5 feeds the head's BatchNorm directly, so both cancel to (nearly) nothing: they are held to their sum |term|."""
    x = _ctx(gpu, case)
    grads = x.backward_to(350)
    h1, dh1 = x.rd("h1", x.NP, 5, 64), x.rd("dh1", x.NP, 5, 64)
    Fm, DF = x.rd("feat", x.NP, 5, 2048), x.rd("df", x.NP, 5, 2048)
    x4, g4 = x.rd("x4", x.NS, 5, 1024), x.rd("g4", x.NS, 5, 1024)
    g0, b0, g1 = x.hp("norm0.weight"), x.hp("norm0.bias"), x.hp("norm1.weight")
    w0 = x.hp("conv0.weight").reshape(64, 2048)
    A64s, A32s, P64s, P32s = [], [], [], []
    for j in range(x.NP):
        ref, A64, on, _ = sr.head_conv0_bwd(h1[j], dh1[j], Fm[j], g1, g0, b0, w0)
        A32 = sr.bn_bwd32(dh1[j], h1[j], g1)
        mag = on * (sr.bn_bwd_mag(dh1[j], h1[j], g1) @ np.abs(w0.astype(np.float64))) + 1e-300
        chain = (on * _fp32_chain(A32, np.ascontiguousarray(w0.T))).astype(np.float32)
        keep = sr.bn_keep(Fm[j], g0, b0)
        assert 1 - keep.mean() <= 0.01, ("borderline ReLU signs", 1 - keep.mean())
        gate("%s head conv0 dgrad pair %d" % (case, j), dr.rms(DF[j], ref, mag, keep), dr.rms(chain, ref, mag, keep), 2.0, n=int(keep.sum()))
        A64s.append(A64); A32s.append(A32)
        P64s.append(np.maximum(sr.bn_pre(Fm[j], g0, b0), 0.0)[:, ::8]); P32s.append(sr.bn32(Fm[j], g0, b0)[:, ::8])
    # measured on the MI355X: 1.46 (S = 640, 2000 terms) and 1.21 (S = 672, 882 terms) of the 64-term blocked reduction; gate 3.0
    _wgrad_gate("%s head conv0 wgrad" % case, grads[HEAD + "conv0.weight"].reshape(64, 2048)[::8, ::8],
                np.concatenate(A64s)[:, ::8], np.concatenate(P64s), np.concatenate(A32s)[:, ::8], np.concatenate(P32s))

    g5 = x.tp("norm5.weight")
    G4, dy5, mag, db, dg, dbm, dgm = sr.norm5_bwd(list(x4), Fm, DF, g0, g5, x.pa, x.pb)
    for s in range(x.NS):
        users = x.NP if s == x.NS - 1 else 1
        # k_g4: one user's path (a, q1 and k from the fp32 tile sums of the head's data gradient, x - mean, the fused multiply-add,
        # the product with a: K_DY5_USER = 142), the product with gamma5, one add per user and the phase tree (stage_ref.k_g4)
        elementwise("%s norm5 backward stream %d (%d user%s)" % (case, s, users, "s" if users > 1 else ""),
                    g4[s], G4[s], np.abs(g5) * mag[s], sr.k_g4(users))
    # k_sums5: a term's own path, xhat5 and the product, <= 80 fp32 adds per thread, one fp32 atomic per (stream, workgroup)
    k = sr.k_sums5(x.H[5] ** 2, x.NS - 1, True)
    elementwise("%s norm5.bias gradient" % case, grads[TRUNK + "norm5.bias"], db, dbm, k)
    elementwise("%s norm5.weight gradient" % case, grads[TRUNK + "norm5.weight"], dg, dgm, k)


@pytest.mark.parametrize("t", [3, 2, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_transition_backward(gpu, case, t):
    """Stop (t - 1) * 100 + 50: behind transition t's backward, before block t's dense layers.  g{t+1} still holds block t+1's final
    G' (the transition only reads it), g{t} holds what E_UNPOOL stored over all its channels.
      * data gradient: g{t}[p][c] = gamma_t[c] * relu'(bn_t(x{t}))[p][c] * 1/4 * sum_k dX[pool(p)][k] * W_t[k][c], dX = the corrected
        gradient of x{t+1}[:, :C0]: 2x chain on a sample of <= 1024 pooled pixels (4096 pixels) per stream + the whole plane;
      * weight gradient: sum over streams and pooled pixels of dX[q][k] * avgpool2(relu(bn_t(x{t})))[q][c]: 3x blocked.
    The yardsticks' fp32 operand dX takes mean(G') and mean(G' * xhat) from sums formed the way the engine forms its backward
    statistics (fp32 over the rows of a tile, fp64 across tiles: stage_ref.tile_sum32), not from fp64 sums: the weight gradient adds a
    deviation of those two means COHERENTLY over all pixels (the other operand is >= 0), so it answers to a tenth of a rounding in them.
    Measured with fp64 sums in the yardstick, S = 640: transition 1's weight gradient at 3.49x the blocked reduction (5.18e-8 against
    1.48e-8), transition 2's at 2.35x; the engine's sums sat 0.06 - 0.10 roundings (rms, of mean |G'|) from the fp64 sums of the stored
    G', and against a reference built on them the same gradients were at 2.76e-8 / 1.63e-8: the products were never off, the yardstick
    left out a rounding the kernels legitimately make."""
    x = _ctx(gpu, case)
    grads = x.backward_to((t - 1) * 100 + 50)
    H, Cp = x.H[1 + t], CT[t - 1]
    C0, Hn = Cp // 2, H // 2
    X, Gt = x.rd("x%d" % t, x.NS, 1 + t, Cp), x.rd("g%d" % t, x.NS, 1 + t, Cp)
    Xn, Gn = x.rd("x%d" % (t + 1), x.NS, 2 + t, CT[t])[:, :, :C0], x.rd("g%d" % (t + 1), x.NS, 2 + t, CT[t])[:, :, :C0]
    g, b = x.tp("transition%d.norm.weight" % t), x.tp("transition%d.norm.bias" % t)
    w = x.tp("transition%d.conv.weight" % t).reshape(C0, Cp)
    q = dr.sample(Hn * Hn)
    qy, qx = q // Hn, q % Hn
    pix = np.stack([(2 * qy + dy) * H + 2 * qx + dx for dy in (0, 1) for dx in (0, 1)], axis=1).ravel()      # the 4 pixels of each pooled pixel
    cols = np.arange(0, Cp, max(1, Cp // 128))
    dX64s, dX32s = [], []
    for n in range(x.NS):
        ref, dX, on = sr.transition_bwd(X[n], H, H, g, b, w, Xn[n], Gn[n])
        dX32 = sr.bn_bwd32(Gn[n], Xn[n], tile_sums=True)
        mag = np.abs(g) * on * 0.25 * sr.unpool2(sr.bn_bwd_mag(Gn[n], Xn[n]) @ np.abs(w.astype(np.float64)), H, H) + 1e-300
        keep = sr.bn_keep(X[n], g, b)
        assert 1 - keep.mean() <= 0.01, ("borderline ReLU signs", 1 - keep.mean())
        up = (np.float32(0.25) * _fp32_chain(dX32[q], np.ascontiguousarray(w.T[cols]))).astype(np.float32)     # [pooled pixel][column]
        sel = np.ix_(pix, cols)
        chain = (g[cols] * (on[sel] * np.repeat(up, 4, axis=0)).astype(np.float32)).astype(np.float32)
        # measured on the MI355X: 0.83 - 0.95 of the chain on every stream but the masked one of S = 640 behind transition 1: 1.64 (sample)
        # / 1.63 (whole plane); gate 2.0.  That stream is mostly background: on its few object pixels |xhat| is large, the term
        # (x - mean) * k carries the gradient, and k = invstd * mean(G' * xhat) is a sum that cancels to 2 % of its terms' size - the
        # engine's sum sat 0.25 roundings (rms, 1.3 at most) of those terms from the fp64 sum of the stored G'.
        gate("%s transition %d dgrad stream %d" % (case, t, n), dr.rms(Gt[n][sel], ref[sel], mag[sel], keep[sel]),
             dr.rms(chain, ref[sel], mag[sel], keep[sel]), 2.0, e_whole=dr.rms(Gt[n], ref, mag, keep), n=int(keep[sel].sum()))
        dX64s.append(dX); dX32s.append(dX32)
    P64 = np.concatenate([sr.pooled_act(X[n], H, H, g, b)[:, ::8] for n in range(x.NS)])
    P32 = np.concatenate([sr.pooled_act32(X[n], H, H, g, b)[:, ::8] for n in range(x.NS)])
    # measured on the MI355X, of the 64-term blocked reduction (gate 3.0): S = 640 transition 3 / 2 / 1 at 1.20 / 1.61 / 2.40 (2400 / 9600
    # / 38400 terms), S = 672 at 1.13 / 1.15 / 0.75 (1323 / 5292 / 21168 terms)
    _wgrad_gate("%s transition %d wgrad" % (case, t), grads[TRUNK + "transition%d.conv.weight" % t].reshape(C0, Cp)[::8, ::8],
                np.concatenate(dX64s)[:, ::8], P64, np.concatenate(dX32s)[:, ::8], P32)
