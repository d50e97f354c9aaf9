"""Operator-level gates on the DENSE LAYERS, per kernel variant: one dense layer's buffers are read back from the engine and the layer is
recomputed in fp64 from its OWN input buffers with its own fp64 batch statistics over [:HW] of each stream (tests/dense_ref.py,
proved against torch and autograd in tests/test_cpu_dense_ref.py, which also shows what each gate catches).  The stages around the
dense layers have theirs in tests/test_gpu_stage_gates.py.

Four cases; the walk picks the kernel instantiation from the plane, the number of streams of the call (of the forward CHAIN: calls of
8 streams and more run as two chains of NS / 2 and NS - NS / 2 streams, forward.hip) and the layer's place in its group.  VARIANTS
below is that choice per case and block, test_geometry_selects_the_variants_of_the_table derives it from eng.H / eng.HWp with the
rules of the source (tests/gate_harness.py) - halo_tile (wgrad_plan.h: 16 x 16 tiles from 200 tiles per launch), HWp % 128 and the
small_wgs = 320 rule of the forward conv1 (forward.hip), w1_partial_tiles / plan_layer_wgrads (wgrad_plan.h: the 1x1 weight gradient adds with fp32 atomics
only in calls of <= 4 streams on planes of <= 1600 pixels) and gs_on_side (backward.hip):

 case  call                          plane (HWp / HW)       conv1 forward   3x3 tile, fwd / bwd        1x1 wgrad        GS / reduces
 A     S = 640, 6 streams            160^2  25600 / 25600   CfgP128x128     16 exact / 16 exact        wave-specialised materialised on the chain,
       (5 rotations + masked),        80^2   6400 /  6400   wave-spec.       8 / 8                     (partial tiles)  one reduce per layer
       sample 3 at dq = 1e-6          40^2   1600 /  1600   CfgP32x64        8 / 8
                                      20^2    448 /   400   CfgP32x64        8 ragged (2.5 tiles)
 B     S = 672, 3 streams            168^2  28288 / 28224   CfgP128x128     16 bounds-checked (10.5)   wave-specialised materialised on the chain
       (the stage gates' scene)       84^2   7104 /  7056   wave-spec.       8 ragged (10.5)           (partial tiles)
                                      42^2   1792 /  1764   CfgP32x64        8 ragged (5.25)           (1764 > 1600)
                                      21^2    448 /   441   CfgP32x64        8 ragged (2.6)            generic, atomics gs_on_side, HALO3_PAIRED reduces
 C     S = 640, 2 streams            160^2                  CfgP128x128     16 exact (200 tiles)       wave-specialised materialised on the chain
       (the single-sample step)       80^2                  wave-spec.       8                         (partial tiles)
                                      40^2, 20^2            CfgP32x64        8                         generic, atomics gs_on_side, HALO3_PAIRED reduces
 D     S = 640, 17 streams           160^2                  CfgP128x128     16 exact                   wave-specialised materialised on the chain
       (16 rotations + masked:        80^2                  CfgP128x128     16 forward (chains of 8    (partial tiles)
       chains of 8 and 9)                                                   and 9: 200 / 225 tiles),
                                                                            16 backward
                                      40^2                  wave-spec.       8
                                      20^2                  CfgP32x64        8 ragged
 The per-layer 1x1 data gradient takes CfgP128x64 / CfgP64x64 and the grouped one GemmCfg<128, 64, 32> / CfgP64x64 by HWp % 128.

Forward (ONE forward per case, every buffer read after it): layers (1,1), (1,6), (2,1), (2,12), (3,1), (3,24), (4,1), (4,8), (4,16) on
the first, a middle and the last (masked) stream; conv1 and conv2 each within 2x the fp32 chain, the chain on a pixel sample (first and
last rows + strided), the kernel's error on the sample AND on the whole plane.
Backward (ONE debug_stop per (case, layer)): the conv2 data gradient (2x chain, exact zeros where the ReLU is clearly off), norm2's
backward in unit form (2e-5 of every 64-row block's maximum, padding rows included), norm2's dgamma / dbeta (_WGRAD_GATE x the blocked
reduction), both weight gradients (_WGRAD_GATE x the blocked reduction over ALL streams x pixels), the conv1 data gradient in the
form(s) the layer takes (2x chain; sample and whole plane).  The layers cover every g_lo with nseg = 4 (blocks 2-4), per-layer widths
32 / 64 / 96, tops and bottoms of groups, and block 4 under every stream regime.

gs_on_side layers: the 3x3 data gradient never reads the materialised GS - it applies the BN backward to the G' / x slices on load.
Its reference is the fp64 GS formed from gsnap[:, cin:cin+32] (the layer's own 1x1 data gradients never touch those columns) and the x
slice.  Its yardstick is the fp32 chain over the fp32 EVALUATION of that operand (dense_ref.gs_on_load: bnb1's roundings and the
statistics' fp32 tile sums are in the chain's operand, factor 2 unchanged; measured 0.66 - 0.69 of the chain), and the roundings
themselves are counted from halo.cuh / gemm.cuh (dense_ref.K_GS_LOAD = 10) and held on the GS the side stream materialises with the
same bnb1 for the weight gradients (measured 1.4 - 2.6).  The weight gradients read gs_ as everywhere.

Padding rows, confirmed from the source before asserting:
  * D2: bn_bwd_apply_split_kernel stores zeros for rows >= HW (elem.cuh) - asserted EXACTLY zero, and part of the unit-form check;
  * x<b>: NO kernel of the forward stores rows >= HW (the halo forward stores in-plane pixels, the tile epilogues skip them) - they hold
    what the allocation held, and the 1x1 kernels that read them clamp (bnrelu4<H>): asserted finite, their largest magnitude printed;
  * GS: bn_bwd_apply_kernel stores rows < HW only and the ring slot is shared with planes of other blocks - its padding rows are
    earlier layers' rows, and the halo kernels that read GS address pixels (y, x) inside the plane: nothing to assert.

Raw output of a run on the MI355X: profiles/dense_gates.txt."""
import numpy as np
import pytest
import torch

import dense_ref as dr
import stage_ref as sr
from gate_harness import SCENES, TRUNK, GateCtx, conv1_fwd_cfg, forward_chains, gate, gpu, halo_tile, wgrad_gate  # noqa: F401  (gpu: the fixture)
from helpers import _WGRAD_BLK, _WGRAD_GATE, _fp32_blocked, product_net

pytestmark = pytest.mark.gpu

CASES = {"A": SCENES["S640x6"], "B": SCENES["S672x3"], "C": SCENES["S640x2"], "D": SCENES["S640x17"]}
# per block: (conv1 forward, 3x3 tile forward, 3x3 tile backward, bounds-checked 16 x 16, gs_on_side); per case: the 1x1 weight gradient of blocks 1-4
VARIANTS = {"A": ([("P128x128", 16, 16, False, False), ("ws", 8, 8, False, False), ("P32x64", 8, 8, False, False), ("P32x64", 8, 8, False, False)], ["ws"] * 4),
            "B": ([("P128x128", 16, 16, True, False), ("ws", 8, 8, False, False), ("P32x64", 8, 8, False, False), ("P32x64", 8, 8, False, True)], ["ws", "ws", "ws", "atomics"]),
            "C": ([("P128x128", 16, 16, False, False), ("ws", 8, 8, False, False), ("P32x64", 8, 8, False, True), ("P32x64", 8, 8, False, True)], ["ws", "ws", "atomics", "atomics"]),
            "D": ([("P128x128", 16, 16, False, False), ("P128x128", 16, 16, False, False), ("ws", 8, 8, False, False), ("P32x64", 8, 8, False, False)], ["ws"] * 4)}
FWD_LAYERS = [(1, 1), (1, 6), (2, 1), (2, 12), (3, 1), (3, 24), (4, 1), (4, 8), (4, 16)]
BWD_LAYERS = {"A": [(1, 3), (1, 6), (2, 5), (2, 6), (3, 21), (4, 1), (4, 14), (4, 16)],
              "B": [(1, 3), (1, 6), (2, 9), (3, 21), (3, 24), (4, 13), (4, 16)],
              "C": [(2, 12), (3, 21), (3, 24), (4, 13), (4, 16)],
              "D": [(2, 9), (2, 12)]}
_STATE, _FWD = {}, {}


def _ctx(gpu, case):
    """the net (one for all cases), and the heightmaps and stream layout of one case"""
    if "net" not in _STATE:
        _STATE["net"] = product_net(0)
        _STATE["sd"] = {k: v.detach().cpu().numpy() for k, v in _STATE["net"].state_dict().items()}
    if case not in _STATE:
        _STATE[case] = GateCtx(_STATE["net"], _STATE["sd"], CASES[case], gpu)
    return _STATE[case]


def _streams(x):
    return sorted({0, x.NS // 2, x.NS - 1})          # the first, a middle one, the last (masked) stream


# ---- the variant table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_geometry_selects_the_variants_of_the_table(gpu, case):
    x = _ctx(gpu, case)
    x.forward()
    NS = x.NS
    chains = forward_chains(NS, x.H[2])
    got = []
    for b in range(4):
        H, HWp = x.H[2 + b], x.HWp[2 + b]
        c1, t_f = {conv1_fwd_cfg(HWp, ns, True) for ns in chains}, {halo_tile(H, ns) for ns in chains}
        assert len(c1) == 1 and len(t_f) == 1, (case, b, c1, t_f)              # both chains take the same instantiations
        t_b = halo_tile(H, NS)
        got.append((c1.pop(), t_f.pop(), t_b, t_b == 16 and H % 16 != 0, NS <= 4 and H * H <= 1600))
    w1 = ["ws" if NS > 4 or H * H > 1600 else "atomics" for H in x.H[2:]]           # w1_partial_tiles (cin > 64: every gated layer)
    print("case %s: %d streams, forward chains %s: %s, 1x1 weight gradient %s" % (case, NS, chains, got, w1))
    assert (got, w1) == VARIANTS[case]


# ---- forward -----------------------------------------------------------------------------------------------------------------------------
def _fwd(gpu, case):
    """ONE forward per case; every buffer the forward gates compare is read after it (the three gated streams only are kept)"""
    if case not in _FWD:
        _FWD.clear()                                                            # one case's buffers at a time
        x = _ctx(gpu, case)
        x.forward()
        B = {}
        for b in range(1, 5):
            full = x.rd("x%d" % b, x.NS, 1 + b, dr.CT[b - 1], pad=True)
            HW = x.H[1 + b] ** 2
            padrows = full[:, HW:]
            # the forward stores no row >= HW of x<b> (module docstring): whatever lies there is read by the 1x1 kernels, which clamp
            print("case %s x%d: %d padding rows per stream, largest |value| %.3e" % (case, b, padrows.shape[1], np.abs(padrows).max() if padrows.size else 0.0))
            assert np.isfinite(padrows).all()
            B["x%d" % b] = full[_streams(x)][:, :HW].copy()
        for b, l in FWD_LAYERS:
            B["bt%d_%d" % (b, l)] = x.rd("bt%d_%d" % (b, l), x.NS, 1 + b, 128, _streams(x))
        _FWD[case] = B
    return _ctx(gpu, case), _FWD[case]


@pytest.mark.parametrize("block,layer", FWD_LAYERS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_forward_layer(gpu, case, block, layer):
    """norm1 + ReLU + conv1 from x<b>[:, :cin] and norm2 + ReLU + conv2 from the bottleneck, on three streams, whole planes"""
    x, B = _fwd(gpu, case)
    H, cin = x.H[1 + block], dr.cin_of(block, layer)
    g1, b1, w1 = x.lp(block, layer, "norm1.weight"), x.lp(block, layer, "norm1.bias"), x.lp(block, layer, "conv1.weight").reshape(128, cin)
    g2, b2, w2 = x.lp(block, layer, "norm2.weight"), x.lp(block, layer, "norm2.bias"), x.lp(block, layer, "conv2.weight")
    pix = dr.sample(H * H)
    for k, n in enumerate(_streams(x)):
        X, BT = B["x%d" % block][k], B["bt%d_%d" % (block, layer)][k]
        ref, mag = dr.conv1_fwd(X[:, :cin], g1, b1, w1)
        chain = dr.conv1_chain(X[:, :cin], g1, b1, w1, pix)
        gate("case %s conv1 (%d,%d) K %d stream %d" % (case, block, layer, cin, n), dr.rms(BT[pix], ref[pix], mag[pix]), dr.rms(chain, ref[pix], mag[pix]), 2.0,
             e_whole=dr.rms(BT, ref, mag), n=chain.size)
        ref, mag = dr.conv2_fwd(BT, H, H, g2, b2, w2)
        chain = dr.conv2_chain(BT, H, H, g2, b2, w2, pix)
        got = X[:, cin:cin + 32]
        gate("case %s conv2 (%d,%d) stream %d" % (case, block, layer, n), dr.rms(got[pix], ref[pix], mag[pix]), dr.rms(chain, ref[pix], mag[pix]), 2.0,
             e_whole=dr.rms(got, ref, mag), n=chain.size)


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
def test_a_stopped_backward_leaves_nothing_in_the_affine_gradient_scratch(gpu):
    """The norm1 / transition-norm dbeta and dgamma go through a scratch that db_flush_kernel adds to the gradients - and zeroes - at
    the END of the walk.  A backward that leaves at a debug_stop must not hand its share to the next call: with this module in front
    of tests/test_gpu_parity.py the end-to-end gradient test once saw 118 tensors (every norm1 weight and bias) at up to 787x its bound.
    The same step before and after a backward stopped behind block 4: two runs differ by the order of their fp32 atomics (parts in
    10^6); a scratch left behind adds block 4's sums a second time (an error of the size of the gradient itself)."""
    x = _ctx(gpu, "C")
    names = [TRUNK + "denseblock%d.denselayer%d.norm1.%s" % (b, l, p) for b, l in ((4, 16), (4, 1), (3, 24), (1, 1)) for p in ("weight", "bias")]

    def step():
        q = x.forward()
        x.net.zero_grad()
        x.net._engine_backward(x.net._saved[1], torch.tensor(CASES["C"]["dq"], dtype=torch.float32, device=gpu).view(q.shape))
        torch.cuda.synchronize()
        g = dict(x.net.named_parameters())
        return {n: g[n].grad.detach().cpu().numpy().astype(np.float64) for n in names}
    before = step()
    x.backward_to(300)
    after = step()
    for n in names:
        rel = np.abs(after[n] - before[n]).max() / np.abs(before[n]).max()
        print("%s: max |difference| / max |gradient| across a stopped backward %.2e" % (n, rel))
        assert rel <= 1e-3, (n, rel)


def _wgrad_gate(what, got, a32, w64, w32):
    """(a is an fp32 buffer on both sides; only the gated 64-term reduction is evaluated: the whole reduction runs over up to 10^5 pixels)"""
    a32, w32 = np.ascontiguousarray(a32), np.ascontiguousarray(w32)
    wgrad_gate(what, got, a32.astype(np.float64), w64, lambda blk: _fp32_blocked(a32, w32, blk), (_WGRAD_BLK,))


@pytest.mark.parametrize("case,block,layer", [(c, b, l) for c in sorted(BWD_LAYERS) for b, l in BWD_LAYERS[c]])
def test_backward_layer(gpu, case, block, layer):
    """Stop behind dense layer (block, layer): GS and D2 from their ring slots, the raw 3x3 data gradient (dy2), G' in front of (gsnap)
    and behind (g<b>) the layer's 1x1 data gradients, the layer's finished gradients.

    Measured on the MI355X (profiles/dense_gates.txt): every 2x-chain gate at 0.61 - 1.67 of the chain (whole planes <= 1.52), the unit
    form at <= 1.4e-6 of a block's maximum (bound 2e-5), norm2's affine gradients at <= 2.54, the conv2 weight gradient at <= 1.79 and the
    conv1 weight gradient at <= 2.67 (case D (2,12); A (1,6) 2.64) of the blocked reduction (gate 3.0).

    Found by this gate and fixed (wgrad_plan.h w1_partial_tiles): the conv1 weight gradient of case B stood at 3.61 on (1,3), 7.32 on
    (1,6) and 2.98 / 2.99 / 3.02 in three runs on (2,9) of the 64-term blocked reduction (9.84e-8 against 2.72e-8, 1.57e-7 against
    2.15e-8, 3.83e-8 against 1.27e-8; gate 3.0).  Traced (backward.hip issue_wgrads -> BwdWeightP, plan_layer_wgrads): a call of <= 4
    streams took the generic kernel with ~128 workgroups per layer on EVERY plane, so on 168^2 one workgroup accumulated a chunk of 1344
    (K = 128) or 2624 (K = 224) pixels in one set of fp32 MFMA accumulators and then added its 128 x 64 tile to dW with fp32 atomics
    (33 - 63 per element, in no fixed order).  A numpy model of exactly that - chunk-long sequential fp32 chains, the chunks added in
    order - reproduced the error's size in all five cases measured (the kernel at 0.24 - 0.26 of the model; spread over the elements,
    no tile missing or counted twice): the products were right, the REDUCTION was ~200 dependent fp32 adds per element where the
    yardstick chains 64.  Shorter chunks only move the adds into the atomics.  Few-stream calls now keep the atomics on planes of <=
    1600 pixels only and take the partial-tile form with the fixed-order reduce above that: (1,3) 1.26, (1,6) 2.35, (2,9) 1.30, and
    reproducible; C (2,12) 1.67 -> 0.88.  The single-sample step measured 5.651 / 5.644 ms before and 5.656 / 5.633 ms after
    (medians of 7 x 40 steps, alternating on one MI355X)."""
    x = _ctx(gpu, case)
    _FWD.clear()
    b, i = block - 1, layer - 1
    grads = x.backward_to(b * 100 + i)
    H, HW, HWp, Ct, cin, Lb = x.H[1 + block], x.H[1 + block] ** 2, x.HWp[1 + block], dr.CT[b], dr.cin_of(block, layer), dr.LAYERS[b]
    tag = "case %s (%d,%d)" % (case, block, layer)
    on_side = x.NS <= 4 and HW <= 1600
    assert on_side == VARIANTS[case][0][b][4]
    S3 = _streams(x)
    X, BT = x.rd("x%d" % block, x.NS, 1 + block, Ct), x.rd("bt%d_%d" % (block, layer), x.NS, 1 + block, 128)
    GS, DY = x.rd("gs_%d_%d" % (block, layer), x.NS, 1 + block, 32), x.rd("dy2", x.NS, 1 + block, 128)
    D2p = x.rd("d2_%d_%d" % (block, layer), x.NS, 1 + block, 128, pad=True)
    D2 = D2p[:, :HW]
    G0, G1 = x.rd("gsnap", x.NS, 1 + block, Ct, S3), x.rd("g%d" % block, x.NS, 1 + block, Ct, S3)
    g1, b1, w1 = x.lp(block, layer, "norm1.weight"), x.lp(block, layer, "norm1.bias"), x.lp(block, layer, "conv1.weight").reshape(128, cin)
    g2, b2, w2 = x.lp(block, layer, "norm2.weight"), x.lp(block, layer, "norm2.bias"), x.lp(block, layer, "conv2.weight")
    pix = dr.sample(HW)

    # ---- padding rows of D2: zeros, exactly (bn_bwd_apply_split_kernel stores them)
    assert not D2p[:, HW:].any(), "D2 padding rows"

    for k, n in enumerate(S3):
        # ---- conv2 data gradient with the ReLU mask
        on, off = dr.relu_sides(BT[n], g2, b2)
        assert dr.excluded_share(on, off) <= 0.01, ("borderline ReLU signs", dr.excluded_share(on, off))
        if on_side:       # the operand is formed on load from the G' / x slices (the materialised gs_ is the weight gradients' operand)
            gs64, gs32, gmag = dr.gs_on_load(G0[k][:, cin:cin + 32], X[n][:, cin:cin + 32])
            ref, mag = dr.conv2_dgrad(gs64, H, H, w2)
            # the same bnb1 runs on the side stream (bn_bwd_apply_kernel): the materialised GS within the counted roundings of the fp64 GS
            # (measured on the MI355X: 1.4 - 2.6 roundings of the magnitudes, cases B and C, against K_GS_LOAD = 10)
            e_mat = float((np.abs(GS[n].astype(np.float64) - gs64) / (gmag + 1e-300)).max())
            print("%s stream %d: the side stream's materialised GS against the fp64 GS of gsnap: max |err| / mag = %.2f x 2^-24 (%d counted)" % (tag, n, e_mat / sr.U, dr.K_GS_LOAD))
            assert e_mat <= dr.K_GS_LOAD * sr.U, (tag, n, e_mat / sr.U)
        else:
            gs32 = GS[n]
            ref, mag = dr.conv2_dgrad(gs32, H, H, w2)
        chain = dr.conv2_dgrad_chain(gs32, H, H, w2, pix)
        gate("%s conv2 dgrad stream %d%s" % (tag, n, " (BN backward on load)" if on_side else ""), dr.rms(DY[n][pix], ref[pix], mag[pix], on[pix]),
             dr.rms(chain, ref[pix], mag[pix], on[pix]), 2.0, e_whole=dr.rms(DY[n], ref, mag, on), n=int(on[pix].sum()))
        assert not DY[n][off].any(), "conv2 dgrad: non-zero where the ReLU is clearly off"

        # ---- norm2 backward as stored for the three 1x1 consumers (units + block scales), padding rows included
        rel = dr.unit_form_error(D2p[n], dr.norm2_bwd(DY[n], BT[n], g2))
        print("%s norm2 backward in unit form, stream %d: max |err| / block max %.3e" % (tag, n, rel))
        assert rel <= dr.UNIT_FORM_BOUND, rel

        # ---- conv1 data gradient: per-layer form on [cs, cin), grouped form on [0, cs) at the bottom of a group
        for layers, c0, c1 in dr.dgrad1_segments(Lb, i, dr.CIN0[b]):
            prm = [(x.lp(block, l + 1, "norm1.weight"), x.lp(block, l + 1, "norm1.bias"), x.lp(block, l + 1, "conv1.weight").reshape(128, -1)) for l in layers]
            d2s = [D2[n] if l == i else x.rd("d2_%d_%d" % (block, l + 1), x.NS, 1 + block, 128, [n])[0] for l in layers]
            ref, mag, _, keep = dr.conv1_dgrad(G0[k], X[n], prm, d2s, c0, c1, chain=False)
            assert 1 - keep.mean() <= 0.01, ("borderline ReLU signs", 1 - keep.mean())
            rs, ms, ch, ks = dr.conv1_dgrad(G0[k], X[n], prm, d2s, c0, c1, take=pix)
            gate("%s conv1 dgrad stream %d, %s form, layers %s, columns %d..%d" % (tag, n, "grouped" if len(layers) > 1 or c0 == 0 else "per-layer", [l + 1 for l in layers], c0, c1),
                 dr.rms(G1[k][pix, c0:c1], rs, ms, ks), dr.rms(ch, rs, ms, ks), 2.0, e_whole=dr.rms(G1[k][:, c0:c1], ref, mag, keep), n=int(ks.sum()))

    # ---- norm2's affine gradients: sums over ALL streams and pixels
    aff = dr.norm2_affine(DY, BT)
    for name, got, ref, mag, terms in (("bias", grads[TRUNK + "denseblock%d.denselayer%d.norm2.bias" % (block, layer)], aff["db"], aff["dbm"], aff["tb"]),
                                       ("weight", grads[TRUNK + "denseblock%d.denselayer%d.norm2.weight" % (block, layer)], aff["dg"], aff["dgm"], aff["tg"])):
        e_prod, e_blk = dr.rms(got, ref, mag), dr.rms(dr.sum_blocked32(terms, _WGRAD_BLK), ref, mag)
        print("%s norm2.%s gradient: err/sum|term| rms product %.3e, blocked fp32 64-term %.3e over %d terms: ratio %.2f" % (tag, name, e_prod, e_blk, len(terms), e_prod / e_blk))
        assert e_prod <= _WGRAD_GATE * e_blk, ("norm2." + name, e_prod, e_blk)

    # ---- conv2 weight gradient on every 9th of the 9 * 128 im2col columns (only those are formed), the whole reduction
    cols = np.arange(0, 9 * 128, 9)
    Gs, A64, A32 = dr.conv2_wgrad_ops(GS, BT, H, H, g2, b2, cols)
    _wgrad_gate("%s conv2 wgrad" % tag, dr.w2_grad_mat(grads[TRUNK + "denseblock%d.denselayer%d.conv2.weight" % (block, layer)])[:, cols], Gs, A64, A32)
    del A64, A32

    # ---- conv1 weight gradient: 16 of the 128 rows x <= 128 columns, the whole reduction
    rows, cols = np.arange(0, 128, 8), np.arange(0, cin, max(1, cin // 128))
    D, A64, A32 = dr.conv1_wgrad_ops(D2, X, g1, b1, rows, cols)
    _wgrad_gate("%s conv1 wgrad K %d" % (tag, cin), grads[TRUNK + "denseblock%d.denselayer%d.conv1.weight" % (block, layer)].reshape(128, cin)[np.ix_(rows, cols)], D, A64, A32)
