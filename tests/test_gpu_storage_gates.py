"""Operator-level gates on the two 16-BIT STORAGE MODES - net.set_precision("bf16") (mode 1: bf16 activations and gradients, one bf16
MFMA term per product; BASELINE.json config 3) and "fp16" (mode 2: fp16 activations and forward products, bf16 gradients and backward
products; config 5).  The mode-0 gates (test_gpu_stage_gates.py, test_gpu_dense_gates.py) hold only the PREC = 0 instantiations of the
kernel templates; the other two were known end to end only, within bounds wide enough to hide a dropped tile row or the wrong half of
a 16-bit pair.  Here every stage is recomputed in fp64 from the buffer the kernel READ (as stored, widened by debug_read) with fp64
batch statistics over the stored values (one exception, below), and held to the 16-bit yardstick of tests/storage_ref.py (proved in
tests/test_cpu_storage_ref.py, which also shows what each gate still catches at 16-bit resolution):
  * matrix products and data gradients: within the project's factor 2.0 of the STORAGE CHAIN - the fp32 multiply-add chain over the
    operands rounded once where the kernel rounds them, its result rounded once to the destination's storage type (rms of err / sum
    |a||w| on the pixel sample of dense_ref.sample AND on the whole plane, both against the sample's chain error);
  * weight gradients: within _WGRAD_GATE x the blocked fp32 reduction over the rounded operands, over all streams x pixels;
  * element-wise stages (pool0 into x1, norm5_bwd into g4): the mode-0 bound k * 2^-24 * mag (stage_ref.K_*) plus half a storage ulp;
  * planes whose producer summed its statistics BEFORE the 16-bit store (every producer of a 16-bit plane does: storage_ref's docstring
    cites them; test_bottleneck_sums_are_taken_before_the_store checks the form on the engine's own fp64 sums): the engine's mean and
    invstd are not those of the stored plane.  The element-wise gates add the derived slack (storage_ref.bn_store_slack /
    xhat_sum_slack), the ReLU keep-mask widens by it (storage_ref.keep_s; its cap stays the project's 1 %).  The PRODUCT gates take no
    slack at all - the stricter form: where the engine's statistics follow from an fp32 buffer the reference takes them from it
    (pool0's 64 channels of x1, from the stem plane: storage_ref.x1_stats), everywhere else it takes the stored plane's, and the factor
    2.0 holds as it stands.  Found by these gates, traced to the source, no bug: with the stored plane's statistics on pool0's channels
    conv1 of layer (1,1) sat at 9.9x (bf16) / 12.5x (fp16) the chain on the first stream of S = 640, layer (1,6) at 3.7x / 4.0x,
    transition 1 at 2.8x / 2.5x - a heightmap's flat background is ONE value on most of the plane, rounds one way, and moves the mean
    by up to half a storage ulp, which (x - mean) * invstd of exactly those pixels magnifies; with the statistics pool0_kernel summed
    (recomputed from the fp32 stem plane) the same products are at 1.00 - 1.24.

One bug these gates did find, in the library: the padding rows [HW, HWp) of the block buffers, which no forward kernel stores and the
1x1 kernels read as they lie, held the OTHER storage type's words after a change of mode on a used engine (x4 at S = 640: NaN among
the 48 rows of every stream; an inf there against the weight gradient's zero gradient rows is a NaN column of dW).  The fixture runs
a default-mode forward in front of every switch so that the padding-row assertion of _fwd meets that state whatever ran before;
smg_engine_set_precision now zeroes the mode-typed buffers when the mode changes.

Measured on the MI355X (profiles/storage_gates.txt; the same in both modes to the figures given): conv1 0.93 - 1.25 of the storage
chain, conv2 0.75 - 1.19, the transitions 0.97 - 1.26, stem / head conv0 forward and the head's data and weight gradient 1.00, the
E_UNPOOL data gradients 0.98 - 1.07, the W_POOL weight gradients 1.07 - 1.33 of the blocked reduction (gate 3.0); pool0 and norm5_bwd
at 0.99 - 1.00 of their bound (half a storage ulp, reached), feat at 0.26 - 0.50, norm5's affine gradients at 0.001.

Two geometries, one forward per (mode, geometry), every buffer read after it:
  S = 672, 3 streams (seed 8, size 236): padded planes 28288 / 7104 / 1792 / 448, ragged 3x3 tiles, bounds-checked 16 x 16 tiles;
  S = 640, 6 streams (seed 0, rotations 0 3 7 10 13): exact tiles, and CfgP64x64 for conv1 at 80^2, where mode 0 goes wave-specialised.
VARIANTS16 is the choice of the walk in modes 1 / 2 (forward.hip: the wave-specialised conv1 and the split scales are `e->prec == 0`
only), asserted from eng.H / eng.HWp; the rules (tests/gate_harness.py) are checked on the CPU in test_cpu_storage_ref.

Forward: dense layers (1,1) (1,6) (2,1) (2,12) (3,24) (4,1) (4,16) on the first and the masked stream - conv1 from x<b>[:, :cin] into
bt<b>_<l>, conv2 from the bottleneck into x<b>[:, cin:cin+32]; stem conv0 in the heightmap form (operands rounded to the mode's forward
operand type - FwdConvP's kOp = fwd_op_plain(PREC) - into the fp32 stem plane); pool0 into the 16-bit x1; the three transitions;
feat_kernel from the 16-bit x4 into fp32; the head's norm0 + ReLU + conv0 (fp32 in and out, 16-bit operands); x<b>'s padding rows finite.
Backward of the stages, the dq of the stage gates (gate_harness.SCENES), one debug_stop per gate: at 350 the head conv0 data and weight gradients (bf16
operands, fp32 buffers), norm5_bwd_kernel into the bf16 g4 on every stream, norm5's affine gradients; at 250 / 150 / 50 the E_UNPOOL
data gradient into g<t> and the W_POOL weight gradient of transitions 3 / 2 / 1.

Backward of the DENSE LAYERS (58 of the net's 64 layers; in modes 1 / 2 none of mode 0's hot kernels run: no split operands, no
unit-form D2, no wave-specialised 1x1 weight gradient, no gs_on_side).  smg_debug_read now answers in every mode: "gsnap", "dy2" (the
stop copies the ring slot between the 3x3 data gradient and the norm2 backward that overwrites it in place), "gs_<b>_<l>" / "d2_<b>_<l>"
and - new - "fs_x<b>" / "bs_x<b>", the forward's and the backward's fp64 sums of a block buffer.  With fs_bt and fs_x every ReLU mask and every xhat of the reference
comes from the statistics the kernels used (storage_ref.engine_stats: the keep-mask's margin is the table's fp32 rounding), the sums
themselves are gated against the stored planes (test_block_buffer_sums_are_taken_before_the_store), and no stream is over the 1 % cap
(DGRAD16_OVER_THE_CAP is empty; the largest borderline share met is 0.0063 %).  VARIANTS16_BWD is the walk's choice with `split16`
false, asserted from eng.H / eng.HWp.  Five stops per (mode, geometry), BWD_LAYERS16, chosen by rule
(test_backward_layers_follow_the_rules): S = 640 x 6 streams - GS materialised (bn_bwd_apply_kernel<PREC> at C = 32), exact tiles;
S = 672 x 3 streams - the BN backward applied on load in both 3x3 kernels, bounds-checked 16 x 16 and ragged 8 x 8 tiles, block 4's conv1
weight gradient on fp32 atomics.  Per stop (test_backward_layer): the storage type of every slot; the 3x3 data gradient
(conv3x3_halo_dgrad_kernel<16 | 8, PREC, edge>) within 2.0 x the storage chain, exact zeros where the ReLU is clearly off; the in-place
norm2 backward (bn_bwd_apply_kernel<PREC> at C = 128) element by element within the counted roundings + the slack of sums taken in front
of dy2's store + half a bf16 ulp; norm2's dgamma / dbeta within the counted roundings of sum |term| + that slack; both weight gradients
(conv3x3_halo_wgrad_kernel, BwdWeightP<.., W_ONE>) within _WGRAD_GATE x the blocked reduction over the bf16 operands; the 1x1 data
gradients in the form(s) the layer takes (BwdDataP<.., E_ACCUM> per layer, BwdDataGroupP with nseg = 4) within 2.0 x the storage chain,
|gsnap| in the magnitude, and the columns no segment covers bit-equal to gsnap.  The slots' padding rows [HW, HWp) are written by no
16-bit kernel (test_backward_layer cites the stores and every consumer's bound): on blocks 3 - 4 EVERY word there is non-zero (S = 640
block 4: 36864 = 6 x 48 x 128; S = 672: 10752 on block 3, 2688 on block 4) and every gate above holds regardless.
Measured on the MI355X (profiles/storage_gates_bwd.txt; both modes alike): 3x3 data gradient 1.00 - 1.01 of the chain on the sample,
0.89 - 1.01 on the whole plane; in-place norm2 backward at 0.89 - 0.99 of its bound (the half ulp, reached); norm2's dbeta at 0.02 - 0.14,
dgamma at 0.03 - 0.20 of theirs; conv2 weight gradient 1.00 - 1.25, conv1 weight gradient 1.00 of the blocked reduction (gate 3.0); 1x1 data
gradient 1.00 on the sample, 0.92 - 1.10 on the whole plane; the materialised GS (bn_bwd_apply_kernel<PREC> at C = 32, every S = 640 stop, the engine's own s1 / s2 from bs_x) at 1.00 of its
bound (the half ulp, reached), on (4,16) also at 0.86 - 0.88 with the sums of gsnap; fs_x within 0.96
of its slack (median channel 0.017 and up).  No gate was missed and no kernel changed.  The transition gate takes its masks from fs_x as
well: its exception table DGRAD_OVER_THE_CAP is empty now, and the stream it left out (bf16, S = 640, transition 1, stream 0) sits at
1.00 of the chain with 0.0000 % of its signs borderline.

Out of scope: the stem / pool0 backward of
the 16-bit modes; input sizes that are no multiple of 32; the Adam and loss kernels.

Raw output of a run on the MI355X: profiles/storage_gates.txt, profiles/storage_gates_bwd.txt (the dense layers' backward)."""
import numpy as np
import pytest
import torch

import dense_ref as dr
import stage_ref as sr
import storage_ref as st
from gate_harness import (BWD_LAYERS16, CT, HEAD, SCENES, TRUNK, GateCtx, bounded, conv1_fwd_cfg, forward_chains, gate, gpu, halo_tile,  # noqa: F401  (gpu: the fixture)
                          transition_cfg, wgrad_gate)
from helpers import MEAN, STD, product_net

pytestmark = pytest.mark.gpu

CASES = {"S640": SCENES["S640x6"], "S672": SCENES["S672x3"]}          # the stage gates' two geometries, and their dq
# per block: (conv1 forward, 3x3 tile, bounds-checked 16 x 16); then the three transitions, the stem, the head conv0
VARIANTS16 = {"S640": ([("P128x128", 16, False), ("P64x64", 8, False), ("P32x64", 8, False), ("P32x64", 8, False)], ["P128x128", "P64x128", "P64x128"], "P128x64", "P64x64"),
              "S672": ([("P128x128", 16, True), ("P64x64", 8, False), ("P32x64", 8, False), ("P32x64", 8, False)], ["P64x128", "P128x128", "P64x128"], "P128x64", "P64x64")}
FWD_LAYERS = [(1, 1), (1, 6), (2, 1), (2, 12), (3, 24), (4, 1), (4, 16)]
# Streams whose E_UNPOOL data-gradient gate is LEFT OUT because the keep-mask's condition - at most 1 % of the plane's ReLU signs
# undetermined - does not hold there: {(mode, geometry, transition): streams}.  The test asserts this set exactly.  EMPTY since the mask
# comes from the engine's own forward sums (debug_read "fs_x<t>": storage_ref.engine_stats).  Before, with the stored plane's statistics
# and the slack of sums taken before the store, bf16 / S = 640 / transition 1 / stream 0 (rotation 0, the unrotated scene) had 1.33 % of
# x1 borderline - the scene's flat background rounds one way on most of the plane, the engine's mean sits up to half a bf16 ulp off the
# stored plane's, and in a few channels the whole background's pre-activation lay inside that uncertainty - and was left out.
DGRAD_OVER_THE_CAP = {}
_STATE = {}


class _ModeCtx(GateCtx):
    """GateCtx of one (mode, geometry): the mode's storage and operand types, the two streams of the dense-layer gates, the buffers of
    the one forward (_fwd)"""

    def __init__(self, net, sd, case, gpu, mode):
        super().__init__(net, sd, CASES[case], gpu, mode)
        self.case, self.dense_streams, self.B = case, [0, self.NS - 1], None
        self.act, self.grd, self.fwd, self.bwd = (st.MODES[mode][k] for k in ("act", "grd", "fwd", "bwd"))


@pytest.fixture(scope="module", params=[(m, c) for m in sorted(st.MODES) for c in sorted(CASES)], ids=lambda p: "%s-%s" % p)
def mc(gpu, request):
    """one (mode, geometry) at a time (pytest groups the tests by this module-scoped parameter): the net in that precision mode, the
    scene, the stream / pair layout; the default mode is restored whatever happens"""
    mode, case = request.param
    if "net" not in _STATE:
        _STATE["net"] = product_net(0)
        _STATE["sd"] = {k: v.detach().cpu().numpy() for k, v in _STATE["net"].state_dict().items()}
    x = _ModeCtx(_STATE["net"], _STATE["sd"], case, gpu, mode)
    try:
        # a default-mode forward first: the engine's buffers then hold fp32 planes when the mode changes, whatever ran before this file -
        # what the padding-row assertion of _fwd needs to mean something (see there)
        x.net.set_precision("fp32")
        x.net.run(0, x.rots, 16, heightmaps=x.hm, mean=MEAN, std=STD)
        torch.cuda.synchronize()
        x.net.set_precision(mode)
        yield x
    finally:
        x.net.set_precision("fp32")
        x.B = None


def _fwd(x):
    """ONE forward per (mode, geometry); every buffer the forward gates compare is read after that one run"""
    if x.B is None:
        x.forward()
        B = {"img": x.eng.debug_read("img").reshape(-1, x.HWp[0], 4)[:x.NS, :x.S * x.S, 0].copy(),
             "stem": x.rd("stem", x.NS, 1, 64), "feat": x.rd("feat", x.NP, 5, 2048), "h1": x.rd("h1", x.NP, 5, 64)}
        for b in range(4):
            full = x.rd("x%d" % (b + 1), x.NS, 2 + b, CT[b], pad=True)
            HW = x.H[2 + b] ** 2
            padrows = full[:, HW:]
            # No kernel of the forward stores rows >= HW of x<b> (test_gpu_dense_gates.py) and the 1x1 kernels read them as they lie - the
            # weight gradient of the 16-bit modes without a clamp, against a zero gradient: an inf there is a NaN column of dW.  FOUND BY
            # THIS ASSERTION, run behind a mode-0 forward on the same engine: x4's 48 padding rows held the mode-0 plane's fp32 words read
            # as bf16 pairs, NaN among them.  smg_engine_set_precision now zeroes the mode-typed buffers when the mode changes.
            print("%s %s x%d: %d padding rows per stream, largest |value| %.3e" % (x.mode, x.case, b + 1, padrows.shape[1], np.abs(padrows).max() if padrows.size else 0.0))
            assert np.isfinite(padrows).all()
            B["x%d" % (b + 1)] = full[:, :HW]
            B["fsx%d" % (b + 1)] = x.eng.debug_read("fs_x%d" % (b + 1)).view(np.float64).reshape(2, -1, CT[b])[:, :x.NS].copy()
            assert np.array_equal(st.rnd(B["x%d" % (b + 1)], x.act), B["x%d" % (b + 1)])          # every stored value is a value of the storage type
        for b, l in FWD_LAYERS:
            B["bt%d_%d" % (b, l)] = x.rd("bt%d_%d" % (b, l), x.NS, 1 + b, 128)[x.dense_streams].copy()
            fs = x.eng.debug_read("fs_bt%d_%d" % (b, l)).view(np.float64).reshape(2, -1, 128)
            B["fs%d_%d" % (b, l)] = fs[:, x.dense_streams].copy()
        x.B = B
    return x.B


def _xstats(x, B, block, n):
    """statistics of x<block> of stream n as the engine holds them, as far as they can be known (storage_ref.plane_stats): pool0's 64
    channels of x1 from the fp32 stem plane, every other channel from the stored plane with its slack"""
    X = B["x%d" % block][n]
    if block == 1:
        return st.x1_stats(X, B["stem"][n], x.H[1], x.tp("norm0.weight"), x.tp("norm0.bias"), x.act)
    return st.plane_stats(X, x.act)


def _rms(got, ref, mag, keep):
    """dense_ref.rms over the kept elements only (the others may carry a sign the reference does not: no quotient is formed there)"""
    return dr.rms(np.asarray(got)[keep], np.asarray(ref)[keep], np.asarray(mag)[keep])


# ---- the variant table ---------------------------------------------------------------------------------------------------------------------
def test_geometry_selects_the_variants_of_the_16_bit_table(mc):
    x = mc
    _fwd(x)
    chains = forward_chains(x.NS, x.H[2])
    blocks = []
    for b in range(4):
        H, HWp = x.H[2 + b], x.HWp[2 + b]
        c1, ts = {conv1_fwd_cfg(HWp, ns, False) for ns in chains}, {halo_tile(H, ns) for ns in chains}
        assert len(c1) == 1 and len(ts) == 1, (x.case, b, c1, ts)
        t = ts.pop()
        blocks.append((c1.pop(), t, t == 16 and H % 16 != 0))
    got = (blocks, [transition_cfg(x.HWp[3 + b]) for b in range(3)], "P128x64" if x.HWp[1] % 128 == 0 else "P64x64", "P128x64" if x.HWp[5] % 128 == 0 else "P64x64")
    print("%s %s: %d streams, forward chains %s: %s" % (x.mode, x.case, x.NS, chains, got))
    assert got == VARIANTS16[x.case]


# ---- forward: dense layers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,layer", FWD_LAYERS)
def test_forward_layer(mc, block, layer):
    """norm1 + ReLU + conv1 and norm2 + ReLU + conv2 of one dense layer on the first and the masked stream, whole planes.
    Measured on the MI355X: conv1 0.93 - 1.25 of the storage chain (whole plane; the masked stream of S = 640 highest), conv2 0.75 - 1.19;
    gate 2.0.  Block 1 reads pool0's channels with the statistics of storage_ref.x1_stats (module docstring)."""
    x = mc
    B = _fwd(x)
    H, cin = x.H[1 + block], dr.cin_of(block, layer)
    g1, b1, w1 = x.lp(block, layer, "norm1.weight"), x.lp(block, layer, "norm1.bias"), x.lp(block, layer, "conv1.weight").reshape(128, cin)
    g2, b2, w2 = x.lp(block, layer, "norm2.weight"), x.lp(block, layer, "norm2.bias"), x.lp(block, layer, "conv2.weight")
    pix = dr.sample(H * H)
    for k, n in enumerate(x.dense_streams):
        X, BT = B["x%d" % block][n], B["bt%d_%d" % (block, layer)][k]
        assert np.array_equal(st.rnd(BT, x.act), BT)
        S = _xstats(x, B, block, n).cols(slice(0, cin))
        a64 = st.act64_s(X[:, :cin], g1, b1, S)
        ref, mag = a64 @ w1.astype(np.float64).T, a64 @ np.abs(w1.astype(np.float64)).T + 1e-300
        chain = st.storage_chain(st.act32_s(X[:, :cin], g1, b1, S)[pix], w1, x.fwd, x.act)
        gate("%s %s conv1 (%d,%d) K %d stream %d" % (x.mode, x.case, block, layer, cin, n), dr.rms(BT[pix], ref[pix], mag[pix]), dr.rms(chain, ref[pix], mag[pix]), 2.0,
             e_whole=dr.rms(BT, ref, mag), n=chain.size, yard="storage chain")
        ref, mag = dr.conv2_fwd(BT, H, H, g2, b2, w2)
        chain = st.conv2_chain(BT, H, H, g2, b2, w2, pix, x.fwd, x.act)
        got = X[:, cin:cin + 32]
        gate("%s %s conv2 (%d,%d) stream %d" % (x.mode, x.case, block, layer, n), dr.rms(got[pix], ref[pix], mag[pix]), dr.rms(chain, ref[pix], mag[pix]), 2.0,
             e_whole=dr.rms(got, ref, mag), n=chain.size, yard="storage chain")


@pytest.mark.parametrize("block,layer", FWD_LAYERS)
def test_bottleneck_sums_are_taken_before_the_store(mc, block, layer):
    """fs_bt<b>_<l>: the engine's own fp64 sums of a bottleneck against the fp64 sums of the STORED plane.  FwdConvP::epilogue sums the
    fp32 accumulators and stores afterwards, so the two differ by what rounding did - within storage_ref.store_stat_slack (+ the fp32
    strip sums of whole tiles, stage_ref.strip_sum_slack), and by far more than sums taken after the store could: those would agree
    to the strip sums' few 2^-24, here the median channel sits above 1e-3 of the bound."""
    x = mc
    B = _fwd(x)
    HW = x.H[1 + block] ** 2
    for k, n in enumerate(x.dense_streams):
        BT, fs = B["bt%d_%d" % (block, layer)][k], B["fs%d_%d" % (block, layer)][:, k]
        mean_e = fs[0] / HW
        inv_e = 1.0 / np.sqrt(fs[1] / HW - mean_e ** 2 + sr.EPS)
        mean, inv = sr.bn_stats(BT)
        M, R = st.store_stat_slack(BT, x.act)
        Ms, Rs = sr.strip_sum_slack(BT, (HW // 32) * 32)
        rm, ri = np.abs(mean_e - mean) / (M + Ms * sr.U + 1e-300), np.abs(inv_e / inv - 1) / (R + Rs * sr.U + 1e-300)
        print("%s %s bt%d_%d stream %d: engine mean off the stored plane's by at most %.3f of the bound (median %.4f), invstd %.3f (median %.4f)"
              % (x.mode, x.case, block, layer, n, rm.max(), np.median(rm), ri.max(), np.median(ri)))
        assert rm.max() <= 1.0 and ri.max() <= 1.0
        assert np.median(rm) > 1e-3


def test_block_buffer_sums_are_taken_before_the_store(mc):
    """fs_x<b>: the engine's fp64 sums of a block buffer against the fp64 sums of the STORED plane, every stream and block - as
    test_bottleneck_sums_are_taken_before_the_store holds fs_bt: within storage_ref.store_stat_slack plus, on the transition's channels
    [0, C0) of x2..x4, the fp32 strip sums of its whole tiles (stage_ref.strip_sum_slack; pool0 and the 3x3 kernels sum per element in
    fp64).  The backward gates take every ReLU mask from these sums: a reference built on them is not built on an unchecked number."""
    x = mc
    B = _fwd(x)
    for b in range(1, 5):
        HW = x.H[1 + b] ** 2
        BM = 128 if x.HWp[1 + b] % 128 == 0 else 64          # transition_cfg: the tile rows of the transition that produced [0, C0)
        C0 = 0 if b == 1 else CT[b - 2] // 2                     # x1: pool0 (64) and the 3x3 kernels only
        for n in range(x.NS):
            X, S = B["x%d" % b][n], st.engine_stats(B["fsx%d" % b][:, n], HW)
            mean, inv = sr.bn_stats(X)
            M, R = st.store_stat_slack(X, x.act)
            Ms, Rs = np.zeros(len(M)), np.zeros(len(M))
            if C0:
                Ms[:C0], Rs[:C0] = sr.strip_sum_slack(X[:, :C0], (HW // BM) * BM)
            rm, ri = np.abs(S.mean - mean) / (M + Ms * sr.U + 1e-300), np.abs(S.inv / inv - 1) / (R + Rs * sr.U + 1e-300)
            print("%s %s x%d stream %d: engine mean off the stored plane's by at most %.3f of the bound (median %.4f), invstd %.3f (median %.4f)"
                  % (x.mode, x.case, b, n, rm.max(), np.median(rm), ri.max(), np.median(ri)))
            assert rm.max() <= 1.0 and ri.max() <= 1.0
            assert np.median(rm) > 1e-3


# ---- forward: the stages around the dense layers ---------------------------------------------------------------------------------------------
def test_stem_conv0_heightmap_form(mc):
    """F_STEM1 in modes 1 / 2: the fp32 image and the PK_STEM1 weights (the fp64 sum of the three channel weights, rounded to fp32) each
    rounded once to the mode's forward operand type, 49 taps accumulated in fp32, stored to the fp32 stem plane"""
    x = mc
    B = _fwd(x)
    S, Hs = x.S, x.H[1]
    w = x.tp("conv0.weight")
    w1 = w.astype(np.float64).sum(1, keepdims=True)
    rows = np.concatenate([np.arange(24), np.arange(Hs - 24, Hs)])
    pix = (rows[:, None] * Hs + np.arange(Hs)[None, :]).ravel()
    for n in range(x.NS):
        img = B["img"][n].reshape(S, S, 1)
        ref, _ = sr.stem_conv(img, w1, rows)
        mag = np.abs(sr.stem_cols(img.astype(np.float64), rows)) @ sr.stem_wmat(np.abs(w.astype(np.float64)).sum(1, keepdims=True)).T + 1e-300
        chain = st.storage_chain(sr.stem_cols(img, rows), sr.stem_wmat(w1.astype(np.float32)), x.fwd)
        gate("%s %s stem conv0, heightmap form, stream %d" % (x.mode, x.case, n), dr.rms(B["stem"][n][pix], ref, mag), dr.rms(chain, ref, mag), 2.0, n=ref.size, yard="storage chain")


def test_pool0_into_16_bit_x1(mc):
    """pool0_kernel: the fp32 maximum (K_BN roundings of bn_mag + the stem statistics' strip sums, as in mode 0) rounded once by stq<XT>"""
    x = mc
    B = _fwd(x)
    Hs = x.H[1]
    g, b = x.tp("norm0.weight"), x.tp("norm0.bias")
    for n in range(x.NS):
        stem = B["stem"][n]
        ref, mag = sr.pool0(stem, Hs, Hs, g, b)
        slack = sr.maxpool3s2(sr.bn_stat_slack(stem, g, (Hs * Hs // 128) * 128), Hs, Hs) * sr.U
        bounded("%s %s pool0 stream %d" % (x.mode, x.case, n), B["x1"][n][:, :64], ref, st.stored_bound(ref, sr.K_BN, mag, x.act, slack))


@pytest.mark.parametrize("t", [1, 2, 3])
def test_transition_forward(mc, t):
    """F_POOL: the 2 x 2 average of relu(bn(x<t>)) formed in fp32, rounded once to the forward operand type; PK_T1 weights rounded to
    it; the result rounded to the activation storage of x<t+1>[:, :C/2]"""
    x = mc
    B = _fwd(x)
    H, Cp = x.H[1 + t], CT[t - 1]
    C0 = Cp // 2
    g, b = x.tp("transition%d.norm.weight" % t), x.tp("transition%d.norm.bias" % t)
    w = x.tp("transition%d.conv.weight" % t).reshape(C0, Cp)
    pix = dr.sample((H // 2) ** 2)
    cols = np.arange(0, C0, max(1, C0 // 128))
    for n in range(x.NS):
        X = B["x%d" % t][n]
        got = B["x%d" % (t + 1)][n][:, :C0]
        S = _xstats(x, B, t, n)
        a64 = st.act64_s(X, g, b, S)
        ref = sr.avgpool2(a64 @ w.astype(np.float64).T, H, H)                          # the reference's order: conv, then pool
        mag = sr.avgpool2(a64, H, H) @ np.abs(w.astype(np.float64)).T + 1e-300
        chain = st.storage_chain(sr.avgpool2(st.act32_s(X, g, b, S), H, H)[pix], np.ascontiguousarray(w[cols]), x.fwd, x.act)
        sel = np.ix_(pix, cols)
        gate("%s %s transition %d stream %d" % (x.mode, x.case, t, n), dr.rms(got[sel], ref[sel], mag[sel]), dr.rms(chain, ref[sel], mag[sel]), 2.0,
             e_whole=dr.rms(got, ref, mag), n=chain.size, yard="storage chain")


def test_norm5_concat_from_16_bit_x4(mc):
    """feat_kernel reads the 16-bit x4 and writes fp32: K_BN roundings of bn_mag, the strip sums of transition 3's whole tiles (mode 0's
    term), and what the store of x4 did to its statistics (storage_ref.bn_store_slack: conv2's and the transition's epilogues summed
    them before the store)"""
    x = mc
    B = _fwd(x)
    g5 = x.tp("norm5.weight")
    ref, mag = sr.feat(list(B["x4"]), g5, x.tp("norm5.bias"), x.pa, x.pb)
    HW = x.H[5] ** 2
    sl = [np.concatenate([sr.bn_stat_slack(v[:, :512], g5[:512], (HW // 64) * 64), np.zeros((HW, 512))], axis=1) * sr.U + st.bn_store_slack(v, g5, x.act) for v in B["x4"]]
    for j in range(x.NP):
        for half, name, s in ((slice(0, 1024), "rotation", x.pa[j]), (slice(1024, 2048), "masked", x.pb[j])):
            bound = sr.K_BN * sr.U * mag[j][:, half] + sl[s]
            err = np.abs(B["feat"][j][:, half].astype(np.float64) - ref[j][:, half])
            print("%s %s feat pair %d, %s half: |err| at most %.3f of the bound; without the storage term %.1f of the fp32 bound"
                  % (x.mode, x.case, j, name, (err / (bound + 1e-300)).max(), (err / (bound - st.bn_store_slack(B["x4"][s], g5, x.act) + 1e-300)).max()))
            assert (err <= bound).all()


def test_head_conv0_forward(mc):
    """head norm0 + ReLU + conv0 (2048 -> 64), fp32 in and out (FwdConvP<.., F32IO = true>), operands rounded to the mode's forward
    operand type; statistics PER PAIR, of the stored fp32 features (feat_kernel sums what it stores)"""
    x = mc
    B = _fwd(x)
    g, b, w = x.hp("norm0.weight"), x.hp("norm0.bias"), x.hp("conv0.weight").reshape(64, 2048)
    for j in range(x.NP):
        ref, a64 = sr.head_conv0(B["feat"][j], g, b, w)
        mag = a64 @ np.abs(w.astype(np.float64)).T + 1e-300
        chain = st.storage_chain(sr.bn32(B["feat"][j], g, b), w, x.fwd)
        gate("%s %s head conv0 pair %d" % (x.mode, x.case, j), dr.rms(B["h1"][j], ref, mag), dr.rms(chain, ref, mag), 2.0, n=ref.size, yard="storage chain")


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
def _wgrad_gate(what, got, a64, w64, a32, w32, op):
    """got [M][N] = sum_k a[k][m] * w[k][n] over ALL streams x pixels; the yardstick: the blocked fp32 reduction over both operands
    rounded once to `op`"""
    wgrad_gate(what, got, a64, w64, lambda blk: st.storage_blocked(a32, w32, op, op, blk), (64, 512), yard="blocked reduction over the %s operands" % op)


def test_head_conv0_and_norm5_backward(mc):
    """Stop 350.  The head's buffers are fp32 in every mode (BwdDataP / BwdWeightP with F32IO = true); its products take bf16 operands
    in both 16-bit modes (bwd_op_plain): the BN-corrected dh1 and the PK_D1-class weights for the data gradient, the corrected dh1 and
    relu(bn0(feat)) for the weight gradient.  norm5_bwd_kernel forms g4 in fp32 from the fp32 df / feat exactly as in mode 0 and rounds
    it once to bf16 (stq<GT>); dgamma5 multiplies by xhat5 of the 16-bit x4, whose statistics were summed before the store."""
    x = mc
    grads = x.backward_to(350)
    h1, dh1 = x.rd("h1", x.NP, 5, 64), x.rd("dh1", x.NP, 5, 64)
    Fm, DF = x.rd("feat", x.NP, 5, 2048), x.rd("df", x.NP, 5, 2048)
    x4, g4 = x.rd("x4", x.NS, 5, 1024), x.rd("g4", x.NS, 5, 1024)
    assert np.array_equal(st.rnd(g4, x.grd), g4)
    g0, b0, g1 = x.hp("norm0.weight"), x.hp("norm0.bias"), x.hp("norm1.weight")
    w0 = x.hp("conv0.weight").reshape(64, 2048)
    A64s, A32s, P64s, P32s = [], [], [], []
    for j in range(x.NP):
        ref, A64, on, _ = sr.head_conv0_bwd(h1[j], dh1[j], Fm[j], g1, g0, b0, w0)
        A32 = sr.bn_bwd32(dh1[j], h1[j], g1)
        mag = on * (sr.bn_bwd_mag(dh1[j], h1[j], g1) @ np.abs(w0.astype(np.float64))) + 1e-300
        chain = (on * st.storage_chain(A32, np.ascontiguousarray(w0.T), x.bwd)).astype(np.float32)
        keep = sr.bn_keep(Fm[j], g0, b0)          # (feat is fp32 and its statistics are those of the stored values: mode 0's rule)
        assert 1 - keep.mean() <= 0.01, ("borderline ReLU signs", 1 - keep.mean())
        gate("%s %s head conv0 dgrad pair %d" % (x.mode, x.case, j), _rms(DF[j], ref, mag, keep), _rms(chain, ref, mag, keep), 2.0, n=int(keep.sum()), yard="storage chain")
        A64s.append(A64); A32s.append(A32)
        P64s.append(np.maximum(sr.bn_pre(Fm[j], g0, b0), 0.0)[:, ::8]); P32s.append(sr.bn32(Fm[j], g0, b0)[:, ::8])
    _wgrad_gate("%s %s head conv0 wgrad" % (x.mode, x.case), grads[HEAD + "conv0.weight"].reshape(64, 2048)[::8, ::8],
                np.concatenate(A64s)[:, ::8], np.concatenate(P64s), np.concatenate(A32s)[:, ::8], np.concatenate(P32s), x.bwd)

    g5 = x.tp("norm5.weight")
    G4, dy5, mag, db, dg, dbm, dgm = sr.norm5_bwd(list(x4), Fm, DF, g0, g5, x.pa, x.pb)
    for s in range(x.NS):
        users = x.NP if s == x.NS - 1 else 1
        bounded("%s %s norm5 backward stream %d (%d user%s)" % (x.mode, x.case, s, users, "s" if users > 1 else ""),
                g4[s], G4[s], st.stored_bound(G4[s], sr.k_g4(users), np.abs(g5) * mag[s], x.grd))
    k = sr.k_sums5(x.H[5] ** 2, x.NS - 1, True)
    bounded("%s %s norm5.bias gradient" % (x.mode, x.case), grads[TRUNK + "norm5.bias"], db, k * sr.U * dbm)
    # xhat5 = (x - mean5) * inv5 with the engine's mean5 / inv5, summed before x4's store: storage_ref.xhat_sum_slack, per stream
    slack = sum(st.xhat_sum_slack(dy5[s], x4[s], st.plane_stats(x4[s], x.act)) for s in range(x.NS))
    print("%s %s norm5.weight gradient: max |err| at %.2f of the fp32 bound alone (%d roundings of sum |term|)"
          % (x.mode, x.case, float((np.abs(grads[TRUNK + "norm5.weight"] - dg) / (k * sr.U * dgm)).max()), k))
    bounded("%s %s norm5.weight gradient" % (x.mode, x.case), grads[TRUNK + "norm5.weight"], dg, k * sr.U * dgm + slack)


@pytest.mark.parametrize("t", [3, 2, 1])
def test_transition_backward(mc, t):
    """Stop (t - 1) * 100 + 50.  E_UNPOOL: the corrected gradient dX of x<t+1>[:, :C0] (affine2 of the stored bf16 G' and the stored
    activation, q1 / k from the engine-style tile sums) rounded once to bf16, the data-gradient pack of the weights rounded to bf16,
    fp32 accumulation, 1/4 and gamma_t and the ReLU mask in fp32, one rounding to the bf16 g<t> (stq<GT>).  W_POOL: dX and the 2 x 2
    average of relu(bn_t(x<t>)) both rounded to bf16 (bwd_op_plain), reduced in fp32.  The ReLU mask and the pooled activation take
    the ENGINE's forward sums of x<t> (fs_x<t>, held by test_block_buffer_sums_are_taken_before_the_store): no stream is left out."""
    x = mc
    grads = x.backward_to((t - 1) * 100 + 50)
    H, Cp = x.H[1 + t], CT[t - 1]
    C0, Hn = Cp // 2, H // 2
    X, Gt = x.rd("x%d" % t, x.NS, 1 + t, Cp), x.rd("g%d" % t, x.NS, 1 + t, Cp)
    Xn, Gn = x.rd("x%d" % (t + 1), x.NS, 2 + t, CT[t])[:, :, :C0], x.rd("g%d" % (t + 1), x.NS, 2 + t, CT[t])[:, :, :C0]
    assert np.array_equal(st.rnd(Gt, x.grd), Gt)
    g, b = x.tp("transition%d.norm.weight" % t), x.tp("transition%d.norm.bias" % t)
    w = x.tp("transition%d.conv.weight" % t).reshape(C0, Cp)
    q = dr.sample(Hn * Hn)
    qy, qx = q // Hn, q % Hn
    pix = np.stack([(2 * qy + dy) * H + 2 * qx + dx for dy in (0, 1) for dx in (0, 1)], axis=1).ravel()
    cols = np.arange(0, Cp, max(1, Cp // 128))
    fsx = x.eng.debug_read("fs_x%d" % t).view(np.float64).reshape(2, -1, Cp)          # (the backward sums into another arena: intact at the stop)
    dX64s, dX32s, stats, over = [], [], [], []
    for n in range(x.NS):
        S = st.engine_stats(fsx[:, n], H * H)
        stats.append(S)
        dX = sr.bn_bwd(Gn[n], Xn[n])
        on = st.bn_pre_s(X[n], g, b, S) > 0
        ref = g.astype(np.float64) * on * 0.25 * sr.unpool2(dX @ w.astype(np.float64), H, H)
        dX32 = sr.bn_bwd32(Gn[n], Xn[n], tile_sums=True)
        dX64s.append(dX); dX32s.append(dX32)
        mag = np.abs(g) * on * 0.25 * sr.unpool2(sr.bn_bwd_mag(Gn[n], Xn[n]) @ np.abs(w.astype(np.float64)), H, H) + 1e-300
        keep = st.keep_s(X[n], g, b, S)
        share = 1 - keep.mean()
        print("%s %s transition %d stream %d: %.4f %% of the ReLU signs borderline at the engine's statistics" % (x.mode, x.case, t, n, 100 * share))
        if share > 0.01:          # the cap is a condition of the gate: no data-gradient gate on this stream (see DGRAD_OVER_THE_CAP)
            over.append(n)
            continue
        up = (np.float32(0.25) * st.storage_chain(dX32[q], np.ascontiguousarray(w.T[cols]), x.bwd)).astype(np.float32)
        sel = np.ix_(pix, cols)
        chain = st.rnd((g[cols] * (on[sel] * np.repeat(up, 4, axis=0)).astype(np.float32)).astype(np.float32), x.grd)
        gate("%s %s transition %d dgrad stream %d" % (x.mode, x.case, t, n), _rms(Gt[n][sel], ref[sel], mag[sel], keep[sel]),
             _rms(chain, ref[sel], mag[sel], keep[sel]), 2.0, e_whole=_rms(Gt[n], ref, mag, keep), n=int(keep[sel].sum()), yard="storage chain")
    assert tuple(over) == DGRAD_OVER_THE_CAP.get((x.mode, x.case, t), ()), ("borderline ReLU signs over the 1 % cap on streams", over)
    c8 = slice(0, Cp, 8)
    P64 = np.concatenate([sr.avgpool2(st.act64_s(X[n][:, c8], g[c8], b[c8], stats[n].cols(c8)), H, H) for n in range(x.NS)])
    P32 = np.concatenate([sr.avgpool2(st.act32_s(X[n][:, c8], g[c8], b[c8], stats[n].cols(c8)), H, H) for n in range(x.NS)])
    _wgrad_gate("%s %s transition %d wgrad" % (x.mode, x.case, t), grads[TRUNK + "transition%d.conv.weight" % t].reshape(C0, Cp)[::8, ::8],
                np.concatenate(dX64s)[:, ::8], P64, np.concatenate(dX32s)[:, ::8], P32, x.bwd)


# ---- backward: the dense layers ------------------------------------------------------------------------------------------------------------------
# per block: (3x3 tile, bounds-checked 16 x 16, ragged tiles, GS form, per-layer 1x1 data gradient, grouped, conv1 weight gradient)
VARIANTS16_BWD = {"S640": [(16, False, False, "materialised", "P128x64", "G128x64x32", "partial tiles"), (8, False, False, "materialised", "P128x64", "G128x64x32", "partial tiles"),
                           (8, False, False, "materialised", "P64x64", "P64x64", "partial tiles"), (8, False, True, "materialised", "P64x64", "P64x64", "partial tiles")],
                  "S672": [(16, True, True, "on load", "P128x64", "G128x64x32", "partial tiles"), (8, False, True, "on load", "P64x64", "P64x64", "partial tiles"),
                           (8, False, True, "on load", "P128x64", "G128x64x32", "partial tiles"), (8, False, True, "on load", "P64x64", "P64x64", "atomics")]}
# the stops: gate_harness.BWD_LAYERS16 - at most five per (mode, geometry), chosen by rule (test_cpu_storage_ref.test_backward_layers_follow_the_rules)
# streams whose ReLU signs are undetermined on more than 1 % of a plane: {(mode, geometry, block, layer, "norm2" | "norm1"): streams},
# asserted exactly.  Empty: the masks come from the engine's own sums (fs_bt, fs_x), their margin is the table's fp32 rounding.
DGRAD16_OVER_THE_CAP = {}


def test_geometry_selects_the_backward_variants_of_the_16_bit_table(mc):
    """backward.hip with `split16` false: halo_tile (wgrad_plan.h, no precision in it) and the bounds-checked instantiation for 16 x 16
    tiles that hang over the edge; gs_materialised = NS > 4; CfgP128x64 / CfgP64x64 and GemmCfg<128, 64, 32> / CfgP64x64 by HWp % 128;
    w1_partial_tiles (wgrad_plan.h: NS > 4 or more than 1600 pixels) - never the wave-specialised kernel (w1_ws needs split16)"""
    x = mc
    _fwd(x)
    got = []
    for b in range(4):
        H, HWp = x.H[2 + b], x.HWp[2 + b]
        t = halo_tile(H, x.NS)
        big = HWp % 128 == 0
        got.append((t, t == 16 and H % 16 != 0, H % t != 0, "materialised" if x.NS > 4 else "on load", "P128x64" if big else "P64x64", "G128x64x32" if big else "P64x64",
                    "partial tiles" if x.NS > 4 or H * H > 1600 else "atomics"))
    print("%s %s: %d streams, backward: %s" % (x.mode, x.case, x.NS, got))
    assert got == VARIANTS16_BWD[x.case]


@pytest.mark.parametrize("k", range(5))
def test_backward_layer(mc, k):
    """Stop behind dense layer BWD_LAYERS16[geometry][k]: the ring slots (gs_ where GS was materialised, d2_), the raw 3x3 data gradient
    as it stood in the slot in front of the in-place norm2 backward (dy2), G' in front of (gsnap) and behind (g<b>) the layer's 1x1 data
    gradients, the layer's finished parameter gradients.  Every ReLU mask and every xhat comes from the ENGINE's forward sums (fs_bt,
    fs_x: storage_ref.engine_stats), which test_bottleneck_sums_are_taken_before_the_store and
    test_block_buffer_sums_are_taken_before_the_store hold; the yardsticks are storage_ref's (its comment block cites every rounding).

    Padding rows [HW, HWp) of the slots, read from the source before asserting: conv3x3_halo_dgrad_kernel stores in-plane pixels only
    (halo.cuh epilogue: `!kEdge || (py < a.pl.H && px < a.pl.W)`, and a tile's pixels address (y, x) < (H, W)), bn_bwd_apply_kernel<PREC>
    stores rows `r < a.pl.HW` only (elem.cuh) and no 16-bit kernel zeroes them (the unit-form apply of mode 0 does:
    bn_bwd_apply_split_kernel) - they hold an earlier layer's rows, possibly of another block's plane.  Every consumer bounds its reads:
    the 1x1 kernels stage A through bload4's size limit and mask `p < pa.HW` (gemm.cuh), the apply clamps its row (`r < a.pl.HW ? r :
    0`), the halo kernels address pixels.  What follows is asserted: the gates below hold whatever lies there; the words are counted.

    GS element by element (S = 640, where bn_bwd_apply_kernel<PREC> at C = 32 materialises it), at every stop: the fp64 BN backward of
    gsnap[:, cin:cin+32] and the x slice with the sums s1 / s2 the kernel read, handed out by debug_read("bs_x<b>") - the counted roundings
    plus half a bf16 ulp, no slack.  The sums cannot come from gsnap: BwdDataP::epilogue adds the UNROUNDED increments to s1 / s2 while G'
    is rounded at every read-modify-write store above this layer, and the running values those stores rounded are in no buffer (the test
    prints how far the engine's s1 is from the stored plane's sum).  Block 4's last layer, whose slice was stored exactly once
    (norm5_bwd_kernel), is ALSO held in that form: sums from gsnap, storage_ref.k_gs_top roundings, the one store's derived slack."""
    x = mc
    block, layer = BWD_LAYERS16[x.case][k]
    b, i = block - 1, layer - 1
    grads = x.backward_to(b * 100 + i)
    H, HWp, Ct, cin, Lb = x.H[1 + block], x.HWp[1 + block], CT[b], dr.cin_of(block, layer), dr.LAYERS[b]
    HW = H * H
    tag = "%s %s (%d,%d)" % (x.mode, x.case, block, layer)
    ts, mat = halo_tile(H, x.NS), x.NS > 4
    assert (ts, "materialised" if mat else "on load") == (VARIANTS16_BWD[x.case][b][0], VARIANTS16_BWD[x.case][b][3])
    X, BT = x.rd("x%d" % block, x.NS, 1 + block, Ct), x.rd("bt%d_%d" % (block, layer), x.NS, 1 + block, 128)
    fsx = x.eng.debug_read("fs_x%d" % block).view(np.float64).reshape(2, -1, Ct)
    fsb = x.eng.debug_read("fs_bt%d_%d" % (block, layer)).view(np.float64).reshape(2, -1, 128)
    Sx, Sb = [st.engine_stats(fsx[:, n], HW) for n in range(x.NS)], [st.engine_stats(fsb[:, n], HW) for n in range(x.NS)]
    DYp, D2p = x.rd("dy2", x.NS, 1 + block, 128, pad=True), x.rd("d2_%d_%d" % (block, layer), x.NS, 1 + block, 128, pad=True)
    DY, D2 = DYp[:, :HW], D2p[:, :HW]
    G0, G1 = x.rd("gsnap", x.NS, 1 + block, Ct), x.rd("g%d" % block, x.NS, 1 + block, Ct)
    GS = x.rd("gs_%d_%d" % (block, layer), x.NS, 1 + block, 32) if mat else None
    g1, b1, w1 = x.lp(block, layer, "norm1.weight"), x.lp(block, layer, "norm1.bias"), x.lp(block, layer, "conv1.weight").reshape(128, cin)
    g2, b2, w2 = x.lp(block, layer, "norm2.weight"), x.lp(block, layer, "norm2.bias"), x.lp(block, layer, "conv2.weight")
    pix, sl = dr.sample(HW), slice(cin, cin + 32)
    over = {}

    # ---- storage type: every value read through the debug names is a bf16 value; the slot's padding rows: counted, never asserted
    for name, v in (("dy2", DYp), ("d2_", D2p), ("gsnap", G0), ("g%d" % block, G1)) + ((("gs_", GS),) if mat else ()):
        assert np.array_equal(st.rnd(v, x.grd), v), name
    print("%s: %d padding rows per stream; non-zero words there: dy2 %d, d2_ %d" % (tag, HWp - HW, np.count_nonzero(DYp[:, HW:]), np.count_nonzero(D2p[:, HW:])))
    assert np.isfinite(G1).all() and np.isfinite(D2).all()

    # ---- the GS operand of the two 3x3 kernels, per stream: as stored, or the BN backward of the G' / x slices applied on load
    if mat:
        gs64, gs32 = [GS[n].astype(np.float64) for n in range(x.NS)], [GS[n] for n in range(x.NS)]
    else:
        gs64, gs32 = zip(*[st.gs_on_load16(G0[n][:, sl], X[n][:, sl], Sx[n].cols(sl)) for n in range(x.NS)])

    # ---- the materialised GS, element by element at EVERY stop: bn_bwd_apply_kernel<PREC> at C = 32 from the stored G' / x slices with the
    # sums s1 / s2 the kernel read (bs_x<b>: this layer's own data gradients add to columns [0, cin) only) - no slack
    if mat:
        bsx = x.eng.debug_read("bs_x%d" % block).view(np.float64).reshape(2, -1, Ct)
        for n in x.dense_streams:
            Sc = Sx[n].cols(sl)
            ref, mag = st.gs_from_sums(G0[n][:, sl], X[n][:, sl], Sc, bsx[:, n, sl], HW)
            stored = G0[n][:, sl].astype(np.float64)
            print("%s stream %d: the engine's s1 of the slice against the sum of the STORED G': off by at most %.3g of sum |G'| (the stores above this layer rounded after summing)"
                  % (tag, n, float((np.abs(bsx[0, n, sl] - stored.sum(0)) / (np.abs(stored).sum(0) + 1e-300)).max())))
            bounded("%s materialised GS stream %d (engine's sums, %d roundings + half a bf16 ulp)" % (tag, n, st.K_GS_APPLY), GS[n], ref, st.stored_bound(ref, st.K_GS_APPLY, mag, "bf16"))
    # ... and on block 4's last layer, whose slice of G' was stored exactly once, also in the form that takes the sums from gsnap
    if mat and (block, layer) == (4, dr.LAYERS[3]):
        for n in x.dense_streams:
            users = x.NP if n == x.NS - 1 else 1
            Sc = Sx[n].cols(sl)
            ref, mag = st.bn_bwd_s(G0[n][:, sl], X[n][:, sl], Sc), st.bn_bwd_sum_mag_s(G0[n][:, sl], X[n][:, sl], Sc)
            bounded("%s materialised GS stream %d (%d user%s, %d roundings + the store of G' + half a bf16 ulp)" % (tag, n, users, "s" if users > 1 else "", st.k_gs_top(users)),
                    GS[n], ref, st.stored_bound(ref, st.k_gs_top(users), mag, "bf16", st.sums_before_store_slack(G0[n][:, sl], X[n][:, sl], Sc)[0]))

    for n in x.dense_streams:
        # ---- conv2 data gradient: mask from fs_bt, exact zeros where the ReLU is clearly off
        keep = st.keep_s(BT[n], g2, b2, Sb[n])
        on = st.bn_pre_s(BT[n], g2, b2, Sb[n]) > 0
        share = 1 - keep.mean()
        print("%s stream %d: %.4f %% of norm2's ReLU signs borderline at the table's fp32 rounding" % (tag, n, 100 * share))
        if share > 0.01:
            over.setdefault((x.mode, x.case, block, layer, "norm2"), []).append(n)
        else:
            ref, mag = dr.conv2_dgrad(gs64[n], H, H, w2)
            ref = on * ref
            chain = st.conv2_dgrad_chain16(gs32[n], H, H, w2, on, pix)
            gate("%s conv2 dgrad stream %d (GS %s)" % (tag, n, "materialised" if mat else "on load"), _rms(DY[n][pix], ref[pix], mag[pix], keep[pix]),
                 _rms(chain, ref[pix], mag[pix], keep[pix]), 2.0, e_whole=_rms(DY[n], ref, mag, keep), n=int(keep[pix].sum()), yard="storage chain")
            assert not DY[n][keep & ~on].any(), "conv2 dgrad: non-zero where the ReLU is clearly off"

        # ---- norm2 backward in place, rows < HW: from the STORED dy2, counted roundings + the sums taken before dy2's store + half a bf16 ulp
        ref, bound = st.norm2_inplace(DY[n], BT[n], g2, Sb[n], ts)
        bounded("%s norm2 backward in place, stream %d (%d roundings)" % (tag, n, st.k_d2_apply(ts)), D2[n], ref, bound)

        # ---- conv1 data gradient in the form(s) the layer takes; masks from fs_x
        for layers, c0, c1 in dr.dgrad1_segments(Lb, i, dr.CIN0[b]):
            prm = [(x.lp(block, l + 1, "norm1.weight"), x.lp(block, l + 1, "norm1.bias"), x.lp(block, l + 1, "conv1.weight").reshape(128, -1)) for l in layers]
            d2s = [D2[n] if l == i else x.rd("d2_%d_%d" % (block, l + 1), x.NS, 1 + block, 128, [n])[0] for l in layers]
            ref, mag, _, keep = st.conv1_dgrad16(G0[n], X[n], Sx[n], prm, d2s, c0, c1, chain=False)
            share = 1 - keep.mean()
            form = "grouped" if len(layers) > 1 or c0 == 0 else "per-layer"
            print("%s stream %d, %s form: %.4f %% of the norm1 ReLU signs borderline" % (tag, n, form, 100 * share))
            if share > 0.01:
                over.setdefault((x.mode, x.case, block, layer, "norm1"), []).append(n)
                continue
            rs, ms, ch, ks = st.conv1_dgrad16(G0[n], X[n], Sx[n], prm, d2s, c0, c1, take=pix)
            gate("%s conv1 dgrad stream %d, %s form, layers %s, columns %d..%d" % (tag, n, form, [l + 1 for l in layers], c0, c1),
                 _rms(G1[n][pix, c0:c1], rs, ms, ks), _rms(ch, rs, ms, ks), 2.0, e_whole=_rms(G1[n][:, c0:c1], ref, mag, keep), n=int(ks.sum()), yard="storage chain")
    assert {k_: tuple(v) for k_, v in over.items()} == {k_: v for k_, v in DGRAD16_OVER_THE_CAP.items() if k_[:4] == (x.mode, x.case, block, layer)}, over

    # ---- columns no segment of this layer covers: bit-equal to the snapshot, every stream (what "gsnap" is for)
    cov = np.zeros(Ct, dtype=bool)
    for _, c0, c1 in dr.dgrad1_segments(Lb, i, dr.CIN0[b]):
        cov[c0:c1] = True
    assert np.array_equal(G1[:, :, ~cov], G0[:, :, ~cov]) and not np.array_equal(G1[:, :, cov], G0[:, :, cov])

    # ---- norm2's affine gradients over ALL streams: (float)s1[n] / (float)s2[n], one fp32 atomic per stream
    db = dg = dbm = dgm = h1 = h2 = 0.0
    for n in range(x.NS):
        d64 = DY[n].astype(np.float64)
        xh = (BT[n].astype(np.float64) - Sb[n].mean) * Sb[n].inv
        _, s1, s2 = st.sums_before_store_slack(DY[n], BT[n], Sb[n])
        db, dg, dbm, dgm, h1, h2 = db + d64.sum(0), dg + (d64 * xh).sum(0), dbm + np.abs(d64).sum(0), dgm + np.abs(d64 * xh).sum(0), h1 + s1, h2 + s2
    pre = TRUNK + "denseblock%d.denselayer%d." % (block, layer)
    bounded("%s norm2.bias gradient (%d roundings of sum |term| + the store)" % (tag, st.k_affine2(ts, x.NS, False)), grads[pre + "norm2.bias"], db, st.k_affine2(ts, x.NS, False) * sr.U * dbm + h1)
    bounded("%s norm2.weight gradient (%d roundings of sum |term| + the store)" % (tag, st.k_affine2(ts, x.NS, True)), grads[pre + "norm2.weight"], dg, st.k_affine2(ts, x.NS, True) * sr.U * dgm + h2)

    # ---- conv2 weight gradient on every 9th of the 9 * 128 im2col columns, conv1 weight gradient on 16 rows x <= 128 columns: ALL streams x pixels
    cols = np.arange(0, 9 * 128, 9)
    _, _, A64, A32 = st.conv2_wgrad_ops16(gs32, BT, H, H, g2, b2, Sb, cols)
    _wgrad_gate("%s conv2 wgrad" % tag, dr.w2_grad_mat(grads[pre + "conv2.weight"])[:, cols], np.concatenate(gs64), A64, np.concatenate(gs32), A32, x.bwd)
    del A64, A32
    rows, cols = np.arange(0, 128, 8), np.arange(0, cin, max(1, cin // 128))
    D64, D32, A64, A32 = st.conv1_wgrad_ops16(D2, X, g1, b1, Sx, rows, cols)
    _wgrad_gate("%s conv1 wgrad K %d (%s)" % (tag, cin, VARIANTS16_BWD[x.case][b][6]), grads[pre + "conv1.weight"].reshape(128, cin)[np.ix_(rows, cols)], D64, A64, D32, A32, x.bwd)
