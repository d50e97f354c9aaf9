"""The 16-bit yardstick of tests/storage_ref.py, proven without a GPU:
  * round_bf16 / round_fp16 bit for bit against torch.Tensor.to(torch.bfloat16 / torch.float16) - ties both ways, subnormals of either
    format, the neighbourhood of 65504 / 65520, the largest finite fp32 values, +-0, +-inf, NaN, and two million random bit patterns;
  * half_ulp bounds what one rounding moves; store_stat_slack bounds what rounding a plane does to its mean and invstd;
  * the storage chain against a torch bf16 / fp16 matmul (16-bit operands, fp32 accumulation, 16-bit result) at a tiny shape;
  * what each storage gate of tests/test_gpu_storage_gates.py still catches at 16-bit resolution: the REFERENCE is perturbed on the
    fp64 oracle's planes (rounded to the mode's storage type) the way a subtly wrong kernel would be - the failure modes the mode-0
    gates list in their docstrings - and the error the gate would take is printed as a ratio to the gate, asserted > 1;
  * the keep-mask of the 16-bit data-gradient gates (storage_ref.keep16 / keep_s) leaves out at most the project's 1 % of any plane it
    is applied to - the cap is a condition on the rule, shown here on the reference's planes alone (at most 0.72 % in bf16, 0.13 % in
    fp16).

Measured (-s prints every one; bf16 / fp16, x the gate): a transition's last tile left zero on the padded planes of S = 672 7.1 - 58 /
57 - 459; conv1 of layer (4,8) dropping its last 64-row tile 32 - 61 / 261 - 486, reading its newest 32-channel slice one slot too
far 48 - 49 / 394; conv2 storing the wrong half of every 16-bit pair 243 - 252 / 1900; a heightmap-form stem summing two of three
channel weights 97 / 770; norm5's backward losing a user of the masked stream 170 x its bound; transition 3's weight gradient
missing one stream's last partial tile 12 / 12.

Held in mode 0 only (printed, not asserted): a head conv0 that takes its statistics by stream instead of by pair.  Every half of F is
a BatchNorm output, so another row's statistics differ through eps / var only - parts in 10^5 - 10^6 of the operand, ten times the
fp32 gate and more, but far below one rounding of the operand to bf16 (2^-9) or fp16 (2^-12): the 16-bit gates cannot see it."""
import numpy as np
import pytest
import torch

import dense_ref as dr
import stage_ref as sr
import storage_ref as st
from gate_harness import conv1_fwd_cfg, forward_chains, halo_tile, transition_cfg
from helpers import _WGRAD_GATE, MEAN, STD, orc
from test_cpu_stage_ref import SCENES, _hp, _oracle_planes, _tiny_head, _tp

KINDS = {"bf16": torch.bfloat16, "fp16": torch.float16}
MODES = sorted(st.MODES)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _special_inputs():
    f = np.float32
    vals = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 65504.0, 65519.0, 65519.996, 65520.0, 65536.0, -65520.0, 3.3895314e38, 3.4028235e38,
            2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 3 * 2.0 ** -25, 2.0 ** -26, 1e-40, 1.17549435e-38, 1e-45]
    a = [np.asarray(vals, dtype=f)]
    # ties of both formats at many exponents: x = (m + 1/2) ulp with m even (rounds down) and odd (rounds up), and one fp32 ulp to either side
    for mant in (8, 11):
        for e in (-30, -20, -14, -13, -1, 0, 1, 7, 14, 15, 60, 100):
            for m in (2 ** (mant - 1), 2 ** (mant - 1) + 1, 2 ** mant - 2, 2 ** mant - 1):
                t = f(np.ldexp(m + 0.5, e - (mant - 1)))
                a.append(np.asarray([t, np.nextafter(t, f(np.inf)), np.nextafter(t, f(0)), -t], dtype=f))
    # fp16 subnormal ties: (m + 1/2) * 2^-24
    a.append(np.asarray([np.ldexp(m + 0.5, -24) for m in (0, 1, 2, 3, 510, 511, 1022, 1023)], dtype=f))
    r = np.random.default_rng(0)
    a.append(r.integers(0, 2 ** 32, size=2_000_000, dtype=np.uint64).astype(np.uint32).view(f))
    a.append((r.standard_normal(200_000) * 10.0 ** r.uniform(-9, 5, 200_000)).astype(f))
    return np.concatenate(a)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_rounding_matches_torch_bit_for_bit(kind):
    x = _special_inputs()
    got = st.rnd(x, kind)
    ref = torch.from_numpy(x).to(KINDS[kind]).float().numpy()
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(got)) and nan.sum() > 0
    assert np.array_equal(_bits(got)[~nan], _bits(ref)[~nan])
    assert np.array_equal(_bits(st.rnd(got, kind))[~nan], _bits(got)[~nan])          # idempotent
    # what one rounding moves is within half an ulp at the value (finite results only)
    fin = np.isfinite(got) & np.isfinite(x)
    d = np.abs(got[fin].astype(np.float64) - x[fin].astype(np.float64))
    assert (d <= st.half_ulp(x[fin], kind)).all() and (d <= st.half_ulp(got[fin], kind)).all()
    assert st.half_ulp(1.0, kind) == 2.0 ** -st.MANT[kind] and st.half_ulp(1.999, kind) == 2.0 ** -st.MANT[kind] and st.half_ulp(2.0, kind) == 2.0 ** (1 - st.MANT[kind])
    assert st.half_ulp(1e-7, "fp16") == 2.0 ** -25


def test_operand_clamps_fp16_only():
    a = np.asarray([0.0, 1.0, 65504.0, 70000.0, 1e9], dtype=np.float32)
    assert np.array_equal(st.operand(a, "fp16"), np.asarray([0.0, 1.0, 65504.0, 65504.0, 65504.0], dtype=np.float32))
    assert np.array_equal(st.operand(a, "bf16"), st.round_bf16(a)) and np.isfinite(st.operand(a, "bf16")).all()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_storage_chain_against_a_torch_16_bit_matmul(kind):
    """M = 24, N = 12, K = 40: (1) the chain's accumulation over the rounded operands against the exact product of torch's rounded
    operands: K + 1 roundings of sum |a||w|; (2) the rounded result against torch's own 16-bit matmul of 16-bit tensors (fp32
    accumulation in another order): two roundings of values that differ by (1), so at most one storage ulp apart - and mostly equal."""
    r = np.random.default_rng(3)
    a = (r.standard_normal((24, 40)) * 3).astype(np.float32)
    w = (r.standard_normal((12, 40)) * 0.1).astype(np.float32)
    ta, tw = torch.from_numpy(a).to(KINDS[kind]), torch.from_numpy(w).to(KINDS[kind])
    assert np.array_equal(st.operand(a, kind), ta.float().numpy()) and np.array_equal(st.rnd(w, kind), tw.float().numpy())
    exact = ta.double().numpy() @ tw.double().numpy().T
    mag = np.abs(ta.double().numpy()) @ np.abs(tw.double().numpy()).T
    acc = st.storage_chain(a, w, kind)
    assert (np.abs(acc - exact) <= 41 * sr.U * mag).all()
    got = st.storage_chain(a, w, kind, dst=kind)
    ref = torch.matmul(ta, tw.T).float().numpy().astype(np.float64)
    assert (np.abs(got - ref) <= 2 * st.half_ulp(exact, kind) + 1e-300).all()
    assert (got == ref).mean() >= 0.9
    # the blocked reduction over rounded operands: same operands, another order
    blk = st.storage_blocked(a.T.copy(), w.T.copy(), kind, kind, 16)
    assert (np.abs(blk - exact) <= 41 * sr.U * mag).all()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_store_stat_slack_bounds_what_rounding_does_to_the_statistics(kind):
    """planes whose statistics were taken BEFORE the store: spread-out channels, near-constant ones (|mean| / std in the thousands: the
    masked stream's background), tiny ones; 400 and 7056 pixels"""
    r = np.random.default_rng(5)
    for HW in (400, 7056):
        x = r.standard_normal((HW, 12)) * np.asarray([1, 3, 0.01, 1e-3, 2, 1, 1e-4, 5, 1, 1, 0.3, 1e-2]) + np.asarray([0, 1, 30, 3, -200, 1e-3, 0.5, 0, 8, -1, 0, 7])
        x = x.astype(np.float32)
        y = st.rnd(x, kind)
        (mx, ix), (my, iy) = sr.bn_stats(x), sr.bn_stats(y)
        M, R = st.store_stat_slack(y, kind)
        print("%s, %d pixels: |delta mean| at most %.3f of its bound, |delta invstd| at most %.3f" % (kind, HW, (np.abs(mx - my) / M).max(), (np.abs(ix / iy - 1) / R).max()))
        assert (np.abs(mx - my) <= M).all() and (np.abs(ix / iy - 1) <= R).all()
        S = st.plane_stats(y, kind, known=(slice(2, 5), x[:, 2:5]))
        assert np.array_equal(S.mean[2:5], mx[2:5]) and np.array_equal(S.inv[2:5], ix[2:5]) and (S.M[2:5] == 0).all() and np.array_equal(S.mean[5:], my[5:])
        g, b = r.standard_normal(12), r.standard_normal(12)
        assert np.array_equal(st.bn_pre_s(y, g, b, st.plane_stats(y, kind)), sr.bn_pre(y, g, b))
        assert np.array_equal(st.act32_s(y, g, b, st.plane_stats(y, kind)), sr.bn32(y, g, b))
        assert np.allclose(st.slack_s(y, g, st.plane_stats(y, kind)), st.bn_store_slack(y, g, kind), rtol=1e-12, atol=0)
        dy = r.standard_normal(y.shape)
        d_sum = np.abs((dy * ((y - mx) * ix)).sum(0) - (dy * ((y - my) * iy)).sum(0))
        assert (d_sum <= st.xhat_sum_slack(dy, y, st.plane_stats(y, kind)) * (1 + 1e-9) + 1e-9 * np.abs(dy).sum(0)).all()
        moved = np.abs(((y - mx) * ix * g + b) - sr.bn_pre(y, g, b))
        assert (moved <= st.bn_store_slack(y, g, kind) * (1 + 1e-9) + 1e-12).all()


# ---- the variant table's rules, restated (the GPU file asserts the table from eng.H / eng.HWp) -------------------------------------------------
def test_variant_rules_of_the_16_bit_modes():
    """forward.hip, modes 1 / 2: conv1 never goes wave-specialised (`e->prec == 0`), so 80^2 with 6 streams (wg128 = 300 < 320 <= wg64 =
    1200) and 84^2 with 3 (HWp % 128 = 64, wg64 = 666) take CfgP64x64 - a configuration the mode-0 table selects in neither scene"""
    S640 = [conv1_fwd_cfg(h, 6, False) for h in (25600, 6400, 1600, 448)]
    S672 = [conv1_fwd_cfg(h, 3, False) for h in (28288, 7104, 1792, 448)]
    assert S640 == ["P128x128", "P64x64", "P32x64", "P32x64"] and S672 == ["P128x128", "P64x64", "P32x64", "P32x64"]
    assert [halo_tile(h, 6) for h in (160, 80, 40, 20)] == [16, 8, 8, 8] and [halo_tile(h, 3) for h in (168, 84, 42, 21)] == [16, 8, 8, 8]
    assert [transition_cfg(h) for h in (6400, 1600, 448)] == ["P128x128", "P64x128", "P64x128"]
    assert [transition_cfg(h) for h in (7104, 1792, 448)] == ["P64x128", "P128x128", "P64x128"]
    assert forward_chains(6, 160) == [6] and forward_chains(3, 168) == [3] and forward_chains(17, 160) == [8, 9]


# ---- what the gates still catch at 16-bit resolution ---------------------------------------------------------------------------------------------
def _report(what, e_pert, gate):
    print("perturbation: %-96s error %.3e = %.3g x the gate (%.3e)" % (what, e_pert, e_pert / gate, gate))
    assert e_pert > gate, (what, e_pert, gate)


@pytest.mark.parametrize("mode", MODES)
def test_transition_that_drops_the_last_tile_row_of_a_padded_plane(mode):
    """S = 672: x<t+1> has 7104 / 1792 / 448 rows for 7056 / 1764 / 441 pixels; the last 64-row tile of the output left zero.  Against
    the whole-plane gate of test_transition_forward: 2 x the storage chain's error on the pixel sample."""
    m = st.MODES[mode]
    P = _oracle_planes("S672")
    sd = P["sd"]
    for t in (1, 2, 3):
        H, Cp = P["S"] // (2 ** (t + 1)), dr.CT[t - 1]
        C0, HWn = Cp // 2, (H // 2) ** 2
        g, b = _tp(sd, "transition%d.norm.weight" % t), _tp(sd, "transition%d.norm.bias" % t)
        w = _tp(sd, "transition%d.conv.weight" % t).reshape(C0, Cp)
        pix, cols = dr.sample(HWn), np.arange(0, C0, max(1, C0 // 128))
        X = st.rnd(P["x"][t - 1][1], m["act"])
        ref = sr.transition_fwd(X, H, H, g, b, w)
        mag = sr.pooled_act(X, H, H, g, b) @ np.abs(w.astype(np.float64)).T + 1e-300
        sel = np.ix_(pix, cols)
        gate = 2.0 * dr.rms(st.storage_chain(sr.pooled_act32(X, H, H, g, b)[pix], np.ascontiguousarray(w[cols]), m["fwd"], m["act"]), ref[sel], mag[sel])
        bad = ref.copy()
        bad[(HWn // 64) * 64:] = 0
        _report("%s transition %d: last tile (rows %d..%d of %d) left zero" % (mode, t, (HWn // 64) * 64, HWn - 1, HWn), dr.rms(bad, ref, mag), gate)


@pytest.mark.parametrize("mode", MODES)
def test_dense_layer_that_drops_a_tile_or_reads_a_shifted_slice(mode):
    """Block 4, layer 8 on the oracle's 20^2 / 21^2 planes rounded to the mode's storage: conv1 drops the last 64-row tile; conv1 reads
    its newest 32-channel slice one slot too far (x[:, cin:cin+32] in place of x[:, cin-32:cin]); conv2 stores the layer's 32 channels
    with the wrong half of every 16-bit pair (channels 2 k and 2 k + 1 swapped)."""
    m = st.MODES[mode]
    for case in sorted(SCENES):
        P = _oracle_planes(case)
        sd, H = P["sd"], P["S"] // 32
        HW, cin = H * H, dr.cin_of(4, 8)
        lp = lambda n: _tp(sd, "denseblock4.denselayer8." + n)      # noqa: E731
        g1, b1, w1 = lp("norm1.weight"), lp("norm1.bias"), lp("conv1.weight").reshape(128, cin)
        g2, b2, w2 = lp("norm2.weight"), lp("norm2.bias"), lp("conv2.weight")
        X = st.rnd(P["x"][3][1], m["act"])
        ref, mag = dr.conv1_fwd(X[:, :cin], g1, b1, w1)
        gate = 2.0 * dr.rms(st.storage_chain(dr.act32(X[:, :cin], g1, b1), w1, m["fwd"], m["act"]), ref, mag)
        bad = ref.copy()
        bad[(HW // 64) * 64:] = 0
        _report("%s %s: conv1 (4,8) drops the last 64-row tile" % (mode, case), dr.rms(bad, ref, mag), gate)
        Xs = np.concatenate([X[:, :cin - 32], X[:, cin:cin + 32]], axis=1)
        _report("%s %s: conv1 (4,8) reads its newest slice one slot too far" % (mode, case), dr.rms(dr.conv1_fwd(Xs, g1, b1, w1)[0], ref, mag), gate)
        BT = st.rnd(ref.astype(np.float32), m["act"])
        ref2, mag2 = dr.conv2_fwd(BT, H, H, g2, b2, w2)
        gate2 = 2.0 * dr.rms(st.conv2_chain(BT, H, H, g2, b2, w2, np.arange(HW), m["fwd"], m["act"]), ref2, mag2)
        swapped = ref2.reshape(HW, 16, 2)[:, :, ::-1].reshape(HW, 32)
        _report("%s %s: conv2 (4,8) stores the wrong half of every 16-bit pair" % (mode, case), dr.rms(swapped, ref2, mag2), gate2)


@pytest.mark.parametrize("mode", MODES)
def test_stem_that_sums_two_of_three_channel_weights(mode):
    """the heightmap-form stem on the masked stream's image of S = 672, both edges' rows; the gate: 2 x the storage chain (image and
    summed weights rounded to the mode's forward operand type, fp32 destination)"""
    import synthetic
    m = st.MODES[mode]
    c = SCENES["S672"]
    depth, masks = synthetic.heightmap_scene(c["seed"], size=c["size"], n_boxes=8)
    img = orc.preprocess(depth * masks[0], [MEAN] * 3, [STD] * 3)[0, 0].numpy().astype(np.float32)[:, :, None]
    w = _tp(_oracle_planes("S672")["sd"], "conv0.weight").astype(np.float32)
    rows = np.concatenate([np.arange(12), np.arange(336 - 12, 336)])
    w1 = w.astype(np.float64).sum(1, keepdims=True)
    ref, _ = sr.stem_conv(img, w1, rows)
    mag = np.abs(sr.stem_cols(img.astype(np.float64), rows)) @ sr.stem_wmat(np.abs(w.astype(np.float64)).sum(1, keepdims=True)).T + 1e-300
    gate = 2.0 * dr.rms(st.storage_chain(sr.stem_cols(img, rows), sr.stem_wmat(w1.astype(np.float32)), m["fwd"]), ref, mag)
    two, _ = sr.stem_conv(img, w[:, :2].astype(np.float64).sum(1, keepdims=True), rows)
    _report("%s: heightmap-form stem sums two of the three channel weights" % mode, dr.rms(two, ref, mag), gate)


@pytest.mark.parametrize("mode", MODES)
def test_norm5_backward_that_loses_a_user_of_the_masked_stream(mode):
    """the oracle's block-4 planes and head gradient, the one pair presented twice (the second with half the gradient): both streams
    have two users.  g4 is stored in bf16 in both modes; its gate is stage_ref.k_g4 roundings of mag plus half a bf16 ulp."""
    m = st.MODES[mode]
    for case in sorted(SCENES):
        P = _oracle_planes(case)
        sd = P["sd"]
        x4 = [st.rnd(P["x"][3][s], m["act"]) for s in range(2)]
        g5, g0, g1 = _tp(sd, "norm5.weight"), _hp(sd, "norm0.weight"), _hp(sd, "norm1.weight")
        df = sr.head_conv0_bwd(P["h1"][0], P["dh1"][0], P["feat"][0], g1, g0, _hp(sd, "norm0.bias"), _hp(sd, "conv0.weight").reshape(64, 2048))[0].astype(np.float32)
        Fm, DF = np.stack([P["feat"][0]] * 2), np.stack([df, 0.5 * df])
        G4, _, mag, *_ = sr.norm5_bwd(x4, Fm, DF, g0, g5, [0, 0], [1, 1])
        lost = sr.norm5_bwd(x4, Fm[:1], DF[:1], g0, g5, [0], [1])[0]
        bound = st.stored_bound(G4[1], sr.k_g4(2), np.abs(g5) * mag[1], m["grd"])
        worst = float((np.abs(lost[1] - G4[1]) / (bound + 1e-300)).max())
        print("perturbation: %s %s: norm5 backward loses the second user of the masked stream: %.3g x the bound" % (mode, case, worst))
        assert worst > 1.0


@pytest.mark.parametrize("mode", MODES)
def test_head_statistics_by_stream_instead_of_by_pair_is_held_in_mode_0_only(mode):
    """(printed, not asserted - see the module docstring) tiny planes as in test_cpu_stage_ref.test_feat_and_head_conv0"""
    m = st.MODES[mode]
    x4, pa, pb, p = _tiny_head(np.random.default_rng(4), 36, 8, 2)
    Fm, _ = sr.feat(x4, p["g5"], p["b5"], pa, pb)
    F0 = Fm[0].astype(np.float32)
    ref, a64 = sr.head_conv0(F0, p["g0"], p["b0"], p["w0"])
    mag = a64 @ np.abs(p["w0"]).T + 1e-300
    gate = 2.0 * dr.rms(st.storage_chain(sr.bn32(F0, p["g0"], p["b0"]), p["w0"].astype(np.float32), m["fwd"]), ref, mag)
    mean1, inv1 = sr.bn_stats(Fm[1])
    other = np.maximum((F0 - mean1) * inv1 * p["g0"] + p["b0"], 0.0) @ p["w0"].T
    print("perturbation: %s: head conv0 with another pair's statistics: %.3g x the 16-bit gate (held in mode 0 only)" % (mode, dr.rms(other, ref, mag) / gate))


@pytest.mark.parametrize("mode", MODES)
def test_transition_weight_gradient_that_misses_a_streams_last_tile(mode):
    """transition 3 of S = 672 (21^2 pooled pixels): the W_POOL weight gradient over both streams with the last stream's last partial
    tile missing, against _WGRAD_GATE x the blocked reduction over the rounded operands (a synthetic gradient of x4's first channels)"""
    m = st.MODES[mode]
    P = _oracle_planes("S672")
    sd = P["sd"]
    H, Cp, C0 = 42, 1024, 512
    g, b = _tp(sd, "transition3.norm.weight"), _tp(sd, "transition3.norm.bias")
    r = np.random.default_rng(9)
    Xs = [st.rnd(P["x"][2][s], m["act"]) for s in range(2)]
    Xn = [st.rnd(P["x"][3][s][:, :C0], m["act"]) for s in range(2)]
    Gn = [st.rnd((r.standard_normal(v.shape) * 1e-3).astype(np.float32), m["grd"]) for v in Xn]
    dX64 = np.concatenate([sr.bn_bwd(G, v) for G, v in zip(Gn, Xn)])[:, ::8]
    dX32 = np.concatenate([sr.bn_bwd32(G, v) for G, v in zip(Gn, Xn)])[:, ::8]
    P64 = np.concatenate([sr.pooled_act(v, H, H, g, b)[:, ::8] for v in Xs])
    P32 = np.concatenate([sr.pooled_act32(v, H, H, g, b)[:, ::8] for v in Xs])
    ref = dX64.T @ P64
    mag = np.abs(dX64).T @ np.abs(P64) + 1e-300
    gate = _WGRAD_GATE * dr.rms(st.storage_blocked(dX32, P32, m["bwd"], m["bwd"]), ref, mag)
    tail = slice(len(dX64) - (441 - 384), len(dX64))
    _report("%s: transition 3 weight gradient misses the last stream's partial tile" % mode, dr.rms(ref - dX64[tail].T @ P64[tail], ref, mag), gate)


# ---- the keep-mask ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(SCENES))
def test_keep_mask_of_the_16_bit_gates_leaves_out_at_most_one_percent(case, mode):
    """storage_ref.keep_s (keep16 with the statistics of storage_ref.plane_stats) on the planes the 16-bit data-gradient gates apply it
    to - the three transition norms over x1..x3 rounded to the mode's activation storage, pool0's channels of x1 with the statistics the
    stem plane determines.  (With the stored plane's statistics and their slack on those 64 channels too, the masked stream of S = 640
    has 1.09 % of x1 borderline in bf16: the whole background of channels 20 and 61 - pool0's - and 206 sits within the slack of zero.)  (The head's norm0 reads the fp32 feature buffer, whose statistics are those of the stored values:
    it keeps stage_ref.bn_keep, shown in test_cpu_stage_ref.)"""
    m = st.MODES[mode]
    P = _oracle_planes(case)
    sd = P["sd"]
    for s in range(2):
        for t in (1, 2, 3):
            X = st.rnd(P["x"][t - 1][s], m["act"])
            g, b = _tp(sd, "transition%d.norm.weight" % t), _tp(sd, "transition%d.norm.bias" % t)
            if t == 1:          # pool0's 64 channels: stored as the rounded fp32 maxima, their statistics known from the stem plane
                Hs = P["S"] // 2
                X = X.copy()
                X[:, :64] = st.rnd(sr.pool0_32(P["stem"][s], Hs, Hs, _tp(sd, "norm0.weight"), _tp(sd, "norm0.bias")), m["act"])
                S = st.x1_stats(X, P["stem"][s], Hs, _tp(sd, "norm0.weight"), _tp(sd, "norm0.bias"), m["act"])
                assert (S.M[:64] == 0).all() and (S.M[64:] > 0).all()
            else:
                S = st.plane_stats(X, m["act"])
                assert np.array_equal(st.keep_s(X, g, b, S), st.keep16(X, g, b, m["act"]))
            keep = st.keep_s(X, g, b, S)
            print("%s %s transition %d stream %d: %.4f %% borderline" % (case, mode, t, s, 100 * (1 - keep.mean())))
            assert 1 - keep.mean() <= 0.01
