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

  * the dense layers' backward in the 16-bit modes (storage_ref's second half): the *_s restatements at fp64 against the tiny dense block
    test_cpu_dense_ref holds to torch autograd, the data-gradient chains against torch's bf16 matmul, the slack of sums taken in front
    of a bf16 store, what each backward gate catches (a zeroed 8-row tile row of dy2 91 - 132 x the gate, swapped halves of every 32-bit
    word 300 - 305 x, a mask from the other stream's statistics 62 - 85 x, a dropped segment of the grouped form 46 - 55 x, the
    accumulate stored as an overwrite 1000 - 1470 x, one stream's pixels missing from a weight gradient 118 - 138 x, its last pixel
    chunk 7.3 - 30 x) and
    the keep-masks of every gated layer with the engine's statistics: at most 0.0043 % borderline; the materialised GS from sums handed in
    (gs_from_sums) and what its element bound trips on (a dropped 128-row workgroup 512 x, everything else 3600 x and more).

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
from gate_harness import BWD_LAYERS16, conv1_fwd_cfg, forward_chains, halo_tile, transition_cfg
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


# ---- the dense layers' backward in the 16-bit modes ---------------------------------------------------------------------------------------------


def test_backward_restatements_at_fp64_equal_the_walk_autograd_proved():
    """storage_ref's *_s forms with the statistics handed in as the engine's sums (engine_stats of plane_sums) against the tiny dense
    block of test_cpu_dense_ref (whose every buffer test_dense_layer_forward_and_backward_equal_torch holds to torch autograd): GS, the
    norm2 backward, both forms of the conv1 data gradient, both weight gradients.  The sums' slack is the table's fp32 rounding."""
    import test_cpu_dense_ref as t
    for H, W in t.PLANES:
        o = t._walk(H, W)
        for s in range(t.NS):
            Sx = st.engine_stats(st.plane_sums(o.X[s]), o.HW)
            mean, inv = sr.bn_stats(o.X[s])
            assert np.allclose(Sx.mean, mean, rtol=1e-12, atol=1e-14) and np.allclose(Sx.inv, inv, rtol=1e-10) and (Sx.R == sr.U).all()
            for i in range(t.L):
                p, cin = o.prm[i], t.CIN0 + t.GROWTH * i
                sl = slice(cin, cin + t.GROWTH)
                _near(st.bn_bwd_s(o.G0[s][i][:, sl], o.X[s][:, sl], Sx.cols(sl)), o.GS[s][i], "GS")
                Sb = st.engine_stats(st.plane_sums(o.BT[s][i]), o.HW)
                _near(st.bn_bwd_s(o.DY[s][i], o.BT[s][i], Sb, p["g2"]), o.D2[s][i], "D2")
                assert (st.bn_bwd_sum_mag_s(o.DY[s][i], o.BT[s][i], Sb, p["g2"]) >= np.abs(o.D2[s][i]) * (1 - 1e-9)).all()
                for layers, c0, c1 in dr.dgrad1_segments(t.L, i, t.CIN0, t.GROWTH):
                    prm = [(o.prm[l]["g1"], o.prm[l]["b1"], o.prm[l]["w1"]) for l in layers]
                    d2s = [o.D2[s][l] for l in layers]
                    ref, mag, _, _ = dr.conv1_dgrad(o.G0[s][i], o.X[s], prm, d2s, c0, c1, chain=False)
                    r16, m16, ch, keep = st.conv1_dgrad16(o.G0[s][i], o.X[s], Sx, prm, d2s, c0, c1)
                    _near(r16, ref, "conv1 data gradient"); _near(m16, mag, "its magnitude")
                    assert np.array_equal(st.rnd(ch, "bf16"), ch) and keep.mean() > 0.99
        for i in range(t.L):
            p, cin = o.prm[i], t.CIN0 + t.GROWTH * i
            Sb = [st.engine_stats(st.plane_sums(o.BT[s][i]), o.HW) for s in range(t.NS)]
            Sx = [st.engine_stats(st.plane_sums(o.X[s]), o.HW) for s in range(t.NS)]
            G64, _, A64, _ = st.conv2_wgrad_ops16([o.GS[s][i] for s in range(t.NS)], [o.BT[s][i] for s in range(t.NS)], H, W, p["g2"], p["b2"], Sb, np.arange(9 * t.BOTT))
            _near(np.concatenate([o.GS[s][i] for s in range(t.NS)]).T @ A64, o.dW2[i], "conv2 weight gradient")
            _, _, A64, _ = st.conv1_wgrad_ops16([o.D2[s][i] for s in range(t.NS)], o.X, p["g1"], p["b1"], Sx, np.arange(t.BOTT), np.arange(cin))
            _near(np.concatenate([o.D2[s][i] for s in range(t.NS)]).T @ A64, o.dW1[i], "conv1 weight gradient")


def _near(a, b, what):
    assert np.abs(np.asarray(a) - b).max() <= 1e-9 * max(np.abs(b).max(), 1e-30), what


def test_backward_chains_against_torch_bf16_matmul():
    """the 3x3 data-gradient chain and the accumulate chain against torch's own bf16 matmul of bf16 tensors (fp32 accumulation in
    another order, bf16 result): two roundings of nearly equal values, at most one bf16 ulp apart and mostly equal"""
    r = np.random.default_rng(11)
    H = W = 6
    gs = st.rnd((r.standard_normal((H * W, 4)) * 1e-2).astype(np.float32), "bf16")
    w2 = (r.standard_normal((4, 8, 3, 3)) * 0.2).astype(np.float32)
    on = r.random((H * W, 8)) > 0.3
    pix = np.arange(H * W)
    ch = st.conv2_dgrad_chain16(gs, H, W, w2, on, pix)
    ta = torch.from_numpy(dr.im2col(gs, H, W, pix, flip=True)).to(torch.bfloat16)
    tw = torch.from_numpy(dr.w2_bwd_mat(w2).astype(np.float32)).to(torch.bfloat16)
    ref = (torch.matmul(ta, tw.T).float().numpy() * on).astype(np.float64)
    assert (np.abs(ch - ref) <= 2 * st.half_ulp(ref, "bf16") + 1e-300).all() and (ch == ref).mean() >= 0.9
    assert not ch[~on].any()
    # the accumulate: one segment, gamma = 1, every ReLU on, statistics of the plane - rnd(G0 + D2 @ W) against torch
    x = r.standard_normal((H * W, 12)).astype(np.float32) + 5.0
    S = st.engine_stats(st.plane_sums(x), H * W)
    g1, b1 = np.ones(12, dtype=np.float32), np.full(12, 9.0, dtype=np.float32)
    w1 = (r.standard_normal((8, 12)) * 0.3).astype(np.float32)
    d2 = st.rnd((r.standard_normal((H * W, 8)) * 1e-2).astype(np.float32), "bf16")
    G0 = st.rnd((r.standard_normal((H * W, 12)) * 1e-2).astype(np.float32), "bf16")
    ref64, mag, ch, keep = st.conv1_dgrad16(G0, x, S, [(g1, b1, w1)], [d2], 0, 12)
    assert keep.all() and (mag >= np.abs(ref64) * (1 - 1e-12)).all()
    prod = torch.matmul(torch.from_numpy(d2).to(torch.bfloat16).float(), torch.from_numpy(w1).to(torch.bfloat16).float())
    ref = (torch.from_numpy(G0) + prod).to(torch.bfloat16).float().numpy().astype(np.float64)
    assert (np.abs(ch - ref) <= 2 * st.half_ulp(ref, "bf16")).all() and (ch == ref).mean() >= 0.9


def test_sums_before_store_slack_bounds_what_the_store_does_to_the_norm2_backward():
    """dy rounded to bf16 AFTER its sums were taken: bn_bwd_s with the sums of the unrounded dy (the engine's) against bn_bwd_s of the
    stored dy alone differs by at most sums_before_store_slack per element; the two sums by its per-channel terms"""
    r = np.random.default_rng(12)
    for HW in (400, 1764):
        dy = (r.standard_normal((HW, 16)) * 10.0 ** r.uniform(-6, -2, 16) * (r.random((HW, 16)) > 0.4)).astype(np.float32)
        bt = (r.standard_normal((HW, 16)) * 2 + r.standard_normal(16)).astype(np.float32)
        g2 = r.standard_normal(16)
        S = st.engine_stats(st.plane_sums(bt), HW)
        dys = st.rnd(dy, "bf16")
        a, q1, mean, k = st.bn_bwd_terms_s(dy, bt, S, g2)          # the engine's coefficients: sums of the unrounded values
        engine = a * ((dys.astype(np.float64) - q1) - (bt.astype(np.float64) - mean) * k)
        sl, h1, h2 = st.sums_before_store_slack(dys, bt, S, g2)
        worst = float((np.abs(engine - st.bn_bwd_s(dys, bt, S, g2)) / (sl + 1e-300)).max())
        print("%d pixels: the sums taken before the bf16 store move the norm2 backward by at most %.3f of the slack" % (HW, worst))
        assert worst <= 1.0
        xh = (bt.astype(np.float64) - S.mean) * S.inv
        assert (np.abs(dy.astype(np.float64).sum(0) - dys.astype(np.float64).sum(0)) <= h1).all()
        assert (np.abs((dy * xh).sum(0) - (dys * xh).sum(0)) <= h2 * (1 + 1e-12)).all()
        assert st.k_d2_apply(16) == 526 and st.k_d2_apply(8) == 142 and st.k_affine2(8, 6, True) == 63 + 5 + 1 + 5 and st.k_gs_top(5) == 187


_BWD = {}


def _bwd_planes(case, block, layer):
    """One dense layer's backward buffers on the oracle's planes of `case` (the rotation and the masked stream), as mode bf16 holds them:
    x<b> and the bottleneck rounded to bf16 with the statistics of the values IN FRONT of the store (what the engine sums), a synthetic
    G' (the oracle walk keeps no gradients: bf16 noise of the size the gates meet, 1e-3), and from it GS, dy2, D2 and - for a layer at
    the bottom of a group - the D2 of the group's other layers (synthetic), each rounded once to bf16 where the kernels round."""
    if (case, block, layer) in _BWD:
        return _BWD[(case, block, layer)]
    P = _oracle_planes(case)
    sd, H = P["sd"], P["S"] // (2 ** (block + 1))
    HW, cin, Lb = H * H, dr.cin_of(block, layer), dr.LAYERS[block - 1]
    lp = lambda l, n: _tp(sd, "denseblock%d.denselayer%d.%s" % (block, l, n))      # noqa: E731
    r = np.random.default_rng(block * 100 + layer)
    o = dict(H=H, HW=HW, cin=cin, g2=lp(layer, "norm2.weight"), b2=lp(layer, "norm2.bias"), w2=lp(layer, "conv2.weight"), streams=[])
    o["segs"] = dr.dgrad1_segments(Lb, layer - 1, dr.CIN0[block - 1])
    o["prm"] = {l: (lp(l + 1, "norm1.weight"), lp(l + 1, "norm1.bias"), lp(l + 1, "conv1.weight").reshape(128, -1)) for sg in o["segs"] for l in sg[0]}
    o["prm"][layer - 1] = (lp(layer, "norm1.weight"), lp(layer, "norm1.bias"), lp(layer, "conv1.weight").reshape(128, cin))
    for s in range(2):
        X32 = P["x"][block - 1][s]
        Sx, X = st.engine_stats(st.plane_sums(X32), HW), st.rnd(X32, "bf16")
        g1, b1, w1 = o["prm"][layer - 1]
        bt32 = (st.act64_s(X[:, :cin], g1, b1, Sx.cols(slice(0, cin))) @ w1.astype(np.float64).T).astype(np.float32)
        Sb, BT = st.engine_stats(st.plane_sums(bt32), HW), st.rnd(bt32, "bf16")
        G0 = st.rnd((r.standard_normal(X.shape) * 1e-3).astype(np.float32), "bf16")
        sl = slice(cin, cin + 32)
        GS = st.rnd(st.bn_bwd_s(G0[:, sl], X[:, sl], Sx.cols(sl)).astype(np.float32), "bf16")
        on = st.bn_pre_s(BT, o["g2"], o["b2"], Sb) > 0
        dy64, dymag = dr.conv2_dgrad(GS, H, H, o["w2"])
        DY = st.rnd((on * dy64).astype(np.float32), "bf16")
        D2 = {layer - 1: st.rnd(st.bn_bwd_s(DY, BT, Sb, o["g2"]).astype(np.float32), "bf16")}
        for l in o["prm"]:
            if l not in D2:
                D2[l] = st.rnd((r.standard_normal((HW, 128)) * np.abs(D2[layer - 1]).mean() * 1.25).astype(np.float32), "bf16")
        o["streams"].append(dict(X=X, Sx=Sx, BT=BT, Sb=Sb, G0=G0, GS=GS, on=on, dy64=on * dy64, dymag=dymag, DY=DY, D2=D2))
    _BWD[(case, block, layer)] = o
    return o


@pytest.mark.parametrize("case,block,layer", [("S640", 4, 13), ("S672", 4, 13), ("S672", 3, 21)])
def test_what_the_16_bit_backward_gates_catch(case, block, layer):
    """The perturbations the issue of these gates lists, on a layer at the bottom of a four-layer group (grouped form, nseg = 4, and the
    per-layer form beside it is empty: the grouped segment is the layer's whole data gradient), each against the gate the GPU test
    applies: 2 x the storage chain for the data gradients (whole plane, kept elements), the element bound for the in-place norm2
    backward, _WGRAD_GATE x the blocked reduction over the bf16 operands for the weight gradients."""
    o = _bwd_planes(case, block, layer)
    H, HW, cin = o["H"], o["HW"], o["cin"]
    pix = np.arange(HW)
    tag = "%s (%d,%d)" % (case, block, layer)
    for s, d in enumerate(o["streams"]):
        ref, mag = d["dy64"], d["dymag"]
        keep2 = st.keep_s(d["BT"], o["g2"], o["b2"], d["Sb"])
        gate = 2.0 * dr.rms(st.conv2_dgrad_chain16(d["GS"], H, H, o["w2"], d["on"], pix), ref, mag, keep2)
        bad = d["DY"].copy()
        bad.reshape(H, H, 128)[8:16] = 0
        _report("%s stream %d: one 8-row tile row of dy2 left zero" % (tag, s), dr.rms(bad, ref, mag, keep2), gate)
        swapped = d["DY"].reshape(HW, 64, 2)[:, :, ::-1].reshape(HW, 128)
        _report("%s stream %d: dy2 stored with the two halves of every 32-bit word swapped" % (tag, s), dr.rms(swapped, ref, mag, keep2), gate)
        other = o["streams"][1 - s]["Sb"]
        on_o = st.bn_pre_s(d["BT"], o["g2"], o["b2"], other) > 0
        _report("%s stream %d: the ReLU mask of dy2 from the other stream's statistics" % (tag, s), dr.rms(on_o * dr.conv2_dgrad(d["GS"], H, H, o["w2"])[0], ref, mag, keep2), gate)
        # the in-place norm2 backward: the same swap and a dropped 64-row tile against the element bound
        r2, bound = st.norm2_inplace(d["DY"], d["BT"], o["g2"], d["Sb"], 8)
        assert (np.abs(d["D2"][layer - 1] - r2) <= bound).all()
        sw = d["D2"][layer - 1].reshape(HW, 64, 2)[:, :, ::-1].reshape(HW, 128)
        worst = float((np.abs(sw - r2) / (bound + 1e-300)).max())
        print("perturbation: %s stream %d: D2 with adjacent channels swapped: %.3g x the element bound" % (tag, s, worst))
        assert worst > 1.0
        (layers, c0, c1), = [sg for sg in o["segs"] if sg[1] == 0]
        assert len(layers) == 4 and len(o["segs"]) == 1
        prm, d2s = [o["prm"][l] for l in layers], [d["D2"][l] for l in layers]
        ref, mag, ch, keep = st.conv1_dgrad16(d["G0"], d["X"], d["Sx"], prm, d2s, c0, c1)
        gate = 2.0 * dr.rms(ch, ref, mag, keep)
        lost = st.conv1_dgrad16(d["G0"], d["X"], d["Sx"], prm[:-1], d2s[:-1], c0, c1, chain=False)[0]
        _report("%s stream %d: one segment of the grouped 1x1 data gradient dropped" % (tag, s), dr.rms(lost, ref, mag, keep), gate)
        _report("%s stream %d: the accumulate stored as an overwrite (G0 lost)" % (tag, s), dr.rms(ref - d["G0"][:, c0:c1], ref, mag, keep), gate)
        sw = ch.reshape(HW, (c1 - c0) // 2, 2)[:, :, ::-1].reshape(HW, c1 - c0)
        _report("%s stream %d: G' stored with adjacent channels swapped" % (tag, s), dr.rms(sw, ref, mag, keep), gate)
        Sx_o = o["streams"][1 - s]["Sx"]
        oth = st.conv1_dgrad16(d["G0"], d["X"], Sx_o, prm, d2s, c0, c1, chain=False)[0]
        _report("%s stream %d: the norm1 masks from the other stream's statistics" % (tag, s), dr.rms(oth, ref, mag, keep), gate)
    # weight gradients over both streams
    S2 = o["streams"]
    cols = np.arange(0, 9 * 128, 9)
    G64, G32, A64, A32 = st.conv2_wgrad_ops16([d["GS"] for d in S2], [d["BT"] for d in S2], H, H, o["g2"], o["b2"], [d["Sb"] for d in S2], cols)
    g1, b1, _ = o["prm"][layer - 1]
    rows, c1x = np.arange(0, 128, 8), np.arange(0, cin, max(1, cin // 128))
    D64, D32, B64, B32 = st.conv1_wgrad_ops16([d["D2"][layer - 1] for d in S2], [d["X"] for d in S2], g1, b1, [d["Sx"] for d in S2], rows, c1x)
    for name, a64, a32, w64, w32 in (("conv2", G64, G32, A64, A32), ("conv1", D64, D32, B64, B32)):
        ref, mag = a64.T @ w64, np.abs(a64).T @ np.abs(w64) + 1e-300
        gate = _WGRAD_GATE * dr.rms(st.storage_blocked(a32, w32, "bf16", "bf16"), ref, mag)
        one = slice(HW, 2 * HW)
        _report("%s: one stream's pixels missing from the %s weight gradient" % (tag, name), dr.rms(ref - a64[one].T @ w64[one], ref, mag), gate)
        tail = slice(2 * HW - (HW - (HW // 64) * 64 or 64), 2 * HW)
        _report("%s: the last pixel chunk (%d rows) missing from the %s weight gradient" % (tag, tail.stop - tail.start, name), dr.rms(ref - a64[tail].T @ w64[tail], ref, mag), gate)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(BWD_LAYERS16))
def test_keep_masks_of_the_16_bit_backward_gates_leave_out_at_most_one_percent(case, mode):
    """The 1 % condition of the backward gates, before any GPU run: the oracle's planes rounded to the mode's activation storage, the
    statistics those of the values in front of the store within the table's fp32 rounding (engine_stats) - norm2's mask of every gated
    layer's bottleneck and the combined norm1 masks of every segment of its conv1 data gradient.  (The oracle's streams are one rotation
    and the masked stream; the GPU gates assert the same cap on the streams they use.)"""
    m = st.MODES[mode]
    P = _oracle_planes(case)
    sd = P["sd"]
    worst = 0.0
    for block, layer in BWD_LAYERS16[case]:
        cin, Lb, HW = dr.cin_of(block, layer), dr.LAYERS[block - 1], len(P["x"][block - 1][0])
        lp = lambda l, n: _tp(sd, "denseblock%d.denselayer%d.%s" % (block, l, n))      # noqa: E731
        for s in range(2):
            X32 = P["x"][block - 1][s]
            Sx, X = st.engine_stats(st.plane_sums(X32), HW), st.rnd(X32, m["act"])
            bt32 = (st.act64_s(X[:, :cin], lp(layer, "norm1.weight"), lp(layer, "norm1.bias"), Sx.cols(slice(0, cin))) @ lp(layer, "conv1.weight").reshape(128, cin).astype(np.float64).T).astype(np.float32)
            sh2 = 1 - st.keep_s(st.rnd(bt32, m["act"]), lp(layer, "norm2.weight"), lp(layer, "norm2.bias"), st.engine_stats(st.plane_sums(bt32), HW)).mean()
            sh1 = 0.0
            for layers, c0, c1 in dr.dgrad1_segments(Lb, layer - 1, dr.CIN0[block - 1]):
                keep = np.ones((HW, c1 - c0), dtype=bool)
                for l in layers:
                    keep &= st.keep_s(X[:, c0:c1], lp(l + 1, "norm1.weight")[c0:c1], lp(l + 1, "norm1.bias")[c0:c1], Sx.cols(slice(c0, c1)))
                sh1 = max(sh1, 1 - keep.mean())
            print("%s %s block %d layer %2d stream %d: borderline %.4f %% (norm2 mask), %.4f %% (norm1 masks of a segment, worst)" % (case, mode, block, layer, s, 100 * sh2, 100 * sh1))
            worst = max(worst, sh1, sh2)
    assert worst <= 0.01, worst


def test_backward_layers_follow_the_rules():
    for case, layers in BWD_LAYERS16.items():
        assert len(layers) <= 5 and {b for b, _ in layers} == {1, 2, 3, 4} and (4, 16) in layers
        forms = {(b, l): [(len(ls), c0) for ls, c0, _ in dr.dgrad1_segments(dr.LAYERS[b - 1], l - 1, dr.CIN0[b - 1])] for b, l in layers}
        assert any(len(f) == 1 and f[0][1] > 0 for f in forms.values()), "a layer in the per-layer form only"
        assert any((4, 0) in f for f in forms.values()), "a bottom of a four-layer group"
    assert any(l == 1 for ls in BWD_LAYERS16.values() for _, l in ls), "a block's first layer"


@pytest.mark.parametrize("case,block,layer", [("S640", 4, 13), ("S672", 3, 21)])
def test_what_the_materialised_gs_gate_catches(case, block, layer):
    """storage_ref.gs_from_sums - GS from the stored G' / x slices with the sums s1 / s2 HANDED IN (the engine's, debug_read "bs_x<b>") -
    equals bn_bwd_s when the sums are those of the slice; and the element bound of the GPU gate (K_GS_APPLY roundings + half a bf16
    ulp, no slack) on the oracle's planes: a dropped 128-row workgroup of bn_bwd_apply_kernel<PREC>, adjacent channels swapped, the x
    slice of the neighbouring layer, the other stream's sums, sums over HWp instead of HW."""
    o = _bwd_planes(case, block, layer)
    HW, cin = o["HW"], o["cin"]
    sl = slice(cin, cin + 32)
    tag = "%s (%d,%d)" % (case, block, layer)
    sums = []
    for d in o["streams"]:
        Sc = d["Sx"].cols(sl)
        g, x = d["G0"][:, sl].astype(np.float64), d["X"][:, sl].astype(np.float64)
        sums.append(np.stack([g.sum(0), (g * ((x - Sc.mean) * Sc.inv)).sum(0)]))
    for s, d in enumerate(o["streams"]):
        Sc = d["Sx"].cols(sl)
        ref, mag = st.gs_from_sums(d["G0"][:, sl], d["X"][:, sl], Sc, sums[s], HW)
        _near(ref, st.bn_bwd_s(d["G0"][:, sl], d["X"][:, sl], Sc), "GS from its sums")
        bound = st.stored_bound(ref, st.K_GS_APPLY, mag, "bf16")
        assert (np.abs(d["GS"] - ref) <= bound).all()
        bad = d["GS"].copy()
        bad[(HW // 128) * 128 - 128:(HW // 128) * 128] = 0
        cases = [("a 128-row workgroup of the apply left zero", bad),
                 ("adjacent channels swapped", d["GS"].reshape(HW, 16, 2)[:, :, ::-1].reshape(HW, 32)),
                 ("the x slice of the layer below", st.gs_from_sums(d["G0"][:, sl], d["X"][:, cin - 32:cin], Sc, sums[s], HW)[0]),
                 ("the other stream's sums", st.gs_from_sums(d["G0"][:, sl], d["X"][:, sl], Sc, sums[1 - s], HW)[0]),
                 ("the sums divided by HWp", st.gs_from_sums(d["G0"][:, sl], d["X"][:, sl], Sc, sums[s], -(-HW // 64) * 64)[0])]
        for what, v in cases:
            worst = float((np.abs(v - ref) / (bound + 1e-300)).max())
            print("perturbation: %s stream %d: materialised GS, %s: %.3g x the element bound" % (tag, s, what, worst))
            assert worst > 1.0
