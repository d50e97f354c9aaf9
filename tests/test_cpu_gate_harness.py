"""tests/gate_harness.py where there is no GPU: the variant tables of the GPU gate modules derived from the geometry table alone with
the expressions those modules use on eng.H / eng.HWp, the gates at their edges (ratio exactly the factor, one step above it, a bound
of zero), the printed line of each gate (profiles/*_gates.txt are raw outputs people diff against), and GateCtx.rd on a stub engine."""
import numpy as np
import pytest
import torch

import gate_harness as gh
import stage_ref as sr
from helpers import _fp32_blocked
from test_gpu_dense_gates import CASES as DENSE_CASES, VARIANTS
from test_gpu_storage_gates import CASES as STORAGE_CASES, VARIANTS16


def _layout(scene):
    """NS and H / HWp by plane index (0 = input, 1 = stem, 2..5 = blocks 1..4), as GateCtx holds them"""
    H, HWp = gh.GEOMETRY[scene["S"]]
    return len(scene["rots"]) + 1, [scene["S"]] + H, [None] + HWp


# ---- the variant tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(DENSE_CASES))
def test_the_dense_variant_table_follows_from_the_geometry(case):
    NS, xH, xHWp = _layout(DENSE_CASES[case])
    chains = gh.forward_chains(NS, xH[2])
    assert chains == ([8, 9] if case == "D" else [NS])
    got = []
    for b in range(4):
        H, HWp = xH[2 + b], xHWp[2 + b]
        c1, t_f = {gh.conv1_fwd_cfg(HWp, ns, True) for ns in chains}, {gh.halo_tile(H, ns) for ns in chains}
        assert len(c1) == 1 and len(t_f) == 1, (case, b, c1, t_f)
        t_b = gh.halo_tile(H, NS)
        got.append((c1.pop(), t_f.pop(), t_b, t_b == 16 and H % 16 != 0, NS <= 4 and H * H <= 1600))
    w1 = ["ws" if NS > 4 or H * H > 1600 else "atomics" for H in xH[2:]]
    assert (got, w1) == VARIANTS[case]


@pytest.mark.parametrize("case", sorted(STORAGE_CASES))
def test_the_16_bit_variant_table_follows_from_the_geometry(case):
    NS, xH, xHWp = _layout(STORAGE_CASES[case])
    chains = gh.forward_chains(NS, xH[2])
    blocks = []
    for b in range(4):
        H, HWp = xH[2 + b], xHWp[2 + b]
        c1, ts = {gh.conv1_fwd_cfg(HWp, ns, False) for ns in chains}, {gh.halo_tile(H, ns) for ns in chains}
        assert len(c1) == 1 and len(ts) == 1, (case, b, c1, ts)
        t = ts.pop()
        blocks.append((c1.pop(), t, t == 16 and H % 16 != 0))
    got = (blocks, [gh.transition_cfg(xHWp[3 + b]) for b in range(3)], "P128x64" if xHWp[1] % 128 == 0 else "P64x64", "P128x64" if xHWp[5] % 128 == 0 else "P64x64")
    assert got == VARIANTS16[case]


def test_halo_tile_at_its_200_tile_threshold():
    assert ((160 + 15) // 16) ** 2 * 2 == 200 and gh.halo_tile(160, 2) == 16          # case C, block 1: exactly 200 tiles
    assert ((80 + 15) // 16) ** 2 * 6 == 150 and gh.halo_tile(80, 6) == 8             # case A, block 2
    assert gh.halo_tile(168, 3) == 16 and gh.halo_tile(80, 8) == 16 and gh.halo_tile(80, 7) == 8      # 363, 200 and 175 tiles


# ---- the gates ---------------------------------------------------------------------------------------------------------------------------------
def test_gate_at_and_above_its_factor(capsys):
    gh.gate("t", 2.0, 1.0, 2.0)
    gh.gate("t", 1.0, 1.0, 2.0, e_whole=2.0, n=7, yard="storage chain")
    assert capsys.readouterr().out == ("t: err/sum|ab| rms product 2.000e+00, fp32 yardstick 1.000e+00: ratio 2.00\n"
                                       "t: err/sum|ab| rms product 1.000e+00, storage chain 1.000e+00: ratio 1.00; whole plane 2.000e+00: ratio 2.00 (7 elements)\n")
    over = float(np.nextafter(2.0, 3.0))
    with pytest.raises(AssertionError):
        gh.gate("t", over, 1.0, 2.0)
    with pytest.raises(AssertionError, match="whole plane"):
        gh.gate("t", 1.0, 1.0, 2.0, e_whole=over)


def test_elementwise_and_bounded_at_their_bounds():
    ref, mag = np.array([1.0, 0.0]), np.array([1.0, 0.0])
    gh.elementwise("t", ref + [4 * sr.U, 0.0], ref, mag, 4)                             # at the bound; the element of bound 0 exact
    gh.elementwise("t", ref + [4 * sr.U, 0.0], ref, mag, 3, slack=np.array([1.0, 0.0]))
    with pytest.raises(AssertionError):
        gh.elementwise("t", ref + [5 * sr.U, 0.0], ref, mag, 4)                         # one rounding over
    with pytest.raises(AssertionError):
        gh.elementwise("t", ref + [0.0, 1e-40], ref, mag, 4)                            # bound 0: must be exact
    bound = np.array([1e-3, 0.0])
    gh.bounded("t", bound, np.zeros(2), bound)
    with pytest.raises(AssertionError):
        gh.bounded("t", [np.nextafter(1e-3, 1.0), 0.0], np.zeros(2), bound)
    with pytest.raises(AssertionError):
        gh.bounded("t", [0.0, 1e-40], np.zeros(2), bound)


def test_wgrad_gate_on_a_192_term_reduction(capsys):
    rng = np.random.default_rng(0)
    a32, w32 = rng.standard_normal((192, 8)).astype(np.float32), rng.standard_normal((192, 8)).astype(np.float32)
    a64, w64, calls = a32.astype(np.float64), w32.astype(np.float64), []

    def blocked(blk):
        calls.append(blk)
        return _fp32_blocked(a32, w32, blk)
    gh.wgrad_gate("t", _fp32_blocked(a32, w32, 64), a64, w64, blocked, (64,))          # the yardstick itself: ratio 1
    assert calls == [64]
    one = capsys.readouterr().out
    assert one.startswith("t: err/sum|ab| rms product ") and one.endswith(" over all 192 terms, 64 elements: ratio 1.00\n")
    assert ", blocked fp32 (chains + pairwise) 64-term " in one and "512-term" not in one
    with pytest.raises(AssertionError):
        gh.wgrad_gate("t", _fp32_blocked(a32[:128], w32[:128], 64), a64, w64, blocked, (64, 512), yard="blocked reduction over the bf16 operands")      # a chain dropped
    assert calls == [64, 64, 512]
    two = capsys.readouterr().out
    assert ", blocked reduction over the bf16 operands 64-term " in two and " / 512-term " in two and " elements: ratios " in two


# ---- GateCtx -----------------------------------------------------------------------------------------------------------------------------------
class _Engine:
    def debug_read(self, name, count=None):
        self.asked = (name, count)
        return np.arange(count, dtype=np.float32)


def test_rd_cuts_a_padded_plane_by_the_plane_index_convention():
    sd = {gh.TRUNK + "norm5.weight": 5, gh.HEAD + "conv0.weight": 0, gh.TRUNK + "denseblock4.denselayer16.conv1.weight": 416}
    x = gh.GateCtx(None, sd, gh.SCENES["S672x3"], torch.device("cpu"))
    assert (x.NS, x.NP, x.pa, x.pb) == (3, 2, [0, 1], [2, 2]) and tuple(x.hm.shape) == (2, 236, 236)
    assert (x.tp("norm5.weight"), x.hp("conv0.weight"), x.lp(4, 16, "conv1.weight")) == (5, 0, 416)
    assert (x.H[0], x.H[1], x.H[1 + 4], x.HWp[1 + 4]) == (672, 336, 21, 448)             # input, stem, block 4: 448 rows for 441 pixels
    x.eng = _Engine()
    a = x.rd("x4", 3, 5, 4)
    assert x.eng.asked == ("x4", 3 * 448 * 4) and a.shape == (3, 441, 4)
    n, p, c = np.meshgrid(np.arange(3), np.arange(441), np.arange(4), indexing="ij")
    assert np.array_equal(a, (n * 448 + p) * 4 + c)
    full = x.rd("x4", 3, 5, 4, pad=True)
    assert full.shape == (3, 448, 4) and np.array_equal(full[:, :441], a) and full[2, 447, 3] == 3 * 448 * 4 - 1
    assert np.array_equal(x.rd("x4", 3, 5, 4, streams=[0, 2]), a[[0, 2]]) and np.array_equal(x.rd("x4", 3, 5, 4, [2], pad=True), full[[2]])
    assert x.rd("stem", 2, 1, 64).shape == (2, 336 * 336, 64)                           # an unpadded plane: HWp = HW
