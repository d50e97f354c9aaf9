"""What the operator-level gate modules (test_gpu_dense_gates.py, test_gpu_stage_gates.py, test_gpu_storage_gates.py) share, each once:
the scenes and the plane geometry they select, the context of one scene on one net (forward, read-back, stopped backward, parameter
lookup), the gates themselves and the variant-selection rules of the walk.  Importable without a GPU; tests/test_cpu_gate_harness.py
pins it there.  Nothing here is written to after import: every module keeps its nets, contexts and read-back buffers in its own
namespace - engine state shared between modules through a helper is how the affine-gradient scratch bug
(test_a_stopped_backward_leaves_nothing_in_the_affine_gradient_scratch) went unseen."""
import numpy as np
import torch

import dense_ref as dr
import stage_ref as sr
from helpers import _WGRAD_BLK, _WGRAD_GATE, MEAN, STD, gpu  # noqa: F401  (gpu: the fixture, for the modules to import by name)

TRUNK, HEAD = "grasp_depth_trunk.features.", "graspnet_val.grasp-val-"
CT = (256, 512, 1024, 1024)
_DQ = [1.0, -1.0, 0.5, 1e-6, -0.25, 0.75, -0.5, 0.3]
# heightmap scene (synthetic.heightmap_scene(seed, size, 8 boxes): the depth plane and its first mask), rotations (streams = rotations +
# the masked stream, pairs = rotations) and the dq the backward gates feed, [pair][Q pixels]
SCENES = {"S640x6": dict(seed=0, size=224, S=640, rots=[0, 3, 7, 10, 13], dq=[[1.0], [-1.0], [0.5], [1e-6], [-0.25]]),      # sample 3: 20 binades low
          "S672x3": dict(seed=8, size=236, S=672, rots=[2, 11], dq=[[1.0, -0.5, 0.25, -2.0], [-0.75, 1.5, -1e-3, 0.4]]),
          "S640x2": dict(seed=0, size=224, S=640, rots=[3], dq=[[1.0]]),                                                    # the single-sample step
          "S640x17": dict(seed=0, size=224, S=640, rots=list(range(16)), dq=[[_DQ[j % 8]] for j in range(16)])}            # forward chains of 8 and 9
# the dense-layer stops of the 16-bit backward gates (test_gpu_storage_gates.test_backward_layer; test_cpu_storage_ref shows their keep-masks'
# 1 % cap on the CPU), (block, layer) 1-based by geometry: every block, a top of a group (per-layer form only), a bottom of a four-layer
# group (nseg = 4), a block's first layer, block 4's last layer
BWD_LAYERS16 = {"S640": [(1, 3), (2, 6), (3, 21), (4, 1), (4, 16)], "S672": [(1, 6), (2, 9), (3, 24), (4, 13), (4, 16)]}
# by S: H and HWp of the stem plane and of blocks 1-4 (eng.H[1:6] / eng.HWp[1:6]); HWp % 128 picks the 128-row or the 64-row configuration.
# Plane indices everywhere: 0 = input, 1 = stem, 2..5 = blocks 1..4 (a dense layer of `block` lives on plane 1 + block).
GEOMETRY = {640: ([320, 160, 80, 40, 20], [102400, 25600, 6400, 1600, 448]),
            672: ([336, 168, 84, 42, 21], [112896, 28288, 7104, 1792, 448])}


class GateCtx:
    """One scene on one net: heightmaps, stream / pair layout, and after forward() the engine.  H[plane] / HWp[plane] come from GEOMETRY
    (forward() asserts the engine's against them); HWp[0], the input plane's, is the engine's own and known after forward()."""

    def __init__(self, net, sd, scene, gpu, mode=None):
        import synthetic
        self.net, self.sd, self.gpu, self.mode, self.eng = net, sd, gpu, mode, None
        self.S, self.rots, self.dq = scene["S"], scene["rots"], scene["dq"]
        depth, masks = synthetic.heightmap_scene(scene["seed"], size=scene["size"], n_boxes=8)
        self.hm = torch.from_numpy(np.stack([depth, depth * masks[0]])).to(gpu)
        self.NS, self.NP = len(self.rots) + 1, len(self.rots)
        self.pa, self.pb = list(range(self.NP)), [self.NS - 1] * self.NP
        self.H, self.HWp = [self.S] + GEOMETRY[self.S][0], [None] + GEOMETRY[self.S][1]

    def forward(self):
        import models
        q = self.net.run(0, self.rots, 16, heightmaps=self.hm, mean=MEAN, std=STD, keep_for_backward=True)
        torch.cuda.synchronize()
        self.eng = models._ENGINES[(0, self.S, self.net.HEAD_OUT)]
        if self.mode is not None:
            assert self.eng.precision == self.mode
        assert list(self.eng.H[1:6]) == self.H[1:] and list(self.eng.HWp[1:6]) == self.HWp[1:], (self.eng.H, self.eng.HWp)
        self.HWp[0] = int(self.eng.HWp[0])
        return q

    def rd(self, name, rows, plane, C, streams=None, pad=False):
        """[rows][HW][C] of a [rows][HWp][C] buffer on `plane` (16-bit buffers arrive widened to fp32); streams: those of the rows only;
        pad: all HWp rows"""
        HW, HWp = self.H[plane] ** 2, self.HWp[plane]
        a = self.eng.debug_read(name, count=rows * HWp * C).reshape(rows, HWp, C)
        a = a if streams is None else a[streams]
        return a if pad else np.ascontiguousarray(a[:, :HW])

    def backward_to(self, stop):
        """a fresh forward, then the backward up to `stop` (honoured in every mode); returns the gradients the walk has finished"""
        q = self.forward()
        dq = torch.tensor(self.dq, dtype=torch.float32, device=self.gpu).view(q.shape)
        self.net.zero_grad()
        self.eng.set_option("debug_stop", stop)
        try:
            self.net._engine_backward(self.net._saved[1], dq)
        finally:
            self.eng.set_option("debug_stop", -1)
        torch.cuda.synchronize()
        return {n: p.grad.detach().cpu().numpy() for n, p in self.net.named_parameters() if p.grad is not None}

    def tp(self, name):
        return self.sd[TRUNK + name]

    def hp(self, name):
        return self.sd[HEAD + name]

    def lp(self, block, layer, name):
        return self.sd[TRUNK + "denseblock%d.denselayer%d.%s" % (block, layer, name)]


# ---- the gates -----------------------------------------------------------------------------------------------------------------------------
def gate(what, e_prod, e_yard, factor, e_whole=None, n=0, yard="fp32 yardstick"):
    msg = "%s: err/sum|ab| rms product %.3e, %s %.3e: ratio %.2f" % (what, e_prod, yard, e_yard, e_prod / e_yard)
    if e_whole is not None:
        msg += "; whole plane %.3e: ratio %.2f" % (e_whole, e_whole / e_yard)
    print(msg + (" (%d elements)" % n if n else ""))
    assert e_prod <= factor * e_yard, (what, e_prod, e_yard)
    if e_whole is not None:
        assert e_whole <= factor * e_yard, (what, "whole plane", e_whole, e_yard)


def wgrad_gate(what, got, a64, w64, blocked, blks, yard="blocked fp32 (chains + pairwise)"):
    """got [M][N] = sum_k a[k][m] * w[k][n] over ALL streams x pixels, on the rows / columns handed in; blocked(blk): the yardstick's
    reduction of the same product in chains of blk terms, evaluated for the lengths `blks` only"""
    ref = a64.T @ w64
    mag = np.abs(a64).T @ np.abs(w64) + 1e-300
    e_blk = {bl: dr.rms(blocked(bl), ref, mag) for bl in blks}
    e_prod = dr.rms(got, ref, mag)
    print("%s: err/sum|ab| rms product %.3e, %s %s over all %d terms, %d elements: ratio%s %s"
          % (what, e_prod, yard, " / ".join("%d-term %.3e" % (bl, e_blk[bl]) for bl in blks), a64.shape[0], ref.size, "s" if len(blks) > 1 else "",
             " / ".join("%.2f" % (e_prod / e_blk[bl]) for bl in blks)))
    assert e_prod <= _WGRAD_GATE * e_blk[_WGRAD_BLK], (what, e_prod, e_blk)


def elementwise(what, got, ref, mag, k, slack=None):
    """max |err| against (k * mag + slack) * 2^-24: k = the fp32 roundings on the kernel's path, slack = what the fp32 strip sums of the
    forward statistics add (stage_ref.bn_stat_slack; None where the statistics are fp64 sums of the elements).  An element whose bound
    is 0 must be exact.  Prints the error in roundings of mag as well."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    bound = k * mag if slack is None else k * mag + slack
    r = float((err / (bound + 1e-300)).max())
    print("%s: max |err| / mag = %.2f x 2^-24; at %.2f of the bound (%d roundings of mag%s)"
          % (what, float((err / (mag + 1e-300)).max() / sr.U), r / sr.U, k, "" if slack is None else " + the statistics' strip sums"))
    assert r <= sr.U, (what, r / sr.U, k)


def bounded(what, got, ref, bound):
    """max |err| / bound <= 1 (an element whose bound is 0 must be exact)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    r = float((err / (bound + 1e-300)).max())
    print("%s: max |err| at %.3f of the bound" % (what, r))
    assert r <= 1.0, (what, r)


# ---- the variant-selection rules of the walk ---------------------------------------------------------------------------------------------------
def halo_tile(H, ns):
    return 16 if ((H + 15) // 16) ** 2 * ns >= 200 else 8                     # wgrad_plan.h halo_tile (no precision in it)


def forward_chains(NS, H1):
    return [NS // 2, NS - NS // 2] if NS >= 2 and NS * H1 * H1 >= 200000 else [NS]      # forward.hip two_chains


def transition_cfg(HWp_next):
    return "P128x128" if HWp_next % 128 == 0 else "P64x128"                   # forward.hip: by the OUTPUT plane's padding


def conv1_fwd_cfg(HWp, ns, mode0):
    """forward conv1 (forward.hip, small_wgs = 320): the wave-specialised kernel is `e->prec == 0` only; modes 1 / 2 choose between the
    three generic configurations"""
    wg128, wg64 = ns * HWp // 128, ns * HWp // 64 * 2
    big = HWp % 128 == 0 and wg128 >= 320
    if mode0 and not big and wg64 >= 320 and HWp % 64 == 0:
        return "ws"
    return "P128x128" if big else ("P32x64" if wg64 < 320 else "P64x64")
