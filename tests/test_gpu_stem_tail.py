"""The pooled-resolution stem tail (stem_tail_kernel + image moments + combine; precision mode 0, heightmap input) against the
stem-resolution pair it replaces (pool0_bwd_kernel + the stem's implicit-GEMM weight gradient over DY0, SMG_CROSSCHECK=8)
and against the fp64 oracle.  One forward + backward per child process under "deterministic": the switch is read at engine creation.

Cases: S = 640 with 2 streams (one rotation + the masked stream) and S = 672 with 3 streams, the smallest inputs the head admits.
The tail kernel walks the pooled plane in tiles of 16 x 4 pixels: the 160^2 plane of S = 640 tiles exactly (10 x 40), the 168^2
plane of S = 672 leaves a PARTIAL last tile in every tile row (10.5 tiles across).  The image-moment kernel's 16 x 16 tiles of the
stem plane are exact in both (320 = 20 x 16, 336 = 21 x 16)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import gpu, MEAN, STD, oracle_net, orc  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu

CASES = {"S640": dict(hm=224, scene=3, rots=[5], labels=[0.4], S=640),
         "S672": dict(hm=236, scene=8, rots=[2, 11], labels=[0.4, 1.6], S=672)}

_CHILD = r"""
import sys, json
import numpy as np, torch
sys.path.insert(0, %(tests)r)
import helpers                      # puts the package on the path
import synthetic, models
from helpers import orc
from trainer import Trainer
case = json.loads(%(case)r)
tr = Trainer('reinforcement', 0.5, False, None, False)
sd = synthetic.make_state_dict(orc.state_layout(1), 2)
tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
tr.model.gnum_rotations = tr.model.snum_rotations = 16
tr.optimizer.lr = 0.0
depth, masks = synthetic.heightmap_scene(case["scene"], size=case["hm"], n_boxes=8)
eng = models.get_engine(0, case["S"], 1, len(case["rots"]) + 1, len(case["rots"]))
eng.set_option("deterministic", 1)
loss, q = tr.train_batch(depth, depth * masks[0], 0, case["rots"], case["labels"], return_q=True)
assert models._ENGINES[(0, case["S"], 1)] is eng
out = {"loss": loss.cpu().numpy(), "q": q.cpu().numpy()}
for n, p in tr.model.named_parameters():
    if p.grad is not None:
        out["g:" + n] = p.grad.cpu().numpy()
np.savez(%(out)r, **out)
print("CHILD OK")
"""

CONV0, NORM0W, NORM0B = ("g:grasp_depth_trunk.features.conv0.weight", "g:grasp_depth_trunk.features.norm0.weight",
                         "g:grasp_depth_trunk.features.norm0.bias")
_RUNS = {}


def _run(case, tag, env, tmp):
    key = (case, tag)
    if key not in _RUNS:
        tests_dir = os.path.dirname(os.path.abspath(__file__))
        out = os.path.join(str(tmp), "%s_%s.npz" % (case, tag))
        e = dict(os.environ)
        e.pop("SMG_CROSSCHECK", None)
        e.update(env)
        r = subprocess.run([sys.executable, "-c", _CHILD % {"tests": tests_dir, "case": json.dumps(CASES[case]), "out": out}],
                           env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stderr[-2000:]
        with np.load(out) as z:
            _RUNS[key] = {k: z[k] for k in z.files}
    return _RUNS[key]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("stem_tail")


def _rel(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum()) / np.sqrt((b.astype(np.float64) ** 2).sum()))


def _atomic_sum(name):
    """Gradients the engine sums with fp32 atomics even under "deterministic" (test_deterministic_option_gives_bit_identical_conv_weight_
    gradients): the BatchNorm affine gradients and the head's 20x20 value convolution.  Their last bits move from run to run of ONE build."""
    return name.startswith("g:") and (".norm" in name or "-norm" in name or "val-conv1" in name or name.endswith(".bias"))


def _same_outside_the_tail(a, b, what):
    """Everything but the tail's three tensors: Q, the losses and every gradient "deterministic" makes bit-reproducible (the 120 other
    convolution weights of the trunk and the head's conv0) bit for bit; the atomically summed ones within the run-to-run bound the
    project holds them to (2e-5 of the tensor's norm + 1e-7 of the largest norm) - measured on the MI355X, S = 640: the stem-resolution
    tail against itself differs in those tensors' last bits too, so bit-identity there is not a property any tail can have."""
    tail = (CONV0, NORM0W, NORM0B)
    exact = [k for k in a if k not in tail and not _atomic_sum(k)]
    assert len(exact) == 120 + 2, len(exact)
    differing = [k for k in exact if not np.array_equal(a[k], b[k])]
    assert not differing, (what, differing[:8])
    loose = [k for k in a if k not in tail and _atomic_sum(k)]
    gmax = max(float(np.sqrt((a[k].astype(np.float64) ** 2).sum())) for k in loose)
    worst = 0.0
    for k in loose:
        d = float(np.sqrt(((a[k].astype(np.float64) - b[k].astype(np.float64)) ** 2).sum()))
        nr = float(np.sqrt((a[k].astype(np.float64) ** 2).sum()))
        worst = max(worst, d / (2e-5 * nr + 1e-7 * gmax))
        assert d <= 2e-5 * nr + 1e-7 * gmax, (what, k, d, nr)
    n_diff = len([k for k in loose if not np.array_equal(a[k], b[k])])
    print("%s: %d tensors bit-identical; %d atomically summed tensors, %d of them differ, worst at %.3f of the run-to-run bound" % (what, len(exact), len(loose), n_diff, worst))


@pytest.mark.parametrize("case", sorted(CASES))
def test_pooled_tail_agrees_with_stem_resolution_tail(gpu, workdir, case):
    """conv0.weight / norm0.weight / norm0.bias within 5e-3 of the tensor's norm between the two tails (the bound between alternative
    kernel paths, test_alternative_kernel_paths_agree); nothing else moves: the tail is a leaf (_same_outside_the_tail)."""
    new = _run(case, "new", {}, workdir)
    old = _run(case, "old", {"SMG_CROSSCHECK": "8"}, workdir)
    assert sorted(new) == sorted(old)
    assert len([k for k in new if k.startswith("g:")]) == 368
    for k in (CONV0, NORM0W, NORM0B):
        r = _rel(new[k], old[k])
        print("%s %s: |pooled - stem-resolution| / |stem-resolution| = %.3e" % (case, k[2:], r))
        assert r <= 5e-3, (k, r)
    _same_outside_the_tail(new, old, case + " pooled vs stem-resolution")


@pytest.mark.parametrize("case", sorted(CASES))
def test_pooled_tail_is_bit_reproducible(gpu, workdir, case):
    """Two runs of the pooled tail: its three tensors bit for bit (fixed-order partial tiles and fp64 sums, no fp32 atomics)."""
    a = _run(case, "new", {}, workdir)
    b = _run(case, "new2", {}, workdir)
    for k in (CONV0, NORM0W, NORM0B):
        assert np.array_equal(a[k], b[k]), k
    _same_outside_the_tail(a, b, case + " pooled, two runs")


@pytest.mark.parametrize("case", sorted(CASES))
def test_pooled_tail_error_against_fp64_oracle(gpu, workdir, case):
    """conv0.weight's gradient against the fp64 oracle: the pooled tail's error within 1.5x the stem-resolution tail's on the same
    inputs (both are fp32-class; the pooled form drops one rounding of x)."""
    import copy
    import synthetic
    c = CASES[case]
    new = _run(case, "new", {}, workdir)
    old = _run(case, "old", {"SMG_CROSSCHECK": "8"}, workdir)
    depth, masks = synthetic.heightmap_scene(c["scene"], size=c["hm"], n_boxes=8)
    x = orc.preprocess(depth, [MEAN] * 3, [STD] * 3)
    mx = orc.preprocess(depth * masks[0], [MEAN] * 3, [STD] * 3)
    assert x.shape[-1] == c["S"]
    o64 = copy.deepcopy(oracle_net(2)).double()
    o64.zero_grad()
    trunk = getattr(o64, orc.STYLE_TRUNK[0]).features
    head = getattr(o64, orc.STYLE_HEAD[0])
    total = 0.0
    for rot, label in zip(c["rots"], c["labels"]):
        q = head(torch.cat((trunk(orc.rotate(x, rot, 16).double()), trunk(mx.double())), 1))
        total = total + orc.huber(q[0, 0, 0, 0], label).sum()
    total.backward()
    g64 = dict(o64.named_parameters())[CONV0[2:]].grad.numpy()
    e_new, e_old = _rel(new[CONV0], g64), _rel(old[CONV0], g64)
    print("%s conv0.weight gradient vs fp64 oracle: pooled tail %.3e, stem-resolution tail %.3e (ratio %.2f)" % (case, e_new, e_old, e_new / e_old))
    assert e_new <= 1.5 * e_old, (e_new, e_old)
