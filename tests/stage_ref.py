"""fp64 restatements (numpy) of the stages around the dense layers - stem conv0, norm0 + ReLU + pool0, the transitions, norm5 + the
two-stream concat, the head's norm0 + ReLU + conv0 - and of their backward, in the engine's buffer conventions: planes are
[pixels][channels] of ONE stream (or pair), already cut to [:HW]; gradients of the block buffers are in the G' form
    G'[p][c] = sum over the consumers j of x of  gamma_j[c] * relu'_j[p][c] * dy_j[p][c],
from which the gradient with respect to x is bn_bwd(G', x): invstd * (G' - mean(G') - xhat * mean(G' * xhat)).
Every function takes its batch statistics from the plane it is handed (training-mode BatchNorm: biased variance, eps 1e-5).

tests/test_cpu_stage_ref.py proves these against torch modules and autograd in fp64; tests/test_gpu_stage_gates.py holds the kernels
to them.  The *32 functions evaluate the same operand formulas in numpy fp32 the way the kernels do (statistics from fp64 sums,
rounded once; centered form): they feed the fp32-chain yardsticks and the checks of the rounding counts K_*."""
import numpy as np

EPS = 1e-5
U = 2.0 ** -24          # unit roundoff of fp32
f32 = np.float32


# ---- BatchNorm, forward --------------------------------------------------------------------------------------------------------------
def bn_stats(v):
    """per-channel (mean, invstd) of one plane [pixels][C] in fp64"""
    v = np.asarray(v, dtype=np.float64)
    return v.mean(0), 1.0 / np.sqrt(v.var(0) + EPS)


def bn_pre(v, g, b):
    """gamma * xhat + beta in fp64 (no ReLU)"""
    mean, inv = bn_stats(v)
    return (np.asarray(v, dtype=np.float64) - mean) * (inv * np.asarray(g, dtype=np.float64)) + np.asarray(b, dtype=np.float64)


def bn_mag(v, g, b):
    """the magnitudes that cancel in bn_pre: (|x| + |mean|) * |gamma * invstd| + |beta|"""
    mean, inv = bn_stats(v)
    return (np.abs(np.asarray(v, dtype=np.float64)) + np.abs(mean)) * np.abs(inv * np.asarray(g, dtype=np.float64)) + np.abs(np.asarray(b, dtype=np.float64))


def bn_keep(v, g, b):
    """the borderline-ReLU rule of the dense-layer gates: |pre| > 1e-5 * (|x - mean| * invstd * |gamma| + |beta|)"""
    mean, inv = bn_stats(v)
    pre = bn_pre(v, g, b)
    sc = np.abs(np.asarray(v, dtype=np.float64) - mean) * inv * np.abs(g) + np.abs(b)
    return np.abs(pre) > 1e-5 * sc


def bn32(v, g, b, relu=True):
    """the kernels' fp32 form: mean and gamma * invstd from the fp64 statistics, rounded once; (x - mean) * sc + beta"""
    mean, inv = bn_stats(v)
    sc = (np.asarray(g, dtype=np.float64) * inv).astype(f32)
    out = ((np.asarray(v, dtype=f32) - mean.astype(f32)) * sc + np.asarray(b, dtype=f32)).astype(f32)
    return np.maximum(out, f32(0)) if relu else out


# ---- stem conv0: 7x7, stride 2, pad 3, no bias -------------------------------------------------------------------------------------------
def stem_cols(img, rows):
    """im2col of the output rows `rows` (an index array): img [H][W][Cin] -> [len(rows) * W/2][49 * Cin], tap-major (ky, kx, channel)"""
    H, W, Cin = img.shape
    Wo = W // 2
    pad = np.zeros((H + 6, W + 6, Cin), dtype=img.dtype)
    pad[3:-3, 3:-3] = img
    rows = np.asarray(rows)
    cols = [pad[(2 * rows + ky)[:, None], (2 * np.arange(Wo) + kx)[None, :]] for ky in range(7) for kx in range(7)]
    return np.concatenate(cols, axis=-1).reshape(len(rows) * Wo, 49 * Cin)


def stem_wmat(w):
    """conv0.weight [64][Cin][7][7] -> [64][49 * Cin] in the column order of stem_cols"""
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1))


def stem_conv(img, w, rows):
    """(reference, sum |a||w|) of the stem's output rows `rows`: [len(rows) * W/2][64] each"""
    c = stem_cols(np.asarray(img, dtype=np.float64), rows)
    wm = stem_wmat(np.asarray(w, dtype=np.float64))
    return c @ wm.T, np.abs(c) @ np.abs(wm).T


# ---- norm0 + ReLU + max pool 3 / 2 / 1 --------------------------------------------------------------------------------------------------
def pool_windows(a, H, W, fill):
    """the <= 9 values of every 3x3 / stride 2 / pad 1 window: a [H * W][C] -> [9][(H/2) * (W/2)][C], `fill` outside the plane"""
    C = a.shape[1]
    pad = np.full((H + 2, W + 2, C), fill, dtype=a.dtype)
    pad[1:-1, 1:-1] = a.reshape(H, W, C)
    Ho, Wo = H // 2, W // 2
    return np.stack([pad[ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2].reshape(Ho * Wo, C) for ky in range(3) for kx in range(3)])


def maxpool3s2(a, H, W):
    pad = np.full((H + 2, W + 2, a.shape[1]), -np.inf, dtype=a.dtype)
    pad[1:-1, 1:-1] = a.reshape(H, W, -1)
    Ho, Wo = H // 2, W // 2
    out = pad[0:2 * Ho:2, 0:2 * Wo:2].copy()
    for ky in range(3):
        for kx in range(3):
            np.maximum(out, pad[ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2], out=out)
    return out.reshape(Ho * Wo, -1)


def pool0(stem, H, W, g, b):
    """(reference, mag): window maximum of the fp64 relu(bn(stem)); an element's mag is the largest bn_mag of its window"""
    return maxpool3s2(np.maximum(bn_pre(stem, g, b), 0.0), H, W), maxpool3s2(bn_mag(stem, g, b), H, W)


def pool0_32(stem, H, W, g, b):
    return maxpool3s2(bn32(stem, g, b), H, W)


# ---- transition: norm + ReLU + conv 1x1 + average pool 2 ------------------------------------------------------------------------------------
def avgpool2(a, H, W):
    """[H * W][C] -> [(H/2) * (W/2)][C]; the four pixels added in the kernels' order ((y, x) + (y, x+1)) + (y+1, x)) + (y+1, x+1)"""
    v = a.reshape(H, W, -1)
    s = ((v[0::2, 0::2] + v[0::2, 1::2]).astype(a.dtype) + v[1::2, 0::2]).astype(a.dtype)
    s = (s + v[1::2, 1::2]).astype(a.dtype)
    return (s * a.dtype.type(0.25)).reshape((H // 2) * (W // 2), -1)


def transition_fwd(x, H, W, g, b, w):
    """the reference's order: conv (w [Cout][Cin]) of relu(bn(x)), then the pool"""
    return avgpool2(np.maximum(bn_pre(x, g, b), 0.0) @ np.asarray(w, dtype=np.float64).T, H, W)


def pooled_act(x, H, W, g, b):
    """the kernels' order, operand of the 1x1: avgpool2(relu(bn(x))) in fp64"""
    return avgpool2(np.maximum(bn_pre(x, g, b), 0.0), H, W)


def pooled_act32(x, H, W, g, b):
    return avgpool2(bn32(x, g, b), H, W)


# ---- norm5 + concat, head norm0 + ReLU + conv0 ------------------------------------------------------------------------------------------------
def feat(x4, g5, b5, pair_a, pair_b):
    """x4 [streams][HW][C] -> (F [pairs][HW][2 C], mag): norm5 (no ReLU) of the pair's rotation stream | of its masked stream"""
    n5 = [bn_pre(x, g5, b5) for x in x4]
    m5 = [bn_mag(x, g5, b5) for x in x4]
    F = np.stack([np.concatenate([n5[a], n5[b]], axis=1) for a, b in zip(pair_a, pair_b)])
    M = np.stack([np.concatenate([m5[a], m5[b]], axis=1) for a, b in zip(pair_a, pair_b)])
    return F, M


def feat32(x4, g5, b5, pair_a, pair_b):
    n5 = [bn32(x, g5, b5, relu=False) for x in x4]
    return np.stack([np.concatenate([n5[a], n5[b]], axis=1) for a, b in zip(pair_a, pair_b)])


def head_conv0(Fj, g0, b0, w0):
    """one pair: h1 = relu(bn0(F_j)) @ w0^T with the statistics of THAT pair's plane; returns (h1, the fp64 operand)"""
    a = np.maximum(bn_pre(Fj, g0, b0), 0.0)
    return a @ np.asarray(w0, dtype=np.float64).T, a


# ---- BatchNorm, backward ----------------------------------------------------------------------------------------------------------------
def bn_bwd_terms(dy, x, gamma=None):
    """The BN backward in the kernels' centered form  a * ((dy - q1) - (x - mean) * k)  with a = gamma * invstd, q1 = mean(dy),
    k = invstd * mean(dy * xhat): returns (a, q1, mean, k)."""
    mean, inv = bn_stats(x)
    dy = np.asarray(dy, dtype=np.float64)
    xh = (np.asarray(x, dtype=np.float64) - mean) * inv
    a = inv if gamma is None else inv * np.asarray(gamma, dtype=np.float64)
    return a, dy.mean(0), mean, inv * (dy * xh).mean(0)


def bn_bwd(dy, x, gamma=None):
    """gradient with respect to the input x of y = gamma * xhat + beta, given dy; gamma None = 1: the G' -> dx form"""
    a, q1, mean, k = bn_bwd_terms(dy, x, gamma)
    return a * ((np.asarray(dy, dtype=np.float64) - q1) - (np.asarray(x, dtype=np.float64) - mean) * k)


def bn_bwd_mag(dy, x, gamma=None):
    """the magnitudes of the three cancelling terms of bn_bwd: |a| * (|dy| + |q1| + |x - mean| * |k|)"""
    a, q1, mean, k = bn_bwd_terms(dy, x, gamma)
    return np.abs(a) * (np.abs(np.asarray(dy, dtype=np.float64)) + np.abs(q1) + np.abs(np.asarray(x, dtype=np.float64) - mean) * np.abs(k))


def bn_bwd_sum_mag(dy, x, gamma=None):
    """bn_bwd_mag with the two means taken as what the kernels SUM in fp32 (mean |dy|, mean |dy * xhat|) and the subtraction x - mean
    at its operands' size: |a| * (|dy| + mean|dy| + (|x| + |mean|) * invstd * mean|dy * xhat|).  The bound of a stage whose q1 / k
    come from fp32 partial sums (the rounding count then includes the length of those partial sums)."""
    mean, inv = bn_stats(x)
    dy = np.abs(np.asarray(dy, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    a = inv if gamma is None else np.abs(inv * np.asarray(gamma, dtype=np.float64))
    return a * (dy + dy.mean(0) + (np.abs(x) + np.abs(mean)) * inv * (dy * np.abs((x - mean) * inv)).mean(0))


def tile_sum32(t):
    """Sum over the pixels of t [HW][C] the way the data-gradient epilogues (BwdDataP::epilogue, gemm.cuh) form a backward statistic:
    per lane a sequential fp32 sum over its 16 rows of a tile, the partials of a 64-row tile then added pairwise in fp32
    (block_col_reduce), the tiles' sums in fp64 (atomics)."""
    t = np.asarray(t, dtype=f32)
    HW, C = t.shape
    n = -(-HW // 64) * 64
    p = np.zeros((n, C), dtype=f32)
    p[:HW] = t
    p = p.reshape(n // 64, 4, 16, C)
    acc = np.zeros((n // 64, 4, C), dtype=f32)
    for r in range(16):
        acc = (acc + p[:, :, r]).astype(f32)
    tile = ((acc[:, 0] + acc[:, 1]).astype(f32) + (acc[:, 2] + acc[:, 3]).astype(f32)).astype(f32)
    return tile.astype(np.float64).sum(0)


def bn_bwd32(dy, x, gamma=None, tile_sums=False):
    """the kernels' fp32 evaluation (affine2): the four coefficients rounded once - from fp64 sums, or (tile_sums) q1 and k from
    sums of dy and dy * xhat formed as tile_sum32 forms them, which is how the engine comes by them"""
    a, q1, mean, k = bn_bwd_terms(dy, x, gamma)
    dy, x = np.asarray(dy, dtype=f32), np.asarray(x, dtype=f32)
    if tile_sums:
        inv = bn_stats(x)[1]
        xh = ((x - mean.astype(f32)) * inv.astype(f32)).astype(f32)
        q1 = tile_sum32(dy) / len(dy)
        k = inv * (tile_sum32((dy * xh).astype(f32)) / len(dy))
    a, q1, mean, k = a.astype(f32), q1.astype(f32), mean.astype(f32), k.astype(f32)
    return (a * ((dy - q1) - (x - mean) * k).astype(f32)).astype(f32)


# ---- transition, backward ------------------------------------------------------------------------------------------------------------------
def unpool2(a, H, W):
    """[(H/2) * (W/2)][C] -> [H * W][C]: every pooled pixel to the four it covers (no factor)"""
    v = a.reshape(H // 2, W // 2, -1)
    return np.repeat(np.repeat(v, 2, axis=0), 2, axis=1).reshape(H * W, -1)


def transition_bwd(x, H, W, g, b, w, x_next, gp_next):
    """Transition x [H * W][Cp] -> x_next[:, :C0] (w [C0][Cp]).  gp_next = G' of x_next's first C0 channels.
    Returns (G' contribution to x: gamma * relu' * 1/4 * unpool(dX @ w), dX [HW/4][C0], relu mask)."""
    dX = bn_bwd(gp_next, x_next)
    on = bn_pre(x, g, b) > 0
    return np.asarray(g, dtype=np.float64) * on * 0.25 * unpool2(dX @ np.asarray(w, dtype=np.float64), H, W), dX, on


def transition_wgrad(xs, H, W, g, b, dXs):
    """dW [C0][Cp] = sum over streams and pooled pixels of dX[q][k] * avgpool2(relu(bn(x)))[q][c]"""
    return sum(dX.T @ pooled_act(x, H, W, g, b) for x, dX in zip(xs, dXs))


# ---- head conv0 + norm5, backward ----------------------------------------------------------------------------------------------------------
def head_conv0_bwd(h1j, dh1j, Fj, g1, g0, b0, w0):
    """one pair: (df = relu'(bn0(F)) * (A @ w0), A = bn_bwd(dh1, h1, gamma1), relu mask, the weight gradient's summand A^T @ relu(bn0(F)))"""
    A = bn_bwd(dh1j, h1j, g1)
    pre = bn_pre(Fj, g0, b0)
    on = pre > 0
    return on * (A @ np.asarray(w0, dtype=np.float64)), A, on, A.T @ np.maximum(pre, 0.0)


def norm5_bwd(x4, F, DF, g0, g5, pair_a, pair_b):
    """x4 [streams][HW][C], F / DF [pairs][HW][2 C] -> (G'_4 [streams][HW][C] = gamma5 * dy5, dy5, mag of dy5 (bn_bwd_sum_mag
    summed over the users), dbeta5, dgamma5, the two sums' sum |term|)."""
    NS, C = len(x4), x4[0].shape[1]
    dy5 = [np.zeros(x4[0].shape, dtype=np.float64) for _ in range(NS)]
    mag = [np.zeros(x4[0].shape, dtype=np.float64) for _ in range(NS)]
    for j, (a, b) in enumerate(zip(pair_a, pair_b)):
        for s, half in ((a, slice(0, C)), (b, slice(C, 2 * C))):
            dy5[s] += bn_bwd(DF[j][:, half], F[j][:, half], g0[half])
            mag[s] += bn_bwd_sum_mag(DF[j][:, half], F[j][:, half], g0[half])
    db = sum(d.sum(0) for d in dy5)
    dbm = sum(m.sum(0) for m in mag)
    dg, dgm = 0.0, 0.0
    for s in range(NS):
        mean, inv = bn_stats(x4[s])
        dg = dg + (dy5[s] * ((x4[s].astype(np.float64) - mean) * inv)).sum(0)
        dgm = dgm + (mag[s] * ((np.abs(x4[s].astype(np.float64)) + np.abs(mean)) * inv)).sum(0)
    g5 = np.asarray(g5, dtype=np.float64)
    return np.stack([g5 * d for d in dy5]), np.stack(dy5), np.stack(mag), db, dg, dbm, dgm


def norm5_bwd32(x4, F, DF, g0, g5, pair_a, pair_b):
    """the same in numpy fp32, users added in order: (G'_4, dbeta5, dgamma5) - the check of the rounding counts"""
    NS, C = len(x4), x4[0].shape[1]
    dy5 = [np.zeros(x4[0].shape, dtype=f32) for _ in range(NS)]
    for j, (a, b) in enumerate(zip(pair_a, pair_b)):
        for s, half in ((a, slice(0, C)), (b, slice(C, 2 * C))):
            dy5[s] = (dy5[s] + bn_bwd32(DF[j][:, half], F[j][:, half], g0[half])).astype(f32)
    db, dg = np.zeros(C, dtype=f32), np.zeros(C, dtype=f32)
    for s in range(NS):
        mean, inv = bn_stats(x4[s])
        xh = ((np.asarray(x4[s], dtype=f32) - mean.astype(f32)) * inv.astype(f32)).astype(f32)
        db = (db + dy5[s].sum(0, dtype=f32)).astype(f32)
        dg = (dg + (dy5[s] * xh).astype(f32).sum(0, dtype=f32)).astype(f32)
    return np.stack([(np.asarray(g5, dtype=f32) * d).astype(f32) for d in dy5]), db, dg


# ---- rounding counts of the element-wise stages (fp32 roundings on the kernel's path, counted from csrc/elem.cuh and csrc/gemm.cuh) -----
# pool0_kernel / feat_kernel: bn_moments rounds mean and invstd to fp32 (2), gamma * invstd (1), then bn1 = fmaf(x - mean, sc, beta):
# the subtraction (1) and the fused multiply-add (1).  The maximum and the ReLU round nothing.  Against bn_mag.
K_BN = 5
# norm5_bwd_kernel, one user's BN-corrected dF (bnb1 = a * fmaf(-(x - mean), k, g - q1)), against bn_bwd_sum_mag:
#   a = hgamma * invstd: invstd rounded (1), the product (1)                                                      2
#   q1 = (float)(f1 / HW): the cast (1) + f1 itself, which the head's data-gradient epilogue sums in fp32 over the
#        64 rows of its tile (CfgP64x128: HWp = 448 is no multiple of 128) before the fp64 atomics: <= 63 adds   64
#   x - mean: mean rounded (1), the subtraction (1)                                                               2
#   k = invstd * q2: invstd (1), the cast of q2 (1), the product (1), f2's 63 fp32 adds, and each of its terms
#       dy * ((x - mean) * invstd) rounds 5 times more (mean, subtraction, invstd, two products)                  71
#   g - q1 (1), the fused multiply-add (1), the product with a (1)                                                3
K_DY5_USER = 2 + 64 + 2 + 71 + 3


def k_g4(users):
    """G'_4 = sum over the users of gamma5 * dy: the product with gamma5 (1) and one add per user - in registers per phase, then
    (p0 + p1) + (p2 + p3) across the four phases, which is no more adds than users (+ 2 for the fixed tree on few users)"""
    return K_DY5_USER + 1 + users + 2


def k_sums5(HW, single_streams, has_multi):
    """dbeta5 / dgamma5: every term carries K_DY5_USER and, for dgamma5, xhat5 = (x - mean5) * inv5 and the product (5: mean5, the
    subtraction, inv5, two products).  A thread adds its terms in fp32: <= 5 chunks x 16 pixels = 80 on a single-user stream, users / 4 x
    16 + the 2 adds of the phase tree on the shared one (<= 80 up to 19 users).  Then one fp32 atomicAdd per (stream, workgroup) onto the
    gradient array: ceil(chunks / 5) per single-user stream, `chunks` for the shared stream."""
    chunks = (HW + 15) // 16
    return K_DY5_USER + 5 + 80 + single_streams * ((chunks + 4) // 5) + (chunks if has_multi else 0)


def strip_sum_slack(v, n_whole):
    """What the FORWARD statistics of a plane cost where its producer is a whole tile of the implicit-GEMM forward (FwdConvP::epilogue,
    gemm.cuh: the stem plane, the transitions' output channels): there the sums are not fp64 sums of the elements but, per lane, fp32
    sums of dx = x - s and dx^2 over a strip of 16 rows about the strip's first value s, widened to fp64 once per strip
    (sum x = S1 + 16 s, sum x^2 = S2 + 2 s S1 + 16 s^2).  A strip is the rows 4 h + {0..3, 8..11, 16..19, 24..27} (h = 0, 1) of a block of
    32 consecutive pixels.  Per strip: each dx rounds once and S1 adds 15 times: |delta S1| <= 16 u sum |dx|; S2 = 16 fused multiply-adds
    of dx^2 (dx rounded): |delta S2| <= 18 u sum dx^2.  The variance E[x^2] - mean^2 sees delta S2 + 2 (s - mean) delta S1.
    `n_whole`: the plane's leading pixels that lie in whole tiles (the rest is summed per element in fp64; the 3x3 kernels' channels
    too: hand in 0).  Returns per channel (M, R) with  |delta mean| <= M u  and  |delta invstd| / invstd <= R u."""
    v = np.asarray(v, dtype=np.float64)
    mean, inv = bn_stats(v)
    if n_whole == 0:
        return np.zeros(v.shape[1]), np.zeros(v.shape[1])
    w = v[:n_whole].reshape(n_whole // 32, 32, -1)
    first = 4 * ((np.arange(32) // 4) % 2)
    s = w[:, first, :]
    dx = np.abs(w - s)
    M = 16.0 * dx.sum((0, 1)) / len(v)
    V = (18.0 * dx * dx + 32.0 * np.abs(s - mean) * dx).sum((0, 1)) / len(v)
    return M, 0.5 * V * inv * inv


def bn_stat_slack(v, g, n_whole):
    """the element-wise bound's share of strip_sum_slack, in units of u: |gamma * invstd| * (M + |x - mean| * R)"""
    mean, inv = bn_stats(v)
    M, R = strip_sum_slack(v, n_whole)
    return np.abs(np.asarray(g, dtype=np.float64) * inv) * (M + np.abs(np.asarray(v, dtype=np.float64) - mean) * R)
