"""fp64 restatement (numpy) of ONE dense layer - norm1 + ReLU + conv1 (1x1, cin -> 128), norm2 + ReLU + conv2 (3x3, pad 1, 128 -> 32) -
and of its backward, in the engine's buffer conventions: a plane is [pixels][channels] of ONE stream, already cut to [:HW] (buffers
are [stream][HWp][C]); every BatchNorm takes its batch statistics per stream over [:HW] of the plane it is handed (training mode,
biased variance, eps 1e-5).  The block's gradient buffer is in the G' form of tests/stage_ref.py:
    G'[p][c] = sum over the consumers j of x of  gamma_j[c] * relu'_j[p][c] * dy_j[p][c],
so that layer i's finished output gradient is GS_i = bn_bwd(G'[:, slice_i], x[:, slice_i]) (gamma = 1).

Backward of layer i, in the order of csrc/backward.hip:
    DY  = relu2' * conv3x3^T(GS_i, W2)                                  conv2 data gradient with the ReLU mask         (conv2_dgrad)
    D2  = bn_bwd(DY, bt_i, gamma2)                                      norm2 backward, affine form                    (norm2_bwd)
          ... stored as fp16 units with one scale per kScaleBlock = 64 rows: held per block                          (unit_form_error)
    dbeta2 = sum DY, dgamma2 = sum DY * xhat2 over streams and pixels                                                  (norm2_affine)
    dW2 = sum GS_i^T im2col(relu(bn2(bt_i)))                            conv2 weight gradient                          (conv2_wgrad_ops)
    G'[:, c0:c1] += gamma1_l * relu1_l' * (D2_l @ W1_l[:, c0:c1])       conv1 data gradient                            (conv1_dgrad)
          per layer on the columns [cs, cin) its own group produced; once per group (i == g_lo) on [0, cs) for every layer
          l = g_lo .. g_hi of the group at once (BwdDataGroupP) - group_of / dgrad1_segments restate kGroup = 4
    dW1 = sum D2_i^T relu(bn1(x[:, :cin]))                              conv1 weight gradient                          (conv1_wgrad_ops)

tests/test_cpu_dense_ref.py proves all of it against torch modules and autograd in fp64 on a tiny dense block and shows what each
gate catches; tests/test_gpu_dense_gates.py and the two layer-product tests of tests/test_gpu_parity.py hold the kernels to it.
The *32 / *_chain builders evaluate the operands in numpy fp32 the way the kernels do (stage_ref.bn32 / bn_bwd32): they feed the
yardsticks - the fp32 multiply-add chain (helpers._fp32_chain) and the blocked fp32 reduction (helpers._fp32_blocked)."""
import numpy as np

import stage_ref as sr
from helpers import _fp32_blocked, _fp32_chain

f32 = np.float32
K_GROUP = 4                  # engine.h kGroup: dense layers per 1x1-dgrad group, counted from the TOP of the block
K_SCALE_BLOCK = 64           # gemm.cuh kScaleBlock: rows per scale of the unit-form D2 (= the plane padding granule)
GROWTH, BOTTLENECK = 32, 128
LAYERS, CIN0, CT = (6, 12, 24, 16), (64, 128, 256, 512), (256, 512, 1024, 1024)
UNIT_FORM_BOUND = 2e-5       # fp32 evaluation of the affine form + 22-bit pieces (2^-22 = 2.4e-7 of the block's maximum)

# The 3x3 data gradient of a gs_on_side layer (few streams, planes of <= 1600 pixels) applies the BN backward WHILE LOADING the G' / x
# slices: halo.cuh conv3x3_halo_dgrad_kernel -> affine2 -> bnb1 = a * fmaf(-(x - mean), k, g - q1) (gemm.cuh) with the parameters of
# grad_src_params (halo.cuh).  Its fp32 roundings, against stage_ref.bn_bwd_sum_mag:
#   a = invstd (bn_moments rounds it)                                                   1
#   q1 = (float)(s1 / HW): the cast                                                     1
#   mean (rounded), x - mean                                                            2
#   k = invstd * (float)(s2 / HW): invstd, the cast, the product                        3
#   g - q1, the fused multiply-add, the product with a                                  3
# The scale by the halo's own maximum is a power of two (exact).  The sums s1 / s2 themselves are the 1x1 data-gradient epilogues' (fp32
# within a tile, fp64 across): the yardstick's fp32 operand takes them as stage_ref.tile_sum32 forms them (gs_on_load), like the
# transition gates.
K_GS_LOAD = 1 + 1 + 2 + 3 + 3


def cin_of(block, layer):
    """input channels of dense layer (block, layer), both 1-based"""
    return CIN0[block - 1] + GROWTH * (layer - 1)


# ---- the 1x1 data gradient's layer groups (backward.hip) ------------------------------------------------------------------------------
def group_of(L, i, k_group=K_GROUP):
    """(g_lo, g_hi) of layer i (0-based) in a block of L layers, exactly as backward.hip computes them"""
    r = (L - 1 - i) % k_group
    g_lo = i - (0 if r == k_group - 1 else min(i, k_group - 1 - r))
    g_hi = L - 1 - ((L - 1 - g_lo) // k_group) * k_group
    return g_lo, g_hi


def dgrad1_segments(L, i, cin0, growth=GROWTH):
    """What lands in G' between the snapshot in front of layer i's 1x1 data gradients and the stop behind them:
    [(layers (0-based), c0, c1)] - the per-layer form on [cs, cin) and, at the bottom of a group, the grouped form on [0, cs)."""
    g_lo, g_hi = group_of(L, i)
    cs, cin = cin0 + growth * g_lo, cin0 + growth * i
    segs = []
    if cin > cs:
        segs.append(([i], cs, cin))
    if i == g_lo:
        segs.append((list(range(g_lo, g_hi + 1)), 0, cs))
    return segs


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def act64(v, g, b):
    """relu(bn(v)) in fp64"""
    return np.maximum(sr.bn_pre(v, g, b), 0.0)


act32 = sr.bn32              # the kernels' fp32 form of the same


def relu_sides(v, g, b, rows=None):
    """(on, off): the elements CLEARLY inside / outside the ReLU, pre > t resp. pre < -t with t = 1e-5 * (|x - mean| * invstd * |gamma| +
    |beta|); what lies between is borderline - its sign is the mask's business, not the product's.  Statistics over the whole plane,
    the result on `rows` (None: all)."""
    mean, inv = sr.bn_stats(v)
    v = np.asarray(v, dtype=np.float64)
    pre = (v - mean) * inv * np.asarray(g, dtype=np.float64) + np.asarray(b, dtype=np.float64)
    t = 1e-5 * (np.abs(v - mean) * inv * np.abs(g) + np.abs(b))
    if rows is not None:
        pre, t = pre[rows], t[rows]
    return pre > t, pre < -t


def excluded_share(on, off):
    """share of the elements a keep-mask built from relu_sides leaves out (the stage gates' rule: at most 1 %)"""
    return 1.0 - float((on | off).mean())


def sample(n, k=256):
    """pixel sample of a plane of n pixels: the first k, the last k and 2 k strided through it (<= 4 k, sorted, unique)"""
    if n <= 4 * k:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(k), np.arange(n - k, n), np.arange(0, n, max(1, n // (2 * k)))[:2 * k]]))


def rms(got, ref, mag, keep=None):
    r = ((np.asarray(got, dtype=np.float64) - ref) / mag) ** 2
    return float(np.sqrt((r if keep is None else r[keep]).mean()))


# ---- 3x3, pad 1 -----------------------------------------------------------------------------------------------------------------------
def _padded(a, H, W):
    C = a.shape[1]
    pad = np.zeros((H + 2, W + 2, C), dtype=a.dtype)
    pad[1:-1, 1:-1] = a.reshape(H, W, C)
    return pad


def im2col(a, H, W, pix=None, cols=None, flip=False):
    """a [H * W][C] -> [len(pix)][9 * C], tap-major (ky, kx, channel): column tap * C + c of pixel p is a[p + d(tap)][c], d = (ky - 1,
    kx - 1), zero outside the plane; flip: a[p - d(tap)][c] (the data gradient's gather).  `pix`: pixel indices (None: all), `cols`:
    sorted column indices to build (None: all) - only those are ever formed."""
    C = a.shape[1]
    pad = _padded(a, H, W)
    pix = np.arange(H * W) if pix is None else np.asarray(pix)
    y, x = pix // W, pix % W
    out = []
    for t in range(9):
        dy, dx = (2 - t // 3, 2 - t % 3) if flip else (t // 3, t % 3)
        if cols is None:
            out.append(pad[y + dy, x + dx])
        else:
            ch = cols[cols // C == t] % C
            if len(ch):
                out.append(pad[(y + dy)[:, None], (x + dx)[:, None], ch[None, :]])
    return np.concatenate(out, axis=1)


def w2_fwd_mat(w2):
    """conv2.weight [32][128][3][3] -> [32][9 * 128] in im2col's column order"""
    return np.ascontiguousarray(w2.transpose(0, 2, 3, 1).reshape(w2.shape[0], -1))


def w2_bwd_mat(w2):
    """conv2.weight [32][128][3][3] -> [128][9 * 32]: the data gradient's matrix over im2col(gs, flip=True)"""
    return np.ascontiguousarray(w2.transpose(1, 2, 3, 0).reshape(w2.shape[1], -1))


def conv3x3(a, H, W, wm, flip=False):
    """(im2col(a) @ wm^T, im2col(|a|) @ |wm|^T) over the WHOLE plane in fp64, tap by tap (the 9 C-column matrix is never formed)"""
    a = np.asarray(a, dtype=np.float64)
    C = a.shape[1]
    wm = np.asarray(wm, dtype=np.float64)
    pad, apad = _padded(a, H, W), _padded(np.abs(a), H, W)
    ref, mag = 0.0, 0.0
    for t in range(9):
        dy, dx = (2 - t // 3, 2 - t % 3) if flip else (t // 3, t % 3)
        wt = wm[:, t * C:(t + 1) * C].T
        ref = ref + pad[dy:dy + H, dx:dx + W].reshape(H * W, C) @ wt
        mag = mag + apad[dy:dy + H, dx:dx + W].reshape(H * W, C) @ np.abs(wt)
    return ref, mag


# ---- forward --------------------------------------------------------------------------------------------------------------------------
def conv1_fwd(x, g1, b1, w1):
    """x [HW][cin], w1 [128][cin] -> (bt, sum |a||w|), whole plane"""
    a = act64(x, g1, b1)
    w = np.asarray(w1, dtype=np.float64)
    return a @ w.T, a @ np.abs(w).T + 1e-300


def conv1_chain(x, g1, b1, w1, pix):
    """the fp32 chain over cin on the pixels `pix` (statistics of the whole plane)"""
    return _fp32_chain(act32(x, g1, b1)[pix], np.ascontiguousarray(w1, dtype=f32))


def conv2_fwd(bt, H, W, g2, b2, w2):
    """bt [HW][128] -> (the layer's 32 new channels, sum |a||w|), whole plane"""
    ref, mag = conv3x3(act64(bt, g2, b2), H, W, w2_fwd_mat(w2))
    return ref, mag + 1e-300


def conv2_chain(bt, H, W, g2, b2, w2, pix):
    return _fp32_chain(im2col(act32(bt, g2, b2), H, W, pix), w2_fwd_mat(w2).astype(f32))


# ---- backward: conv2 data gradient, norm2 -----------------------------------------------------------------------------------------------
def conv2_dgrad(gs, H, W, w2):
    """gs [HW][32] -> (sum_{tap, c} gs[p - d(tap)][c] * w2[c][k][tap], sum |.||.|), whole plane, WITHOUT the ReLU mask"""
    ref, mag = conv3x3(gs, H, W, w2_bwd_mat(w2), flip=True)
    return ref, mag + 1e-300


def conv2_dgrad_chain(gs32, H, W, w2, pix):
    return _fp32_chain(im2col(np.asarray(gs32, dtype=f32), H, W, pix, flip=True), w2_bwd_mat(w2).astype(f32))


def gs_on_load(gp, x):
    """The operand of a gs_on_side layer's 3x3 data gradient, which never reads the materialised GS: (fp64 GS, its fp32 evaluation with
    the statistics' fp32 tile sums, the magnitudes K_GS_LOAD counts against) from the G' and x slices of the layer's 32 channels."""
    return sr.bn_bwd(gp, x), sr.bn_bwd32(gp, x, tile_sums=True), sr.bn_bwd_sum_mag(gp, x)


def norm2_bwd(dy, bt, g2):
    """D2 from the affine form: gamma2 * invstd * (dy - mean(dy) - xhat * mean(dy * xhat))"""
    return sr.bn_bwd(dy, bt, g2)


def unit_form_error(d2, ref):
    """max over the kScaleBlock-row blocks of |d2 - ref| / (the block's max |ref|).  d2 may carry the plane's padding rows ([HWp][128]):
    the reference is zero there, as bn_bwd_apply_split_kernel writes them."""
    n = -(-len(d2) // K_SCALE_BLOCK) * K_SCALE_BLOCK
    r = np.zeros((n, ref.shape[1]))
    r[:len(ref)] = ref
    d = np.zeros((n, ref.shape[1]))
    d[:len(d2)] = d2
    blk = np.abs(r).reshape(-1, K_SCALE_BLOCK, ref.shape[1]).max(axis=(1, 2), keepdims=True)
    return float((np.abs(d - r).reshape(-1, K_SCALE_BLOCK, ref.shape[1]) / np.maximum(blk, 1e-300)).max())


def sum_blocked32(t, blk=64):
    """column sums of t [terms][C] as the blocked fp32 reduction of helpers._fp32_blocked (blk-term chains, then pairwise)"""
    t = np.ascontiguousarray(t, dtype=f32)
    return _fp32_blocked(t, np.ones((len(t), 1), dtype=f32), blk)[:, 0]


def norm2_affine(DY, BT):
    """DY, BT [streams][HW][128] -> dict: dbeta / dgamma in fp64, their sum |term|, and the fp32 terms ([streams * HW][128]) of the
    blocked yardstick: dy, and dy * xhat with xhat = (bt - mean) * invstd evaluated in fp32"""
    db = dg = dbm = dgm = 0.0
    tb, tg = [], []
    for dy, bt in zip(DY, BT):
        mean, inv = sr.bn_stats(bt)
        d64 = np.asarray(dy, dtype=np.float64)
        xh = (np.asarray(bt, dtype=np.float64) - mean) * inv
        db, dg = db + d64.sum(0), dg + (d64 * xh).sum(0)
        dbm, dgm = dbm + np.abs(d64).sum(0), dgm + np.abs(d64 * xh).sum(0)
        xh32 = ((np.asarray(bt, dtype=f32) - mean.astype(f32)) * inv.astype(f32)).astype(f32)
        tb.append(np.asarray(dy, dtype=f32))
        tg.append((np.asarray(dy, dtype=f32) * xh32).astype(f32))
    return dict(db=db, dg=dg, dbm=dbm + 1e-300, dgm=dgm + 1e-300, tb=np.concatenate(tb), tg=np.concatenate(tg))


# ---- backward: weight gradients ---------------------------------------------------------------------------------------------------------
def conv2_wgrad_ops(GS, BT, H, W, g2, b2, cols):
    """dW2[c][tap * 128 + k] = sum_{stream, p} gs[p][c] * relu(bn2(bt))[p + d(tap)][k] on the im2col columns `cols` (sorted): returns
    (Gs [streams * HW][32], A64, A32 [streams * HW][len(cols)]) - only the sampled columns are formed"""
    cols = np.asarray(cols)
    A64 = np.concatenate([im2col(act64(bt, g2, b2), H, W, cols=cols) for bt in BT])
    A32 = np.concatenate([im2col(act32(bt, g2, b2), H, W, cols=cols) for bt in BT])
    return np.concatenate([np.asarray(g, dtype=f32) for g in GS]), A64, A32


def w2_grad_mat(dw2):
    """conv2.weight.grad [32][128][3][3] -> [32][9 * 128] in im2col's column order"""
    return dw2.transpose(0, 2, 3, 1).reshape(dw2.shape[0], -1)


def conv1_wgrad_ops(D2, X, g1, b1, rows, cols):
    """dW1[k][c] = sum_{stream, p} d2[p][k] * relu(bn1(x))[p][c] on the rows k / columns c handed in: (D [streams * HW][len(rows)],
    A64, A32 [streams * HW][len(cols)])"""
    A64 = np.concatenate([act64(x[:, cols], g1[cols], b1[cols]) for x in X])
    A32 = np.concatenate([act32(x[:, cols], g1[cols], b1[cols]) for x in X])
    return np.concatenate([np.asarray(d, dtype=f32)[:, rows] for d in D2]), A64, A32


def wgrad_errors(got, a32, w64, w32, blks=(64, 512)):
    """got [M][N] against sum_k a[k][m] * w[k][n] over ALL streams x pixels (a is an fp32 buffer on both sides): (the product's err / sum
    |a||w| rms, {blk: the blocked fp32 reduction's}, the fp64 reference, sum |a||w|)"""
    a64 = np.asarray(a32, dtype=np.float64)
    ref = a64.T @ w64
    mag = np.abs(a64).T @ np.abs(w64) + 1e-300
    e_blk = {bl: rms(_fp32_blocked(np.ascontiguousarray(a32), np.ascontiguousarray(w32), bl), ref, mag) for bl in blks}
    return rms(got, ref, mag), e_blk, ref, mag


# ---- backward: conv1 data gradient, per-layer and grouped -------------------------------------------------------------------------------
def conv1_dgrad(G0, X, params, d2s, c0, c1, take=None, chain=True):
    """One stream.  G0 [HW][Ct]: G' in front of the layer's 1x1 data gradients, X [HW][Ct] the block buffer, `params` = [(gamma1, beta1,
    w1 [128][cin_l])] and `d2s` = [D2_l [HW][128]] of the segment's layers, [c0, c1) its columns, `take` the rows compared.
    Returns (reference = G0 + sum_l gamma1_l * relu1_l' * (D2_l @ W1_l), sum |term| (|G0| included), the fp32 chain (None unless `chain`),
    keep)."""
    take = slice(None) if take is None else take
    x = np.asarray(X, dtype=np.float64)[:, c0:c1]
    mean, inv = sr.bn_stats(x)
    x = x[take]
    ref = np.asarray(G0, dtype=np.float64)[take, c0:c1]
    mag = np.abs(ref) + 1e-300
    ch = np.asarray(G0, dtype=f32)[take, c0:c1].copy()
    keep = np.ones(ref.shape, dtype=bool)
    for (g1, b1, w1), d2 in zip(params, d2s):
        g1, b1, w1 = g1[c0:c1], b1[c0:c1], w1[:, c0:c1]
        d2 = np.asarray(d2)[take]
        pre = (x - mean) * inv * g1 + b1
        keep &= np.abs(pre) > 1e-5 * (np.abs(x - mean) * inv * np.abs(g1) + np.abs(b1))
        m = pre > 0
        ref = ref + g1.astype(np.float64) * m * (d2.astype(np.float64) @ w1.astype(np.float64))
        mag = mag + np.abs(g1).astype(np.float64) * m * (np.abs(d2).astype(np.float64) @ np.abs(w1).astype(np.float64))
        if chain:
            ch = (ch + (g1 * m).astype(f32) * _fp32_chain(d2.astype(f32), np.ascontiguousarray(w1.T, dtype=f32))).astype(f32)
    return ref, mag, ch if chain else None, keep
