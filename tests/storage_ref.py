"""The 16-bit yardstick of the storage-mode gates (tests/test_gpu_storage_gates.py): numpy models of what precision modes 1 ('bf16':
bf16 storage of activations and gradients, one bf16 MFMA term per product) and 2 ('fp16': fp16 activations and forward products,
bf16 gradients and backward products) round, and where.  tests/test_cpu_storage_ref.py proves them on the CPU (rounding against
torch bit for bit, the storage chain against a torch 16-bit matmul, what each gate still catches, the keep-mask shares).

Every rounding point below was read out of the kernel source; the citation stands next to the code that models it:
  * every fp32 -> 16-bit conversion of the library is round-to-nearest-even: gemm.cuh pack_bf16 / pack_f16 are
    __builtin_convertvector of a float pair (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32), st1 casts through them or through (_Float16),
    stq / store_acc_rows / pack_unit / split4<1 | 2> go through pack2.  No store truncates (there is no round-toward-zero pack in csrc/).
  * the A operand: the kernel forms it in fp32 - BN + ReLU of the stored input (bnrelu4, for fp16 operands clamped to 65504:
    bnrelu4<H = true>, gemm.cuh kH), the 2 x 2 average of four of them (F_POOL / W_POOL), or the BN-corrected gradient (affine2) - and
    rounds it ONCE to the operand type when it stages it (pack_unit<OP> / split4<OP>, OP = fwd_op / bwd_op_plain of the mode);
  * the weights: pack_weights_kernel (elem.cuh) rounds each fp32 weight once, to `prec` for the forward packs and to bf16 for the
    data-gradient packs; PK_STEM1 first rounds the fp64 sum of the three channel weights to fp32;
  * the accumulator is fp32 (v_mfma_f32_32x32x16_bf16 / _f16); the epilogue rounds it once to the destination's storage type
    (FwdConvP::epilogue st1 / store_acc_rows<DstT>, the halo forward's stq<ST>, BwdDataP::epilogue stq<GT> / st1<GT>).  The
    destinations stem, feat, h1, df and dh1 are fp32 buffers in every mode (F32IO policies; smg_debug_read converts only x*, g*, bt*).

The statistics trap.  Every producer of a 16-bit plane sums its BatchNorm statistics from the fp32 values BEFORE the 16-bit store:
  * FwdConvP::epilogue (gemm.cuh): whole tiles sum dx = acc - s and dx^2 from the accumulator registers, partial tiles (double)acc;
    the store of the same registers rounds afterwards (conv1 -> bt, the transitions -> x<t+1>[:, :C0]);
  * conv3x3_halo_fwd_kernel (halo.cuh): `xd = (double)v[k]` of the accumulator, then stq<ST> (conv2 -> x<b>[:, cin:cin+32]);
  * pool0_kernel (elem.cuh): `s[c] += (double)best[c]` of the fp32 maximum, after stq<XT> of the same values (x1[:, :64]);
  * bn_stat_kernel only turns the fp64 sums into mean / invstd: it inherits its producer's form.
  feat_kernel writes fp32 and sums what it wrote: the head's statistics are those of the stored values in every mode.
The gates recompute each stage from the buffer the kernel read, with fp64 statistics over the STORED values, so the engine's mean
and invstd differ from the reference's by what rounding did to the plane.  store_stat_slack bounds that: |x_stored - x| <= h, half a
storage ulp per element, hence |delta mean| <= mean(h) and |delta var| <= 2 mean(|x - mean| h) + mean(h^2).  The element-wise gates
add it to their bound (bn_store_slack, xhat_sum_slack), the keep-mask widens by it (keep16 / keep_s); no factor is widened.  Where the
values before the store follow from an fp32 buffer - pool0's channels of x1, from the stem plane - the engine's statistics are
recomputed instead of bounded (plane_stats / x1_stats): the product gates then need no slack.  The backward gates of the dense layers
go one step further (second half of this file): smg_debug_read hands out the engine's forward sums (fs_bt, fs_x), and the reference
takes the engine's OWN statistics (engine_stats)."""
import numpy as np

import dense_ref as dr
import stage_ref as sr
from helpers import _fp32_blocked, _fp32_chain

f32 = np.float32
F16_MAX = 65504.0            # gemm.cuh kF16Max
# per mode (models.set_precision name): storage of activations / of gradients, operand type of the forward / backward products
MODES = {"bf16": dict(act="bf16", grd="bf16", fwd="bf16", bwd="bf16"),       # engine.h prec 1: ActT<1> / GrdT<1> = e_bf16, fwd_op(1) = bwd_op(1) = 1
         "fp16": dict(act="fp16", grd="bf16", fwd="fp16", bwd="bf16")}       # prec 2: ActT<2> = e_f16, GrdT<2> = e_bf16, fwd_op(2) = 2, bwd_op(2) = 1
MANT = {"bf16": 8, "fp16": 11}      # significand bits, the hidden one included


# ---- rounding ----------------------------------------------------------------------------------------------------------------------------
def round_bf16(x):
    """fp32 -> bf16 -> fp32, round-to-nearest-even on the bits (v_cvt_pk_bf16_f32): add 0x7FFF + the lowest kept bit, cut 16 bits; NaN
    stays NaN (quiet), inf stays inf, the largest finite values round up to inf"""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    r = ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000))
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, (u | np.uint32(0x00400000)) & np.uint32(0xFFFF0000), r).astype(np.uint32).view(f32)


def round_fp16(x):
    """fp32 -> fp16 -> fp32, round-to-nearest-even on the bits (v_cvt_pk_f16_f32): subnormals below 2^-14 in steps of 2^-24, everything
    from 65520 up becomes inf"""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    sign = u & np.uint32(0x80000000)
    a = (u & np.uint32(0x7FFFFFFF)).view(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        # subnormal range (|x| < 2^-14): |x| * 2^24 < 2^10 is exact, and adding 2^23 - where fp32's ulp is 1 - rounds it to the nearest
        # integer, ties to even, in fp32's own arithmetic; the subtraction and the scaling back are exact
        sub = (((a * f32(2.0 ** 24)) + f32(2.0 ** 23)) - f32(2.0 ** 23)) * f32(2.0 ** -24)
        au = a.view(np.uint32)
        nrm = ((au + (np.uint32(0xFFF) + ((au >> np.uint32(13)) & np.uint32(1)))) & np.uint32(0xFFFFE000)).view(f32)
        nrm = np.where(nrm >= f32(65520.0), f32(np.inf), nrm)
    out = np.where(a < f32(2.0 ** -14), sub, nrm)
    out = np.where(np.isnan(a), f32(np.nan), out).astype(f32)
    return (out.view(np.uint32) | sign).view(f32)


def rnd(x, kind):
    """round an fp32 array once to `kind` ('bf16' / 'fp16'; None or 'fp32': left as it is)"""
    x = np.asarray(x, dtype=f32)
    return round_bf16(x) if kind == "bf16" else round_fp16(x) if kind == "fp16" else x


def half_ulp(v, kind):
    """half a unit in the last place of `kind` at |v| (fp64 in, fp64 out): what one rounding to storage can move a value of that size;
    below fp16's normal range the ulp is the subnormal step 2^-24"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.frexp(np.maximum(v, 1e-300))[1] - 1                      # floor(log2 |v|)
    e = np.maximum(e, -14 if kind == "fp16" else -126)
    return np.ldexp(0.5, e - (MANT[kind] - 1))


# ---- operands and products -------------------------------------------------------------------------------------------------------------------
def operand(a32, kind):
    """the A operand as the kernel stages it: the fp32 value, clamped to fp16's largest finite value where it becomes an fp16 operand
    (bnrelu4<H>: v_med3_f32(., 0, 65504) - in-range values untouched), rounded once (pack_unit<OP>)"""
    a32 = np.asarray(a32, dtype=f32)
    return rnd(np.minimum(a32, f32(F16_MAX)) if kind == "fp16" else a32, kind)


def storage_chain(a32, w32, op, dst=None):
    """out[m][n] = sum_k a[m][k] * w[n][k]: operands rounded once to `op` (the A operand handed in is the fp32 value the kernel forms;
    the weight as pack_weights_kernel packs it), accumulated as helpers._fp32_chain does, the result rounded once to the destination's
    storage type `dst` (None: an fp32 buffer)"""
    return rnd(_fp32_chain(operand(a32, op), rnd(w32, op)), dst)


def storage_blocked(a32, w32, op_a, op_w, blk=64):
    """out[m][n] = sum_k a[k][m] * w[k][n] over a long k (the weight gradients): both operands rounded once to their operand types,
    reduced as helpers._fp32_blocked does; the weight gradient itself is fp32 in every mode"""
    return _fp32_blocked(np.ascontiguousarray(operand(a32, op_a)), np.ascontiguousarray(operand(w32, op_w)), blk)


def conv2_chain(bt, H, W, g2, b2, w2, pix, op, dst):
    """the storage chain of a dense layer's 3x3: BN + ReLU of the stored bottleneck rounded once per element (the halo kernel packs the
    halo once: conv3x3_halo_fwd_kernel s_store -> pack_unit<OP>; zero padding applies after it), the PK_HF weights rounded to `op`"""
    return storage_chain(dr.im2col(dr.act32(bt, g2, b2), H, W, pix), dr.w2_fwd_mat(w2).astype(f32), op, dst)


def stored_bound(ref, k, mag, kind, slack=0.0):
    """bound of an element-wise stage whose result is stored in `kind`: the mode-0 bound k * 2^-24 * mag (+ slack, absolute) on the fp32
    value, plus half a storage ulp at the largest value that bound allows"""
    b32 = k * sr.U * np.asarray(mag, dtype=np.float64) + slack
    return b32 + half_ulp(np.abs(ref) + b32, kind)


# ---- statistics summed before the 16-bit store -----------------------------------------------------------------------------------------------
def store_stat_slack(v, kind):
    """v [pixels][C]: a plane as STORED in `kind`, whose producer summed the unrounded fp32 values.  Per channel (M, R) with
    |mean_engine - mean(v)| <= M  and  |invstd_engine / invstd(v) - 1| <= R  (derivation in the module docstring; R from
    invstd' / invstd = 1 / sqrt(1 - delta_var * invstd^2) at the largest delta_var)."""
    v = np.asarray(v, dtype=np.float64)
    mean, inv = sr.bn_stats(v)
    h = half_ulp(v, kind)
    M = h.mean(0)
    dvar = 2.0 * (np.abs(v - mean) * h).mean(0) + (h * h).mean(0)
    t = np.minimum(dvar * inv * inv, 0.75)
    return M, 1.0 / np.sqrt(1.0 - t) - 1.0


def bn_store_slack(v, g, kind):
    """what store_stat_slack moves gamma * (x - mean) * invstd + beta by, per element, in absolute units"""
    v = np.asarray(v, dtype=np.float64)
    mean, inv = sr.bn_stats(v)
    M, R = store_stat_slack(v, kind)
    return np.abs(np.asarray(g, dtype=np.float64) * inv) * (M * (1.0 + R) + np.abs(v - mean) * R)


def xhat_sum_slack(dy, v, S):
    """What the statistics' slack moves sum_p dy[p] * xhat[p] by (a BatchNorm weight gradient over a 16-bit plane v), per channel.  With
    the engine's mean_e = mean - d and invstd_e = (1 + r) invstd:  xhat_e = (1 + r) (xhat + d * invstd), so the sum moves by EXACTLY
    r * sum(dy * xhat) + (1 + r) d invstd sum(dy):  <= R |sum dy xhat| + (1 + R) M invstd |sum dy|  - the two sums as they cancel, not
    their terms' magnitudes (behind a BatchNorm both are what eps leaves of them)."""
    dy, v = np.asarray(dy, dtype=np.float64), np.asarray(v, dtype=np.float64)
    xh = (v - S.mean) * S.inv
    return S.R * np.abs((dy * xh).sum(0)) + (1.0 + S.R) * S.M * S.inv * np.abs(dy.sum(0))


def keep16(v, g, b, kind):
    """the borderline-ReLU rule of the data-gradient gates for a 16-bit plane: stage_ref.bn_keep's threshold plus bn_store_slack - an
    element whose pre-activation the engine's statistics can carry across zero is the mask's business, not the product's"""
    mean, inv = sr.bn_stats(v)
    pre = sr.bn_pre(v, g, b)
    sc = np.abs(np.asarray(v, dtype=np.float64) - mean) * inv * np.abs(g) + np.abs(b)
    return np.abs(pre) > 1e-5 * sc + bn_store_slack(v, g, kind)


# ---- BN + ReLU of a 16-bit plane with the statistics the ENGINE holds, as far as they can be known ------------------------------------------
class PlaneStats:
    """per channel: mean, invstd (fp64) and the slack (M, R) of store_stat_slack - zero where the engine's statistics are known"""
    def __init__(self, mean, inv, M, R):
        self.mean, self.inv, self.M, self.R = mean, inv, M, R

    def cols(self, c):
        return PlaneStats(self.mean[c], self.inv[c], self.M[c], self.R[c])


def plane_stats(v, kind, known=None):
    """Statistics of the stored plane v [pixels][C] with their slack.  known = (channel slice, the plane's values BEFORE the store on
    those channels, recomputed to fp32 accuracy from an fp32 buffer): there the engine's statistics are those of that plane, no slack.
    The one such case is x1[:, :64]: pool0_kernel's fp32 maxima follow from the fp32 stem plane (x1_stats).  It matters: a rotated or
    masked heightmap is mostly one background value, which rounds ONE way on thousands of pixels - the engine's mean sits up to half a
    storage ulp off the stored plane's, and (x - mean) * invstd of exactly those background pixels is the small difference of the two."""
    mean, inv = sr.bn_stats(v)
    M, R = store_stat_slack(v, kind)
    if known is not None:
        c, pre = known
        mean, inv, M, R = mean.copy(), inv.copy(), M.copy(), R.copy()
        mean[c], inv[c] = sr.bn_stats(pre)
        M[c] = R[c] = 0.0
    return PlaneStats(mean, inv, M, R)


def x1_stats(x1, stem, Hs, g0, b0, kind):
    """x1 [HW1][256] as stored, stem [Hs * Hs][64] the fp32 stem plane of the same stream: channels 0..63 are pool0's, whose fp32 values
    before the store are stage_ref.pool0_32 of the stem (K_BN fp32 roundings from the kernel's: nothing at 16-bit resolution)"""
    pre = sr.pool0_32(stem, Hs, Hs, g0, b0)
    assert pre.shape == (len(x1), 64)
    return plane_stats(x1, kind, known=(slice(0, 64), pre))


def bn_pre_s(v, g, b, S):
    """gamma * (x - mean) * invstd + beta in fp64 with the statistics S"""
    return (np.asarray(v, dtype=np.float64) - S.mean) * (S.inv * np.asarray(g, dtype=np.float64)) + np.asarray(b, dtype=np.float64)


def act64_s(v, g, b, S):
    return np.maximum(bn_pre_s(v, g, b, S), 0.0)


def act32_s(v, g, b, S):
    """stage_ref.bn32 with the statistics S: mean and gamma * invstd rounded once, (x - mean) * sc + beta, ReLU"""
    sc = (np.asarray(g, dtype=np.float64) * S.inv).astype(f32)
    return np.maximum(((np.asarray(v, dtype=f32) - S.mean.astype(f32)) * sc + np.asarray(b, dtype=f32)).astype(f32), f32(0))


def slack_s(v, g, S):
    """bn_store_slack with the statistics S (zero on the channels whose statistics are known)"""
    return np.abs(np.asarray(g, dtype=np.float64) * S.inv) * (S.M * (1.0 + S.R) + np.abs(np.asarray(v, dtype=np.float64) - S.mean) * S.R)


def keep_s(v, g, b, S):
    """keep16 with the statistics S"""
    sc = np.abs(np.asarray(v, dtype=np.float64) - S.mean) * S.inv * np.abs(g) + np.abs(b)
    return np.abs(bn_pre_s(v, g, b, S)) > 1e-5 * sc + slack_s(v, g, S)


# ---- the dense layers' BACKWARD in the 16-bit modes ----------------------------------------------------------------------------------------
# In modes 1 / 2 the backward of a dense layer runs (backward.hip, `split16` false): conv3x3_halo_dgrad_kernel<16 | 8, PREC, edge> on the
# MATERIALISED gs_ (calls of more than 4 streams: gs_materialised = NS > 4; bn_bwd_apply_kernel<PREC> at C = 32 wrote it) or with the BN
# backward applied ON LOAD (affine2 of the G' / x slices, then pack_unit<OP>: halo.cuh s_store), bn_bwd_apply_kernel<PREC> at C = 128 IN
# PLACE on the ring slot that holds the raw 3x3 data gradient, conv3x3_halo_wgrad_kernel, BwdWeightP<.., W_ONE>, and the two
# read-modify-write 1x1 data gradients BwdDataP<.., E_ACCUM> / BwdDataGroupP.  Where each rounds:
#   * gradients are bf16 in both modes (engine.h GrdT<1 | 2> = e_bf16) and every backward product takes bf16 operands (bwd_op_plain);
#   * the 3x3 data gradient: operand GS as stored (bf16: no further rounding) or the fp32 affine2 rounded once (pack_unit<OP>), the PK_HD
#     weights rounded to bf16 (pack_weights_kernel), fp32 accumulators, the ReLU mask from the forward's fp32 table (bn1(x, mean, sc, be) >
#     0), one rounding by stq<GT> (halo.cuh epilogue: `dyv = in && bn1(..) > 0 ? acc : 0`, `s1 += dyv`, then stq<GT>: the sums s1 / s2 of
#     norm2 see the fp32 dyv, the slot its bf16 rounding);
#   * the norm2 backward in place: affine2 of the stored dy2 and the stored bottleneck in fp32, rounded once (elem.cuh bn_bwd_apply_kernel:
#     pack_unit<1>), rows < HW only (`r < a.pl.HW`);
#   * the 1x1 data gradients: D2 as stored, the PK_D1 pack rounded to bf16, fp32 accumulators, mask and gamma in fp32, `gold + gam * dy`
#     (BwdDataP::epilogue) or `gold + run` with run the fp32 sum over the group's segments (BwdDataGroupP::epilogue), ONE rounding to bf16
#     (st1<GT> / store_acc_rows<GT>), rows p < pa.HW only;
#   * the weight gradients: both operands rounded to bf16 when staged (GS / D2 are bf16 already), fp32 reduction.
# The statistics: the backward's per-layer kernels read (mean, invstd) of x<b> and of the bottleneck from the fp32 table the forward
# finished - "the very floats bn_moments would produce from the fp64 sums" (gemm.cuh StatTab): mean = (float)(sum / n), invstd =
# (float)(1 / sqrt(var + eps)).  debug_read("fs_x<b>") / ("fs_bt<b>_<l>") hand out those sums, so the reference takes the engine's OWN
# statistics (engine_stats) and the keep-mask's margin is the table's fp32 rounding and nothing more.

# bn_bwd_apply_kernel<PREC> at C = 128 behind the halo data gradient, against bn_bwd_sum_mag_s; ts = the halo tile (16 or 8): the halo
# epilogue sums s1 / s2 in fp32 over the ts * ts pixels of its tile (per lane, then shfl, then across the waves: ts^2 - 1 adds whatever
# the tree), then fp64 atomics.  As stage_ref.K_DY5_USER counts the same affine2 with 64-row tile sums:
#   a = gamma * invstd: invstd rounded (1), the product (1)                                              2
#   q1 = (float)(s1 / HW): the cast (1) + the tile's ts^2 - 1 fp32 adds                                  ts^2
#   x - mean: mean rounded (1), the subtraction (1)                                                      2
#   k = invstd * q2: invstd (1), the cast (1), the product (1), ts^2 - 1 adds, and each term
#       dyv * ((x - mean) * invstd) rounds 5 times (mean, subtraction, invstd, two products)             ts^2 + 7
#   g - q1 (1), the fused multiply-add (1), the product with a (1)                                       3
def k_d2_apply(ts):
    return 2 + ts * ts + 2 + (ts * ts + 7) + 3


# norm2's dbeta / dgamma in the 16-bit modes: bn_bwd_apply_kernel adds (float)s1[n] / (float)s2[n] per stream with one fp32 atomic each
# (elem.cuh: affine_sink_add2 under blockIdx.x == 0): per term the tile's ts^2 - 1 fp32 adds, for dgamma the 5 roundings of
# dyv * ((x - mean) * invstd); then the cast (1) and NS - 1 atomic adds.  Against sum |term|.
def k_affine2(ts, ns, gamma):
    return (ts * ts - 1) + (5 if gamma else 0) + 1 + (ns - 1)


# bn_bwd_apply_kernel<PREC> at C = 32 (the MATERIALISED GS) for block 4's LAST layer, against bn_bwd_sum_mag_s of the G' / x slices.  Its
# slice of G' has been stored exactly ONCE when the layer runs - by norm5_bwd_kernel (elem.cuh), which also summed s1 / s2 - so what the
# store did to the sums is derivable (sums_before_store_slack with h = half a bf16 ulp of gsnap).  Every lower layer's slice has been
# read-modify-written by the layers above it, each store rounding a running value that no buffer keeps: no slack can be derived there, and
# those layers' GS is gated with the engine's own sums instead (gs_from_sums, above).  norm5_bwd_kernel: a thread sums dd over its pixels in fp32 (<= 80
# terms: 5 chunks x 16 pixels on a single-user stream, users / 4 x 16 + 2 on the shared one: stage_ref.k_sums5), multiplies by gamma5,
# fp64 atomics from there; the stored value is sum over the users of fl(gamma5 * dd) (1 + users roundings).
#   a = invstd (the table's rounding)                                                                    1
#   q1 = (float)(s1 / HW): the cast (1), gamma5 * s1 (1), 79 adds, the stored terms' own 1 + users       82 + users
#   x - mean: mean rounded (1), the subtraction (1)                                                      2
#   k = invstd * q2: invstd, the cast, the product (3), gamma5 * s2 (1), 79 adds, 1 + users, and each
#       term dd * ((x - mean5) * inv5) rounds 5 times                                                    89 + users
#   g - q1 (1), the fused multiply-add (1), the product with a (1)                                       3
def k_gs_top(users):
    return 1 + (82 + users) + 2 + (89 + users) + 3


# bn_bwd_apply_kernel<PREC> at C = 32 (the MATERIALISED GS) at ANY layer, with the sums s1 / s2 the kernel read handed in (debug_read
# "bs_x<b>": the backward arena's fp64 sums of the block buffer; the stopped layer's own 1x1 data gradients add to columns [0, cin) only,
# so those of its slice [cin, cin + 32) are what the apply read).  grad_src_coef / bnb1 (gemm.cuh), as dense_ref.K_GS_LOAD counts them:
#   a = 1.f * invstd (the table's rounding)                 1
#   q1 = (float)(s1 / HW): the cast                         1
#   mean (the table's rounding), x - mean                   2
#   k = invstd * (float)(s2 / HW): invstd, cast, product    3
#   g - q1, the fused multiply-add, the product with a      3
# against |a| (|g| + |q1| + (|x| + |mean|) |k|).  No slack: nothing of the reference is taken from a rounded buffer's sums.
K_GS_APPLY = 1 + 1 + 2 + 3 + 3


def gs_from_sums(gp, x, S, bs, HW):
    """gp, x [HW][32]: the stored G' / x slices, S their forward statistics (engine_stats), bs [2][32] the engine's s1 | s2 of the slice:
    (fp64 GS = invstd * ((g - s1 / HW) - (x - mean) * invstd * s2 / HW), the magnitudes K_GS_APPLY counts against)"""
    g, x = np.asarray(gp, dtype=np.float64), np.asarray(x, dtype=np.float64)
    q1, k = np.asarray(bs[0], dtype=np.float64) / HW, S.inv * np.asarray(bs[1], dtype=np.float64) / HW
    return S.inv * ((g - q1) - (x - S.mean) * k), S.inv * (np.abs(g) + np.abs(q1) + (np.abs(x) + np.abs(S.mean)) * np.abs(k))


def engine_stats(fs, HW):
    """fs [2][C]: the engine's fp64 sums (sum | sumsq) of one stream's plane -> PlaneStats with mean and invstd as bn_moments forms
    them in fp64 (gemm.cuh), and as slack the one fp32 rounding of each on their way into the table"""
    mean = np.asarray(fs[0], dtype=np.float64) / HW
    inv = 1.0 / np.sqrt(np.maximum(np.asarray(fs[1], dtype=np.float64) / HW - mean * mean, 0.0) + sr.EPS)
    return PlaneStats(mean, inv, np.abs(mean) * sr.U, np.full(mean.shape, sr.U))


def plane_sums(v):
    """[sum | sumsq][C] in fp64 of a plane: what fs_* would hold had the producer summed the stored values"""
    v = np.asarray(v, dtype=np.float64)
    return np.stack([v.sum(0), (v * v).sum(0)])


def bn_bwd_terms_s(dy, x, S, gamma=None):
    """stage_ref.bn_bwd_terms with the statistics S of x: (a, q1, mean, k)"""
    dy = np.asarray(dy, dtype=np.float64)
    xh = (np.asarray(x, dtype=np.float64) - S.mean) * S.inv
    a = S.inv if gamma is None else S.inv * np.asarray(gamma, dtype=np.float64)
    return a, dy.mean(0), S.mean, S.inv * (dy * xh).mean(0)


def bn_bwd_s(dy, x, S, gamma=None):
    a, q1, mean, k = bn_bwd_terms_s(dy, x, S, gamma)
    return a * ((np.asarray(dy, dtype=np.float64) - q1) - (np.asarray(x, dtype=np.float64) - mean) * k)


def bn_bwd_sum_mag_s(dy, x, S, gamma=None):
    """stage_ref.bn_bwd_sum_mag with the statistics S"""
    dy = np.abs(np.asarray(dy, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    a = S.inv if gamma is None else np.abs(S.inv * np.asarray(gamma, dtype=np.float64))
    return a * (dy + dy.mean(0) + (np.abs(x) + np.abs(S.mean)) * S.inv * (dy * np.abs((x - S.mean) * S.inv)).mean(0))


def bn_bwd32_s(dy, x, S, gamma=None, tile_sums=True):
    """stage_ref.bn_bwd32 with the statistics S (affine2 in fp32, the coefficients rounded once; q1 and k from engine-style tile sums)"""
    a, q1, mean, k = bn_bwd_terms_s(dy, x, S, gamma)
    dy, x = np.asarray(dy, dtype=f32), np.asarray(x, dtype=f32)
    if tile_sums:
        xh = ((x - mean.astype(f32)) * S.inv.astype(f32)).astype(f32)
        q1 = sr.tile_sum32(dy) / len(dy)
        k = S.inv * (sr.tile_sum32((dy * xh).astype(f32)) / len(dy))
    a, q1, mean, k = a.astype(f32), q1.astype(f32), mean.astype(f32), k.astype(f32)
    return (a * ((dy - q1) - (x - mean) * k).astype(f32)).astype(f32)


def gs_on_load16(gp, x, S):
    """The GS operand of the 3x3 kernels where it is NOT materialised (calls of <= 4 streams): (the fp64 GS, the fp32 affine2 of the G' /
    x slices with engine-style tile sums rounded once to the backward operand type bf16 - halo.cuh s_store: pack_unit<OP>(affine2(..)))"""
    return bn_bwd_s(gp, x, S), rnd(bn_bwd32_s(gp, x, S), "bf16")


def conv2_dgrad_chain16(gs32, H, W, w2, on, pix):
    """the storage chain of the 3x3 data gradient on the pixels `pix`: GS (bf16 already, or gs_on_load16's), the PK_HD weights rounded to
    bf16, fp32 accumulation, the ReLU mask `on` [HW][128], one rounding to bf16 (stq<GT>)"""
    ch = _fp32_chain(dr.im2col(rnd(gs32, "bf16"), H, W, pix, flip=True), rnd(dr.w2_bwd_mat(w2).astype(f32), "bf16"))
    return rnd((ch * on[pix]).astype(f32), "bf16")


def sums_before_store_slack(dy, x, S, gamma=None):
    """What bn_bwd_s moves by, per element, when the sums s1 = sum dy and s2 = sum dy * xhat were taken from the fp32 values IN FRONT of
    dy's 16-bit store (halo.cuh epilogue: `s1 += dyv` before stq<GT>): every stored element lies within h = half a bf16 ulp of what was
    summed, so |delta q1| <= mean(h), |delta q2| <= mean(h |xhat|), and the result a * ((dy - q1) - xhat * q2) moves by at most
    |a| * (mean(h) + |xhat| * mean(h |xhat|)).  Also returns the two sums' own slack (per channel): (element slack, sum h, sum h |xhat|)."""
    h = half_ulp(dy, "bf16")
    xh = np.abs((np.asarray(x, dtype=np.float64) - S.mean) * S.inv)
    a = np.abs(S.inv if gamma is None else S.inv * np.asarray(gamma, dtype=np.float64))
    return a * (h.mean(0) + xh * (h * xh).mean(0)), h.sum(0), (h * xh).sum(0)


def norm2_inplace(dy2, bt, g2, S, ts):
    """bn_bwd_apply_kernel<PREC> at C = 128, in place: (fp64 D2 from the STORED dy2 and the stored bottleneck with the engine's
    statistics S, its bound: k_d2_apply(ts) fp32 roundings of bn_bwd_sum_mag_s + sums_before_store_slack, + half a bf16 ulp)"""
    ref = bn_bwd_s(dy2, bt, S, g2)
    return ref, stored_bound(ref, k_d2_apply(ts), bn_bwd_sum_mag_s(dy2, bt, S, g2), "bf16", sums_before_store_slack(dy2, bt, S, g2)[0])


def conv1_dgrad16(G0, X, S, params, d2s, c0, c1, take=None, chain=True):
    """dense_ref.conv1_dgrad for the 16-bit modes, one stream: S = the engine's statistics of the block buffer X (engine_stats of
    fs_x<b>), G0 = the widened gsnap.  The chain: D2 as stored (bf16), the PK_D1 weights rounded to bf16, fp32 accumulation, mask and
    gamma in fp32, the segments summed in fp32 (BwdDataGroupP: `run`), added to G0, ONE rounding to bf16.  sum |term| includes |G0|: the
    stored SUM is what gets rounded.  Returns (reference, sum |term|, chain or None, keep)."""
    take = slice(None) if take is None else take
    Sc = S.cols(slice(c0, c1))
    x = np.asarray(X, dtype=np.float64)[take, c0:c1]
    ref = np.asarray(G0, dtype=np.float64)[take, c0:c1]
    mag = np.abs(ref) + 1e-300
    run = np.zeros(ref.shape, dtype=f32)
    keep = np.ones(ref.shape, dtype=bool)
    for (g1, b1, w1), d2 in zip(params, d2s):
        g1, b1, w1 = g1[c0:c1], b1[c0:c1], w1[:, c0:c1]
        d2 = np.asarray(d2)[take]
        keep &= keep_s(x, g1, b1, Sc)
        m = bn_pre_s(x, g1, b1, Sc) > 0
        ref = ref + g1.astype(np.float64) * m * (d2.astype(np.float64) @ w1.astype(np.float64))
        mag = mag + np.abs(g1).astype(np.float64) * m * (np.abs(d2).astype(np.float64) @ np.abs(w1).astype(np.float64))
        if chain:
            run = (run + (g1 * m).astype(f32) * _fp32_chain(rnd(d2, "bf16"), rnd(np.ascontiguousarray(w1.T, dtype=f32), "bf16"))).astype(f32)
    return ref, mag, rnd((np.asarray(G0, dtype=f32)[take, c0:c1] + run).astype(f32), "bf16") if chain else None, keep


def conv2_wgrad_ops16(GS32, BT, H, W, g2, b2, stats, cols):
    """dense_ref.conv2_wgrad_ops for the 16-bit modes: GS32 = per stream the operand's fp32 value (the stored gs_, or gs_on_load16's),
    the activation relu(bn2(bt)) with the engine's statistics; storage_blocked rounds both to bf16.  (Gs64, Gs32, A64, A32)"""
    cols = np.asarray(cols)
    A64 = np.concatenate([dr.im2col(act64_s(bt, g2, b2, S), H, W, cols=cols) for bt, S in zip(BT, stats)])
    A32 = np.concatenate([dr.im2col(act32_s(bt, g2, b2, S), H, W, cols=cols) for bt, S in zip(BT, stats)])
    G = np.concatenate([np.asarray(g, dtype=f32) for g in GS32])
    return G.astype(np.float64), G, A64, A32


def conv1_wgrad_ops16(D2, X, g1, b1, stats, rows, cols):
    """dense_ref.conv1_wgrad_ops for the 16-bit modes: the stored D2 against relu(bn1(x)) with the engine's statistics"""
    A64 = np.concatenate([act64_s(x[:, cols], g1[cols], b1[cols], S.cols(cols)) for x, S in zip(X, stats)])
    A32 = np.concatenate([act32_s(x[:, cols], g1[cols], b1[cols], S.cols(cols)) for x, S in zip(X, stats)])
    D = np.concatenate([np.asarray(d, dtype=f32)[:, rows] for d in D2])
    return D.astype(np.float64), D, A64, A32
