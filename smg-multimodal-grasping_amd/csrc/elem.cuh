// elem.cuh - the HBM-bound kernels around the MFMA convolutions: input
// preparation (zoom/pad/normalise/rotate gather), weight repacking, max-pool forward
// and backward, head feature assembly (norm5 + two-stream concat), the 20x20 value
// convolution and its backward, losses, BN running-statistics update, Adam.
#pragma once
#include "gemm.cuh"

namespace smg {

// ------------------------------------------------------------------------------------
// K1: fused Trainer.forward preprocessing (code/trainer.py:165-191) + per-stream
// rotation (code/models.py:372-382) -> NHWC4 image (4th channel zero).
//
// The sampling arithmetic restates torch's CPU operators bit for bit (pinned by
// golden vector G1): linspace(-1,1,S)[i] = fma(step, i, -1) for i < S/2 else
// fma(-step, S-1-i, 1); affine_grid = fma(y, a01, x*a00) + a02; grid_sample nearest,
// align_corners=True: rint(((g+1)/2)*(S-1)), zero outside [0, S-1].
// ------------------------------------------------------------------------------------
struct PrepArgs {
    const float* images_nchw;   // [n_images][3][S][S] or null
    const double* heightmaps;   // [n_images][hm][hm] or null
    int hm, pad, S;
    double mean, stdv;
    const int* stream_image;
    const float* stream_affine;
    const int* stream_rotated;
    float* img4;                // [streams][HWp][4]
    float* img1;                // if set (heightmap form): ONE channel per pixel [streams][HWp] instead - the three are identical
    int HWp;
    const double* masks;        // [n_masks][hm][hm] or null: object masks applied here (code/main.py:160,187)
    const int* stream_mask_a;   // per stream: mask index or -1
    const int* stream_mask_b;   // per stream: second mask index (ES pairs: mask[g] + mask[s]) or -1
};

__device__ __forceinline__ float lin_coord(int i, int S, float step) {
    return (i < S / 2) ? fmaf(step, (float)i, -1.f) : fmaf(-step, (float)(S - 1 - i), 1.f);
}

static __global__ void prep_rotate_kernel(const PrepArgs a) {
    const int s = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int S = a.S;
    if (p >= S * S) return;
    const int y = p / S, x = p - y * S;
    int sx = x, sy = y;
    bool inside = true;
    if (a.stream_rotated[s]) {
        const float* th = a.stream_affine + 6 * s;
        const float step = 2.0f / (float)(S - 1);
        const float lx = lin_coord(x, S, step), ly = lin_coord(y, S, step);
        const float gx = fmaf(ly, th[1], __fmul_rn(lx, th[0])) + th[2];
        const float gy = fmaf(ly, th[4], __fmul_rn(lx, th[3])) + th[5];
        const float fx = rintf(__fmul_rn(__fdiv_rn(__fadd_rn(gx, 1.f), 2.f), (float)(S - 1)));
        const float fy = rintf(__fmul_rn(__fdiv_rn(__fadd_rn(gy, 1.f), 2.f), (float)(S - 1)));
        inside = fx >= 0.f && fx <= (float)(S - 1) && fy >= 0.f && fy <= (float)(S - 1);
        sx = (int)fx;
        sy = (int)fy;
    }
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) {
        const int img = a.stream_image[s];
        if (a.images_nchw) {
            const float* b = a.images_nchw + (int64_t)img * 3 * S * S + (int64_t)sy * S + sx;
            out.x = b[0];
            out.y = b[(int64_t)S * S];
            out.z = b[(int64_t)2 * S * S];
        } else {
            const int hy = sy - a.pad, hx = sx - a.pad;
            double v = 0.0;
            if (hy >= 0 && hx >= 0 && hy < 2 * a.hm && hx < 2 * a.hm) {
                const int64_t at = (int64_t)(hy >> 1) * a.hm + (hx >> 1);
                v = a.heightmaps[(int64_t)img * a.hm * a.hm + at];
                if (a.masks) {
                    const int ma = a.stream_mask_a[s], mb = a.stream_mask_b[s];
                    if (ma >= 0) {
                        double m = a.masks[(int64_t)ma * a.hm * a.hm + at];
                        if (mb >= 0) m += a.masks[(int64_t)mb * a.hm * a.hm + at];
                        v *= m;                                  // depth * (mask[g] + mask[s]), float64 like numpy
                    }
                }
            }
            const float f = (float)((v - a.mean) / a.stdv);
            out.x = out.y = out.z = f;
        }
    }
    if (a.img1) a.img1[(int64_t)s * a.HWp + p] = out.x;
    else *reinterpret_cast<float4*>(a.img4 + ((int64_t)s * a.HWp + p) * 4) = out;
}

// ------------------------------------------------------------------------------------
// Weight repack: reference layout [cout][cin][kh][kw] -> what the kernels stream.  One launch for a
// whole trunk + head through a descriptor table.
//   split modes: the B operand of the MFMA GEMMs as 16-byte units [piece][K/8][N] of 8 consecutive k of one
//   output column n, already split into its pieces (two scaled fp16 pieces behind a header unit for operand kind 3, three bf16
//   pieces for kind 0; gemm.cuh) - staging them is a plain copy;
//   PK_HF / PK_HD: the per-stage LDS images of the LDS-halo 3x3 kernels; PK_HEAD: the value convolution's fp32 layout.
// ------------------------------------------------------------------------------------
enum { PK_T1 = 0, PK_D1 = 1, PK_3F = 2, PK_3D = 3, PK_STEM = 4, PK_HEAD = 5, PK_HF = 6, PK_HD = 7, PK_STEM1 = 8 };
struct PackDesc { int64_t src, dst; int cout, cin, mode, K8tot, N, count, op0; };   // dst: unit offset (split modes) / float offset (fp32 modes); op0: operand kind of the pack in precision mode 0 (0 = 3-piece bf16 split, 3 = 2-piece fp16 split with a header unit at dst - 1)

// Scales of operand kind 3 (gemm.cuh), one launch per forward in front of pack_weights_kernel:
//   blockIdx.y <  n_pack: the weight tensor of pack descriptor y (kind-3 packs only): s = 2^(13 - floor(log2 max|w|)) -> header
//                         unit {s, 1 / s, 0, 0} in front of the pack
//   blockIdx.y >= n_pack: BatchNorm + ReLU operand y - n_pack: m = max_c hypot(gamma_c, beta_c), s = 2^(4 - floor(log2 m))
//                         (m * s in [16, 32)) -> asc[2 * (y - n_pack)] = {s, 1 / s}
struct ActScaleDesc { int64_t gamma, beta; int C; };
static __global__ __launch_bounds__(1024) void scale_kernel(const PackDesc* descs, int n_pack, const ActScaleDesc* adescs, const float* params, u32x4* packed_u,
                                                           float* asc, int prec) {
    __shared__ float red[16];
    const int t = threadIdx.x, y = blockIdx.y;
    float m = 0.f;
    int target;
    if (y < n_pack) {
        const PackDesc d = descs[y];
        if (prec != 0 || d.op0 != 3) return;               // (workgroup-uniform)
        const int taps = (d.mode == PK_3F || d.mode == PK_3D || d.mode == PK_HF || d.mode == PK_HD) ? 9 : 1;
        const int64_t count = (int64_t)d.cout * d.cin * taps;
        const float* w = params + d.src;
        float m4[4] = {0.f, 0.f, 0.f, 0.f};                 // four independent loads in flight per thread (127 k floats in the largest tensor)
        int64_t i = t;
        if ((d.src & 3) == 0) {                             // 16-byte aligned tensors (all of the layout's): four float4 in flight, 8 trips instead of 31
            const float4* w4 = reinterpret_cast<const float4*>(w);
            const int64_t c4 = count >> 2;
            int64_t j = t;
            for (; j + 3 * 1024 < c4; j += 4 * 1024) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 v = w4[j + u * 1024];
                    m4[u] = fmaxf(m4[u], fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
                }
            }
            for (; j < c4; j += 1024) { const float4 v = w4[j]; m4[0] = fmaxf(m4[0], fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)))); }
            i = 4 * c4 + t;                                 // (the up to three floats behind the last whole float4)
        } else
        for (; i + 3 * 1024 < count; i += 4 * 1024) {
#pragma unroll
            for (int u = 0; u < 4; ++u) m4[u] = fmaxf(m4[u], fabsf(w[i + u * 1024]));
        }
        for (; i < count; i += 1024) m4[0] = fmaxf(m4[0], fabsf(w[i]));
        m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
        target = 13;
    } else {
        const ActScaleDesc d = adescs[y - n_pack];
        for (int c = t; c < d.C; c += 1024) { const float g = params[d.gamma + c], b = params[d.beta + c]; m = fmaxf(m, g * g + b * b); }
        m = sqrtf(m);
        target = 4;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((t & 63) == 0) red[t >> 6] = m;
    __syncthreads();
    if (t == 0) {
        m = 0.f;
#pragma unroll
        for (int u = 0; u < 16; ++u) m = fmaxf(m, red[u]);
        int e = (int)(__float_as_uint(m) >> 23) - 127;     // floor(log2 m); 0, subnormal or non-finite maxima: scale 1
        float sc = 1.f, inv = 1.f;
        if (m > 0.f && e > -100 && e < 100) { sc = __uint_as_float((unsigned)(127 + target - e) << 23); inv = __uint_as_float((unsigned)(127 - target + e) << 23); }
        if (y < n_pack) {
            float* h = reinterpret_cast<float*>(packed_u + descs[y].dst - 1);
            h[0] = sc; h[1] = inv; h[2] = 0.f; h[3] = 0.f;
        } else {
            asc[2 * (y - n_pack)] = sc; asc[2 * (y - n_pack) + 1] = inv;
        }
    }
}

// prec: the engine's precision mode.  Operand kind of a pack: the forward packs (PK_T1, PK_STEM, PK_3F, PK_HF) take the
// forward kind (the desc's split kind op0 / bf16 / fp16), the data-gradient packs (PK_D1, PK_3D, PK_HD) the backward kind (op0 / bf16).
// Single-piece kinds store ONE piece (the kernels copy a third of the bytes); the halo forward image then holds 32 channels
// per chunk instead of 16 (halo_ck).
static __global__ void pack_weights_kernel(const PackDesc* descs, const float* params, u32x4* packed_u, float* packed_f, const int prec) {
    const PackDesc d = descs[blockIdx.y];
    const float* s = params + d.src;
    if (d.mode == PK_HEAD) {                       // fp32 dst[o][tap][c] = src[o][c][tap] (value convolution)
        float* o = packed_f + d.dst;
        const int taps = 400;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d.count; i += gridDim.x * blockDim.x) {
            const int o_ = i / (taps * d.cin), r = i - o_ * taps * d.cin;
            const int tap = r / d.cin, c = r - tap * d.cin;
            o[i] = s[((int64_t)o_ * d.cin + c) * taps + tap];
        }
        return;
    }
    const bool bwd = d.mode == PK_D1 || d.mode == PK_3D || d.mode == PK_HD;
    const int op = prec == 0 ? d.op0 : (bwd ? 1 : prec);    // 0 bf16 split (3 pieces), 1 bf16, 2 fp16, 3 fp16 split (2 pieces, scaled)
    const int np = np_of(op);
    const int total = d.K8tot * d.N;               // units per piece
    u32x4* o = packed_u + d.dst;
    const float wsc = op == 3 ? reinterpret_cast<const float*>(o - 1)[0] : 1.f;      // header written by scale_kernel
    auto put = [&](const float (&v)[8], int64_t base, int64_t pstride) {
        const float4 v0 = make_float4(v[0] * wsc, v[1] * wsc, v[2] * wsc, v[3] * wsc), v1 = make_float4(v[4] * wsc, v[5] * wsc, v[6] * wsc, v[7] * wsc);
        const Split4 lo = op == 0 ? split4<0>(v0) : op == 1 ? split4<1>(v0) : op == 2 ? split4<2>(v0) : split4<3>(v0);
        const Split4 hi = op == 0 ? split4<0>(v1) : op == 1 ? split4<1>(v1) : op == 2 ? split4<2>(v1) : split4<3>(v1);
#pragma unroll
        for (int pc = 0; pc < NPIECE; ++pc)
            if (pc < np) o[base + pc * pstride] = u32x4{lo.p[pc].x, lo.p[pc].y, hi.p[pc].x, hi.p[pc].y};
    };
    if (d.mode == PK_HF || d.mode == PK_HD) {
        // LDS-halo 3x3 kernels: the image of one stage, per stage (halo.cuh)
        //   PK_HF forward       [chunk = c/CK][piece][tap][k8 (CK/8)][n (32)]  unit = 8 input channels c of output channel n
        //   PK_HD data gradient [cgroup = c/32][tap][piece][k8 (4)][c (32)]    unit = 8 output channels n of input channel c
        const int k8c = (prec ? 32 : 16) / 8;      // halo_ck(prec) / 8
        for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
            float v[8];
            int64_t base, pstride;
            if (d.mode == PK_HF) {
                const int n = e & 31, k8 = (e >> 5) % k8c, tap = (e / (32 * k8c)) % 9, chunk = e / (9 * 32 * k8c);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = s[((int64_t)n * d.cin + chunk * 8 * k8c + 8 * k8 + j) * 9 + tap];
                pstride = 9 * k8c * 32;
                base = ((int64_t)chunk * np * 9 + tap) * (k8c * 32) + k8 * 32 + n;
            } else {
                const int c = e & 31, k8 = (e >> 5) & 3, tap = (e >> 7) % 9, cg = e / 1152;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = s[((int64_t)(8 * k8 + j) * d.cin + cg * 32 + c) * 9 + tap];
                base = (((int64_t)cg * 9 + tap) * np) * 128 + k8 * 32 + c; pstride = 128;
            }
            put(v, base, pstride);
        }
        return;
    }
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int k8 = e / d.N, n = e - k8 * d.N;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * k8 + j;
            if (d.mode == PK_T1) {                 // B(k = c, n) = src[n][c]
                v[j] = s[(int64_t)n * d.cin + k];
            } else if (d.mode == PK_D1) {          // B(k = cout index, n = c) = src[k][c]
                v[j] = s[(int64_t)k * d.cin + n];
            } else if (d.mode == PK_3F) {          // B(k = tap*cin + c, n) = src[n][c][tap]
                const int tap = k / d.cin, c = k - tap * d.cin;
                v[j] = s[((int64_t)n * d.cin + c) * 9 + tap];
            } else if (d.mode == PK_3D) {          // B(k = tap*cout + nn, n = c) = src[nn][c][tap]
                const int tap = k / d.cout, nn = k - tap * d.cout;
                v[j] = s[((int64_t)nn * d.cin + n) * 9 + tap];
            } else if (d.mode == PK_STEM1) {       // k = tap (49 padded to 64): the weights summed over the 3 (identical) input channels
                v[j] = k < 49 ? (float)((double)s[((int64_t)n * 3 + 0) * 49 + k] + (double)s[((int64_t)n * 3 + 1) * 49 + k] + (double)s[((int64_t)n * 3 + 2) * 49 + k]) : 0.f;
            } else {                               // PK_STEM: k = tap*4 + c (K padded to 224), src[n][c][tap]
                const int tap = k >> 2, c = k & 3;
                v[j] = (c < 3 && tap < 49) ? s[((int64_t)n * 3 + c) * 49 + tap] : 0.f;
            }
        }
        put(v, e, total);
    }
}

// ------------------------------------------------------------------------------------
// BN statistics table entries for channels whose producer is not a dense layer (block inputs after pool0 / a
// transition, the head's concatenated features): fp64 sums -> fp32 mean | invstd, once.  The channels a dense
// layer appends are finished by their first consumer instead (ActSrc, gemm.cuh) - no launch of their own.
// ------------------------------------------------------------------------------------
struct BnStatArgs {
    const double* sum; const double* sq; int sstride;          // [row][sstride] statistics
    float eps; double inv_count;
    float* mean; float* invstd; int ld;                        // tables [row][ld]
    int c0, C, rows;                                           // channels [c0, c0 + C)
};
static __global__ void bn_stat_kernel(const BnStatArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.rows * a.C) return;
    const int n = idx / a.C, c = a.c0 + idx - n * a.C;
    float mean, invstd;
    bn_moments(a.sum, a.sq, (int64_t)n * a.sstride + c, a.inv_count, a.eps, mean, invstd);
    a.mean[(int64_t)n * a.ld + c] = mean;
    a.invstd[(int64_t)n * a.ld + c] = invstd;
}

// ------------------------------------------------------------------------------------
// pool0: BN(norm0)+ReLU+MaxPool(3,2,1) of the stem output -> channels 0..63 of the
// block-1 buffer, + their per-stream statistics, + argmax (for the backward).
// Workgroup = 64 pooled pixels x 64 channels; thread = (channel quad, pixel slot).
// ------------------------------------------------------------------------------------
struct Pool0Args {
    ActSrc stem; Plane ps;                 // raw stem output [n][HWp][64] (fp32), its statistics [n][64] and norm0
    void* x1; int ldx; Plane po;            // block-1 buffer (activation storage of the mode)
    StatSink st;                            // sum x | sum x^2 of the 64 pooled channels
    unsigned char* argmax;                  // [n][po.HWp][64]
    float* stemv;                           // [n][po.HWp][64] the raw stem value at the argmax (stem_tail_kernel), or nullptr
};

template <int PREC>
static __global__ __launch_bounds__(256) void pool0_kernel(const Pool0Args a) {
    using XT = act_t<PREC>;
    __shared__ float prm[192];
    __shared__ double red[2][16][64];
    const int n = blockIdx.y, t = threadIdx.x, cq = t & 15, slot = t >> 4;
    if (t < 64) {
        act_prm_store(prm + t, 64, act_src_coef<A_SUMS>(a.stem, n, t, 1.0 / (double)a.ps.HW), 1.f);
    }
    __syncthreads();
    double s[4] = {0, 0, 0, 0}, ss[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        const int p = blockIdx.x * 64 + slot + 16 * i;
        if (p >= a.po.HW) continue;
        const int y = p / a.po.W, x = p - y * a.po.W;
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int bi[4] = {0, 0, 0, 0};
        float raw[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 9; ++k) {
            const int yy = 2 * y - 1 + k / 3, xx = 2 * x - 1 + k % 3;
            if ((unsigned)yy >= (unsigned)a.ps.H || (unsigned)xx >= (unsigned)a.ps.W) continue;
            const float4 r = ld4(static_cast<const float*>(a.stem.x) + ((int64_t)n * a.ps.HWp + yy * a.ps.W + xx) * 64 + 4 * cq);
            const float4 v = bnrelu4(r, prm + 4 * cq, 64);
            const float vv[4] = {v.x, v.y, v.z, v.w}, rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (vv[c] > best[c]) { best[c] = vv[c]; bi[c] = k; raw[c] = rr[c]; }
        }
        const int64_t o = (int64_t)n * a.po.HWp + p;
        stq<XT>(a.x1, o * a.ldx + 4 * cq, make_float4(best[0], best[1], best[2], best[3]));
        if (a.argmax) *reinterpret_cast<uchar4*>(a.argmax + o * 64 + 4 * cq) = make_uchar4(bi[0], bi[1], bi[2], bi[3]);
        if (a.stemv) *reinterpret_cast<float4*>(a.stemv + o * 64 + 4 * cq) = make_float4(raw[0], raw[1], raw[2], raw[3]);
#pragma unroll
        for (int c = 0; c < 4; ++c) { s[c] += (double)best[c]; ss[c] += (double)best[c] * (double)best[c]; }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) { red[0][slot][4 * cq + c] = s[c]; red[1][slot][4 * cq + c] = ss[c]; }
    __syncthreads();
    if (t < 128) {
        const int q = t >> 6, c = t & 63;
        double tot = 0.0;
        for (int k = 0; k < 16; ++k) tot += red[q][k][c];
        stat_sink_add<S_FWD>(a.st, n, c, q, tot);
    }
}

// ------------------------------------------------------------------------------------
// Head feature assembly: F[pair] = concat(norm5(X4[a]), norm5(X4[b]))  (no ReLU after
// norm5 - the reference calls .features directly, code/models.py:384-386) and the
// per-(pair, channel) statistics the head's norm0 needs.
// ------------------------------------------------------------------------------------
struct FeatArgs {
    ActSrc x4; Plane p4;                    // [n][HWp][1024] (activation storage of the mode), its statistics [n][1024] and norm5
    const int* pair_a; const int* pair_b;
    float* F;                               // [pair][HWp][2048]
    StatSink st;                            // [pair][2048]
    int chunk;
};

template <int PREC>
static __global__ __launch_bounds__(256) void feat_kernel(const FeatArgs a) {
    using XT = act_t<PREC>;
    const int j = blockIdx.y, cq = blockIdx.x * 256 + threadIdx.x;   // channel quad of 2048/4
    const int ch = 4 * cq, slot = ch >> 10, c5 = ch & 1023;
    const int s = slot ? a.pair_b[j] : a.pair_a[j];
    float mu[4], sc[4], be[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const ActCoef f = act_src_coef<A_SUMS>(a.x4, s, c5 + c, 1.0 / (double)a.p4.HW);
        mu[c] = f.mean;
        sc[c] = f.gamma * f.invstd;
        be[c] = f.beta;
    }
    double sm[4] = {0, 0, 0, 0}, sq[4] = {0, 0, 0, 0};
    const int p0 = blockIdx.z * a.chunk;
    const int p1 = min(p0 + a.chunk, a.p4.HW);
    for (int p = p0; p < p1; ++p) {
        const float4 v = ldq<XT>(a.x4.x, ((int64_t)s * a.p4.HWp + p) * 1024 + c5);
        float4 o;
        o.x = bn1(v.x, mu[0], sc[0], be[0]); o.y = bn1(v.y, mu[1], sc[1], be[1]);
        o.z = bn1(v.z, mu[2], sc[2], be[2]); o.w = bn1(v.w, mu[3], sc[3], be[3]);
        *reinterpret_cast<float4*>(a.F + ((int64_t)j * a.p4.HWp + p) * 2048 + ch) = o;
        const double od[4] = {(double)o.x, (double)o.y, (double)o.z, (double)o.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) { sm[c] += od[c]; sq[c] += od[c] * od[c]; }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) stat_sink_add2<S_FWD>(a.st, j, ch + c, sm[c], sq[c]);
}

// ------------------------------------------------------------------------------------
// Value convolution: 20x20 valid conv over BN+ReLU(H1) (code/models.py:322,332).
// One workgroup per output element; fixed summation order -> reproducible argmax.
// ------------------------------------------------------------------------------------
struct ValueArgs {
    ActSrc h1; Plane p4;                     // [pair][HWp][64] (fp32), its statistics [pair][64] and the head's norm1
    const float* w2p;                        // packed [out][400][64]
    float* q; int out_ch, OH, OW;
};

static __global__ __launch_bounds__(256) void value_conv_kernel(const ValueArgs a) {
    __shared__ float prm[192];
    __shared__ float red[256];
    const int t = threadIdx.x, cq = t & 15, slot = t >> 4;
    int id = blockIdx.x;
    const int ox = id % a.OW; id /= a.OW;
    const int oy = id % a.OH; id /= a.OH;
    const int o = id % a.out_ch;
    const int j = id / a.out_ch;
    if (t < 64) {
        act_prm_store(prm + t, 64, act_src_coef<A_SUMS>(a.h1, j, t, 1.0 / (double)a.p4.HW), 1.f);
    }
    __syncthreads();
    float acc = 0.f;
    for (int tap = slot; tap < 400; tap += 16) {
        const int pix = (oy + tap / 20) * a.p4.W + ox + tap % 20;
        const float4 v = bnrelu4(ld4(static_cast<const float*>(a.h1.x) + ((int64_t)j * a.p4.HWp + pix) * 64 + 4 * cq), prm + 4 * cq, 64);
        const float4 w = ld4(a.w2p + ((int64_t)o * 400 + tap) * 64 + 4 * cq);
        acc = fmaf(v.x, w.x, acc); acc = fmaf(v.y, w.y, acc); acc = fmaf(v.z, w.z, acc); acc = fmaf(v.w, w.w, acc);
    }
    red[t] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {     // (block_sum's tree, written out: through the function this kernel's listing grows by two instructions)
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) a.q[blockIdx.x] = red[0];
}

// Backward of the value convolution + ReLU + BN(norm1) statistics:
//   dact[p][c] = sum_{o,oy,ox} dq[o][oy][ox] * W[o][c][py-oy][px-ox]
//   dy = dact * [BN(h1) > 0] -> DH1 ; sums of dy, dy*xhat per (pair, c);
//   dW[o][c][tap] += dq * act.
struct ValueBwdArgs {
    ActSrc h1; Plane p4;                      // [pair][HWp][64] (fp32), its statistics [pair][64] and the head's norm1
    const float* w2p;                         // packed [out][400][64]
    const float* dq; int out_ch, OH, OW;
    float* dh1;                               // [pair][HWp][64]
    StatSink st; AffineSink aff;              // [pair][64] sums and norm1's affine gradients
    float* dw2;                               // native [out][64][20][20]
};

// The two ends the backward kernels below share.  Front: norm1's per-channel parameters of pair j,
// prm[t] = gamma * invstd | beta | mean | invstd (the caller's barrier publishes them).  Back: the threads' sums of dy and dy * xhat
// have met in red[2][16][64] (written and published by the caller: a barrier inside the inlined function leaves a dead exec-mask
// instruction behind in the dense kernels); per channel a 16-way sum in slot order, one double atomic to the statistic sink and one float
// atomic to the affine sink per workgroup.
__device__ __forceinline__ void value_bwd_params(const ValueBwdArgs& a, int j, int t, float* prm) {
    if (t < 64) act_mask_store(prm + t, 64, act_src_coef<A_SUMS>(a.h1, j, t, 1.0 / (double)a.p4.HW));
}
__device__ __forceinline__ void value_bwd_sums(const ValueBwdArgs& a, int j, int t, const float (*red)[16][64]) {
    if (t < 128) {
        const int q = t >> 6, c = t & 63;
        float tot = 0.f;
        for (int k = 0; k < 16; ++k) tot += red[q][k][c];
        stat_sink_add<S_BWD>(a.st, j, c, q, (double)tot);
        affine_sink_add(a.aff, c, q, tot);
    }
}

static __global__ __launch_bounds__(256) void value_bwd_kernel(const ValueBwdArgs a) {
    __shared__ float prm[256];
    __shared__ float red[2][16][64];
    const int j = blockIdx.y, t = threadIdx.x, cq = t & 15, slot = t >> 4;
    value_bwd_params(a, j, t, prm);
    __syncthreads();
    float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        const int p = blockIdx.x * 64 + slot + 16 * i;
        if (p >= a.p4.HW) continue;
        const int py = p / a.p4.W, px = p - py * a.p4.W;
        const int64_t row = (int64_t)j * a.p4.HWp + p;
        const float4 hv = ld4(static_cast<const float*>(a.h1.x) + row * 64 + 4 * cq);
        const float h[4] = {hv.x, hv.y, hv.z, hv.w};
        float act[4], dact[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; ++c) act[c] = fmaxf(bn1(h[c], prm[128 + 4 * cq + c], prm[4 * cq + c], prm[64 + 4 * cq + c]), 0.f);
        for (int o = 0; o < a.out_ch; ++o)
            for (int oy = max(0, py - 19); oy <= min(py, a.OH - 1); ++oy)
                for (int ox = max(0, px - 19); ox <= min(px, a.OW - 1); ++ox) {
                    const float g = a.dq[(((int64_t)j * a.out_ch + o) * a.OH + oy) * a.OW + ox];
                    if (g == 0.f) continue;
                    const int tap = (py - oy) * 20 + (px - ox);
                    const float4 w = ld4(a.w2p + ((int64_t)o * 400 + tap) * 64 + 4 * cq);
                    dact[0] = fmaf(g, w.x, dact[0]); dact[1] = fmaf(g, w.y, dact[1]);
                    dact[2] = fmaf(g, w.z, dact[2]); dact[3] = fmaf(g, w.w, dact[3]);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        atomicAdd(a.dw2 + ((int64_t)o * 64 + 4 * cq + c) * 400 + tap, g * act[c]);
                }
        float dy[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            dy[c] = act[c] > 0.f ? dact[c] : 0.f;
            s1[c] += dy[c];
            s2[c] += dy[c] * ((h[c] - prm[128 + 4 * cq + c]) * prm[192 + 4 * cq + c]);
        }
        *reinterpret_cast<float4*>(a.dh1 + row * 64 + 4 * cq) = make_float4(dy[0], dy[1], dy[2], dy[3]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) { red[0][slot][4 * cq + c] = s1[c]; red[1][slot][4 * cq + c] = s2[c]; }
    __syncthreads();
    value_bwd_sums(a, j, t, red);
}

// The same backward for a DENSE dq (a whole weighted map per pair: smg_loss_map on a one-channel head, smg_loss_map_ce on a
// 3-class one).  value_bwd_kernel above walks the output elements a pixel feeds and adds four fp32 atomics per non-zero dq and tap: fine for the one element the Huber
// of code/trainer.py:345 reads, 1444 x 400 x 64 = 37 M atomics per pair and output channel onto 25 600 addresses for a full
// 38 x 38 map.  Here the work is split by what it reuses:
//   value_bwd_dense_kernel   (data pass)   dact, DH1, the norm1 sums - per workgroup 64 pixels of one pair, looping over the 400
//                                          TAPS: one float4 of packed weights per tap and output channel serves the thread's
//                                          four pixels, dq comes from a zero-framed copy in LDS (no bounds test in the loop);
//   value_wgrad_dense_kernel (weight pass) dW - per workgroup one tap row and channel quad (and output channel), pairs in index
//                                          order, every element of dW written by exactly one thread: a fixed summation order
//                                          and no atomic at all.
// Both are templates on the head's OC output channels (1, or the 3 classes).  The data pass's frame holds the OC dq maps,
// [OC][OH + 38][OW + 38], and every tap reads OC float4 of packed weights and 4 OC frame values.  With three maps the frame is
// 69 312 B at 38 x 38, above the 64 KB default: the launch path raises the kernel's limit, and the raised limit of 160 KiB is the
// whole CU's, so a kernel that takes it must not hold static LDS beside it (the raise is refused and the launch fails) - for
// OC > 1 the parameter and reduction arrays follow the frame in the DYNAMIC area.
constexpr int kVFrame = 19;     // the 20 x 20 window reaches 19 outputs up / left of a pixel
static inline size_t value_bwd_dense_lds(int OC, int OH, int OW) {
    return ((size_t)OC * (OH + 2 * kVFrame) * (OW + 2 * kVFrame) + (OC == 1 ? 0 : 256 + 2 * 16 * 64)) * sizeof(float);
}

template <int OC>
static __global__ __launch_bounds__(256) void value_bwd_dense_kernel(const ValueBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];    // dq of the pair in a frame of zeros: [OC][OH + 38][OW + 38]
    const int j = blockIdx.y, t = threadIdx.x, cq = t & 15, slot = t >> 4;
    const int PW = a.OW + 2 * kVFrame, PH = a.OH + 2 * kVFrame;
    float* prm;                      // [256]
    float (*red)[16][64];            // [2][16][64]
    if constexpr (OC == 1) {
        __shared__ float prm1[256];
        __shared__ float red1[2][16][64];
        prm = prm1; red = red1;
    } else {
        prm = smem + OC * PH * PW;
        red = reinterpret_cast<float (*)[16][64]>(prm + 256);
    }
    value_bwd_params(a, j, t, prm);
    // (the two loops over the output channels are do-whiles: written as `for`, their single trip at OC == 1 lives long enough to
    // move what the compiler hoists out of the fill loop and to flip the tap loop's exit compare)
    int o = 0;
#pragma unroll
    do {
        for (int i = t; i < PH * PW; i += 256) {
            const int y = i / PW - kVFrame, x = i % PW - kVFrame;
            smem[o * PH * PW + i] = (y >= 0 && y < a.OH && x >= 0 && x < a.OW) ? a.dq[(((int64_t)j * OC + o) * a.OH + y) * a.OW + x] : 0.f;
        }
    } while (++o < OC);
    __syncthreads();
    // frame position of output (py, px) for each of the thread's four pixels; output (py - ty, px - tx) lies ty rows and tx columns
    // in front of it (rows -19 .. OH + 18 of the frame: always inside)
    int base[4]; bool live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = blockIdx.x * 64 + slot + 16 * i;
        live[i] = p < a.p4.HW;
        const int py = live[i] ? p / a.p4.W : 0, px = live[i] ? p - py * a.p4.W : 0;
        base[i] = (py + kVFrame) * PW + px + kVFrame;
    }
    float dact[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) dact[i][c] = 0.f;
    const float* wq = a.w2p + 4 * cq;
    for (int ty = 0; ty < 20; ++ty) {
#pragma unroll 5
        for (int tx = 0; tx < 20; ++tx) {
            o = 0;
#pragma unroll
            do {
                const float4 w = ld4(wq + (o * 400 + ty * 20 + tx) * 64);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float g = smem[o * PH * PW + base[i] - ty * PW - tx];
                    dact[i][0] = fmaf(g, w.x, dact[i][0]); dact[i][1] = fmaf(g, w.y, dact[i][1]);
                    dact[i][2] = fmaf(g, w.z, dact[i][2]); dact[i][3] = fmaf(g, w.w, dact[i][3]);
                }
            } while (++o < OC);
        }
    }
    float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!live[i]) continue;
        const int64_t row = (int64_t)j * a.p4.HWp + blockIdx.x * 64 + slot + 16 * i;
        const float4 hv = ld4(static_cast<const float*>(a.h1.x) + row * 64 + 4 * cq);
        const float h[4] = {hv.x, hv.y, hv.z, hv.w};
        float dy[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float act = fmaxf(bn1(h[c], prm[128 + 4 * cq + c], prm[4 * cq + c], prm[64 + 4 * cq + c]), 0.f);
            dy[c] = act > 0.f ? dact[i][c] : 0.f;
            s1[c] += dy[c];
            s2[c] += dy[c] * ((h[c] - prm[128 + 4 * cq + c]) * prm[192 + 4 * cq + c]);
        }
        *reinterpret_cast<float4*>(a.dh1 + row * 64 + 4 * cq) = make_float4(dy[0], dy[1], dy[2], dy[3]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) { red[0][slot][4 * cq + c] = s1[c]; red[1][slot][4 * cq + c] = s2[c]; }
    __syncthreads();
    value_bwd_sums(a, j, t, red);
}

// dW[c][ty][tx] += sum over pairs, oy, ox of dq[j][oy][ox] * act[j][oy + ty][ox + tx][c].
// Workgroup = (tap row ty, channel quad): 20 x 16 of them.  Per pair (in index order) and chunk of up to 64 output rows it stages
// the BN + ReLU activations of the feature rows those outputs meet under this tap row - [rows][Wp][4 channels], columns past the
// plane zero-filled - and the dq rows (zero-filled to a multiple of four columns); thread (row, channel) slides along its row four
// outputs at a time: 4 dq values and 23 activations feed 80 multiply-adds into its 20 per-tap-column accumulators (fp32 along a
// row, carried in fp64 from row chunk to row chunk and pair to pair).  The rows meet in LDS (fp64, over the staging area) in row
// order, and one thread per element adds the rounded total to the gradient array.
// OC output channels (dq [pair][OC][OH][OW], dW [OC][64][20][20]): the output channel is the third grid dimension, 20 x 16 x OC
// workgroups that each stage the activations for themselves (the 60 per-tap-column accumulators of a 3-class head, in fp32 and fp64,
// would not fit one thread's registers without scratch), same order of summation per element.
struct ValueWgradDenseArgs {
    ActSrc h1; Plane p4;                      // the descriptor ValueBwdArgs holds
    const float* dq; int OH, OW, n_pairs;
    float* dw2;                               // native [out][64][20][20]
    int RC, OWp, Wp;                          // output rows per chunk (<= 64), OW rounded up to 4, OWp + 19 staged columns
};
static inline size_t value_wgrad_dense_lds(const ValueWgradDenseArgs& a) {
    const size_t stage = ((size_t)a.RC * a.Wp * 4 + (size_t)a.RC * a.OWp) * sizeof(float), meet = 64 * 80 * sizeof(double);
    return std::max(stage, meet) + 16 * sizeof(float);
}

template <int OC>
static __global__ __launch_bounds__(256) void value_wgrad_dense_kernel(const ValueWgradDenseArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* acts = smem;                                   // [RC][Wp] float4
    float* dqs = acts + (size_t)a.RC * a.Wp * 4;          // [RC][OWp]
    double* red = reinterpret_cast<double*>(smem);        // [64][20][4], once the last chunk has been read
    float* prm = smem + max(a.RC * (a.Wp * 4 + a.OWp), 64 * 80 * 2);      // mean[4], scale[4], beta[4]
    const int ty = blockIdx.x, cq = blockIdx.y, t = threadIdx.x, c = t & 3, g = t >> 2;
    const int o = OC == 1 ? 0 : blockIdx.z;
    const int W = a.p4.W;
    double tot[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) tot[k] = 0.0;
    for (int j = 0; j < a.n_pairs; ++j) {
        if (t < 4) act_prm_store(prm + t, 4, act_src_coef<A_SUMS>(a.h1, j, 4 * cq + t, 1.0 / (double)a.p4.HW), 1.f);
        for (int r0 = 0; r0 < a.OH; r0 += a.RC) {
            const int nr = min(a.RC, a.OH - r0);
            __syncthreads();        // the parameters are written; the previous chunk has been read
            for (int i = t; i < nr * a.Wp; i += 256) {
                const int row = i / a.Wp, x = i - row * a.Wp;
                float4 v = zero4();
                if (x < W) v = bnrelu4(ld4(static_cast<const float*>(a.h1.x) + ((int64_t)j * a.p4.HWp + (r0 + row + ty) * W + x) * 64 + 4 * cq), prm, 4);
                *reinterpret_cast<float4*>(acts + (size_t)i * 4) = v;
            }
            for (int i = t; i < nr * a.OWp; i += 256) {
                const int row = i / a.OWp, x = i - row * a.OWp;
                dqs[i] = x < a.OW ? a.dq[(((int64_t)j * OC + o) * a.OH + r0 + row) * a.OW + x] : 0.f;
            }
            __syncthreads();
            if (g < nr) {
                float acc[20];
#pragma unroll
                for (int k = 0; k < 20; ++k) acc[k] = 0.f;
                const float* ar = acts + (size_t)g * a.Wp * 4 + c;
                const float* dr = dqs + g * a.OWp;
                for (int ox = 0; ox < a.OWp; ox += 4) {
                    const float4 d4 = ld4(dr + ox);
                    const float d[4] = {d4.x, d4.y, d4.z, d4.w};
                    float av[23];
#pragma unroll
                    for (int k = 0; k < 23; ++k) av[k] = ar[(ox + k) * 4];
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int tx = 0; tx < 20; ++tx) acc[tx] = fmaf(d[b], av[b + tx], acc[tx]);
                }
#pragma unroll
                for (int k = 0; k < 20; ++k) tot[k] += (double)acc[k];
            }
        }
    }
    __syncthreads();             // the staging area becomes the meeting place
#pragma unroll
    for (int tx = 0; tx < 20; ++tx) red[g * 80 + tx * 4 + c] = tot[tx];
    __syncthreads();
    if (t < 80) {
        double sum = 0.0;
        for (int k = 0; k < 64; ++k) sum += red[k * 80 + t];
        const int tx = t >> 2, ch = 4 * cq + (t & 3);
        float* dst = a.dw2 + ((int64_t)o * 64 + ch) * 400 + ty * 20 + tx;
        *dst = *dst + (float)sum;       // one writer per element
    }
}

// ------------------------------------------------------------------------------------
// norm5 backward (no ReLU) fused with the head's norm0 backward and the two-stream
// concat backward: for stream s, sum over every (pair, slot) that consumed its
// features the BN-corrected gradient of F, then start the block-4 gradient buffer:
//   G'_4[s] = gamma5 * dy5,  s1/s2 += gamma5 * sums,  norm5's dbeta/dgamma += sums.
// ------------------------------------------------------------------------------------
struct Norm5BwdArgs {
    GradSrc df; Plane p4;                           // the head's gradient of F through norm0: fp32 [pair][HWp][2048], statistics [pair][2048]
    ActSrc x4;                                      // [n][HWp][1024] (activation storage), its statistics [n][1024] and norm5: the descriptor FeatArgs holds
    const int* user_ptr; const int* user_pair; const int* user_slot;  // CSR over streams
    void* G4;                                       // [n][HWp][1024] (gradient storage of the mode)
    StatSink st; AffineSink aff;                    // s1 / s2 of X4 [n][1024] and norm5's affine gradients
    int chunk;
};

template <int PREC>
static __global__ __launch_bounds__(256) void norm5_bwd_kernel(const Norm5BwdArgs a) {
    using XT = act_t<PREC>;
    using GT = grd_t<PREC>;
    // Workgroup = (256 channels, one stream, 16 pixels): 64 channel quads x 4 user phases.  A stream with several users (the masked
    // stream feeds every pair) is a serial chain of parameter + pixel round trips per user; its users are dealt round-robin to the
    // four phases, which meet in LDS in a fixed order (one thread per quad over all users: 175 us, a 16x longer tail than the
    // single-user streams).
    constexpr int CH = 16;                               // pixels per workgroup (= a.chunk, checked at the launch)
    __shared__ float4 red[3][CH][64];
    __shared__ float reds[3][8][64];
    const int s = blockIdx.y, cq = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int c5 = 4 * (blockIdx.x * 64 + cq);
    const int u0 = a.user_ptr[s], u1 = a.user_ptr[s + 1];
    const bool multi = u1 - u0 > 1;                      // (workgroup-uniform)
    // single-user streams: kSpan chunks per workgroup, so that the per-channel dbeta / dgamma (one address for every stream and
    // chunk) see a fifth of the atomics - 425 same-address atomics per channel were 38 of the kernel's 110 us
    constexpr int kSpan = 5;
    const int n_sub = multi ? 1 : kSpan;
    const int z0 = multi ? blockIdx.z : blockIdx.z * kSpan;
    if (z0 * a.chunk >= a.p4.HW) return;
    const double inv = 1.0 / (double)a.p4.HW;
    float mean5[4], inv5[4], g5[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const ActCoef f = act_src_coef<A_SUMS, 1>(a.x4, s, c5 + c, inv);
        mean5[c] = f.mean; inv5[c] = f.invstd; g5[c] = f.gamma;
    }
    float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    for (int sub = 0; sub < n_sub; ++sub) {
    const int p0 = (z0 + sub) * a.chunk, p1 = min(p0 + a.chunk, a.p4.HW);
    if (p0 >= p1) break;
    // G4 of the chunk's pixels accumulates in registers over the users of the stream (a read-modify-write of G4 per user was a
    // chain of dependent global round trips per pixel)
    float4 gacc[CH];
#pragma unroll
    for (int q = 0; q < CH; ++q) gacc[q] = zero4();
    for (int u = u0 + ph; u < u1; u += 4) {
        const int j = a.user_pair[u], ch = a.user_slot[u] * 1024 + c5;
        float cf[16];   // a[4], q1[4], mean[4], k[4]
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const GradCoef f = grad_src_coef(a.df, j, ch + c, inv);
            cf[c] = f.a;
            cf[4 + c] = f.q1;
            cf[8 + c] = f.mean;
            cf[12 + c] = f.k;
        }
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int p = p0 + q;
            if (p < p1) {
                const int64_t fr = ((int64_t)j * a.p4.HWp + p) * 2048 + ch;
                const float4 d = affine2(ld4(static_cast<const float*>(a.df.g) + fr), ld4(static_cast<const float*>(a.df.x) + fr), cf, 4);
                const int64_t xr = ((int64_t)s * a.p4.HWp + p) * 1024 + c5;
                const float4 xv = ldq<XT>(a.x4.x, xr);
                const float dd[4] = {d.x, d.y, d.z, d.w}, xx[4] = {xv.x, xv.y, xv.z, xv.w};
                gacc[q].x += g5[0] * dd[0]; gacc[q].y += g5[1] * dd[1]; gacc[q].z += g5[2] * dd[2]; gacc[q].w += g5[3] * dd[3];
#pragma unroll
                for (int c = 0; c < 4; ++c) { s1[c] += dd[c]; s2[c] += dd[c] * ((xx[c] - mean5[c]) * inv5[c]); }
            }
        }
    }
    if (multi) {
        if (ph) {
#pragma unroll
            for (int q = 0; q < CH; ++q) red[ph - 1][q][cq] = gacc[q];
#pragma unroll
            for (int c = 0; c < 4; ++c) { reds[ph - 1][c][cq] = s1[c]; reds[ph - 1][4 + c][cq] = s2[c]; }
        }
        __syncthreads();
        if (ph == 0) {
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const float4 r0 = red[0][q][cq], r1 = red[1][q][cq], r2 = red[2][q][cq];
                gacc[q].x = (gacc[q].x + r0.x) + (r1.x + r2.x); gacc[q].y = (gacc[q].y + r0.y) + (r1.y + r2.y);
                gacc[q].z = (gacc[q].z + r0.z) + (r1.z + r2.z); gacc[q].w = (gacc[q].w + r0.w) + (r1.w + r2.w);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                s1[c] = (s1[c] + reds[0][c][cq]) + (reds[1][c][cq] + reds[2][c][cq]);
                s2[c] = (s2[c] + reds[0][4 + c][cq]) + (reds[1][4 + c][cq] + reds[2][4 + c][cq]);
            }
        }
    }
    if (ph == 0) {
#pragma unroll
        for (int q = 0; q < CH; ++q)
            if (p0 + q < p1) stq<GT>(a.G4, ((int64_t)s * a.p4.HWp + p0 + q) * 1024 + c5, gacc[q]);
    }
    }   // sub-chunks
    if (ph || u0 == u1) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        stat_sink_add2<S_BWD>(a.st, s, c5 + c, (double)(g5[c] * s1[c]), (double)(g5[c] * s2[c]));
        affine_sink_add2(a.aff, c5 + c, s1[c], s2[c]);
    }
}

// ------------------------------------------------------------------------------------
// pool0 + relu0 backward: route the (BN-corrected) gradient of block-1 channels 0..63
// back through the 3x3/stride-2 max pool to the stem output, apply the ReLU mask of
// norm0, and collect norm0's backward sums.  Gather form: each stem pixel looks at
// the <= 4 pooled windows covering it and takes those whose argmax points at it.
// ------------------------------------------------------------------------------------
struct Pool0BwdArgs {
    GradSrc g1; Plane p1;                                    // block 1's G' / X, channels 0..63 (gradient / activation storage of the mode)
    const unsigned char* argmax;                             // [n][p1.HWp][64]
    ActSrc stem; Plane ps;                                   // raw stem output [n][HWp][64] (fp32), its statistics [n][64] and norm0
    float* DY0;                                              // [n][ps.HWp][64]
    StatSink st; AffineSink aff;                             // [n][64]; norm0's (db_flush_kernel adds them from the sums, not this kernel)
    int tiles_per_wg;                                        // consecutive 8x8 tiles per workgroup (one flush of the sums)
};

template <int PREC>
static __global__ __launch_bounds__(256) void pool0_bwd_kernel(const Pool0BwdArgs a) {
    using XT = act_t<PREC>;
    using GT = grd_t<PREC>;
    // Workgroup = an 8x8 tile of stem pixels x 64 channels.  The <= 5x5 pooled pixels whose windows
    // cover the tile are finalised (BN-backward-corrected) ONCE into LDS together with their argmax;
    // every stem pixel then picks its <= 4 windows from LDS.  (The gather straight from global memory
    // chained argmax load -> compare -> conditional gradient load: one memory round trip per window.)
    // A workgroup walks tiles_per_wg tiles and flushes its BN-backward sums once: one tile per workgroup meant
    // 27 200 workgroups x 256 atomics on 2 x 64 x (1 + streams) addresses.
    __shared__ float prm[8 * 64];
    __shared__ float gl[25][64];
    __shared__ unsigned char al[25][64];
    __shared__ float red[2][16][64];
    const int n = blockIdx.y, t = threadIdx.x, cq = t & 15, slot = t >> 4;
    const int tiles_x = a.ps.W / 8, n_tiles = tiles_x * (a.ps.H / 8);
    if (t < 64) {
        act_mask_store(prm + t, 64, act_src_coef<A_SUMS>(a.stem, n, t, 1.0 / (double)a.ps.HW));
        const double inv = 1.0 / (double)a.p1.HW;
        const GradCoef f = grad_src_coef(a.g1, n, t, inv);
        prm[256 + t] = f.a; prm[320 + t] = f.q1; prm[384 + t] = f.mean; prm[448 + t] = f.k;
    }
    float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    const int tile0 = blockIdx.x * a.tiles_per_wg, tile1 = min(tile0 + a.tiles_per_wg, n_tiles);
    for (int tile = tile0; tile < tile1; ++tile) {
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * 8, x0 = tx * 8;
    // stem values of this thread's 4 pixels: issue early
    float4 sv[4];
    int64_t srow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int lp = slot + 16 * i;                       // local pixel 0..63
        srow[i] = (int64_t)n * a.ps.HWp + (y0 + (lp >> 3)) * a.ps.W + x0 + (lp & 7);
        sv[i] = ld4(static_cast<const float*>(a.stem.x) + srow[i] * 64 + 4 * cq);
    }
    // pooled pixels wy in [y0/2, y0/2 + 4], wx likewise
    const int wy0 = y0 >> 1, wx0 = x0 >> 1;
    float4 gq[2], xq[2];
    uchar4 aq[2];
    bool okq[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int item = t + 256 * k;                       // 25 pooled pixels x 16 quads = 400 items
        const int pp = item >> 4, q = item & 15;
        const int wy = wy0 + pp / 5, wx = wx0 + pp % 5;
        okq[k] = item < 400 && wy < a.p1.H && wx < a.p1.W;
        const int64_t pr = (int64_t)n * a.p1.HWp + (okq[k] ? wy * a.p1.W + wx : 0);
        gq[k] = ldq<GT>(a.g1.g, pr * a.g1.ldg + 4 * q);
        xq[k] = ldq<XT>(a.g1.x, pr * a.g1.ldx + 4 * q);
        aq[k] = *reinterpret_cast<const uchar4*>(a.argmax + pr * 64 + 4 * q);
    }
    __syncthreads();                                        // prm ready; previous tile's gl / al consumed
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int item = t + 256 * k;
        if (item < 400) {
            const int pp = item >> 4, q = item & 15;
            float4 gv = affine2(gq[k], xq[k], prm + 256 + 4 * q, 64);
            if (!okq[k]) gv = zero4();
            *reinterpret_cast<float4*>(&gl[pp][4 * q]) = gv;
            *reinterpret_cast<uchar4*>(&al[pp][4 * q]) = okq[k] ? aq[k] : make_uchar4(255, 255, 255, 255);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int lp = slot + 16 * i;
        const int y = y0 + (lp >> 3), x = x0 + (lp & 7);
        float g[4] = {0, 0, 0, 0};
        const int py0 = y >> 1, py1 = (y + 1) >> 1, px0 = x >> 1, px1 = (x + 1) >> 1;
        for (int wy = py0; wy <= py1; ++wy)
            for (int wx = px0; wx <= px1; ++wx) {
                const int k = (y - (2 * wy - 1)) * 3 + (x - (2 * wx - 1));   // my index inside that window
                const int pp = (wy - wy0) * 5 + (wx - wx0);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (al[pp][4 * cq + c] == k) g[c] += gl[pp][4 * cq + c];
            }
        const float st[4] = {sv[i].x, sv[i].y, sv[i].z, sv[i].w};
        float dy[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            dy[c] = bn1(st[c], prm[128 + 4 * cq + c], prm[4 * cq + c], prm[64 + 4 * cq + c]) > 0.f ? g[c] : 0.f;
            s1[c] += dy[c];
            s2[c] += dy[c] * ((st[c] - prm[128 + 4 * cq + c]) * prm[192 + 4 * cq + c]);
        }
        *reinterpret_cast<float4*>(a.DY0 + srow[i] * 64 + 4 * cq) = make_float4(dy[0], dy[1], dy[2], dy[3]);
    }
    }   // tiles
#pragma unroll
    for (int c = 0; c < 4; ++c) { red[0][slot][4 * cq + c] = s1[c]; red[1][slot][4 * cq + c] = s2[c]; }
    __syncthreads();
    if (t < 128) {
        const int q = t >> 6, c = t & 63;
        float tot = 0.f;
        for (int k = 0; k < 16; ++k) tot += red[q][k][c];
        stat_sink_add<S_BWD>(a.st, n, c, q, (double)tot);
        // (norm0's dbeta / dgamma are these sums over the streams: db_flush_kernel adds them - 3400 workgroups on one address per
        // channel here were the tail of this kernel)
    }
}

// ------------------------------------------------------------------------------------
// The same tail at POOLED resolution (precision mode 0, one-channel stem): conv0's weight gradient without a pass over the stem
// plane and without DY0.  The gradient that pool0 / relu0 route to the stem is sparse - each (pooled pixel q, channel c) sends
// gm[q, c] to ONE stem pixel pos(q, c), the argmax of its window, and the argmax element passed the ReLU exactly when
// X1[q, c] > 0 - and conv0 is linear without bias, so with A = a*dy + b*x + c (the BN-backward operand of BwdWeightP: a = gamma *
// invstd, b = -a * k, c = a * (k * mean - q1)) and x[p, c] = sum_t' w[c, t'] * I[2p + t' - 3]
//   dW0[c, t] = sum_n ( a_nc * T1_n[c, t] + b_nc * sum_t' w[c, t'] * R_n[t', t] + c_nc * S_n[t] )
//   T1_n[c, t] = sum_q gm_n[q, c] * I_n[2 pos(q, c) + t - 3]             stem_tail_kernel (+ norm0's s1 / s2 sums, as pool0_bwd_kernel)
//   R_n[t', t] = sum_p I_n[2p + t' - 3] * I_n[2p + t - 3],  S_n[t] = sum_p I_n[2p + t - 3]     stem_moments_kernel: the image only
// stem_combine_kernel adds the b and c terms in fp64.  (tests/test_cpu_stem_tail_identity.py checks the identity in float64.)
// ------------------------------------------------------------------------------------
// stem_tail_kernel: workgroup = tiles of 16 x 4 pooled pixels x 64 channels.  Per tile the 71 x 23 image pixels its patches can
// touch (image row of tap ty of window element ky of pooled row qy: 4 qy - 5 + 2 ky + ty) sit in LDS together with gm and each
// (pixel, channel)'s patch origin; thread = (channel, a quarter of the 49 taps) then walks the tile's 64 pixels.  Lanes of a
// half-wave read at most the 9 origins of one pooled pixel: pitch 75 = 11 mod 32 keeps {0, 2, 4} + {0, 2, 4} * pitch on
// nine banks.  A workgroup leaves ONE 64 x 64 partial tile (columns 49.. zero), already scaled by a_nc: reduce_partials_kernel
// sums them in a fixed order - no atomics on the gradient.
constexpr int kTailTW = 16, kTailTH = 4, kTailIW = 4 * kTailTW + 7, kTailIH = 4 * kTailTH + 7, kTailPitch = 75, kTailGl = 65;
struct StemTailArgs {
    GradSrc g1; Plane p1;                                    // block 1's G' / X, channels 0..63 (fp32: mode 0)
    const unsigned char* argmax; const float* stemv;         // [n][p1.HWp][64] (pool0_kernel)
    ActSrc stem; Plane ps;                                   // stem stats [n][64] and norm0 (no plane: x unset)
    const float* img; Plane pi;                              // one-channel image [n][pi.HWp]
    StatSink st;                                             // [n][64]
    float* part;                                             // [n][gridDim.x][64][64]
    int tiles_x, n_tiles, tiles_per_wg;
};

template <int T0, int NT>
__device__ __forceinline__ void stem_tail_taps(float (&acc)[13], const float* gl, const unsigned short* ol, const float* it, int c) {
#pragma unroll 2
    for (int q = 0; q < kTailTW * kTailTH; ++q) {
        const float g = gl[q * kTailGl + c];
        const float* ip = it + ol[q * 64 + c];
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = fmaf(g, ip[((T0 + j) / 7) * kTailPitch + (T0 + j) % 7], acc[j]);
    }
}
template <int T0, int NT>
__device__ __forceinline__ void stem_tail_put(const float (&acc)[13], float* gl, int c, float a) {
#pragma unroll
    for (int j = 0; j < NT; ++j) gl[c * kTailGl + T0 + j] = acc[j] * a;
}

static __global__ __launch_bounds__(256) void stem_tail_kernel(const StemTailArgs a) {
    __shared__ float prm[7 * 64];
    __shared__ float gl[64 * kTailGl];                       // gm [pixel][channel]; at the end the partial tile [channel][tap], then the sums
    __shared__ unsigned short ol[64 * 64];                   // patch origin in `it`
    __shared__ float it[kTailIH * kTailPitch];
    static_assert(2 * 16 * 64 <= 64 * kTailGl, "the s1 / s2 reduction reuses gl");
    const int n = blockIdx.y, t = threadIdx.x, cq = t & 15, slot = t >> 4;
    if (t < 64) {
        const ActCoef s0 = act_src_coef<A_SUMS, 1>(a.stem, n, t, 1.0 / (double)a.ps.HW);      // (gamma alone)
        prm[256 + t] = s0.mean; prm[320 + t] = s0.invstd; prm[384 + t] = s0.gamma * s0.invstd;
        const double inv = 1.0 / (double)a.p1.HW;
        const GradCoef f = grad_src_coef(a.g1, n, t, inv);
        prm[t] = f.a; prm[64 + t] = f.q1; prm[128 + t] = f.mean; prm[192 + t] = f.k;
    }
    float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    float acc[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const float* img = a.img + (int64_t)n * a.pi.HWp;
    const int tile0 = blockIdx.x * a.tiles_per_wg, tile1 = min(tile0 + a.tiles_per_wg, a.n_tiles);
    for (int tile = tile0; tile < tile1; ++tile) {
        const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        const int qy0 = ty * kTailTH, qx0 = tx * kTailTW;
        float4 gq[4], xq[4], sq[4];
        uchar4 aq[4];
        bool okq[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int lp = slot + 16 * i;                       // local pixel 0..63 = 4 rows of 16
            const int qy = qy0 + (lp >> 4), qx = qx0 + (lp & 15);
            okq[i] = qy < a.p1.H && qx < a.p1.W;
            const int64_t pr = (int64_t)n * a.p1.HWp + (okq[i] ? qy * a.p1.W + qx : 0);
            gq[i] = ld4(static_cast<const float*>(a.g1.g) + pr * a.g1.ldg + 4 * cq);
            xq[i] = ld4(static_cast<const float*>(a.g1.x) + pr * a.g1.ldx + 4 * cq);
            sq[i] = ld4(a.stemv + pr * 64 + 4 * cq);
            aq[i] = *reinterpret_cast<const uchar4*>(a.argmax + pr * 64 + 4 * cq);
        }
        constexpr int kImg = kTailIH * kTailIW, kImgLoads = (kImg + 255) / 256;
        float iv[kImgLoads];
        const int iy0 = 4 * qy0 - 5, ix0 = 4 * qx0 - 5;
#pragma unroll
        for (int j = 0; j < kImgLoads; ++j) {
            const int idx = t + 256 * j, r = idx / kTailIW, cc = idx - r * kTailIW;
            const int y = iy0 + r, x = ix0 + cc;
            const bool in = idx < kImg && (unsigned)y < (unsigned)a.pi.H && (unsigned)x < (unsigned)a.pi.W;      // zero outside the image
            iv[j] = img[in ? y * a.pi.W + x : 0];
            if (!in) iv[j] = 0.f;
        }
        __syncthreads();                                        // prm ready; the previous tile's gl / ol / it consumed
#pragma unroll
        for (int j = 0; j < kImgLoads; ++j) {
            const int idx = t + 256 * j, r = idx / kTailIW, cc = idx - r * kTailIW;
            if (idx < kImg) it[r * kTailPitch + cc] = iv[j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int lp = slot + 16 * i;
            const float4 gv = affine2(gq[i], xq[i], prm + 4 * cq, 64);
            const float g4[4] = {gv.x, gv.y, gv.z, gv.w}, x4[4] = {xq[i].x, xq[i].y, xq[i].z, xq[i].w}, v4[4] = {sq[i].x, sq[i].y, sq[i].z, sq[i].w};
            const int k4[4] = {aq[i].x, aq[i].y, aq[i].z, aq[i].w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool on = okq[i] && x4[c] > 0.f;          // the argmax element passed the ReLU
                const float gm = on ? g4[c] : 0.f;
                s1[c] += gm;
                s2[c] += gm * ((v4[c] - prm[256 + 4 * cq + c]) * prm[320 + 4 * cq + c]);
                const int k = on ? k4[c] : 0;
                gl[lp * kTailGl + 4 * cq + c] = gm;
                ol[lp * 64 + 4 * cq + c] = (unsigned short)((4 * (lp >> 4) + 2 * (k / 3)) * kTailPitch + 4 * (lp & 15) + 2 * (k % 3));
            }
        }
        __syncthreads();
        switch (t >> 6) {                                       // (wave-uniform)
            case 0: stem_tail_taps<0, 13>(acc, gl, ol, it, t & 63); break;
            case 1: stem_tail_taps<13, 12>(acc, gl, ol, it, t & 63); break;
            case 2: stem_tail_taps<25, 12>(acc, gl, ol, it, t & 63); break;
            default: stem_tail_taps<37, 12>(acc, gl, ol, it, t & 63); break;
        }
    }
    __syncthreads();
    {
        const int c = t & 63;
        const float an = prm[384 + c];
        switch (t >> 6) {
            case 0: stem_tail_put<0, 13>(acc, gl, c, an); break;
            case 1: stem_tail_put<13, 12>(acc, gl, c, an); break;
            case 2: stem_tail_put<25, 12>(acc, gl, c, an); break;
            default: stem_tail_put<37, 12>(acc, gl, c, an); break;
        }
    }
    __syncthreads();
    float* po = a.part + ((int64_t)n * gridDim.x + blockIdx.x) * (64 * 64);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = t + 256 * i, c = e >> 6, col = e & 63;
        po[e] = col < 49 ? gl[c * kTailGl + col] : 0.f;
    }
    __syncthreads();
    float* red = gl;                                            // [2][16][64]
#pragma unroll
    for (int c = 0; c < 4; ++c) { red[(0 * 16 + slot) * 64 + 4 * cq + c] = s1[c]; red[(1 * 16 + slot) * 64 + 4 * cq + c] = s2[c]; }
    __syncthreads();
    if (t < 128) {
        const int q = t >> 6, c = t & 63;
        float tot = 0.f;
        for (int k = 0; k < 16; ++k) tot += red[(q * 16 + k) * 64 + c];
        stat_sink_add<S_BWD>(a.st, n, c, q, (double)tot);      // (db_flush_kernel: norm0's dbeta / dgamma)
    }
}

// stem_moments_kernel: R_n and S_n of one stream's image over tiles of 16 x 16 stem pixels, whose 37 x 37 image pixels sit in LDS.
// The 49 x 49 matrix R is symmetric: its tap ROWS pair up into 28 blocks (ra <= rb) of 7 x 7 products, and seven more blocks
// (ra, a row {1, 0, ..}) carry S in their first column - thread = (one of 7 pixel slices, block), 49 fp32 accumulators, 14 LDS reads per
// 49 multiply-adds.  A workgroup sums its slices in a fixed order and leaves 35 x 49 floats; stem_moments_sum_kernel adds the
// workgroups of a stream in fp64.  (pitch 39 = 7 mod 32: the 7 rows x 2 slices a half-wave reads lie on 14 banks)
constexpr int kMomT = 16, kMomI = 2 * kMomT + 5, kMomPitch = 39, kMomJobs = 35, kMomSlices = 7, kMomVals = kMomJobs * 49;
struct StemMomArgs {
    const float* img; Plane pi; Plane ps;                     // one-channel image [n][pi.HWp]; the stem plane
    float* part;                                             // [n][gridDim.x][kMomVals]
    int tiles_x, n_tiles, tiles_per_wg;
};
__host__ __device__ __forceinline__ int stem_mom_block(int ra, int rb) { return ra * 7 - ra * (ra - 1) / 2 + (rb - ra); }      // ra <= rb < 7

static __global__ __launch_bounds__(256) void stem_moments_kernel(const StemMomArgs a) {
    __shared__ float it[kMomI * kMomPitch + 8];
    __shared__ float red[kMomVals];
    const int n = blockIdx.y, t = threadIdx.x;
    const int slice = t / kMomJobs, job = t - slice * kMomJobs;      // (threads 245..255 only load)
    int ra = 0, rb = 7;
    if (job >= 28) ra = job - 28;
    else {
        int j = job;
        while (j >= 7 - ra) { j -= 7 - ra; ++ra; }
        rb = ra + j;
    }
    float acc[7][7];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) acc[i][j] = 0.f;
    if (t < 8) it[kMomI * kMomPitch + t] = t == 0 ? 1.f : 0.f;
    const float* img = a.img + (int64_t)n * a.pi.HWp;
    const int tile0 = blockIdx.x * a.tiles_per_wg, tile1 = min(tile0 + a.tiles_per_wg, a.n_tiles);
    for (int tile = tile0; tile < tile1; ++tile) {
        const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        const int y0 = ty * kMomT, x0 = tx * kMomT;
        constexpr int kImg = kMomI * kMomI, kImgLoads = (kImg + 255) / 256;
        float iv[kImgLoads];
#pragma unroll
        for (int j = 0; j < kImgLoads; ++j) {
            const int idx = t + 256 * j, r = idx / kMomI, cc = idx - r * kMomI;
            const int y = 2 * y0 - 3 + r, x = 2 * x0 - 3 + cc;
            const bool in = idx < kImg && (unsigned)y < (unsigned)a.pi.H && (unsigned)x < (unsigned)a.pi.W;
            iv[j] = img[in ? y * a.pi.W + x : 0];
            if (!in) iv[j] = 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kImgLoads; ++j) {
            const int idx = t + 256 * j, r = idx / kMomI, cc = idx - r * kMomI;
            if (idx < kImg) it[r * kMomPitch + cc] = iv[j];
        }
        __syncthreads();
        if (slice < kMomSlices) {
            for (int p = slice; p < kMomT * kMomT; p += kMomSlices) {
                const int ly = p >> 4, lx = p & 15;
                if (y0 + ly >= a.ps.H || x0 + lx >= a.ps.W) continue;
                const float* pa = it + (2 * ly + ra) * kMomPitch + 2 * lx;
                const float* pb = rb < 7 ? it + (2 * ly + rb) * kMomPitch + 2 * lx : it + kMomI * kMomPitch;
                float av[7], bv[7];
#pragma unroll
                for (int i = 0; i < 7; ++i) { av[i] = pa[i]; bv[i] = pb[i]; }
#pragma unroll
                for (int i = 0; i < 7; ++i)
#pragma unroll
                    for (int j = 0; j < 7; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
            }
        }
    }
    float tot[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < kMomSlices; ++s) {
        __syncthreads();
        if (slice == s) {
#pragma unroll
            for (int i = 0; i < 7; ++i)
#pragma unroll
                for (int j = 0; j < 7; ++j) red[job * 49 + i * 7 + j] = acc[i][j];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const int e = t + 256 * i;
            if (e < kMomVals) tot[i] += red[e];
        }
    }
    float* po = a.part + ((int64_t)n * gridDim.x + blockIdx.x) * kMomVals;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int e = t + 256 * i;
        if (e < kMomVals) po[e] = tot[i];
    }
}

// stem_moments_sum_kernel: the workgroups' partials of a stream in fp64, unfolded for the combine: mom[n] = 50 rows of 49 - row u < 49 is
// R_n[u][.] (both triangles), row 49 is S_n.
constexpr int kMomRows = 50, kMomOut = kMomRows * 49;
static __global__ void stem_moments_sum_kernel(const float* part, int groups, double* mom) {      // mom [n][kMomOut]
    const int n = blockIdx.y, o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= kMomOut) return;
    const int u = o / 49, t = o - u * 49, uy = u / 7, ux = u - uy * 7, ty = t / 7, tx = t - ty * 7;
    const int e = u == 49 ? (28 + ty) * 49 + tx * 7
                          : uy <= ty ? stem_mom_block(uy, ty) * 49 + ux * 7 + tx : stem_mom_block(ty, uy) * 49 + tx * 7 + ux;
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s += (double)part[((int64_t)n * groups + g) * kMomVals + e];
    mom[(int64_t)n * kMomOut + o] = s;
}

// stem_combine_kernel: dW0[c, t] += sum_n ( b_nc * sum_u w[c, u] * R_n[u, t] + c_nc * S_n[t] ) in fp64, to all three input channels
// (behind the reduce of stem_tail_kernel's partial tiles on the same stream).  a | q1 | mean | k are those of the operand
// a * ((dy - q1) - (x - mean) * k) that BwdWeightP forms from the same descriptor (grad_src_coef).  Workgroup = channel c: the sum over
// (stream, row of mom) is one dot product of ns * 50 terms per tap, cut into four fixed quarters (thread = (tap, quarter)).
struct StemCombineArgs {
    const double* mom; const float* w0;                      // moments [n][kMomOut]; conv0's master weight [64][3][49]
    GradSrc dy;                                              // dy0 through norm0 - its statistics only: stem stats, norm0's backward sums [n][64], gamma
    int HW; int ns;
    float* dw;                                               // [64][3][49]
};
static __global__ __launch_bounds__(256) void stem_combine_kernel(const StemCombineArgs a) {
    extern __shared__ double cmb[];                          // coef [ns][50] | red [4][64]
    double* coef = cmb;
    double* red = cmb + a.ns * kMomRows;
    const int c = blockIdx.x, tid = threadIdx.x;
    const double inv = 1.0 / (double)a.HW;
    for (int n = tid; n < a.ns; n += 256) {
        const GradCoef f = grad_src_coef(a.dy, n, c, inv);
        coef[n * kMomRows + 48] = -(double)f.a * (double)f.k;                                      // b_nc: times w[c, u] into slots 0..48 below
        coef[n * kMomRows + 49] = (double)f.a * ((double)f.k * (double)f.mean - (double)f.q1);     // c_nc
    }
    __syncthreads();
    for (int k = tid; k < a.ns * 49; k += 256) {
        const int n = k / 49, u = k - n * 49;
        if (u == 48) continue;
        coef[n * kMomRows + u] = coef[n * kMomRows + 48] * ((double)a.w0[c * 147 + u] + (double)a.w0[c * 147 + 49 + u] + (double)a.w0[c * 147 + 98 + u]);
    }
    __syncthreads();
    for (int n = tid; n < a.ns; n += 256) coef[n * kMomRows + 48] *= (double)a.w0[c * 147 + 48] + (double)a.w0[c * 147 + 97] + (double)a.w0[c * 147 + 146];
    __syncthreads();
    const int t = tid & 63, qt = tid >> 6, K = a.ns * kMomRows;
    const int k0 = (int)((int64_t)K * qt / 4), k1 = (int)((int64_t)K * (qt + 1) / 4);
    double v0 = 0.0, v1 = 0.0;
    if (t < 49) {
        int k = k0;
        for (; k + 1 < k1; k += 2) {
            v0 += coef[k] * a.mom[(int64_t)k * 49 + t];
            v1 += coef[k + 1] * a.mom[(int64_t)(k + 1) * 49 + t];
        }
        if (k < k1) v0 += coef[k] * a.mom[(int64_t)k * 49 + t];
    }
    red[qt * 64 + t] = v0 + v1;
    __syncthreads();
    if (tid < 49) {
        const float v = (float)((red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]));
        for (int cc = 0; cc < 3; ++cc) a.dw[c * 147 + cc * 49 + tid] += v;
    }
}

// ------------------------------------------------------------------------------------
// BN backward applied once: out = a*((g - q1) - (x - mean)*k) for a C-channel slice
// of one stream's plane (C = 32: the finalized gradient of a dense layer's output
// slice; C = 128: the gradient of a bottleneck through norm2).  The data- and
// weight-gradient GEMMs that follow then stream ONE array instead of two.
// ------------------------------------------------------------------------------------
struct BnBwdApplyArgs {
    GradSrc src;                                  // G' and x of the C channels, gradient / activation storage of the mode
    Plane pl; int C;
    void* out; int ldo;
    AffineSink aff;                               // if set: the affine gradients, dbeta += sum_n s1[n], dgamma += sum_n s2[n]
                                                  // (one fp32 atomic per stream and channel instead of one per producer tile)
    unsigned* amax;                               // if set: [streams][kAmaxRep] - the largest |out| of each stream as float bits (atomicMax per
                                                  // workgroup): the scale of the consumers' fp16-split operand (gemm.cuh, operand kind 3)
};

// rows of a plane per workgroup: the 16-bit modes move half the bytes per row, so a workgroup takes twice the rows
constexpr int bn_apply_rows(int prec) { return prec ? 128 : 64; }
template <int PREC>
static __global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const BnBwdApplyArgs a) {
    using XT = act_t<PREC>;
    using GT = grd_t<PREC>;
    constexpr int E = 16 / GT::size;              // channels per 16-byte slot: 4 (fp32 storage) or 8 (16-bit storage)
    constexpr int RPW = bn_apply_rows(PREC);      // rows per workgroup
    static_assert(GT::size == XT::size, "one slot geometry");
    __shared__ float prm[4 * 128];
    const int n = blockIdx.y, t = threadIdx.x;
    const int spr = a.C / E;                      // slots per row
    const int rows_per_pass = 256 / spr;
    const int cs = t % spr;
    const int r0 = blockIdx.x * RPW + t / spr;
    // RPW rows per workgroup: up to 8 row slots per thread.  The data loads go out FIRST (unconditional, clamped row) so that
    // they share one memory round trip with the parameter prologue below; all loads before any store (the output may alias
    // the gradient input - it does for the in-place norm2 case).
    float4 gv[8], xv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int r = r0 + k * rows_per_pass;
        if (k * rows_per_pass >= RPW) break;           // (workgroup-uniform: C = 32 uses two slots, C = 128 eight)
        const int64_t pix = (int64_t)n * a.pl.HWp + (r < a.pl.HW ? r : 0);
        gv[k] = ld16(a.src.g, (int64_t)GT::size * (pix * a.src.ldg + E * cs));
        xv[k] = ld16(a.src.x, (int64_t)XT::size * (pix * a.src.ldx + E * cs));
    }
    if (t < a.C) {
        const GradCoef f = grad_src_coef(a.src, n, t, 1.0 / (double)a.pl.HW);
        prm[t] = f.a;
        prm[a.C + t] = f.q1;
        prm[2 * a.C + t] = f.mean;
        prm[3 * a.C + t] = f.k;
        if (a.aff.dbeta && blockIdx.x == 0)       // (the whole sums, not coefficients)
            affine_sink_add2(a.aff, t, (float)stat_get(a.src.s1, (int64_t)n * a.src.sstride + t), (float)stat_get(a.src.s2, (int64_t)n * a.src.sstride + t));
    }
    __syncthreads();
    float vmax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int r = r0 + k * rows_per_pass;
        if (k * rows_per_pass < RPW && r < a.pl.HW) {
            const int64_t pix = (int64_t)n * a.pl.HWp + r;
            if constexpr (E == 4) {
                const float4 o = affine2(gv[k], xv[k], prm + 4 * cs, a.C);
                stq<GT>(a.out, pix * a.ldo + 4 * cs, o);
                vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
            } else {
                const u32x4 u = pack_unit<1>(affine2(slot_quad<GT>(gv[k], 0), slot_quad<XT>(xv[k], 0), prm + 8 * cs, a.C),
                                             affine2(slot_quad<GT>(gv[k], 1), slot_quad<XT>(xv[k], 1), prm + 8 * cs + 4, a.C));   // gradients: bf16
                *reinterpret_cast<u32x4*>(static_cast<char*>(a.out) + (int64_t)GT::size * (pix * a.ldo + 8 * cs)) = u;
            }
        }
    }
    if constexpr (E == 4) {
        if (a.amax) {                             // (launch-uniform) largest |out| of the workgroup -> this stream's replica
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
            __syncthreads();                      // prm is free again
            if ((t & 63) == 0) prm[t >> 6] = vmax;
            __syncthreads();
            if (t == 0) {
                vmax = fmaxf(fmaxf(prm[0], prm[1]), fmaxf(prm[2], prm[3]));
                if (vmax > 0.f) atomicMax(a.amax + (int64_t)n * kAmaxRep + (blockIdx.x % kAmaxRep), __float_as_uint(vmax));
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// The same for the bottleneck gradient of precision mode 0 (C = 128, through norm2), written in UNIT form (gemm.cuh, kD2K8):
// a workgroup owns one 64-pixel scale block of one stream - it computes the block's 64 x 128 outputs in registers, takes their
// largest magnitude, scales by the power of two that puts it into [2^13, 2^14), splits into the two fp16 pieces and stores them
// as 16-byte units [piece][channel / 8][pixel]: what the three consumers' MFMAs read, with no arithmetic left for their k-loops.
// Rows of the plane padding are written as zeros (the consumers need no row mask).  Thread t: channel quad t / 8, rows t % 8 + 8 k -
// eight consecutive pixels of one quad side by side, so loads and stores both move 128-byte runs.
// ------------------------------------------------------------------------------------
struct BnBwdApplySplitArgs {
    GradSrc src;                                  // raw 3x3 data gradient dy and the bottleneck activation norm2 normalised: fp32 [n][HWp][128]
    Plane pl;
    u32x4* out;                                   // units of this ring slot
    float* binv;                                  // [streams][HWp / 64] inverse block scales
    AffineSink aff;                               // norm2's affine gradients (one fp32 atomic per stream and channel)
};
static __global__ __launch_bounds__(256) void bn_bwd_apply_split_kernel(const BnBwdApplySplitArgs a) {
    constexpr int C = 8 * kD2K8;
    __shared__ float prm[4 * C];
    __shared__ float red[4];
    const int n = blockIdx.y, t = threadIdx.x;
    const int cs = t >> 3, rr = t & 7;
    const int r0 = blockIdx.x * kScaleBlock + rr;
    float4 gv[8], xv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                 // the data loads first: one memory round trip with the parameter prologue
        const int r = r0 + 8 * k;
        const int64_t pix = (int64_t)n * a.pl.HWp + (r < a.pl.HW ? r : 0);
        gv[k] = ld4(static_cast<const float*>(a.src.g) + pix * C + 4 * cs);
        xv[k] = ld4(static_cast<const float*>(a.src.x) + pix * C + 4 * cs);
    }
    if (t < C) {
        const double inv = 1.0 / (double)a.pl.HW;
        float mean, invstd;
        // (not grad_src_coef: s1 / s2 stay doubles here, for the coefficients AND the affine gradients below)
        const GradSrc& g = a.src;
        tab_or_moments(g.xtab, n, t, g.xsum, g.xsq, (int64_t)n * g.sstride + t, inv, g.eps, mean, invstd);
        const double s1 = stat_get(g.s1, (int64_t)n * g.sstride + t), s2 = stat_get(g.s2, (int64_t)n * g.sstride + t);
        prm[t] = g.gamma[t] * invstd;
        prm[C + t] = (float)(s1 * inv);
        prm[2 * C + t] = mean;
        prm[3 * C + t] = invstd * (float)(s2 * inv);
        if (a.aff.dbeta && blockIdx.x == 0) affine_sink_add2(a.aff, t, (float)s1, (float)s2);
    }
    __syncthreads();
    float vmax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 o = r0 + 8 * k < a.pl.HW ? affine2(gv[k], xv[k], prm + 4 * cs, C) : zero4();
        gv[k] = o;
        vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
    if ((t & 63) == 0) red[t >> 6] = vmax;
    __syncthreads();
    vmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    ActScale sc{1.f, 1.f};
    if (vmax > 0.f) sc = scale_of_max(__float_as_uint(vmax));      // (a block of zeros keeps scale 1)
    if (t == 0) a.binv[(int64_t)n * (a.pl.HWp / kScaleBlock) + blockIdx.x] = sc.inv;
    char* ob = reinterpret_cast<char*>(a.out + d2_stream_units(n, a.pl.HWp));
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const Split4 s = split4<3>(mul4(gv[k], sc.s));
        const int64_t at = ((int64_t)(cs >> 1) * a.pl.HWp + r0 + 8 * k) * 16 + (cs & 1) * 8;
        *reinterpret_cast<uint2*>(ob + at) = s.p[0];
        *reinterpret_cast<uint2*>(ob + at + (int64_t)kD2K8 * a.pl.HWp * 16) = s.p[1];
    }
}

// Sum the replicas of the dbeta / dgamma scratch (engine.h) into the gradient array and leave the scratch zeroed for the next call.
struct DbSegD { int64_t grad_off; int scr_off; int n; };
static __global__ void db_flush_kernel(const DbSegD* segs, float* scr, int rep_stride, int reps, float* grads,
                                       const double* stem1, const double* stem2, int ns, float* dbeta0, float* dgamma0) {
    if (blockIdx.y == gridDim.y - 1) {       // norm0: dbeta / dgamma = pool0_bwd's per-stream sums, summed over the streams
        if (blockIdx.x == 0 && threadIdx.x < 128 && stem1) {
            const int q = threadIdx.x >> 6, c = threadIdx.x & 63;
            double v = 0.0;
            for (int n = 0; n < ns; ++n) v += stat_get(q ? stem2 : stem1, (int64_t)n * 64 + c);
            (q ? dgamma0 : dbeta0)[c] += (float)v;
        }
        return;
    }
    const DbSegD sg = segs[blockIdx.y];
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < sg.n; k += gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int r = 0; r < reps; ++r) {
            float* q = scr + (int64_t)r * rep_stride + sg.scr_off + k;
            v += *q;
            *q = 0.f;
        }
        grads[sg.grad_off + k] += v;
    }
}

// Zero the rows/columns of a gradient plane that an odd-sized 2x2/stride-2 average
// pool never reads (they receive no gradient from the transition).
template <int PREC>
static __global__ void zero_uncovered_kernel(void* G, int ld, Plane p, int Hc, int Wc, int C) {
    using GT = grd_t<PREC>;
    const int n = blockIdx.y;
    const int64_t total = (int64_t)p.HW * (C / 4);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int pix = (int)(i / (C / 4)), cq = (int)(i - (int64_t)pix * (C / 4));
        const int y = pix / p.W, x = pix - y * p.W;
        if (y >= Hc || x >= Wc) stq<GT>(G, ((int64_t)n * p.HWp + pix) * ld + 4 * cq, zero4());
    }
}

// ------------------------------------------------------------------------------------
// The two trees a workgroup's 256 threads end in: the best (value, index) and the sum.
// ------------------------------------------------------------------------------------
// Largest value and its index, exactly like np.argmax: lowest index on ties, and a NaN beats every number (the FIRST NaN
// wins) - a diverged network surfaces as a NaN best value instead of an arbitrary but valid-looking action.
__device__ __forceinline__ bool argmax_better(float x, int i, float bx, int bi) {
    if (bi == 0x7fffffff) return true;                  // nothing held yet
    const bool xn = x != x, bn = bx != bx;
    if (xn != bn) return xn;
    if (xn) return i < bi;
    return x > bx || (x == bx && i < bi);
}
// The tree over a workgroup's 256 (value, index) slots, thread t's own in bv[t], bi[t] (LDS): the best by argmax_better's rules ends
// in slot 0.  A slot with index 0x7fffffff is empty and never wins.
__device__ __forceinline__ void block_argmax(float* bv, int* bi, int t) {
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            const float x = bv[t + s]; const int j = bi[t + s];
            if (j != 0x7fffffff && argmax_better(x, j, bv[t], bi[t])) { bv[t] = x; bi[t] = j; }
        }
        __syncthreads();
    }
}
// The fixed sum tree over a workgroup's 256 slots of one or more LDS arrays (thread t's own in r[t]): the sums end in slot 0 of
// each.  The pairing order is part of the results (double sums, bit for bit).
template <class... T>
__device__ __forceinline__ void block_sum(int t, T*... r) {
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { ((r[t] += r[t + s]), ...); }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------
// Losses (code/trainer.py:345-348 Huber on element [0,0,0,0]; :296-299 +
// code/utils.py:306-313 class-weighted cross entropy, weights {1,1,0}).
// ------------------------------------------------------------------------------------
static __global__ void loss_kernel(int mode, const float* q, const float* labels, int n_pairs, int per_pair,
                            float* loss, float* dq) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_pairs) return;
    const float* qj = q + (int64_t)j * per_pair;
    float* dj = dq + (int64_t)j * per_pair;
    for (int i = 0; i < per_pair; ++i) dj[i] = 0.f;
    if (mode == 0) {
        const float d = qj[0] - labels[j];
        if (fabsf(d) < 1.f) { loss[j] = 0.5f * (d * d); dj[0] = d; }
        else { loss[j] = fabsf(d) - 0.5f; dj[0] = d > 0.f ? 1.f : -1.f; }
    } else {
        // labels outside {0, 1, 2} count as class 2 ("no loss", weight 0); the reference only ever emits 0 / 1
        // (code/trainer.py:220-234).  A zero class weight gives loss 0 and no gradient - torch's weighted mean
        // would be 0/0 there and poison every gradient and Adam moment with NaN.
        const float lf = labels[j];
        const int y = (lf >= 0.f && lf < 2.5f) ? (int)lf : 2;
        const float m = fmaxf(qj[0], fmaxf(qj[1], qj[2]));
        const float e0 = expf(qj[0] - m), e1 = expf(qj[1] - m), e2 = expf(qj[2] - m);
        const float se = e0 + e1 + e2, lse = logf(se) + m;
        if (y == 2) {
            loss[j] = 0.f;
        } else {
            loss[j] = lse - qj[y];                   // size_average: weighted mean over 1 element of weight 1
            const float sm[3] = {e0 / se, e1 / se, e2 / se};
            for (int c = 0; c < 3; ++c) dj[c] = sm[c] - (c == y ? 1.f : 0.f);
        }
    }
}

// Whole-map Huber (smg_loss_map): loss[j] = sum over the map of w * huber(q - label), dq = w * huber'(q - label), the Huber of
// code/trainer.py:345-348 per element; weight == nullptr: all ones, a weight of 0 masks its element.  One workgroup per pair: thread t takes elements t, t + 256, ...
// in that order, and the 256 partial sums meet in LDS in a fixed tree.
static __global__ __launch_bounds__(256) void loss_map_kernel(const float* q, const float* label, const float* weight, int per_pair,
                                                              float* loss, float* dq) {
    __shared__ float red[256];
    const int j = blockIdx.x, t = threadIdx.x;
    const int64_t o = (int64_t)j * per_pair;
    float sum = 0.f;
    for (int i = t; i < per_pair; i += 256) {
        const float d = q[o + i] - label[o + i];
        const float w = weight ? weight[o + i] : 1.f;
        float l, g;
        if (fabsf(d) < 1.f) { l = 0.5f * (d * d); g = d; }
        else { l = fabsf(d) - 0.5f; g = d > 0.f ? 1.f : -1.f; }
        // a weight of exactly zero masks the element whatever q holds there (no -0, no 0 * inf)
        sum += w == 0.f ? 0.f : w * l;
        dq[o + i] = w == 0.f ? 0.f : w * g;
    }
    red[t] = sum;
    block_sum(t, red);
    if (t == 0) loss[j] = red[0];
}

// Whole-map cross entropy of a 3-class head (smg_loss_map_ce): the reference's CrossEntropyLoss2d (code/utils.py:306-313, class
// weights {1, 1, 0}: code/trainer.py:38-60) on the whole head output instead of the one pixel of code/trainer.py:296-299 - torch's
// weighted-mean nll_loss per pair.  q [n][3][P], label [n][1][P] float class indices (anything but 0 / 1 is class 2, "no loss"):
//     nll_p = logsumexp(q[:, p]) - q[y_p, p],  W = number of pixels of class 0 / 1,  loss = sum nll_p / W,
//     dq[c][p] = (softmax(q[:, p])[c] - [c == y_p]) / W;   class-2 pixels: no term, dq exactly 0 whatever q holds;  W == 0: loss 0, dq 0.
// Per pixel the arithmetic of loss_kernel mode 1, operation for operation (a map with one weighted pixel reproduces it bit for
// bit: x / 1 and 1 * x are exact).  One workgroup per pair, two passes: the two sums (thread t takes pixels t, t + 256, ... in that
// order, the 256 partial sums meet in LDS in a fixed tree), then dq.
static __global__ __launch_bounds__(256) void loss_map_ce_kernel(const float* q, const float* label, int P, float* loss, float* dq) {
    __shared__ float red[2][256];
    const int j = blockIdx.x, t = threadIdx.x;
    const float* qj = q + (int64_t)j * 3 * P;
    const float* lj = label + (int64_t)j * P;
    float* dj = dq + (int64_t)j * 3 * P;
    float sum = 0.f, cnt = 0.f;
    for (int p = t; p < P; p += 256) {
        const float lf = lj[p];
        if (lf != 0.f && lf != 1.f) continue;
        const float q0 = qj[p], q1 = qj[P + p], q2 = qj[2 * P + p];
        const float m = fmaxf(q0, fmaxf(q1, q2));
        const float e0 = expf(q0 - m), e1 = expf(q1 - m), e2 = expf(q2 - m);
        const float se = e0 + e1 + e2, lse = logf(se) + m;
        sum += lse - (lf == 0.f ? q0 : q1);
        cnt += 1.f;
    }
    red[0][t] = sum; red[1][t] = cnt;
    block_sum(t, red[0], red[1]);
    const float W = red[1][0];
    if (t == 0) loss[j] = W > 0.f ? red[0][0] / W : 0.f;
    const float scale = 1.f / W;                 // (unused when W == 0: every pixel is masked then)
    for (int p = t; p < P; p += 256) {
        const float lf = lj[p];
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (lf == 0.f || lf == 1.f) {
            const float q0 = qj[p], q1 = qj[P + p], q2 = qj[2 * P + p];
            const float m = fmaxf(q0, fmaxf(q1, q2));
            const float e0 = expf(q0 - m), e1 = expf(q1 - m), e2 = expf(q2 - m);
            const float se = e0 + e1 + e2;
            d0 = scale * (e0 / se - (lf == 0.f ? 1.f : 0.f));
            d1 = scale * (e1 / se - (lf == 1.f ? 1.f : 0.f));
            d2 = scale * (e2 / se - 0.f);
        }
        dj[p] = d0; dj[P + p] = d1; dj[2 * P + p] = d2;
    }
}

// ------------------------------------------------------------------------------------
// Heightmap generation, the step in front of Trainer.forward (utils.get_heightmap, code/utils.py:38-68): camera depth
// image -> robot-frame z of every pixel (get_pointcloud + cam_pose, :12-47) -> perspective warp onto the table
// (cv2.warpPerspective with an INTER_LINEAR / BORDER_CONSTANT inverse map, :62-66), fused: one thread per heightmap
// pixel gathers its four taps and converts them on the fly.  Arithmetic restated in oracle/heightmap.py: coordinates in
// double, rounded to 1/32 pixel, float32 table weights.
// ------------------------------------------------------------------------------------
struct HeightmapArgs {
    const double* depth; int h, w;          // camera depth image [h][w]
    double fx, fy, cx, cy;                  // intrinsics
    double r20, r21, r22, t2;               // third row of the camera pose (robot-frame z)
    double mi[9];                           // INVERSE of the source -> heightmap homography
    double* out; int ow, oh;
};
static __global__ void heightmap_warp_kernel(const HeightmapArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.ow) return;
    const double xd = (double)x, yd = (double)y;
    const double den = a.mi[6] * xd + a.mi[7] * yd + a.mi[8];
    const double scale = den != 0.0 ? 32.0 / den : 0.0;
    double fxs = (a.mi[0] * xd + a.mi[1] * yd + a.mi[2]) * scale, fys = (a.mi[3] * xd + a.mi[4] * yd + a.mi[5]) * scale;
    fxs = fmin(fmax(fxs, -2147483648.0), 2147483647.0);
    fys = fmin(fmax(fys, -2147483648.0), 2147483647.0);
    const long long ix = (long long)rint(fxs), iy = (long long)rint(fys);      // saturate_cast<int>: round half to even
    const long long x0 = ix >> 5, y0 = iy >> 5;
    const float ax = (float)(ix & 31) * (1.0f / 32.0f), ay = (float)(iy & 31) * (1.0f / 32.0f);
    const float w00 = (1.0f - ay) * (1.0f - ax), w01 = (1.0f - ay) * ax, w10 = ay * (1.0f - ax), w11 = ay * ax;
    auto tap = [&](long long yy, long long xx) -> double {
        if (yy < 0 || yy >= a.h || xx < 0 || xx >= a.w) return 0.0;
        const double d = a.depth[yy * a.w + xx];
        const double px = ((double)xx - a.cx) * (d / a.fx), py = ((double)yy - a.cy) * (d / a.fy);
        return a.r20 * px + a.r21 * py + a.r22 * d + a.t2;
    };
    a.out[(int64_t)y * a.ow + x] = tap(y0, x0) * (double)w00 + tap(y0, x0 + 1) * (double)w01 + tap(y0 + 1, x0) * (double)w10 +
                                   tap(y0 + 1, x0 + 1) * (double)w11;
}

// np.argmax of an array by argmax_better's rules (smg_argmax).  One workgroup.
static __global__ __launch_bounds__(256) void argmax_kernel(const float* v, int n, int* idx_out, float* val_out) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int t = threadIdx.x;
    float best = -INFINITY; int at = 0x7fffffff;
    for (int i = t; i < n; i += 256) {
        const float x = v[i];
        if (argmax_better(x, i, best, at)) { best = x; at = i; }
    }
    bv[t] = best; bi[t] = at;
    block_argmax(bv, bi, t);
    if (t == 0) { *idx_out = bi[0] == 0x7fffffff ? 0 : bi[0]; *val_out = bv[0]; }
}

// ------------------------------------------------------------------------------------
// BN running statistics: momentum 0.1, unbiased variance,
// one update per entry of the reference-order sequence, num_batches_tracked += len.
// ------------------------------------------------------------------------------------
struct BnUpdDesc { int64_t rm, rv, nbt; int64_t stat_off; int stride, coff, C, count, head; };

static __global__ void bn_update_kernel(const BnUpdDesc* descs, const double* stats_sum, const double* stats_sq,
                                 float* bufs, int64_t* nbt, const int* seq_trunk, int n_trunk,
                                 const int* seq_head, int n_head,
                                 const int* pair_a, const int* pair_b, int n_pairs, int per_pair, float* q_out, int n_streams, int update) {
    // update == 0 (a forward that leaves the running statistics alone): only the non-finite check below, over every stream / pair of the batch
    const BnUpdDesc d = descs[blockIdx.y];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int* seq = d.head ? seq_head : seq_trunk;
    const int ns = update ? (d.head ? n_head : n_trunk) : (d.head ? n_pairs : n_streams);
    if (update && c == 0 && ns > 0) nbt[d.nbt] += ns;
    if (c >= d.C || ns == 0) return;
    double rm = bufs[d.rm + c], rv = bufs[d.rv + c];
    const double inv = 1.0 / (double)d.count;
    for (int i = 0; i < ns; ++i) {
        const int sq = update ? seq[i] : i;
        const int64_t idx = d.stat_off + (int64_t)sq * d.stride + d.coff + c;
        const double m = fstat_get(stats_sum, idx) * inv;
        double var = fstat_get(stats_sq, idx) * inv - m * m;
        var = var < 0 ? 0 : var;
        const double unb = var * (double)d.count / (double)(d.count - 1);
        rm = (double)(float)(0.1 * m + 0.9 * rm);
        rv = (double)(float)(0.1 * unb + 0.9 * rv);
        // A non-finite batch statistic (NaN / inf anywhere in that channel of that sample) makes every later activation of the
        // sample NaN in the reference: BN turns the whole channel into NaN, torch's relu / max_pool keep NaN, the next convolution
        // sums over the channel.  The kernels' v_max_f32 ReLU returns the non-NaN operand instead, so the NaN would die at the
        // first ReLU and a valid-looking Q come out - a diverged network, or the released mean = std = 0 constants
        // (code/trainer.py:176-185, golden G2), would go unnoticed.  Restore the reference's result here: Q of every sample that
        // used the stream (trunk statistics) / of the pair (head statistics) becomes NaN.
        if (!(m - m == 0.0) || !(var - var == 0.0)) {
            const int s = sq;
            for (int p = 0; p < n_pairs; ++p)
                if (d.head ? p == s : (pair_a[p] == s || pair_b[p] == s))
                    for (int j = 0; j < per_pair; ++j) q_out[(int64_t)p * per_pair + j] = __builtin_nanf("");
        }
    }
    if (update) {
        bufs[d.rm + c] = (float)rm;
        bufs[d.rv + c] = (float)rv;
    }
}

// ------------------------------------------------------------------------------------
// Adam (torch.optim.Adam, no amsgrad, no weight decay).
// ------------------------------------------------------------------------------------
// one element's step; the two step-dependent scalars are lr / (1 - beta1^t) and sqrt(1 - beta2^t)
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float lr_over_bc1, float b1, float b2, float eps, float bc2_sqrt) {
    const float mi = m + (g - m) * (1.f - b1);           // torch: exp_avg.lerp_(grad, 1-beta1)
    const float vi = v * b2 + (1.f - b2) * g * g;        // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
    m = mi;
    v = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p = p - lr_over_bc1 * (mi / denom);
}

static __global__ void adam_kernel(float* p, const float* g, float* m, float* v, int64_t n, float lr_over_bc1, float b1, float b2,
                            float eps, float bc2_sqrt) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        adam_update(p[i], g[i], m[i], v[i], lr_over_bc1, b1, b2, eps, bc2_sqrt);
}

// The same step with its two scalars read from device memory: the form a captured training step replays (smg_train_step_graph) -
// the host refreshes the scalars, the graph's kernel arguments stay.
static __global__ void adam_dev_kernel(float* p, const float* g, float* m, float* v, int64_t n, const float* sc, float b1, float b2, float eps) {
    const float lr_over_bc1 = sc[0], bc2_sqrt = sc[1];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        adam_update(p[i], g[i], m[i], v[i], lr_over_bc1, b1, b2, eps, bc2_sqrt);
}

}  // namespace smg
