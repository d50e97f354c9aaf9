// scene.cuh - dense Q maps in the SCENE frame: every rotation's [OH][OW] map rotated back and bilinearly upsampled onto the
// heightmap's pixel grid (smg_scene_maps), the best (rotation, heightmap pixel) without materialising those maps
// (smg_scene_argmax), and the Huber loss on labelled heightmap pixels with its gradient on the map (smg_loss_scene).
//
// Geometry (include/smg_hip.h has the derivation), all in double, coordinates (x = column, y = row):
//   heightmap pixel (iy, ix) -> centre of its 2x2 block of the padded input   x = 2 ix + 0.5 + pad
//   -> align_corners=True normalisation                                       u = 2 x / (S - 1) - 1
//   -> seen in the rotated frame at (the forward sampled rotated[p] = image[A p])   p = A^T u
//   -> input pixels                                                           px = (p + 1) / 2 * (S - 1)
//   -> Q map coordinates (element ox is the 20x20 window over input pixels 32 ox .. 32 ox + 639)   qx = (px - 319.5) / 32
// valid when 0 <= qx <= OW - 1 and 0 <= qy <= OH - 1; the value is the bilinear interpolation of the map there, x0 =
// min(floor(qx), OW - 2), rounded to fp32 once; an invalid pixel is -inf (no window of the head is centred there).
#pragma once
#include "elem.cuh"

namespace smg {

constexpr int kSceneMaps = 32;           // maps (pairs) per launch: their 2x2 matrices travel as kernel arguments
constexpr int kSceneTile = 8192;         // heightmap pixels per workgroup: 256 threads x 4 consecutive pixels x 8 passes
struct SceneAffine { float a[kSceneMaps][4]; };       // per map: a00 a01 a10 a11 of the forward's fp32 theta
struct SceneGeo { int hm, pad, S, OH, OW; double inv_sm1; };      // inv_sm1 = 1 / (S - 1), from the host: the chain holds no division

struct ScenePoint { int y0, x0; double fy, fx; bool valid; };

// the coordinate chain for one heightmap pixel
__device__ __forceinline__ ScenePoint scene_point(const SceneGeo& g, double a00, double a01, double a10, double a11, int iy, int ix) {
    const double sm1 = (double)(g.S - 1);
    const double x = 2.0 * (double)ix + 0.5 + (double)g.pad, y = 2.0 * (double)iy + 0.5 + (double)g.pad;
    const double ux = 2.0 * x * g.inv_sm1 - 1.0, uy = 2.0 * y * g.inv_sm1 - 1.0;
    const double pxn = a00 * ux + a10 * uy, pyn = a01 * ux + a11 * uy;            // A^T u
    const double px = (pxn + 1.0) * 0.5 * sm1, py = (pyn + 1.0) * 0.5 * sm1;
    const double qx = (px - 319.5) * 0.03125, qy = (py - 319.5) * 0.03125;
    ScenePoint p;
    p.valid = qx >= 0.0 && qx <= (double)(g.OW - 1) && qy >= 0.0 && qy <= (double)(g.OH - 1);     // (false for a NaN too)
    p.x0 = p.valid ? min((int)floor(qx), g.OW - 2) : 0;
    p.y0 = p.valid ? min((int)floor(qy), g.OH - 2) : 0;
    p.fx = qx - (double)p.x0;
    p.fy = qy - (double)p.y0;
    return p;
}

// bilinear value of a valid point on the map `Q` ([OH][OW], LDS or global), in double
template <class QPtr>
__device__ __forceinline__ double scene_interp(const ScenePoint& p, QPtr Q, int OW) {
    const int o = p.y0 * OW + p.x0;
    const double q00 = (double)Q[o], q01 = (double)Q[o + 1], q10 = (double)Q[o + OW], q11 = (double)Q[o + OW + 1];
    return (1.0 - p.fy) * ((1.0 - p.fx) * q00 + p.fx * q01) + p.fy * ((1.0 - p.fx) * q10 + p.fx * q11);
}

// scene_map_kernel / scene_argmax_kernel.  One workgroup = one tile of kSceneTile consecutive pixels of one scene-frame map (blockIdx.y = map of this launch).  The map is
// staged in LDS (OH x OW floats, dynamic), the matrix sits in registers.  ARGMAX == false: thread t of pass i owns pixels
// 4 (256 i + t) .. + 3 of the tile and stores them as one 16-byte unit (`vec4`: hm^2 a multiple of 4 and `out` 16-byte aligned;
// else four guarded 4-byte stores).  ARGMAX == true: nothing is stored; the workgroup's best (value, index into [maps][hm][hm]) by
// argmax_better's rules - invalid pixels are skipped, not compared - goes to slot blockIdx.y * gridDim.x + blockIdx.x of the
// partial arrays.
template <bool ARGMAX>
__device__ __forceinline__ void scene_walk(const float* q, int64_t map_stride, int map0, const SceneAffine& aff,
                                           const SceneGeo& g, float* out, int vec4, float* part_val, int* part_idx) {
    extern __shared__ float sq[];
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int t = threadIdx.x, m = blockIdx.y;
    const int P = g.OH * g.OW;
    const float* qm = q + (int64_t)(map0 + m) * map_stride;
    for (int i = t; i < P; i += 256) sq[i] = qm[i];
    __syncthreads();
    const double a00 = (double)aff.a[m][0], a01 = (double)aff.a[m][1], a10 = (double)aff.a[m][2], a11 = (double)aff.a[m][3];
    const int npix = g.hm * g.hm;                       // (the host refuses maps of 2^31 pixels or more)
    const int base = blockIdx.x * kSceneTile;
    float best = -INFINITY; int at = 0x7fffffff;
    for (int pass = 0; pass < kSceneTile / 1024; ++pass) {
        const int i0 = base + 4 * (pass * 256 + t);
        if (i0 >= npix) break;
        int iy = i0 / g.hm, ix = i0 - iy * g.hm;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k, ++ix) {
            const int i = i0 + k;
            if (ix == g.hm) { ix = 0; ++iy; }
            v[k] = -INFINITY;
            if (i < npix) {
                const ScenePoint p = scene_point(g, a00, a01, a10, a11, iy, ix);
                if (p.valid) {
                    v[k] = (float)scene_interp(p, sq, g.OW);
                    if (ARGMAX) {
                        const int flat = (map0 + m) * npix + i;       // (< 2^31: checked by the host)
                        if (argmax_better(v[k], flat, best, at)) { best = v[k]; at = flat; }
                    }
                }
            }
        }
        if (!ARGMAX) {
            float* o = out + (int64_t)(map0 + m) * npix + i0;
            if (vec4) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
            else
                for (int k = 0; k < 4; ++k) if (i0 + k < npix) o[k] = v[k];
        }
    }
    if (ARGMAX) {
        bv[t] = best; bi[t] = at;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) {
                const float x = bv[t + s]; const int j = bi[t + s];
                if (j != 0x7fffffff && argmax_better(x, j, bv[t], bi[t])) { bv[t] = x; bi[t] = j; }
            }
            __syncthreads();
        }
        if (t == 0) { const int slot = blockIdx.y * gridDim.x + blockIdx.x; part_val[slot] = bv[0]; part_idx[slot] = bi[0]; }
    }
}
static __global__ __launch_bounds__(256) void scene_map_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                               const SceneGeo g, float* out, int vec4) {
    scene_walk<false>(q, map_stride, map0, aff, g, out, vec4, nullptr, nullptr);
}
static __global__ __launch_bounds__(256) void scene_argmax_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                  const SceneGeo g, float* part_val, int* part_idx) {
    scene_walk<true>(q, map_stride, map0, aff, g, nullptr, 0, part_val, part_idx);
}

// The second launch of smg_scene_argmax: one workgroup reduces the n partials (thread t takes slots t, t + 256, ... in that
// order) and, with `carry`, the result a previous group of maps left in the outputs.  Empty slots hold index 0x7fffffff; when
// nothing at all was valid the result is index -1, value -inf.
static __global__ __launch_bounds__(256) void scene_argmax_reduce_kernel(const float* part_val, const int* part_idx, int n, int carry,
                                                                         int* idx_out, float* val_out) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int t = threadIdx.x;
    float best = -INFINITY; int at = 0x7fffffff;
    if (t == 0 && carry && *idx_out >= 0) { best = *val_out; at = *idx_out; }
    for (int i = t; i < n; i += 256) {
        const float x = part_val[i]; const int j = part_idx[i];
        if (j != 0x7fffffff && argmax_better(x, j, best, at)) { best = x; at = j; }
    }
    bv[t] = best; bi[t] = at;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            const float x = bv[t + s]; const int j = bi[t + s];
            if (j != 0x7fffffff && argmax_better(x, j, bv[t], bi[t])) { bv[t] = x; bi[t] = j; }
        }
        __syncthreads();
    }
    if (t == 0) { *idx_out = bi[0] == 0x7fffffff ? -1 : bi[0]; *val_out = bv[0]; }
}

// smg_loss_scene: K labelled heightmap pixels per pair (one workgroup per pair, blockIdx.x = pair of this launch).  With v_k the
// interpolated value of point k (double, not rounded), d = v_k - label_k and the Huber of code/trainer.py:345-348:
//     loss[j] = sum_k w_k huber(d)          dq[j][oy][ox] = sum_k w_k huber'(d) * (bilinear weight of (oy, ox) at point k)
// Gather form: the points are taken 256 at a time - thread t works point t of the group out into LDS (corner, fractions, w huber')
// - then every thread walks the group in index order for the map elements it owns (t, t + 256, ...), adding in double to its own
// LDS accumulators.  No atomics: duplicate points simply add twice, and every element of dq is written once, zeros included,
// rounded once.  A point that is invalid in the pair's rotation, or outside the heightmap, contributes nothing; a weight of
// exactly 0 masks its point.  Dynamic LDS: OH * OW doubles (accumulators) + OH * OW floats (the map).
static __global__ __launch_bounds__(256) void loss_scene_kernel(const float* q, int pair0, const SceneAffine aff, const SceneGeo g, int K,
                                                                const int* pixels, const float* label, const float* weight,
                                                                float* loss, float* dq) {
    extern __shared__ double sacc[];
    __shared__ double red[256];
    __shared__ double p_fy[256], p_fx[256], p_g[256];
    __shared__ int p_o[256];
    const int t = threadIdx.x, m = blockIdx.x, j = pair0 + m;
    const int P = g.OH * g.OW;
    float* sq = reinterpret_cast<float*>(sacc + P);
    const float* qj = q + (int64_t)j * P;
    for (int i = t; i < P; i += 256) { sq[i] = qj[i]; sacc[i] = 0.0; }
    __syncthreads();
    const double a00 = (double)aff.a[m][0], a01 = (double)aff.a[m][1], a10 = (double)aff.a[m][2], a11 = (double)aff.a[m][3];
    double lsum = 0.0;
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int k = k0 + t;
        int o = -1; double fy = 0.0, fx = 0.0, gk = 0.0;
        if (k < K) {
            const int64_t at = (int64_t)j * K + k;
            const int iy = pixels[2 * at], ix = pixels[2 * at + 1];
            const double w = weight ? (double)weight[at] : 1.0;
            if (iy >= 0 && iy < g.hm && ix >= 0 && ix < g.hm && w != 0.0) {
                const ScenePoint p = scene_point(g, a00, a01, a10, a11, iy, ix);
                if (p.valid) {
                    const double d = scene_interp(p, sq, g.OW) - (double)label[at];
                    double l, gr;
                    if (fabs(d) < 1.0) { l = 0.5 * (d * d); gr = d; }
                    else { l = fabs(d) - 0.5; gr = d > 0.0 ? 1.0 : -1.0; }
                    lsum += w * l;
                    o = p.y0 * g.OW + p.x0; fy = p.fy; fx = p.fx; gk = w * gr;
                }
            }
        }
        p_o[t] = o; p_fy[t] = fy; p_fx[t] = fx; p_g[t] = gk;
        __syncthreads();
        const int n = min(256, K - k0);
        for (int i = t; i < P; i += 256) {
            const int ey = i / g.OW, ex = i - ey * g.OW;
            double acc = sacc[i];
            for (int kk = 0; kk < n; ++kk) {
                const int oo = p_o[kk];
                if (oo < 0) continue;
                const int y0 = oo / g.OW, x0 = oo - y0 * g.OW;
                const int dy = ey - y0, dx = ex - x0;
                if ((unsigned)dy > 1u || (unsigned)dx > 1u) continue;
                const double wy = dy ? p_fy[kk] : 1.0 - p_fy[kk], wx = dx ? p_fx[kk] : 1.0 - p_fx[kk];
                acc += p_g[kk] * (wy * wx);
            }
            sacc[i] = acc;
        }
        __syncthreads();
    }
    red[t] = lsum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) loss[j] = (float)red[0];
    float* dj = dq + (int64_t)j * P;
    for (int i = t; i < P; i += 256) dj[i] = (float)sacc[i];
}

}  // namespace smg
