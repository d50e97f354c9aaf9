// scene.cuh - dense Q maps in the SCENE frame: every rotation's [OH][OW] map rotated back and bilinearly upsampled onto the
// heightmap's pixel grid (smg_scene_maps), the best (rotation, heightmap pixel) without materialising those maps
// (smg_scene_argmax), and the Huber loss on labelled heightmap pixels with its gradient on the map (smg_loss_scene: K listed pixels;
// smg_loss_scene_map: a whole label image and weight image); further down the same four for the class logits of a 3-class head
// (smg_scene_class_maps / smg_scene_class_argmax / smg_loss_scene_ce: K listed pixels / smg_loss_scene_map_ce: a whole class-label
// image, the cross entropy).
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

// The heightmap box of map element (oy, ox), shared by the two label-map kernels (loss_scene_map_kernel, loss_scene_map_ce_kernel):
// pixels bx0 .. bx0 + bw - 1 of rows by0 .., n = bw * rows of them in row-major order (0 when the box is empty).  The kernels' comment
// below has the construction.
struct SceneBox { int bx0, by0, bw, n; };
__device__ __forceinline__ SceneBox scene_element_box(const SceneGeo& g, double a00, double a01, double a10, double a11, int oy, int ox) {
    // the box: the map square [ox - 1, ox + 1] x [oy - 1, oy + 1] (clipped) pushed back onto the heightmap
    const double sm1 = (double)(g.S - 1);
    const double qx0 = (double)max(ox - 1, 0), qx1 = (double)min(ox + 1, g.OW - 1), qy0 = (double)max(oy - 1, 0), qy1 = (double)min(oy + 1, g.OH - 1);
    const double det = a00 * a11 - a10 * a01;                 // of A^T = [a00 a10; a01 a11], whose inverse is [a11 -a10; -a01 a00] / det
    const bool inv_ok = fabs(det) > 1e-6 * (a00 * a00 + a01 * a01 + a10 * a10 + a11 * a11) && fabs(det) < INFINITY;      // (false for a NaN)
    const double rdet = inv_ok ? 1.0 / det : 0.0;
    double lox = INFINITY, hix = -INFINITY, loy = INFINITY, hiy = -INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double qx = (c & 1) ? qx1 : qx0, qy = (c & 2) ? qy1 : qy0;
        const double pxn = 2.0 * (32.0 * qx + 319.5) * g.inv_sm1 - 1.0, pyn = 2.0 * (32.0 * qy + 319.5) * g.inv_sm1 - 1.0;
        const double ux = (a11 * pxn - a10 * pyn) * rdet, uy = (a00 * pyn - a01 * pxn) * rdet;            // A^-T p
        const double fx = ((ux + 1.0) * 0.5 * sm1 - 0.5 - (double)g.pad) * 0.5, fy = ((uy + 1.0) * 0.5 * sm1 - 0.5 - (double)g.pad) * 0.5;
        lox = fmin(lox, fx); hix = fmax(hix, fx); loy = fmin(loy, fy); hiy = fmax(hiy, fy);
    }
    // (clamped in double first: the conversions below stay in range whatever the matrix holds)
    const double top = (double)g.hm;
    if (!inv_ok) { lox = loy = 0.0; hix = hiy = top; }
    const int bx0 = max((int)floor(fmin(fmax(lox, 0.0), top)) - 1, 0), bx1 = min((int)ceil(fmin(fmax(hix, -2.0), top)) + 1, g.hm - 1);
    const int by0 = max((int)floor(fmin(fmax(loy, 0.0), top)) - 1, 0), by1 = min((int)ceil(fmin(fmax(hiy, -2.0), top)) + 1, g.hm - 1);
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
    const int n = bw > 0 && bh > 0 ? bw * bh : 0;             // (<= hm^2 < 2^31: checked by the host)
    SceneBox b;
    b.bx0 = bx0; b.by0 = by0; b.bw = bw; b.n = n;
    return b;
}

// smg_loss_scene_map: loss_scene_kernel's Huber with a whole [hm][hm] label image and weight image per pair instead of K listed
// pixels - every pixel that is valid in the pair's rotation and whose weight is not exactly 0 is a point:
//     loss[j] = sum_pixels w huber(v - label)      dq[j][oy][ox] = sum_pixels w huber'(v - label) * (bilinear weight of (oy, ox) at the pixel)
// Gather by map element: one workgroup owns one (pair, oy, ox) - blockIdx.x = oy * OW + ox, blockIdx.y = pair of this launch.  Only
// pixels whose corner (y0, x0) lies in {oy - 1, oy} x {ox - 1, ox} touch that element: they lie at map coordinates
// [ox - 1, ox + 1] x [oy - 1, oy + 1], clipped to the map.  The four corners of that square go back through the chain with the
// inverse of A^T (u = A^-T p, whatever the 2x2 matrix is: scene_point asks for no rotation); the heightmap bounding box of the
// four images, widened by one pixel per side and clipped to the heightmap, holds every such pixel (for a rotation about 34 x 34 at
// a multiple of a quarter turn, 46 x 46 at 45 degrees).  A matrix without a usable inverse (determinant 0, not finite, or below
// 1e-6 of the squared norm) maps whole lines of pixels onto one map point: the box is then the whole heightmap.  Thread t takes pixels t, t + 256, ... of the box in
// row-major order, runs scene_point on each, keeps the valid ones that touch the element, and adds in double; a fixed tree over
// the 256 threads follows.  The weight is read only under a valid touching pixel, the label only where the weight is not 0, the
// map's four corners from global memory (the map sits in L2).  No atomics, every element of dq written once, rounded once:
// identical calls are bit-identical, and a pair's results do not depend on which launch carries it.
// The loss counts a pixel at its HOME element (y0, x0) only; the per-element sums go to `lpart` ([pairs of this launch][OH * OW]
// doubles, every slot written) for loss_scene_map_reduce_kernel.
static __global__ __launch_bounds__(256) void loss_scene_map_kernel(const float* q, int pair0, const SceneAffine aff, const SceneGeo g,
                                                                    const float* label, const float* weight, double* lpart, float* dq) {
    __shared__ double racc[256], rloss[256];
    const int t = threadIdx.x, m = blockIdx.y, j = pair0 + m, el = blockIdx.x;
    const int P = g.OH * g.OW;
    const int oy = el / g.OW, ox = el - oy * g.OW;
    const float* qj = q + (int64_t)j * P;
    const double a00 = (double)aff.a[m][0], a01 = (double)aff.a[m][1], a10 = (double)aff.a[m][2], a11 = (double)aff.a[m][3];
    const SceneBox box = scene_element_box(g, a00, a01, a10, a11, oy, ox);
    const int bx0 = box.bx0, by0 = box.by0, bw = box.bw, n = box.n;
    double acc = 0.0, lsum = 0.0;
    for (int i = t; i < n; i += 256) {
        const int ry = i / bw;
        const int iy = by0 + ry, ix = bx0 + (i - ry * bw);
        const ScenePoint p = scene_point(g, a00, a01, a10, a11, iy, ix);
        if (!p.valid) continue;
        const int dy = oy - p.y0, dx = ox - p.x0;
        if ((unsigned)dy > 1u || (unsigned)dx > 1u) continue;
        const int64_t at = ((int64_t)j * g.hm + iy) * g.hm + ix;
        const double w = weight ? (double)weight[at] : 1.0;
        if (w == 0.0) continue;
        const double d = scene_interp(p, qj, g.OW) - (double)label[at];
        double l, gr;
        if (fabs(d) < 1.0) { l = 0.5 * (d * d); gr = d; }
        else { l = fabs(d) - 0.5; gr = d > 0.0 ? 1.0 : -1.0; }
        if (dy == 0 && dx == 0) lsum += w * l;
        const double wy = dy ? p.fy : 1.0 - p.fy, wx = dx ? p.fx : 1.0 - p.fx;
        acc += (w * gr) * (wy * wx);
    }
    racc[t] = acc; rloss[t] = lsum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { racc[t] += racc[t + s]; rloss[t] += rloss[t + s]; }
        __syncthreads();
    }
    if (t == 0) { dq[(int64_t)j * P + el] = (float)racc[0]; lpart[(int64_t)m * P + el] = rloss[0]; }
}

// The second launch of smg_loss_scene_map: one workgroup per pair of the launch sums its P per-element loss partials - thread t
// takes slots t, t + 256, ... in that order, then the fixed tree - and rounds to fp32 once.
static __global__ __launch_bounds__(256) void loss_scene_map_reduce_kernel(const double* lpart, int P, int pair0, float* loss) {
    __shared__ double red[256];
    const int t = threadIdx.x, m = blockIdx.x;
    double s = 0.0;
    for (int i = t; i < P; i += 256) s += lpart[(int64_t)m * P + i];
    red[t] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) red[t] += red[t + k];
        __syncthreads();
    }
    if (t == 0) loss[pair0 + m] = (float)red[0];
}

// ---- the reactive net's three class planes in the scene frame (smg_scene_class_maps / smg_scene_class_argmax / smg_loss_scene_ce / smg_loss_scene_map_ce) ----
// The three LOGIT planes of a map ([3][OH][OW], `P` = OH * OW apart) are interpolated at the scene point - same corners, same
// fractions - and the softmax is taken there, in double: z_c = bilinear(plane c), m = max z, e_c = exp(z_c - m), s = e_0 + e_1 + e_2,
// P_c = e_c / s rounded to fp32 once.  Logits are interpolated, not probabilities: the cross entropy below is that of these very
// z, so picking and training see one function of the head output.  Nothing is special-cased: a NaN corner, or an inf that gives
// inf - inf, makes s NaN and with it all three probabilities, as torch.softmax does in fp64.
struct SceneClass { double z0, z1, z2, m, e0, e1, e2, s; };

template <class QPtr>
__device__ __forceinline__ SceneClass scene_class(const ScenePoint& p, QPtr Q, int P, int OW) {
    SceneClass c;
    c.z0 = scene_interp(p, Q, OW); c.z1 = scene_interp(p, Q + P, OW); c.z2 = scene_interp(p, Q + 2 * P, OW);
    c.m = fmax(c.z0, fmax(c.z1, c.z2));
    c.e0 = exp(c.z0 - c.m); c.e1 = exp(c.z1 - c.m); c.e2 = exp(c.z2 - c.m);
    c.s = c.e0 + c.e1 + c.e2;
    return c;
}
// P(class cls) of that point: the one expression both kernels below take their values from (so the argmax is bit-equal to the maps).
// (By value and as two flat selects: a chain of conditionals on the members of a reference became an indexed load from a copy of
// the struct in scratch memory, 72 bytes per lane.)
__device__ __forceinline__ float scene_class_prob(const SceneClass c, int cls) {
    const double e01 = cls == 0 ? c.e0 : c.e1;
    return (float)((cls == 2 ? c.e2 : e01) / c.s);
}

// scene_class_map_kernel / scene_class_argmax_kernel: scene_walk's tiling (one workgroup = kSceneTile consecutive pixels of one
// map, blockIdx.y = map of this launch, the matrix in registers) with all three planes of the map staged in LDS (3 OH OW floats,
// dynamic); scene_point runs once per pixel.  q is [maps][3][OH][OW].  ARGMAX == false: cls in {0, 1, 2} stores P(class cls) to
// out [maps][hm][hm], cls == -1 all three to out [maps][3][hm][hm] - a thread's pixel group goes to three addresses hm^2 apart -
// as 16-byte units (`vec4`) or guarded 4-byte stores; an invalid pixel is -inf in every plane.  ARGMAX == true: cls in {0, 1, 2},
// nothing stored, the workgroup's best (P(class cls), index into [maps][hm][hm]) goes to its slot of the partial arrays exactly
// as in scene_walk, for scene_argmax_reduce_kernel.
template <bool ARGMAX>
__device__ __forceinline__ void scene_class_walk(const float* q, int map0, const SceneAffine& aff, const SceneGeo& g, int cls,
                                                 float* out, int vec4, float* part_val, int* part_idx) {
    extern __shared__ float sq[];
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int t = threadIdx.x, m = blockIdx.y;
    const int P = g.OH * g.OW;
    const float* qm = q + (int64_t)(map0 + m) * 3 * P;
    for (int i = t; i < 3 * P; i += 256) sq[i] = qm[i];
    __syncthreads();
    const double a00 = (double)aff.a[m][0], a01 = (double)aff.a[m][1], a10 = (double)aff.a[m][2], a11 = (double)aff.a[m][3];
    const int npix = g.hm * g.hm;                       // (the host refuses maps of 2^31 pixels or more)
    const int base = blockIdx.x * kSceneTile;
    const int planes = cls < 0 ? 3 : 1;
    float best = -INFINITY; int at = 0x7fffffff;
    for (int pass = 0; pass < kSceneTile / 1024; ++pass) {
        const int i0 = base + 4 * (pass * 256 + t);
        if (i0 >= npix) break;
        int iy = i0 / g.hm, ix = i0 - iy * g.hm;
        float v[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k, ++ix) {
            const int i = i0 + k;
            if (ix == g.hm) { ix = 0; ++iy; }
            v[0][k] = v[1][k] = v[2][k] = -INFINITY;
            if (i < npix) {
                const ScenePoint p = scene_point(g, a00, a01, a10, a11, iy, ix);
                if (p.valid) {
                    const SceneClass c = scene_class(p, sq, P, g.OW);
                    if (cls < 0) { v[0][k] = scene_class_prob(c, 0); v[1][k] = scene_class_prob(c, 1); v[2][k] = scene_class_prob(c, 2); }
                    else v[0][k] = scene_class_prob(c, cls);
                    if (ARGMAX) {
                        const int flat = (map0 + m) * npix + i;       // (< 2^31: checked by the host)
                        if (argmax_better(v[0][k], flat, best, at)) { best = v[0][k]; at = flat; }
                    }
                }
            }
        }
        if (!ARGMAX) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c >= planes) break;
                float* o = out + ((int64_t)(map0 + m) * planes + c) * npix + i0;
                if (vec4) *reinterpret_cast<float4*>(o) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
                else
                    for (int k = 0; k < 4; ++k) if (i0 + k < npix) o[k] = v[c][k];
            }
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
static __global__ __launch_bounds__(256) void scene_class_map_kernel(const float* q, int map0, const SceneAffine aff, const SceneGeo g, int cls,
                                                                     float* out, int vec4) {
    scene_class_walk<false>(q, map0, aff, g, cls, out, vec4, nullptr, nullptr);
}
static __global__ __launch_bounds__(256) void scene_class_argmax_kernel(const float* q, int map0, const SceneAffine aff, const SceneGeo g, int cls,
                                                                        float* part_val, int* part_idx) {
    scene_class_walk<true>(q, map0, aff, g, cls, nullptr, 0, part_val, part_idx);
}

// smg_loss_scene_ce: the cross entropy (CrossEntropyLoss2d, class weights {1, 1, 0}) of the interpolated logits at K labelled
// heightmap pixels per pair - loss_scene_kernel's gather form on three planes.  A point COUNTS when its label is 0 or 1, it lies in
// the heightmap and it is valid in the pair's rotation; W = the number of such points; every other point (class 2 included,
// whatever logits lie under it) is skipped before anything is read.  Per counted point, in double:
//     nll_k = log(s) + m - z_y        g_c = e_c / s - [c == y]
// loss[j] = (sum nll_k) / W and dq[j][c][oy][ox] = (sum_k g_c * bilinear weight of (oy, ox) at point k) / W: summed unnormalised
// in point order, divided once, rounded once; W == 0 gives loss 0 and dq 0.  The points are taken 256 at a time, thread t owns map
// elements t, t + 256, ... in all three planes.  Dynamic LDS: the 3 OH OW double accumulators only - the logits are read from
// global memory (a few corners per point of a map that sits in L2), which keeps 38 x 38 maps at 35 KB + 14 KB static.
static __global__ __launch_bounds__(256) void loss_scene_ce_kernel(const float* q, int pair0, const SceneAffine aff, const SceneGeo g, int K,
                                                                   const int* pixels, const float* label, float* loss, float* dq) {
    extern __shared__ double sacc[];
    __shared__ double red[256];
    __shared__ int cnt[256];
    __shared__ double p_fy[256], p_fx[256], p_g[3][256];
    __shared__ int p_o[256];
    const int t = threadIdx.x, m = blockIdx.x, j = pair0 + m;
    const int P = g.OH * g.OW;
    const float* qj = q + (int64_t)j * 3 * P;
    for (int i = t; i < 3 * P; i += 256) sacc[i] = 0.0;
    __syncthreads();
    const double a00 = (double)aff.a[m][0], a01 = (double)aff.a[m][1], a10 = (double)aff.a[m][2], a11 = (double)aff.a[m][3];
    double lsum = 0.0; int w = 0;
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int k = k0 + t;
        int o = -1; double fy = 0.0, fx = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
        if (k < K) {
            const int64_t at = (int64_t)j * K + k;
            const int iy = pixels[2 * at], ix = pixels[2 * at + 1];
            const float lf = label[at];
            if ((lf == 0.f || lf == 1.f) && iy >= 0 && iy < g.hm && ix >= 0 && ix < g.hm) {
                const ScenePoint p = scene_point(g, a00, a01, a10, a11, iy, ix);
                if (p.valid) {
                    const SceneClass c = scene_class(p, qj, P, g.OW);
                    lsum += (log(c.s) + c.m) - (lf == 0.f ? c.z0 : c.z1);
                    ++w;
                    o = p.y0 * g.OW + p.x0; fy = p.fy; fx = p.fx;
                    g0 = c.e0 / c.s - (lf == 0.f ? 1.0 : 0.0); g1 = c.e1 / c.s - (lf == 1.f ? 1.0 : 0.0); g2 = c.e2 / c.s;
                }
            }
        }
        p_o[t] = o; p_fy[t] = fy; p_fx[t] = fx; p_g[0][t] = g0; p_g[1][t] = g1; p_g[2][t] = g2;
        __syncthreads();
        const int n = min(256, K - k0);
        for (int i = t; i < P; i += 256) {
            const int ey = i / g.OW, ex = i - ey * g.OW;
            double acc0 = sacc[i], acc1 = sacc[P + i], acc2 = sacc[2 * P + i];
            for (int kk = 0; kk < n; ++kk) {
                const int oo = p_o[kk];
                if (oo < 0) continue;
                const int y0 = oo / g.OW, x0 = oo - y0 * g.OW;
                const int dy = ey - y0, dx = ex - x0;
                if ((unsigned)dy > 1u || (unsigned)dx > 1u) continue;
                const double wy = dy ? p_fy[kk] : 1.0 - p_fy[kk], wx = dx ? p_fx[kk] : 1.0 - p_fx[kk];
                const double wgt = wy * wx;
                acc0 += p_g[0][kk] * wgt; acc1 += p_g[1][kk] * wgt; acc2 += p_g[2][kk] * wgt;
            }
            sacc[i] = acc0; sacc[P + i] = acc1; sacc[2 * P + i] = acc2;
        }
        __syncthreads();
    }
    red[t] = lsum; cnt[t] = w;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { red[t] += red[t + s]; cnt[t] += cnt[t + s]; }
        __syncthreads();
    }
    const int W = cnt[0];
    const double dW = (double)W;
    if (t == 0) loss[j] = W > 0 ? (float)(red[0] / dW) : 0.f;
    float* dj = dq + (int64_t)j * 3 * P;
    for (int i = t; i < 3 * P; i += 256) dj[i] = W > 0 ? (float)(sacc[i] / dW) : 0.f;
}

// smg_loss_scene_map_ce: loss_scene_ce_kernel's cross entropy with a whole [hm][hm] class-label image per pair instead of K listed
// pixels - loss_scene_map_kernel's structure on three planes.  A heightmap pixel is a POINT of pair j when it is valid in the pair's
// rotation and its label is exactly 0.f or 1.f; every other pixel (class 2, NaN, any other value) is skipped before a logit is
// read, and the label of an invalid pixel is never read.  W = the number of points.  Per point, in double (scene_class as it stands):
//     nll = (log(s) + m) - z_y        g_c = e_c / s - [c == y]
//     loss[j] = (sum nll) / W         dq[j][c][oy][ox] = (sum g_c * bilinear weight of (oy, ox) at the pixel) / W
// Gather by map element exactly as in loss_scene_map_kernel: one workgroup owns one (pair, oy, ox) - blockIdx.x = oy * OW + ox,
// blockIdx.y = pair of this launch - and walks scene_element_box's pixels t, t + 256, ... in row-major order; a pixel adds its nll
// and its count at its HOME element (y0, x0) only (the logarithm is taken there alone) and its gradient share at every element it
// touches, so a point's softmax is evaluated by up to four workgroups: the price of a form without atomics.  The twelve corner
// logits of a pixel come from global memory (three [OH][OW] planes that sit in L2; staging the 27 logits around the element in LDS
// measured 0.755 against 0.776 ms at S = 1824, inside the spread between repeats, and was not kept).
// W is known only when all elements of a pair are done, so this launch writes UNNORMALISED partials into scratch the engine owns,
// every slot written: gpart [pairs of this launch][3][OH * OW] doubles, lpart [pairs][OH * OW] doubles, cpart [pairs][OH * OW]
// ints.  No accumulator of the map's size in LDS (4 x 256 doubles + 256 ints of reduction arrays), hence no limit on the map's size
// beyond scene_geometry's.
static __global__ __launch_bounds__(256) void loss_scene_map_ce_kernel(const float* q, int pair0, const SceneAffine aff, const SceneGeo g,
                                                                       const float* label, double* gpart, double* lpart, int* cpart) {
    __shared__ double racc[3][256], rloss[256];
    __shared__ int rcnt[256];
    const int t = threadIdx.x, m = blockIdx.y, j = pair0 + m, el = blockIdx.x;
    const int P = g.OH * g.OW;
    const int oy = el / g.OW, ox = el - oy * g.OW;
    const float* qj = q + (int64_t)j * 3 * P;
    const double a00 = (double)aff.a[m][0], a01 = (double)aff.a[m][1], a10 = (double)aff.a[m][2], a11 = (double)aff.a[m][3];
    const SceneBox box = scene_element_box(g, a00, a01, a10, a11, oy, ox);
    const int bx0 = box.bx0, by0 = box.by0, bw = box.bw, n = box.n;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, lsum = 0.0; int w = 0;
    for (int i = t; i < n; i += 256) {
        const int ry = i / bw;
        const int iy = by0 + ry, ix = bx0 + (i - ry * bw);
        const ScenePoint p = scene_point(g, a00, a01, a10, a11, iy, ix);
        if (!p.valid) continue;
        const int dy = oy - p.y0, dx = ox - p.x0;
        if ((unsigned)dy > 1u || (unsigned)dx > 1u) continue;
        const float lf = label[((int64_t)j * g.hm + iy) * g.hm + ix];
        if (!(lf == 0.f || lf == 1.f)) continue;
        const SceneClass c = scene_class(p, qj, P, g.OW);
        if (dy == 0 && dx == 0) { lsum += (log(c.s) + c.m) - (lf == 0.f ? c.z0 : c.z1); ++w; }
        const double wy = dy ? p.fy : 1.0 - p.fy, wx = dx ? p.fx : 1.0 - p.fx;
        const double wgt = wy * wx;
        acc0 += (c.e0 / c.s - (lf == 0.f ? 1.0 : 0.0)) * wgt; acc1 += (c.e1 / c.s - (lf == 1.f ? 1.0 : 0.0)) * wgt; acc2 += (c.e2 / c.s) * wgt;
    }
    racc[0][t] = acc0; racc[1][t] = acc1; racc[2][t] = acc2; rloss[t] = lsum; rcnt[t] = w;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            racc[0][t] += racc[0][t + s]; racc[1][t] += racc[1][t + s]; racc[2][t] += racc[2][t + s];
            rloss[t] += rloss[t + s]; rcnt[t] += rcnt[t + s];
        }
        __syncthreads();
    }
    if (t < 3) gpart[((int64_t)m * 3 + t) * P + el] = racc[t][0];
    if (t == 0) { lpart[(int64_t)m * P + el] = rloss[0]; cpart[(int64_t)m * P + el] = rcnt[0]; }
}

// The second launch of smg_loss_scene_map_ce: one workgroup per pair of the launch sums its P loss partials and counts - thread t
// takes slots t, t + 256, ... in that order, then the fixed tree - which gives W, then writes loss = (float)(sum / W) and
// dq = (float)(partial / W) for all 3 P elements: divided once, rounded once, every element written once.  W == 0: loss 0.f and dq
// exactly 0.f everywhere.
static __global__ __launch_bounds__(256) void loss_scene_map_ce_finish_kernel(const double* gpart, const double* lpart, const int* cpart,
                                                                              int P, int pair0, float* loss, float* dq) {
    __shared__ double red[256];
    __shared__ int cnt[256];
    const int t = threadIdx.x, m = blockIdx.x, j = pair0 + m;
    double s = 0.0; int w = 0;
    for (int i = t; i < P; i += 256) { s += lpart[(int64_t)m * P + i]; w += cpart[(int64_t)m * P + i]; }
    red[t] = s; cnt[t] = w;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) { red[t] += red[t + k]; cnt[t] += cnt[t + k]; }
        __syncthreads();
    }
    const int W = cnt[0];
    const double dW = (double)W;
    if (t == 0) loss[j] = W > 0 ? (float)(red[0] / dW) : 0.f;
    const double* gm = gpart + (int64_t)m * 3 * P;
    float* dj = dq + (int64_t)j * 3 * P;
    for (int i = t; i < 3 * P; i += 256) dj[i] = W > 0 ? (float)(gm[i] / dW) : 0.f;
}

}  // namespace smg
