// scene.cuh - the head's maps in the SCENE frame: every rotation's [OH][OW] map rotated back and bilinearly interpolated on the
// heightmap's pixel grid.  In the order of the file:
//   scene_point / scene_interp / scene_class   the coordinate chain of one heightmap pixel and the value(s) of the map there: one Q
//                                  value, or the softmax of the three interpolated logits of a 3-class head
//   scene_walk<PLANES, ARGMAX, SELECT, PICKS, NOISE>  the one tiling behind smg_scene_maps / smg_scene_class_maps (ARGMAX false: the maps are
//                                  stored), smg_scene_argmax / smg_scene_class_argmax (true: the best (rotation, pixel), nothing
//                                  stored) and smg_scene_argmax_objects / smg_scene_class_argmax_objects (SELECT: every map on the
//                                  pixels its masks select, one result per group of maps; PICKS: one round of smg_scene_topk_objects /
//                                  smg_scene_class_topk_objects, which also skips the discs around the group's earlier picks;
//                                  NOISE: one draw of smg_scene_sample_objects / smg_scene_class_sample_objects, the selected walk
//                                  that keeps the candidate with the best Gumbel-perturbed score, scene_sample_score)
//   scene_softmax_walk<PLANES>     smg_scene_softmax_objects / smg_scene_class_softmax_objects: the selected walk that accumulates a
//                                  streaming log-sum-exp state (SceneSoft) per workgroup instead of an argmax, its grouped reduce
//                                  and the one-thread-per-group finish
//   scene_best_walk<PLANES>        smg_scene_best_maps / smg_scene_class_best_maps: per GROUP of maps and heightmap pixel the best
//                                  value over the group's maps and the map that gives it - parallel over groups and pixel tiles,
//                                  the group's maps staged one at a time, launches of maps carried through the outputs
//   scene_values_kernel<PLANES>    smg_scene_values / smg_scene_class_values: the same value(s) at K LISTED pixels per map, the
//                                  corners read from global memory, nothing staged
//   SceneHuber / SceneCe           the per-point terms of the two losses, each written once
//   scene_list_walk                the loss on K LISTED pixels per pair (smg_loss_scene_ce; smg_loss_scene's kernel keeps the same
//                                  loop in a copy of its own, for the reason its comment gives)
//   scene_box_walk                 the loss on a whole label IMAGE per pair (smg_loss_scene_map, smg_loss_scene_map_ce)
//   ScenePolicy                    the Boltzmann policy's log-likelihood and entropy loss per group of pairs (smg_loss_scene_policy):
//                                  scene_box_walk's third Loss, behind the softmax kernels' normaliser
// The __global__ kernels are thin instantiations of these; the block trees they end in are block_argmax and block_sum (elem.cuh).
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

// The reactive net's three class planes at a scene point (smg_scene_class_maps / smg_scene_class_argmax / smg_loss_scene_ce /
// smg_loss_scene_map_ce).  The three LOGIT planes of a map ([3][OH][OW], `P` = OH * OW apart) are interpolated at the scene point - same corners, same
// fractions - and the softmax is taken there, in double: z_c = bilinear(plane c), m = max z, e_c = exp(z_c - m), s = e_0 + e_1 + e_2,
// P_c = e_c / s rounded to fp32 once.  Logits are interpolated, not probabilities: the cross entropy (SceneCe) is that of these very
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
// P(class cls) of that point: the one expression the map and the argmax kernel take their values from (so the argmax is bit-equal to the maps).
// (By value and as two flat selects: a chain of conditionals on the members of a reference became an indexed load from a copy of
// the struct in scratch memory, 72 bytes per lane.)
__device__ __forceinline__ float scene_class_prob(const SceneClass c, int cls) {
    const double e01 = cls == 0 ? c.e0 : c.e1;
    return (float)((cls == 2 ? c.e2 : e01) / c.s);
}

// Per map of a launch of smg_scene_argmax_objects / smg_scene_class_argmax_objects, as kernel arguments beside SceneAffine: the two mask terms that select the map's
// heightmap pixels (an index into masks [n_masks][hm][hm] float64, -1 = no such term, both -1 = every pixel) and the group whose
// result the map competes for.
struct SceneSelect { int a[kSceneMaps], b[kSceneMaps], group[kSceneMaps]; };

// The greedy top-K of smg_scene_topk_objects / smg_scene_class_topk_objects: the most ranks a call may ask for, and what round n's
// walk knows of the rounds before it - idx [n_groups][K] = the output itself, whose slots 0 .. n - 1 of every group are final, and
// r2 = the squared suppression radius (clamped to 32 bits by the host).
constexpr int kSceneTopK = 32;
struct ScenePicks { const int* idx; int K, n; unsigned r2; };

// The Boltzmann draw of smg_scene_sample_objects / smg_scene_class_sample_objects: draw d of a call picks, per group, the candidate
// with the best SCORE s = (float)fma(beta, (double)v, G), v = the candidate's float32 map value and G = standard Gumbel noise that is
// a pure function of (seed, d, the candidate's flattened index i into [n_maps][hm][hm], i < 2^31) - the Gumbel-max identity: the
// argmax of beta v + G over independent G is a draw from softmax(beta v).  All integers mod 2^64:
//   x = seed + (d << 32) + i
//   mix(x): x += 0x9E3779B97F4A7C15; z = x; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
//           return z ^ z >> 31                                   (the splitmix64 finaliser)
//   h = mix(mix(x))
//   u = ((h >> 12) + 0.5) * 2^-52      exact in double, strictly inside (0, 1): from 2^-53 to 1 - 2^-53
//   G = -log(-log(u))                  double, finite, in about [-3.61, 36.74]
// The score is rounded to float32 once.  scene_sample_score is the ONE place that forms it: the walk and the grouped reduce both
// call it, so the two cannot round differently.  A NaN value gives a NaN score (and wins, by argmax_better's rules).
constexpr int kSceneDraws = 32;          // the most draws a call may ask for
struct SceneNoise { unsigned long long seed; double beta; int d; };
__device__ __forceinline__ unsigned long long scene_mix(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float scene_sample_score(float v, int flat, const SceneNoise& nz) {
    const unsigned long long h = scene_mix(scene_mix(nz.seed + ((unsigned long long)(unsigned)nz.d << 32) + (unsigned long long)(unsigned)flat));
    const double u = ((double)(h >> 12) + 0.5) * 0x1p-52;
    const double G = -log(-log(u));
    return (float)fma(nz.beta, (double)v, G);
}

// Which of the 4 consecutive pixels i0 .. i0 + 3 mask `term` selects, OR-ed into s: a pixel is selected when its double is not
// exactly 0 - the bit pattern without its sign is tested, so -0.0 does not select, a NaN does, and the value never enters any
// arithmetic.  vec: two 16-byte loads (masks 16-byte aligned and hm^2 a multiple of 4, so the thread's 32 bytes are aligned and
// inside the mask); else guarded 8-byte loads.
__device__ __forceinline__ void scene_select4(const double* masks, int term, int npix, int i0, int vec, bool (&s)[4]) {
    if (term < 0) return;
    const unsigned long long* p = reinterpret_cast<const unsigned long long*>(masks) + (int64_t)term * npix + i0;
    unsigned long long w[4] = {0ull, 0ull, 0ull, 0ull};
    if (vec) {
        const ulonglong2 lo = *reinterpret_cast<const ulonglong2*>(p), hi = *reinterpret_cast<const ulonglong2*>(p + 2);
        w[0] = lo.x; w[1] = lo.y; w[2] = hi.x; w[3] = hi.y;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (i0 + k < npix) w[k] = p[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = s[k] || (w[k] << 1) != 0ull;
}

// The map / argmax kernels.  One workgroup = one tile of kSceneTile consecutive pixels of one scene-frame map (blockIdx.y = map
// of this launch, `map_stride` floats apart in q).  The map's PLANES planes are staged in LDS (PLANES x OH x OW floats, dynamic; the
// three logit planes of a class map lie OH * OW apart, so its map_stride is 3 OH OW), the matrix sits in registers, scene_point runs
// once per pixel.  PLANES == 1: the value is the interpolated Q value, `cls` is not read.  PLANES == 3: P(class cls) of the softmax,
// or with cls == -1 all three.
// ARGMAX == false: thread t of pass i owns pixels 4 (256 i + t) .. + 3 of the tile and stores them as one 16-byte unit (`vec4`: hm^2
// a multiple of 4 and `out` 16-byte aligned; else four guarded 4-byte stores) to out [maps][hm][hm], or with cls == -1 to out
// [maps][3][hm][hm] - a thread's pixel group goes to three addresses hm^2 apart; an invalid pixel is -inf in every plane.
// ARGMAX == true (cls in {0, 1, 2}): nothing is stored; the workgroup's best (value, index into [maps][hm][hm]) by argmax_better's
// rules - invalid pixels are skipped, not compared - goes to slot blockIdx.y * gridDim.x + blockIdx.x of the partial arrays.
// SELECT (with ARGMAX; smg_scene_argmax_objects, smg_scene_class_argmax_objects): the map only sees the pixels its two mask terms sel->a[m] / sel->b[m] select
// (scene_select4, `mvec` = its 16-byte loads).  The masks are read BEFORE the geometry: a pixel that is not selected is skipped like
// an invalid one and never enters the double-precision chain - objects are compact, so whole waves skip it.  A workgroup without a
// selected valid pixel leaves an empty slot (index 0x7fffffff).
// PICKS (with SELECT; smg_scene_topk_objects, smg_scene_class_topk_objects): round pk->n of the greedy top-K.  The map's group has
// pk->n earlier picks in pk->idx [n_groups][pk->K] (written by the reduces of the earlier rounds, earlier on the stream); a selected
// pixel within the disc pk->r2 (squared radius, integer arithmetic) of one of them - in whichever map of the group it was picked -
// is skipped like an unselected one, before the geometry.  The picks are decoded once per workgroup, idx % hm^2 -> (py << 16 | px),
// into kSceneTopK ints of dynamic LDS behind the planes.  A group whose last pick is -1 has nothing left: the workgroup leaves an
// empty slot and walks nothing.
// NOISE (with SELECT; smg_scene_sample_objects, smg_scene_class_sample_objects): draw nz->d of the Boltzmann sample.  Masks before
// geometry as above; only a selected valid pixel pays the hash and the two double logarithms of scene_sample_score.  The thread and
// the workgroup keep the candidate with the best SCORE by argmax_better's rules applied to the score (lowest flattened index on
// ties, a NaN score wins), and the slot receives that candidate's VALUE and index: the tree runs on (score, index), then the one
// thread that holds the winning index - flattened indices are unique - writes its value.  The grouped reduce recomputes the score
// from (value, index).
template <int PLANES, bool ARGMAX, bool SELECT = false, bool PICKS = false, bool NOISE = false>
__device__ __forceinline__ void scene_walk(const float* q, int64_t map_stride, int map0, const SceneAffine& aff, const SceneGeo& g, int cls,
                                           float* out, int vec4, float* part_val, int* part_idx,
                                           const SceneSelect* sel = nullptr, const double* masks = nullptr, int mvec = 0,
                                           const ScenePicks* pk = nullptr, const SceneNoise* nz = nullptr) {
    static_assert(ARGMAX || !SELECT, "the selected walk is an argmax");
    static_assert(SELECT || !PICKS, "the picks suppress selected pixels");
    static_assert(SELECT || !NOISE, "the sample is drawn among selected pixels");
    extern __shared__ float sq[];
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int t = threadIdx.x, m = blockIdx.y;
    const int P = g.OH * g.OW;
    const float* qm = q + (int64_t)(map0 + m) * map_stride;
    if constexpr (PICKS) {
        const int* mine = pk->idx + (int64_t)sel->group[m] * pk->K;
        if (pk->n > 0 && mine[pk->n - 1] < 0) {             // (the same for every thread: nobody reaches the barrier)
            if (t == 0) { const int slot = blockIdx.y * gridDim.x + blockIdx.x; part_val[slot] = -INFINITY; part_idx[slot] = 0x7fffffff; }
            return;
        }
        if (t < pk->n) {                                    // (pk->n <= kSceneTopK; every earlier pick is >= 0 here)
            const int at = mine[t] % (g.hm * g.hm), py = at / g.hm;
            reinterpret_cast<unsigned*>(sq + PLANES * P)[t] = (unsigned)py << 16 | (unsigned)(at - py * g.hm);
        }
    }
    for (int i = t; i < PLANES * P; i += 256) sq[i] = qm[i];
    __syncthreads();
    const double a00 = (double)aff.a[m][0], a01 = (double)aff.a[m][1], a10 = (double)aff.a[m][2], a11 = (double)aff.a[m][3];
    const int npix = g.hm * g.hm;                       // (the host refuses maps of 2^31 pixels or more)
    const int base = blockIdx.x * kSceneTile;
    const int planes = PLANES == 3 && cls < 0 ? 3 : 1;  // planes stored per map
    float best = -INFINITY; int at = 0x7fffffff;
    float held = -INFINITY;                             // NOISE: the value of the candidate whose score `best` is
    for (int pass = 0; pass < kSceneTile / 1024; ++pass) {
        const int i0 = base + 4 * (pass * 256 + t);
        if (i0 >= npix) break;
        int iy = i0 / g.hm, ix = i0 - iy * g.hm;
        float v[PLANES][4];
        bool s[4] = {true, true, true, true};
        if constexpr (SELECT) {
            const int ta = sel->a[m], tb = sel->b[m];
            if (ta >= 0 || tb >= 0) {
                s[0] = s[1] = s[2] = s[3] = false;
                scene_select4(masks, ta, npix, i0, mvec, s);
                scene_select4(masks, tb, npix, i0, mvec, s);
            }
        }
        if constexpr (PICKS) {
            if (s[0] || s[1] || s[2] || s[3]) {
                const unsigned* pick = reinterpret_cast<const unsigned*>(sq + PLANES * P);
                for (int p = 0; p < pk->n; ++p) {
                    const int py = (int)(pick[p] >> 16), px = (int)(pick[p] & 0xffffu);
                    int y = iy, x = ix;
#pragma unroll
                    for (int k = 0; k < 4; ++k, ++x) {
                        if (x == g.hm) { x = 0; ++y; }
                        const int dy = y - py, dx = x - px;        // (hm^2 < 2^31, checked by the host: each square fits an int, their sum 32 bits unsigned)
                        if ((unsigned)(dy * dy) + (unsigned)(dx * dx) <= pk->r2) s[k] = false;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k, ++ix) {
            const int i = i0 + k;
            if (ix == g.hm) { ix = 0; ++iy; }
#pragma unroll
            for (int c = 0; c < PLANES; ++c) v[c][k] = -INFINITY;
            if (i < npix && (!SELECT || s[k])) {
                const ScenePoint p = scene_point(g, a00, a01, a10, a11, iy, ix);
                if (p.valid) {
                    if constexpr (PLANES == 1) v[0][k] = (float)scene_interp(p, sq, g.OW);
                    else {
                        const SceneClass c = scene_class(p, sq, P, g.OW);
                        if (cls < 0) { v[0][k] = scene_class_prob(c, 0); v[1][k] = scene_class_prob(c, 1); v[2][k] = scene_class_prob(c, 2); }
                        else v[0][k] = scene_class_prob(c, cls);
                    }
                    if (ARGMAX) {
                        const int flat = (map0 + m) * npix + i;       // (< 2^31: checked by the host)
                        if constexpr (NOISE) {
                            const float sc = scene_sample_score(v[0][k], flat, *nz);
                            if (argmax_better(sc, flat, best, at)) { best = sc; at = flat; held = v[0][k]; }
                        } else if (argmax_better(v[0][k], flat, best, at)) { best = v[0][k]; at = flat; }
                    }
                }
            }
        }
        if (!ARGMAX) {
#pragma unroll
            for (int c = 0; c < PLANES; ++c) {
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
        block_argmax(bv, bi, t);
        const int slot = blockIdx.y * gridDim.x + blockIdx.x;
        if constexpr (NOISE) {
            const int win = bi[0];
            if (win == 0x7fffffff) { if (t == 0) { part_val[slot] = -INFINITY; part_idx[slot] = win; } }
            else if (at == win) { part_val[slot] = held; part_idx[slot] = win; }
        } else if (t == 0) { part_val[slot] = bv[0]; part_idx[slot] = bi[0]; }
    }
}
static __global__ __launch_bounds__(256) void scene_map_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                               const SceneGeo g, float* out, int vec4) {
    scene_walk<1, false>(q, map_stride, map0, aff, g, 0, out, vec4, nullptr, nullptr);
}
static __global__ __launch_bounds__(256) void scene_argmax_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                  const SceneGeo g, float* part_val, int* part_idx) {
    scene_walk<1, true>(q, map_stride, map0, aff, g, 0, nullptr, 0, part_val, part_idx);
}
static __global__ __launch_bounds__(256) void scene_class_map_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                     const SceneGeo g, int cls, float* out, int vec4) {
    scene_walk<3, false>(q, map_stride, map0, aff, g, cls, out, vec4, nullptr, nullptr);
}
static __global__ __launch_bounds__(256) void scene_class_argmax_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                        const SceneGeo g, int cls, float* part_val, int* part_idx) {
    scene_walk<3, true>(q, map_stride, map0, aff, g, cls, nullptr, 0, part_val, part_idx);
}

static __global__ __launch_bounds__(256) void scene_argmax_objects_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                          const SceneSelect sel, const SceneGeo g, const double* masks, int mvec,
                                                                          float* part_val, int* part_idx) {
    scene_walk<1, true, true>(q, map_stride, map0, aff, g, 0, nullptr, 0, part_val, part_idx, &sel, masks, mvec);
}
// smg_scene_class_argmax_objects: the selected walk on the three logit planes (dynamic LDS 3 x OH x OW floats, as
// scene_class_argmax_kernel's).  An unselected pixel never reaches scene_class and its three double exponentials.
static __global__ __launch_bounds__(256) void scene_class_argmax_objects_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                                const SceneSelect sel, const SceneGeo g, int cls, const double* masks,
                                                                                int mvec, float* part_val, int* part_idx) {
    scene_walk<3, true, true>(q, map_stride, map0, aff, g, cls, nullptr, 0, part_val, part_idx, &sel, masks, mvec);
}
// One round of smg_scene_topk_objects / smg_scene_class_topk_objects: the selected walk that also skips the discs of the group's
// earlier picks (dynamic LDS: the planes + kSceneTopK ints).  Round 0 (pk.n == 0) walks what scene_argmax_objects_kernel walks.
static __global__ __launch_bounds__(256) void scene_topk_objects_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                        const SceneSelect sel, const SceneGeo g, const double* masks, int mvec,
                                                                        const ScenePicks pk, float* part_val, int* part_idx) {
    scene_walk<1, true, true, true>(q, map_stride, map0, aff, g, 0, nullptr, 0, part_val, part_idx, &sel, masks, mvec, &pk);
}
static __global__ __launch_bounds__(256) void scene_class_topk_objects_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                              const SceneSelect sel, const SceneGeo g, int cls, const double* masks,
                                                                              int mvec, const ScenePicks pk, float* part_val, int* part_idx) {
    scene_walk<3, true, true, true>(q, map_stride, map0, aff, g, cls, nullptr, 0, part_val, part_idx, &sel, masks, mvec, &pk);
}
// One draw of smg_scene_sample_objects / smg_scene_class_sample_objects: the selected walk by the Gumbel-perturbed score (dynamic LDS:
// the planes).  The slots receive the winning candidate's value and index.
static __global__ __launch_bounds__(256) void scene_sample_objects_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                          const SceneSelect sel, const SceneGeo g, const double* masks, int mvec,
                                                                          const SceneNoise nz, float* part_val, int* part_idx) {
    scene_walk<1, true, true, false, true>(q, map_stride, map0, aff, g, 0, nullptr, 0, part_val, part_idx, &sel, masks, mvec, nullptr, &nz);
}
static __global__ __launch_bounds__(256) void scene_class_sample_objects_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                                const SceneSelect sel, const SceneGeo g, int cls, const double* masks,
                                                                                int mvec, const SceneNoise nz, float* part_val, int* part_idx) {
    scene_walk<3, true, true, false, true>(q, map_stride, map0, aff, g, cls, nullptr, 0, part_val, part_idx, &sel, masks, mvec, nullptr, &nz);
}

// The second launch of smg_scene_argmax / smg_scene_class_argmax: one workgroup reduces the n partials (thread t takes slots t,
// t + 256, ... in that order) and, with `carry`, the result a previous group of maps left in the outputs.  Empty slots hold index
// 0x7fffffff; when nothing at all was valid the result is index -1, value -inf.
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
    block_argmax(bv, bi, t);
    if (t == 0) { *idx_out = bi[0] == 0x7fffffff ? -1 : bi[0]; *val_out = bv[0]; }
}

// The grouped form, the second launch of smg_scene_argmax_objects / smg_scene_class_argmax_objects: one workgroup per group (blockIdx.x) scans the slots of this
// launch's `n_maps` maps (`tiles` slots each, map-major) whose map belongs to its group - thread t takes slots t, t + 256, ... in that
// order - and, with `carry`, the result an earlier launch of maps left in the group's outputs.  Every group's pair is written: a
// group without a map in any launch, or without a selected valid pixel, ends at index -1, value -inf.  A group's pair lies at
// element grp * stride of the outputs: stride 1 for the argmax, K for rank j of a top-K (the caller passes the outputs + j).
// NOISE (smg_scene_sample_objects / smg_scene_class_sample_objects, `stride` = n_draws, the outputs + d): the slots and the carried pair hold VALUES; each is
// compared by the score scene_sample_score recomputes from (value, index, nz) - the function the walk used, so the same float - and
// the winner's value is what is written: the outputs carry the running winner between launches with no further scratch.
template <bool NOISE>
__device__ __forceinline__ void scene_group_reduce(const float* part_val, const int* part_idx, int tiles, int n_maps, const SceneSelect& sel, int carry,
                                                   int* idx_out, float* val_out, int stride, const SceneNoise* nz = nullptr) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int t = threadIdx.x, grp = blockIdx.x;
    idx_out += (int64_t)grp * stride; val_out += (int64_t)grp * stride;
    float best = -INFINITY; int at = 0x7fffffff;
    float held = -INFINITY;                             // NOISE: the value whose score `best` is
    if (t == 0 && carry && *idx_out >= 0) {
        at = *idx_out;
        if constexpr (NOISE) { held = *val_out; best = scene_sample_score(held, at, *nz); }
        else best = *val_out;
    }
    for (int i = t; i < tiles * n_maps; i += 256) {
        if (sel.group[i / tiles] != grp) continue;
        const float x = part_val[i]; const int j = part_idx[i];
        if (j == 0x7fffffff) continue;
        if constexpr (NOISE) {
            const float sc = scene_sample_score(x, j, *nz);
            if (argmax_better(sc, j, best, at)) { best = sc; at = j; held = x; }
        } else if (argmax_better(x, j, best, at)) { best = x; at = j; }
    }
    bv[t] = best; bi[t] = at;
    block_argmax(bv, bi, t);
    if constexpr (NOISE) {
        const int win = bi[0];                          // (a slot's index and the carried one are all different: one thread holds the winner)
        if (win == 0x7fffffff) { if (t == 0) { *idx_out = -1; *val_out = -INFINITY; } }
        else if (at == win) { *idx_out = win; *val_out = held; }
    } else if (t == 0) { *idx_out = bi[0] == 0x7fffffff ? -1 : bi[0]; *val_out = bv[0]; }
}
static __global__ __launch_bounds__(256) void scene_argmax_group_reduce_kernel(const float* part_val, const int* part_idx, int tiles, int n_maps,
                                                                               const SceneSelect sel, int carry, int* idx_out, float* val_out, int stride) {
    scene_group_reduce<false>(part_val, part_idx, tiles, n_maps, sel, carry, idx_out, val_out, stride);
}
static __global__ __launch_bounds__(256) void scene_sample_group_reduce_kernel(const float* part_val, const int* part_idx, int tiles, int n_maps,
                                                                               const SceneSelect sel, int carry, const SceneNoise nz,
                                                                               int* idx_out, float* val_out, int stride) {
    scene_group_reduce<true>(part_val, part_idx, tiles, n_maps, sel, carry, idx_out, val_out, stride, &nz);
}

// ---- the normaliser of the Boltzmann policy: per group the log-sum-exp and the Boltzmann mean of its candidates ----
// (smg_scene_softmax_objects, smg_scene_class_softmax_objects).  The candidates of a group are smg_scene_argmax_objects': the
// selected valid pixels of the group's maps, each with the float32 value v smg_scene_maps stores there.  The STATE of a set of
// candidates is (n, M, S, T): n = how many, M = the largest value, S = sum exp(beta (v - M)) and T = sum v exp(beta (v - M)) in
// double; the empty set is (0, -inf, 0, 0).  M is a candidate's float32 itself, so it is exact.
// scene_soft_add puts one candidate in, at the price of one double exp:
//   the first candidate:  (1, v, 1, v)
//   v <= M, or M a NaN:   e = exp(beta (v - M));  S += e;  T = fma(v, e, T)                  (a NaN M stays)
//   else (a NaN v too):   r = exp(beta (M - v));  S = fma(S, r, 1);  T = fma(T, r, v);  M = v
// scene_soft_merge joins A (the earlier one) and B: an empty side yields the other side unchanged; else M = MA if MA > MB or MA is
// a NaN, else MB (so a NaN on either side stays), S = SA exp(beta (MA - M)) + SB exp(beta (MB - M)), T likewise, n = nA + nB.  One
// of the two factors is exp(0) = 1.  A NaN candidate makes M, S and T of every state it enters NaN and is counted like any other;
// infinite values are outside the contract (exp(beta (inf - inf)) is a NaN, nothing faults, n stays exact).
// Everything runs in a fixed order - a thread's pixels ascending, scene_soft_tree over the 256 threads, the slots t, t + 256, ... of
// a group, the carried state first - and there are no atomics: identical calls are bit-identical.
struct SceneSoft { int n; float M; double S, T; };
__device__ __forceinline__ SceneSoft scene_soft_empty() { SceneSoft a; a.n = 0; a.M = -INFINITY; a.S = 0.0; a.T = 0.0; return a; }
__device__ __forceinline__ void scene_soft_add(SceneSoft& a, float v, double beta) {
    if (a.n == 0) { a.M = v; a.S = 1.0; a.T = (double)v; }
    else {
        const bool below = v <= a.M || a.M != a.M;
        const double e = exp(beta * (below ? (double)v - (double)a.M : (double)a.M - (double)v));
        if (below) { a.S += e; a.T = fma((double)v, e, a.T); }
        else { a.S = fma(a.S, e, 1.0); a.T = fma(a.T, e, (double)v); a.M = v; }
    }
    ++a.n;
}
__device__ __forceinline__ SceneSoft scene_soft_merge(const SceneSoft A, const SceneSoft B, double beta) {
    if (B.n == 0) return A;
    if (A.n == 0) return B;
    SceneSoft r;
    r.n = A.n + B.n;
    r.M = A.M > B.M || A.M != A.M ? A.M : B.M;
    const double fa = exp(beta * ((double)A.M - (double)r.M)), fb = exp(beta * ((double)B.M - (double)r.M));
    r.S = A.S * fa + B.S * fb;
    r.T = A.T * fa + B.T * fb;
    return r;
}
// The fixed tree over the workgroup's 256 states: (S, T) as two doubles per thread (4 KB of LDS), M and n beside them; at every
// level thread t < s merges its state (the earlier one) with that of thread t + s.  Thread 0 returns the workgroup's state.
__device__ __forceinline__ SceneSoft scene_soft_tree(SceneSoft a, double beta, int t) {
    __shared__ double2 st[256];
    __shared__ float sm[256];
    __shared__ int sn[256];
    st[t] = make_double2(a.S, a.T); sm[t] = a.M; sn[t] = a.n;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            SceneSoft b;
            b.n = sn[t + s]; b.M = sm[t + s]; b.S = st[t + s].x; b.T = st[t + s].y;
            a = scene_soft_merge(a, b, beta);
            st[t] = make_double2(a.S, a.T); sm[t] = a.M; sn[t] = a.n;
        }
        __syncthreads();
    }
    return a;
}
// The walk: scene_walk's tiling, selection and order - one workgroup = one tile of kSceneTile consecutive pixels of one map
// (blockIdx.y), the planes staged in dynamic LDS (PLANES x OH x OW floats), the masks read BEFORE the geometry (scene_select4), then
// scene_point, then the very expression scene_walk stores: (float)scene_interp, or scene_class_prob(scene_class, cls).  Only a
// selected valid pixel pays the exponential of scene_soft_add.  The workgroup's state goes to slot blockIdx.y * gridDim.x +
// blockIdx.x: M into part_val, n into part_idx, (S, T) into part_st.  A workgroup without a candidate leaves the empty state.
template <int PLANES>
__device__ __forceinline__ void scene_softmax_walk(const float* q, int64_t map_stride, int map0, const SceneAffine& aff, const SceneSelect& sel,
                                                   const SceneGeo& g, int cls, const double* masks, int mvec, double beta,
                                                   float* part_val, int* part_idx, double2* part_st) {
    extern __shared__ float sq[];
    const int t = threadIdx.x, m = blockIdx.y;
    const int P = g.OH * g.OW;
    const float* qm = q + (int64_t)(map0 + m) * map_stride;
    for (int i = t; i < PLANES * P; i += 256) sq[i] = qm[i];
    __syncthreads();
    const double a00 = (double)aff.a[m][0], a01 = (double)aff.a[m][1], a10 = (double)aff.a[m][2], a11 = (double)aff.a[m][3];
    const int npix = g.hm * g.hm;                       // (the host refuses maps of 2^31 pixels or more)
    const int base = blockIdx.x * kSceneTile;
    const int ta = sel.a[m], tb = sel.b[m];
    SceneSoft a = scene_soft_empty();
    for (int pass = 0; pass < kSceneTile / 1024; ++pass) {
        const int i0 = base + 4 * (pass * 256 + t);
        if (i0 >= npix) break;
        int iy = i0 / g.hm, ix = i0 - iy * g.hm;
        bool s[4] = {true, true, true, true};
        if (ta >= 0 || tb >= 0) {
            s[0] = s[1] = s[2] = s[3] = false;
            scene_select4(masks, ta, npix, i0, mvec, s);
            scene_select4(masks, tb, npix, i0, mvec, s);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k, ++ix) {
            if (ix == g.hm) { ix = 0; ++iy; }
            if (i0 + k < npix && s[k]) {
                const ScenePoint p = scene_point(g, a00, a01, a10, a11, iy, ix);
                if (p.valid) {
                    float v;
                    if constexpr (PLANES == 1) v = (float)scene_interp(p, sq, g.OW);
                    else v = scene_class_prob(scene_class(p, sq, P, g.OW), cls);
                    scene_soft_add(a, v, beta);
                }
            }
        }
    }
    a = scene_soft_tree(a, beta, t);
    if (t == 0) {
        const int slot = blockIdx.y * gridDim.x + blockIdx.x;
        part_val[slot] = a.M; part_idx[slot] = a.n; part_st[slot] = make_double2(a.S, a.T);
    }
}
static __global__ __launch_bounds__(256) void scene_softmax_objects_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                           const SceneSelect sel, const SceneGeo g, const double* masks, int mvec,
                                                                           double beta, float* part_val, int* part_idx, double2* part_st) {
    scene_softmax_walk<1>(q, map_stride, map0, aff, sel, g, 0, masks, mvec, beta, part_val, part_idx, part_st);
}
static __global__ __launch_bounds__(256) void scene_class_softmax_objects_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                                 const SceneSelect sel, const SceneGeo g, int cls, const double* masks,
                                                                                 int mvec, double beta, float* part_val, int* part_idx, double2* part_st) {
    scene_softmax_walk<3>(q, map_stride, map0, aff, sel, g, cls, masks, mvec, beta, part_val, part_idx, part_st);
}
// The grouped reduce, the second launch per launch of maps: one workgroup per group (blockIdx.x) merges the slots of this launch's
// `n_maps` maps (`tiles` slots each, map-major) whose map belongs to its group - thread t takes slots t, t + 256, ... in that order,
// then the tree.  With `carry` thread 0 starts from the state the earlier launches left in the group's row of stats
// ([n_groups][4] doubles = n, M, S, T: the row carries the RAW state between launches, n and M exactly as doubles, so there is no
// per-group scratch).  Every group's row is written: a group without a map, or without a candidate, holds the empty state.
static __global__ __launch_bounds__(256) void scene_softmax_group_reduce_kernel(const float* part_val, const int* part_idx, const double2* part_st,
                                                                                int tiles, int n_maps, const SceneSelect sel, int carry,
                                                                                double beta, double* stats) {
    const int t = threadIdx.x, grp = blockIdx.x;
    double* row = stats + (int64_t)grp * 4;
    SceneSoft a = scene_soft_empty();
    if (t == 0 && carry) { a.n = (int)row[0]; a.M = (float)row[1]; a.S = row[2]; a.T = row[3]; }
    for (int i = t; i < tiles * n_maps; i += 256) {
        if (sel.group[i / tiles] != grp) continue;
        SceneSoft b;
        b.n = part_idx[i]; b.M = part_val[i]; b.S = part_st[i].x; b.T = part_st[i].y;
        a = scene_soft_merge(a, b, beta);
    }
    a = scene_soft_tree(a, beta, t);
    if (t == 0) { row[0] = (double)a.n; row[1] = (double)a.M; row[2] = a.S; row[3] = a.T; }
}
// The last launch, one thread per group: the raw state becomes the row {count, vmax, lse = fma(beta, M, log S), mean = T / S}, in
// place; a group without a candidate gets (0, -inf, -inf, NaN).
static __global__ __launch_bounds__(256) void scene_softmax_finish_kernel(double* stats, int n_groups, double beta) {
    const int grp = blockIdx.x * 256 + threadIdx.x;
    if (grp >= n_groups) return;
    double* row = stats + (int64_t)grp * 4;
    const double n = row[0], M = row[1], S = row[2], T = row[3];
    if (n == 0.0) { row[1] = -INFINITY; row[2] = -INFINITY; row[3] = NAN; }
    else { row[2] = fma(beta, M, log(S)); row[3] = T / S; }
}

// ---- the collapsed map: per group and heightmap pixel the best value over the group's maps and which map gives it ----
// (smg_scene_best_maps, smg_scene_class_best_maps).  scene_walk is parallel over MAPS; this walk is parallel over GROUPS: one
// workgroup = one tile of kSceneBestTile consecutive heightmap pixels of one group (blockIdx.y = group, blockIdx.x = tile), thread t
// owns pixels 4 t .. 4 t + 3 of the tile and keeps their running best (value, map index of the whole call) in 8 registers.  The
// workgroup visits the launch's maps in ascending order and skips those of other groups (sel.group[m], a kernel argument: the same
// for every thread); a map of its own is staged in dynamic LDS (PLANES x OH x OW floats, one map at a time, a barrier before and
// after) and every thread offers its pixels: the mask terms first (scene_select4; read again only when the terms differ from the
// previous map's, which for an object's rotations they never do), then scene_point, then the very expression scene_walk stores -
// scene_interp, or scene_class_prob(scene_class, cls) - compared by argmax_better with the map index as the index.  An unselected or
// invalid pixel is skipped, not compared.  Maps are visited in ascending index, so the lowest map wins a tie and the first NaN stays.
// The tile is 1024 pixels, not scene_walk's 8192: the groups are few (one for a sweep), so the pixel tiles have to supply the
// workgroups - 400 per group at hm = 640 - and eight registers of running bests leave the double-precision chain its occupancy; the
// price is that a map is staged once per 1024 pixels, 6 (18) loads per thread from L2 beside 4 pixels of the chain.
// Launches after the first (map0 > 0) carry the outputs: the thread reads its four pairs back as the running best (index -1 =
// nothing held), and a workgroup whose group has no map in this launch returns at once and leaves its pixels as they are.  In the
// first launch it stores the empty pair (-inf, -1) instead.  That decision reads kernel arguments only and is taken before any
// barrier.  Every element of both outputs is written by the first launch; no atomics, no scratch of the engine.
// Stores (and the carry's loads) are one 16-byte unit per output when hm^2 is a multiple of 4 and that output is 16-byte aligned
// (`vvec` / `avec`: scene_vec4's split, taken per output), else guarded 4-byte ones; `mvec` is the same split on the masks.
constexpr int kSceneBestTile = 1024;     // heightmap pixels per workgroup: 256 threads x 4 consecutive pixels, one pass
template <int PLANES>
__device__ __forceinline__ void scene_best_walk(const float* q, int64_t map_stride, int map0, int n_maps, const SceneAffine& aff,
                                                const SceneSelect& sel, const SceneGeo& g, int cls, const double* masks, int mvec,
                                                float* val_out, int* arg_out, int vvec, int avec) {
    extern __shared__ float sq[];
    const int t = threadIdx.x, grp = blockIdx.y;
    bool any = false;
    for (int m = 0; m < n_maps; ++m) any = any || sel.group[m] == grp;
    if (!any && map0 > 0) return;                       // (the same for every thread: nobody reaches a barrier)
    const int P = g.OH * g.OW;
    const int npix = g.hm * g.hm;                       // (the host refuses n_groups * hm^2 beyond 2^31 - 1)
    const int i0 = blockIdx.x * kSceneBestTile + 4 * t;
    const bool mine = i0 < npix;
    const int iy0 = i0 / g.hm, ix0 = i0 - iy0 * g.hm;
    float* vo = val_out + (int64_t)grp * npix + i0;
    int* ao = arg_out + (int64_t)grp * npix + i0;
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int at[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
    if (map0 > 0 && mine) {                             // what the earlier launches left
        int a[4] = {-1, -1, -1, -1};
        if (vvec) { const float4 v = *reinterpret_cast<const float4*>(vo); best[0] = v.x; best[1] = v.y; best[2] = v.z; best[3] = v.w; }
        else
            for (int k = 0; k < 4; ++k) if (i0 + k < npix) best[k] = vo[k];
        if (avec) { const int4 v = *reinterpret_cast<const int4*>(ao); a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }
        else
            for (int k = 0; k < 4; ++k) if (i0 + k < npix) a[k] = ao[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) at[k] = a[k] < 0 ? 0x7fffffff : a[k];
    }
    int la = -2, lb = -2;                               // the mask terms s[] was read for (-2: none yet)
    bool s[4] = {true, true, true, true};
    for (int m = 0; m < n_maps; ++m) {
        if (sel.group[m] != grp) continue;              // (uniform)
        __syncthreads();                                // the previous map's readers are done
        const float* qm = q + (int64_t)(map0 + m) * map_stride;
        for (int i = t; i < PLANES * P; i += 256) sq[i] = qm[i];
        __syncthreads();
        if (mine) {
            const int ta = sel.a[m], tb = sel.b[m];
            if (ta != la || tb != lb) {
                la = ta; lb = tb;
                const bool every = ta < 0 && tb < 0;
                s[0] = s[1] = s[2] = s[3] = every;
                if (!every) {
                    scene_select4(masks, ta, npix, i0, mvec, s);
                    scene_select4(masks, tb, npix, i0, mvec, s);
                }
            }
            const double a00 = (double)aff.a[m][0], a01 = (double)aff.a[m][1], a10 = (double)aff.a[m][2], a11 = (double)aff.a[m][3];
            int iy = iy0, ix = ix0;
#pragma unroll
            for (int k = 0; k < 4; ++k, ++ix) {
                if (ix == g.hm) { ix = 0; ++iy; }
                if (i0 + k < npix && s[k]) {
                    const ScenePoint p = scene_point(g, a00, a01, a10, a11, iy, ix);
                    if (p.valid) {
                        float v;
                        if constexpr (PLANES == 1) v = (float)scene_interp(p, sq, g.OW);
                        else v = scene_class_prob(scene_class(p, sq, P, g.OW), cls);
                        if (argmax_better(v, map0 + m, best[k], at[k])) { best[k] = v; at[k] = map0 + m; }
                    }
                }
            }
        }
    }
    if (!mine) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (at[k] == 0x7fffffff) at[k] = -1;
    if (vvec) *reinterpret_cast<float4*>(vo) = make_float4(best[0], best[1], best[2], best[3]);
    else
        for (int k = 0; k < 4; ++k) if (i0 + k < npix) vo[k] = best[k];
    if (avec) *reinterpret_cast<int4*>(ao) = make_int4(at[0], at[1], at[2], at[3]);
    else
        for (int k = 0; k < 4; ++k) if (i0 + k < npix) ao[k] = at[k];
}
static __global__ __launch_bounds__(256) void scene_best_maps_kernel(const float* q, int64_t map_stride, int map0, int n_maps, const SceneAffine aff,
                                                                     const SceneSelect sel, const SceneGeo g, const double* masks, int mvec,
                                                                     float* val_out, int* arg_out, int vvec, int avec) {
    scene_best_walk<1>(q, map_stride, map0, n_maps, aff, sel, g, 0, masks, mvec, val_out, arg_out, vvec, avec);
}
// smg_scene_class_best_maps: the same walk on the three logit planes (dynamic LDS 3 x OH x OW floats); an unselected pixel never
// reaches scene_class and its three double exponentials.
static __global__ __launch_bounds__(256) void scene_class_best_maps_kernel(const float* q, int64_t map_stride, int map0, int n_maps, const SceneAffine aff,
                                                                           const SceneSelect sel, const SceneGeo g, int cls, const double* masks, int mvec,
                                                                           float* val_out, int* arg_out, int vvec, int avec) {
    scene_best_walk<3>(q, map_stride, map0, n_maps, aff, sel, g, cls, masks, mvec, val_out, arg_out, vvec, avec);
}

// ---- the value of a map at K listed heightmap pixels (smg_scene_values, smg_scene_class_values) ----
// blockIdx.y = map of this launch, blockIdx.x * 256 + threadIdx.x = point k of that map's K; pixels [maps][K][2] = (iy, ix), 4-byte
// aligned only, hence two 4-byte loads.  A point outside the heightmap is -inf before the geometry: whatever int32 it holds enters
// no arithmetic and no address.  A point inside goes through scene_point and scene_interp (PLANES == 1) or scene_class +
// scene_class_prob (PLANES == 3; cls == -1: all three), the functions scene_walk calls, so the float stored here is the one
// scene_walk stores at [map][iy][ix].  The corners are read from global memory: 4 (12) loads per point of a map that sits in L2,
// against staging PLANES x OH x OW floats per workgroup for at most 256 points.  No LDS, no barrier, one 4-byte store per plane:
// out [maps][K], or with cls == -1 [maps][3][K].
template <int PLANES>
static __global__ __launch_bounds__(256) void scene_values_kernel(const float* q, int64_t map_stride, int map0, const SceneAffine aff,
                                                                  const SceneGeo g, int cls, int K, const int* pixels, float* out) {
    const int m = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int64_t at = (int64_t)(map0 + m) * K + k;
    const int iy = pixels[2 * at], ix = pixels[2 * at + 1];
    const int planes = PLANES == 3 && cls < 0 ? 3 : 1;  // planes stored per map
    float v[PLANES];
#pragma unroll
    for (int c = 0; c < PLANES; ++c) v[c] = -INFINITY;
    if (iy >= 0 && iy < g.hm && ix >= 0 && ix < g.hm) {
        const ScenePoint p = scene_point(g, (double)aff.a[m][0], (double)aff.a[m][1], (double)aff.a[m][2], (double)aff.a[m][3], iy, ix);
        if (p.valid) {
            const float* qm = q + (int64_t)(map0 + m) * map_stride;
            if constexpr (PLANES == 1) v[0] = (float)scene_interp(p, qm, g.OW);
            else {
                const SceneClass c = scene_class(p, qm, g.OH * g.OW, g.OW);
                if (cls < 0) { v[0] = scene_class_prob(c, 0); v[1] = scene_class_prob(c, 1); v[2] = scene_class_prob(c, 2); }
                else v[0] = scene_class_prob(c, cls);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < PLANES; ++c) {
        if (c >= planes) break;
        out[((int64_t)(map0 + m) * planes + c) * K + k] = v[c];
    }
}

// ---- the two losses: what one labelled point contributes, each written once ----
// A loss has three members.  mask(at) reads what decides whether the point whose label (and weight) sit at index `at` counts -
// apart from the geometry, so the list form issues this load beside the one of its pixel; counts(m) decides, before the map is
// read; terms(g, p, m, at, home, l, gk) on a valid counted point p gives l = its loss term (needed where `home` is set only) and
// gk[c] = the derivative of the pair's unnormalised loss by the interpolated value of plane c.  kPlanes planes, Q = the pair's
// map(s), in LDS or global.  (l by reference and gk as a pointer to the caller's array: both stay in registers, scratch is 0.)
//
// The Huber of code/trainer.py:345-348 on one Q plane, weighted: d = v - label in double (v not rounded), l = w huber(d),
// gk = w huber'(d).  weight == nullptr is all ones; a weight of exactly 0 masks its point (the label under it is not read).
struct HuberTerm { double l, gr; };
__device__ __forceinline__ HuberTerm scene_huber(double d) {
    HuberTerm h;
    if (fabs(d) < 1.0) { h.l = 0.5 * (d * d); h.gr = d; }
    else { h.l = fabs(d) - 0.5; h.gr = d > 0.0 ? 1.0 : -1.0; }
    return h;
}
struct SceneHuber {
    static constexpr int kPlanes = 1;
    const float *Q, *label, *weight;
    __device__ __forceinline__ double mask(int64_t at) const { return weight ? (double)weight[at] : 1.0; }
    __device__ __forceinline__ bool counts(double w) const { return w != 0.0; }
    __device__ __forceinline__ void terms(const SceneGeo& g, const ScenePoint& p, double w, int64_t at, bool home, double& l, double* gk) const {
        const HuberTerm h = scene_huber(scene_interp(p, Q, g.OW) - (double)label[at]);
        l = w * h.l; gk[0] = w * h.gr;
    }
};
// The cross entropy (CrossEntropyLoss2d, class weights {1, 1, 0}) of the three interpolated logits: a point COUNTS when its label
// is exactly 0.f or 1.f; every other label (class 2, NaN, any other value) masks it, whatever logits lie under it.  Per counted
// point, in double:     nll = (log(s) + m) - z_y        g_c = e_c / s - [c == y]
// (the logarithm is taken under `home` alone).  The caller counts the points and divides by their number W.
struct CeTerm { double nll, g0, g1, g2; };
__device__ __forceinline__ CeTerm scene_ce(const SceneClass c, float lf, bool home) {       // (by value: see scene_class_prob)
    CeTerm r;
    r.nll = 0.0;
    if (home) r.nll = (log(c.s) + c.m) - (lf == 0.f ? c.z0 : c.z1);
    r.g0 = c.e0 / c.s - (lf == 0.f ? 1.0 : 0.0); r.g1 = c.e1 / c.s - (lf == 1.f ? 1.0 : 0.0); r.g2 = c.e2 / c.s;
    return r;
}
struct SceneCe {
    static constexpr int kPlanes = 3;
    const float *Q, *label;
    __device__ __forceinline__ float mask(int64_t at) const { return label[at]; }
    __device__ __forceinline__ bool counts(float lf) const { return lf == 0.f || lf == 1.f; }
    __device__ __forceinline__ void terms(const SceneGeo& g, const ScenePoint& p, float lf, int64_t at, bool home, double& l, double* gk) const {
        const CeTerm r = scene_ce(scene_class(p, Q, g.OH * g.OW, g.OW), lf, home);
        l = r.nll; gk[0] = r.g0; gk[1] = r.g1; gk[2] = r.g2;
    }
};

// ---- the list form: K labelled heightmap pixels per pair (smg_loss_scene_ce, and in its own copy smg_loss_scene) ----
// One workgroup per pair (blockIdx.x = pair of this launch); `sacc` = kPlanes x OH x OW double accumulators in dynamic LDS, zeroed
// by the caller.  Gather form: the points are taken 256 at a time - thread t works point t of the group out into LDS (corner,
// fractions, gk) - then every thread walks the group in index order for the map elements it owns (t, t + 256, ... in every plane),
// adding gk[c] * (bilinear weight of the element at the point) in double to its own accumulators.  No atomics: duplicate points
// simply add twice, and every element is written once.  A point outside the heightmap, invalid in the pair's rotation or masked by
// the loss contributes nothing; the others add their loss term to the thread's `lsum` and 1 to its `cnt`.
template <class Loss>
__device__ __forceinline__ void scene_list_walk(const SceneGeo& g, double a00, double a01, double a10, double a11, int j, int K, const int* pixels,
                                                const Loss& L, double* sacc, double& lsum, int& cnt) {
    constexpr int C = Loss::kPlanes;
    __shared__ double p_fy[256], p_fx[256], p_g[C][256];
    __shared__ int p_o[256];
    const int t = threadIdx.x;
    const int P = g.OH * g.OW;
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int k = k0 + t;
        int o = -1; double fy = 0.0, fx = 0.0, gk[C];
#pragma unroll
        for (int c = 0; c < C; ++c) gk[c] = 0.0;
        if (k < K) {
            const int64_t at = (int64_t)j * K + k;
            const int iy = pixels[2 * at], ix = pixels[2 * at + 1];
            const auto m = L.mask(at);
            if (L.counts(m) && iy >= 0 && iy < g.hm && ix >= 0 && ix < g.hm) {
                const ScenePoint p = scene_point(g, a00, a01, a10, a11, iy, ix);
                if (p.valid) {
                    double l;
                    L.terms(g, p, m, at, true, l, gk);
                    lsum += l; ++cnt;
                    o = p.y0 * g.OW + p.x0; fy = p.fy; fx = p.fx;
                }
            }
        }
        p_o[t] = o; p_fy[t] = fy; p_fx[t] = fx;
#pragma unroll
        for (int c = 0; c < C; ++c) p_g[c][t] = gk[c];
        __syncthreads();
        const int n = min(256, K - k0);
        for (int i = t; i < P; i += 256) {
            const int ey = i / g.OW, ex = i - ey * g.OW;
            double acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = sacc[c * P + i];
            for (int kk = 0; kk < n; ++kk) {
                const int oo = p_o[kk];
                if (oo < 0) continue;
                const int y0 = oo / g.OW, x0 = oo - y0 * g.OW;
                const int dy = ey - y0, dx = ex - x0;
                if ((unsigned)dy > 1u || (unsigned)dx > 1u) continue;
                const double wy = dy ? p_fy[kk] : 1.0 - p_fy[kk], wx = dx ? p_fx[kk] : 1.0 - p_fx[kk];
                const double wgt = wy * wx;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += p_g[c][kk] * wgt;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) sacc[c * P + i] = acc[c];
        }
        __syncthreads();
    }
}

// smg_loss_scene: the list form with the Huber - loss[j] = sum_k w_k huber(d_k), dq[j][oy][ox] = the accumulator, unnormalised,
// every element written once, zeros included, rounded once.  The map is staged in LDS behind the accumulators: dynamic LDS OH * OW
// doubles + OH * OW floats.  This kernel keeps a loop of its own, the same as scene_list_walk's on one plane: as an instantiation
// of scene_list_walk it ran 0.5 to 1.8 % slower at K = 409 600 (291.3 to 293.8 ms against 288.4 to 289.8, repeats 0.3 to 2 ms
// apart) with the same instructions in the inner loop.
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
                    const HuberTerm h = scene_huber(d);
                    lsum += w * h.l;
                    o = p.y0 * g.OW + p.x0; fy = p.fy; fx = p.fx; gk = w * h.gr;
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
    block_sum(t, red);
    if (t == 0) loss[j] = (float)red[0];
    float* dj = dq + (int64_t)j * P;
    for (int i = t; i < P; i += 256) dj[i] = (float)sacc[i];
}

// smg_loss_scene_ce: W = the number of counted points; loss[j] = (sum nll_k) / W and dq[j][c][oy][ox] = accumulator / W: summed
// unnormalised in point order, divided once, rounded once; W == 0 gives loss 0 and dq 0.  Dynamic LDS: the 3 OH OW double
// accumulators only - the logits are read from global memory (a few corners per point of a map that sits in L2), which keeps
// 38 x 38 maps at 35 KB + 14 KB static.
static __global__ __launch_bounds__(256) void loss_scene_ce_kernel(const float* q, int pair0, const SceneAffine aff, const SceneGeo g, int K,
                                                                   const int* pixels, const float* label, float* loss, float* dq) {
    extern __shared__ double sacc[];
    __shared__ double red[256];
    __shared__ int rcnt[256];
    const int t = threadIdx.x, m = blockIdx.x, j = pair0 + m;
    const int P = g.OH * g.OW;
    for (int i = t; i < 3 * P; i += 256) sacc[i] = 0.0;
    __syncthreads();
    double lsum = 0.0; int cnt = 0;
    scene_list_walk(g, (double)aff.a[m][0], (double)aff.a[m][1], (double)aff.a[m][2], (double)aff.a[m][3], j, K, pixels,
                    SceneCe{q + (int64_t)j * 3 * P, label}, sacc, lsum, cnt);
    red[t] = lsum; rcnt[t] = cnt;
    block_sum(t, red, rcnt);
    const int W = rcnt[0];
    const double dW = (double)W;
    if (t == 0) loss[j] = W > 0 ? (float)(red[0] / dW) : 0.f;
    float* dj = dq + (int64_t)j * 3 * P;
    for (int i = t; i < 3 * P; i += 256) dj[i] = W > 0 ? (float)(sacc[i] / dW) : 0.f;
}

// ---- the image form: a whole [hm][hm] label image per pair (smg_loss_scene_map, smg_loss_scene_map_ce) ----
// The heightmap box of map element (oy, ox): pixels bx0 .. bx0 + bw - 1 of rows by0 .., n = bw * rows of them in row-major order
// (0 when the box is empty).  scene_box_walk's comment below has the construction.
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

// Every pixel of the image that is valid in the pair's rotation and not masked by the loss is a point.  Gather by map element: one
// workgroup owns one (pair, oy, ox) - blockIdx.x = oy * OW + ox, blockIdx.y = pair of this launch.  Only
// pixels whose corner (y0, x0) lies in {oy - 1, oy} x {ox - 1, ox} touch that element: they lie at map coordinates
// [ox - 1, ox + 1] x [oy - 1, oy + 1], clipped to the map.  The four corners of that square go back through the chain with the
// inverse of A^T (u = A^-T p, whatever the 2x2 matrix is: scene_point asks for no rotation); the heightmap bounding box of the
// four images, widened by one pixel per side and clipped to the heightmap, holds every such pixel (for a rotation about 34 x 34 at
// a multiple of a quarter turn, 46 x 46 at 45 degrees).  A matrix without a usable inverse (determinant 0, not finite, or below
// 1e-6 of the squared norm) maps whole lines of pixels onto one map point: the box is then the whole heightmap.  Thread t takes
// pixels t, t + 256, ... of the box in row-major order, runs scene_point on each, keeps the valid ones that touch the element, and
// adds gk[c] * (bilinear weight of the element at the pixel) in double to its acc[c]; the caller's fixed tree over the 256 threads
// follows.  Label and weight are read only under a valid touching pixel, the map's corners only under an unmasked one and from global
// memory (the map sits in L2; for the twelve corner logits of the cross entropy, staging the 27 logits around the element in LDS
// measured 0.755 against 0.776 ms at S = 1824, inside the spread between repeats, and was not kept).  A pixel's gradient share goes to
// every element it touches, so its terms are evaluated by up to four workgroups: the price of a form without atomics, in which
// identical calls are bit-identical and a pair's results do not depend on which launch carries it.  Its loss term and its count go to
// its HOME element (y0, x0) only.
template <class Loss>
__device__ __forceinline__ void scene_box_walk(const SceneGeo& g, double a00, double a01, double a10, double a11, int j, int oy, int ox,
                                               const Loss& L, double (&acc)[Loss::kPlanes], double& lsum, int& cnt) {
    const SceneBox box = scene_element_box(g, a00, a01, a10, a11, oy, ox);
    const int bx0 = box.bx0, by0 = box.by0, bw = box.bw, n = box.n;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int ry = i / bw;
        const int iy = by0 + ry, ix = bx0 + (i - ry * bw);
        const ScenePoint p = scene_point(g, a00, a01, a10, a11, iy, ix);
        if (!p.valid) continue;
        const int dy = oy - p.y0, dx = ox - p.x0;
        if ((unsigned)dy > 1u || (unsigned)dx > 1u) continue;
        const bool home = dy == 0 && dx == 0;
        const int64_t at = ((int64_t)j * g.hm + iy) * g.hm + ix;
        const auto m = L.mask(at);
        if (!L.counts(m)) continue;
        double l, gk[Loss::kPlanes];
        L.terms(g, p, m, at, home, l, gk);
        if (home) { lsum += l; ++cnt; }
        const double wy = dy ? p.fy : 1.0 - p.fy, wx = dx ? p.fx : 1.0 - p.fx;
        const double wgt = wy * wx;
#pragma unroll
        for (int c = 0; c < Loss::kPlanes; ++c) acc[c] += gk[c] * wgt;
    }
}

// smg_loss_scene_map: loss_scene_kernel's Huber on the image - loss[j] = sum_pixels w huber(v - label), dq[j][oy][ox] = the
// element's sum, written once, rounded once.  The per-element loss sums go to `lpart` ([pairs of this launch][OH * OW] doubles,
// every slot written) for loss_scene_map_reduce_kernel.
static __global__ __launch_bounds__(256) void loss_scene_map_kernel(const float* q, int pair0, const SceneAffine aff, const SceneGeo g,
                                                                    const float* label, const float* weight, double* lpart, float* dq) {
    __shared__ double racc[256], rloss[256];
    const int t = threadIdx.x, m = blockIdx.y, j = pair0 + m, el = blockIdx.x;
    const int P = g.OH * g.OW;
    double acc[1] = {0.0}, lsum = 0.0; int cnt = 0;
    scene_box_walk(g, (double)aff.a[m][0], (double)aff.a[m][1], (double)aff.a[m][2], (double)aff.a[m][3], j, el / g.OW, el % g.OW,
                   SceneHuber{q + (int64_t)j * P, label, weight}, acc, lsum, cnt);
    racc[t] = acc[0]; rloss[t] = lsum;
    block_sum(t, racc, rloss);
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
    block_sum(t, red);
    if (t == 0) loss[pair0 + m] = (float)red[0];
}

// smg_loss_scene_map_ce: loss_scene_ce_kernel's cross entropy on the image - loss[j] = (sum nll) / W, dq[j][c][oy][ox] = (the
// element's sum) / W, W = the number of counted pixels.  W is known only when all elements of a pair are done, so this launch writes
// UNNORMALISED partials into scratch the engine owns, every slot written: gpart [pairs of this launch][3][OH * OW] doubles, lpart
// [pairs][OH * OW] doubles, cpart [pairs][OH * OW] ints.  No accumulator of the map's size in LDS (4 x 256 doubles + 256 ints of
// reduction arrays), hence no limit on the map's size beyond scene_geometry's.
static __global__ __launch_bounds__(256) void loss_scene_map_ce_kernel(const float* q, int pair0, const SceneAffine aff, const SceneGeo g,
                                                                       const float* label, double* gpart, double* lpart, int* cpart) {
    __shared__ double racc[3][256], rloss[256];
    __shared__ int rcnt[256];
    const int t = threadIdx.x, m = blockIdx.y, j = pair0 + m, el = blockIdx.x;
    const int P = g.OH * g.OW;
    double acc[3] = {0.0, 0.0, 0.0}, lsum = 0.0; int cnt = 0;
    scene_box_walk(g, (double)aff.a[m][0], (double)aff.a[m][1], (double)aff.a[m][2], (double)aff.a[m][3], j, el / g.OW, el % g.OW,
                   SceneCe{q + (int64_t)j * 3 * P, label}, acc, lsum, cnt);
    racc[0][t] = acc[0]; racc[1][t] = acc[1]; racc[2][t] = acc[2]; rloss[t] = lsum; rcnt[t] = cnt;
    block_sum(t, racc[0], racc[1], racc[2], rloss, rcnt);
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
    block_sum(t, red, cnt);
    const int W = cnt[0];
    const double dW = (double)W;
    if (t == 0) loss[j] = W > 0 ? (float)(red[0] / dW) : 0.f;
    const double* gm = gpart + (int64_t)m * 3 * P;
    float* dj = dq + (int64_t)j * 3 * P;
    for (int i = t; i < 3 * P; i += 256) dj[i] = W > 0 ? (float)(gm[i] / dW) : 0.f;
}

// ---- the loss of the Boltzmann policy: log-likelihood of an executed action and entropy, per group (smg_loss_scene_policy) ----
// The candidates of group g are smg_scene_softmax_objects': the selected valid pixels of its pairs, each with the float32 v the walks
// store; pi_i = exp(beta v_i - lse).  With act = the group's executed action (a flattened index into [n_pairs][hm][hm], -1 = none)
// and the weights {w_nll, w_ent}:
//     H    = lse - beta mean
//     loss = w_nll (lse - beta v_act) - w_ent H
//     dloss/dv_i = pi_i (A + B (v_i - mean)) + C [i == act],      A = w_nll beta,  B = w_ent beta^2,  C = -w_nll beta
// (the float32 rounding of v_i counts as the identity); with act == -1 the w_nll terms are absent and w_nll is not read into any
// arithmetic.  Three phases on one stream: the normaliser (the softmax kernels above, unchanged) fills every group's row {count,
// vmax, lse, mean}; loss_scene_policy_kernel gathers dq; loss_scene_policy_finish_kernel forms the losses.
//
// ScenePolicy is the gather's Loss.  `at` is the pixel's flattened index ((pair j) * hm + iy) * hm + ix, the number an action is
// compared with - no address is ever formed from the action.  mask(at) tests the pair's two mask terms at the pixel by
// scene_select4's rule on the single double - the bit pattern without its sign, so -0.0 does not select and a NaN does - read as two
// 4-byte words: masks that are only 4-byte aligned work.  terms() forms v by the very expression the walks store and the one
// thread that meets the action at its HOME element writes v into the group's slot of `loss` (flattened indices are unique and a
// pixel has one home: a single writer; the slot holds the caller's NaN prefill until then).
struct ScenePolicy {
    static constexpr int kPlanes = 1;
    const float* Q;
    const unsigned* masks;           // the masks tensor as 4-byte words
    int ta, tb, npix;
    int64_t first;                   // the flattened index of the pair's pixel 0
    double beta, lse, mean, A, B, C;
    int act;
    float* vact;
    __device__ __forceinline__ bool term(int t, int64_t pix) const {
        const unsigned* w = masks + 2 * ((int64_t)t * npix + pix);
        return ((w[1] << 1) | w[0]) != 0u;
    }
    __device__ __forceinline__ bool mask(int64_t at) const {
        if (ta < 0 && tb < 0) return true;
        const int64_t pix = at - first;
        return (ta >= 0 && term(ta, pix)) || (tb >= 0 && term(tb, pix));
    }
    __device__ __forceinline__ bool counts(bool selected) const { return selected; }
    __device__ __forceinline__ void terms(const SceneGeo& g, const ScenePoint& p, bool, int64_t at, bool home, double& l, double* gk) const {
        const float v = (float)scene_interp(p, Q, g.OW);
        const double pi = exp(fma(beta, (double)v, -lse));
        const bool is = act >= 0 && (int64_t)act == at;
        gk[0] = pi * (A + B * ((double)v - mean)) + (is ? C : 0.0);
        if (is && home) *vact = v;
        l = 0.0;
    }
};
// Phase 2: one workgroup per (pair, map element) - blockIdx.x = element, blockIdx.y = pair of this launch - as loss_scene_map_kernel.
// The group's {lse, mean} come from its finished row of `stats`, {A, B, C} from `weight` [n_groups][2] and `action` [n_groups].
// dq[j][el] = the element's sum, accumulated in double, reduced by block_sum's tree, rounded once, written once, zeros included; a
// group without a candidate never reaches terms(), so its pairs' dq is exactly 0.  A group whose lse is a NaN (a NaN candidate)
// gets NaN in EVERY element of its pairs, also where no candidate touches the element.
static __global__ __launch_bounds__(256) void loss_scene_policy_kernel(const float* q, int pair0, const SceneAffine aff, const SceneSelect sel,
                                                                       const SceneGeo g, const double* masks, double beta, const int* action,
                                                                       const double* weight, const double* stats, float* loss, float* dq) {
    __shared__ double racc[256];
    const int t = threadIdx.x, m = blockIdx.y, j = pair0 + m, el = blockIdx.x;
    const int P = g.OH * g.OW, grp = sel.group[m];
    const double lse = stats[(int64_t)grp * 4 + 2], mean = stats[(int64_t)grp * 4 + 3];
    const int act = action[grp];
    const double w_nll = act >= 0 ? weight[2 * (int64_t)grp] : 0.0, w_ent = weight[2 * (int64_t)grp + 1];
    const int npix = g.hm * g.hm;                       // (the host refuses n_pairs * hm^2 beyond 2^31 - 1)
    double acc[1] = {0.0}, lsum = 0.0; int cnt = 0;
    scene_box_walk(g, (double)aff.a[m][0], (double)aff.a[m][1], (double)aff.a[m][2], (double)aff.a[m][3], j, el / g.OW, el % g.OW,
                   ScenePolicy{q + (int64_t)j * P, reinterpret_cast<const unsigned*>(masks), sel.a[m], sel.b[m], npix, (int64_t)j * npix,
                               beta, lse, mean, w_nll * beta, w_ent * (beta * beta), -(w_nll * beta), act, loss + grp},
                   acc, lsum, cnt);
    racc[t] = acc[0];
    block_sum(t, racc);
    if (t == 0) dq[(int64_t)j * P + el] = lse != lse ? NAN : (float)racc[0];
}
// Before phase 2: every group's slot of `loss` is a NaN until the action is met.
static __global__ __launch_bounds__(256) void loss_scene_policy_prefill_kernel(float* loss, int n_groups) {
    const int grp = blockIdx.x * 256 + threadIdx.x;
    if (grp < n_groups) loss[grp] = NAN;
}
// Phase 3, one thread per group: loss[g] turns in place from v_act into the loss, in double, rounded once.  A group without a
// candidate: 0 with act == -1, else NaN.  An action that was no candidate of its group left the prefill: the loss stays NaN.
static __global__ __launch_bounds__(256) void loss_scene_policy_finish_kernel(const double* stats, const int* action, const double* weight,
                                                                              int n_groups, double beta, float* loss) {
    const int grp = blockIdx.x * 256 + threadIdx.x;
    if (grp >= n_groups) return;
    const double* row = stats + (int64_t)grp * 4;
    const int act = action[grp];
    double r;
    if (row[0] == 0.0) r = act < 0 ? 0.0 : (double)NAN;
    else {
        r = -(weight[2 * (int64_t)grp + 1] * (row[2] - beta * row[3]));
        if (act >= 0) r = weight[2 * (int64_t)grp] * (row[2] - beta * (double)loss[grp]) + r;
    }
    loss[grp] = (float)r;
}

}  // namespace smg
