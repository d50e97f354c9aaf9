/*
 * smg_hip.h - C ABI of the MI355X (gfx950) affordance engine.
 *
 * Drop-in boundary for ONE path of fukangl/SMG-multimodal-grasping: the
 * Trainer.forward / Trainer.backprop -> reinforcement_net / reactive_net .forward
 * loop.  The reference is pure Python on torch (no FFI of its own), so these entry
 * points are what a ctypes binding for that path binds (INTEGRATION.md shows the
 * stub); every function cites the reference interface it stands in for, paths
 * relative to the reference repository root.
 *
 * Conventions
 *   - plain pointers and sizes only; every `dev` pointer is device memory of the
 *     engine's GPU, every `host` pointer is ordinary host memory;
 *   - all work is enqueued on the hipStream_t passed as `stream` (void*, 0 = the
 *     null stream); functions with host outputs synchronise that stream;
 *   - return 0 on success, a negative errno-style code on failure;
 *     smg_last_error() gives the message (thread-local);
 *   - one engine per GPU per process; an engine is not re-entrant.
 *
 * Network state lives in three caller-owned flat device arrays whose layout is
 * defined by smg_layout_*():
 *     params  float32[smg_layout_param_floats]   (weights, BN gamma/beta, classifier)
 *     grads   float32[same]                      (same offsets)
 *     bufs    float32[smg_layout_buffer_floats]  (BN running_mean / running_var)
 *     nbt     int64  [smg_layout_nbt_count]      (BN num_batches_tracked)
 * Entry i of the layout carries the torchvision/torch state_dict key of the
 * reference model (code/models.py:308-343; torchvision densenet121 names), so a
 * reference snapshot (code/logger.py:121-125) maps 1:1 onto the arrays.
 */
#ifndef SMG_HIP_H
#define SMG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smg_engine smg_engine;

/* ---- library ------------------------------------------------------------------ */
const char* smg_last_error(void);
/* ABI revision of this header: a binding must refuse a library whose smg_version() differs (stale .so) and should
 * compare its own struct sizes with smg_abi_struct_bytes(0 = smg_batch, 1 = smg_net, 2 = smg_adam) before the first call. */
#define SMG_ABI_VERSION 9
int smg_version(void);
int smg_abi_struct_bytes(int which);

/* ---- state layout (replaces nn.Module.state_dict() ordering of
 *      code/models.py:301-358 reinforcement_net / :15-69 reactive_net) ------------- */
enum { SMG_KIND_PARAM = 0, SMG_KIND_RUNNING_MEAN = 1, SMG_KIND_RUNNING_VAR = 2, SMG_KIND_NBT = 3 };
int     smg_layout_count(int head_out);               /* 2217 entries                  */
int64_t smg_layout_param_floats(int head_out);        /* 24 419 256 (head_out=1)       */
int64_t smg_layout_buffer_floats(int head_out);
int64_t smg_layout_nbt_count(int head_out);
/* name: caller buffer of name_cap bytes; offset: element offset into the array the
 * kind selects; shape: up to 4 dims (ndim 0 for nbt scalars). */
int smg_layout_entry(int head_out, int index, char* name, int name_cap, int* kind,
                     int64_t* offset, int* ndim, int64_t shape[4]);

/* ---- engine ------------------------------------------------------------------- */
/* input_size S = side of the padded network input (640 for a 224x224 heightmap,
 * code/trainer.py:165-173); max_streams = most trunk passes per call; max_pairs =
 * most (rotated, masked) head evaluations per call; head_out = 1 (reinforcement_net)
 * or 3 (reactive_net). Allocates all activation / gradient workspaces once. */
int smg_engine_create(int device, int input_size, int max_streams, int max_pairs, int head_out,
                      smg_engine** out);
void smg_engine_destroy(smg_engine* e);
int64_t smg_engine_workspace_bytes(const smg_engine* e);

/* Network binding: the three flat arrays of ONE model instance (model or
 * model_target, code/trainer.py:73-75). */
typedef struct {
    float*   params;
    float*   grads;     /* may be NULL for inference-only nets */
    float*   bufs;
    int64_t* nbt;
} smg_net;

/* One batch of work.  A "stream" is one DenseNet-121 `.features` pass over one image
 * (code/models.py:384-385); a "pair" is one head evaluation on the concatenation of
 * two streams' features (code/models.py:386-387).
 *
 * Images come in one of two forms:
 *   images_nchw != NULL : n_images tensors [3,S,S] float32, what
 *       reinforcement_net.forward receives (code/models.py:361);
 *   heightmaps  != NULL : n_images arrays [hm_size,hm_size] float64, what
 *       Trainer.forward receives (code/trainer.py:162); the engine applies the x2
 *       nearest zoom, zero padding to S, 3-channel replication and (x-mean)/std of
 *       code/trainer.py:165-191 on the fly.
 * stream_image[s]  : which image stream s reads;
 * stream_affine[s] : 6 float32 (row-major 2x3 theta of F.affine_grid,
 *       code/models.py:374-378); the stream samples its image through
 *       affine_grid + grid_sample(nearest, align_corners=True) (code/models.py:378-382);
 * stream_rotated[s]: 0 = feed the image as is (the masked stream, models.py:385).
 * pair_a / pair_b  : stream indices whose norm5 features form channels 0..1023 /
 *       1024..2047 of the head input.
 * bn_seq_trunk     : stream indices in the order the reference would have run them
 *       (BN running statistics are updated once per entry);
 *       bn_seq_head the same for pairs.  NULL/0 = do not touch running statistics.
 */
typedef struct {
    int n_images;
    const float*  images_nchw_dev;
    const double* heightmaps_dev;
    int hm_size;
    double image_mean, image_std;
    int n_streams;
    const int*   stream_image;     /* host */
    const float* stream_affine;    /* host, 6 per stream */
    const int*   stream_rotated;   /* host */
    int n_pairs;
    const int* pair_a;             /* host */
    const int* pair_b;             /* host */
    int n_bn_seq_trunk;
    const int* bn_seq_trunk;       /* host */
    int n_bn_seq_head;
    const int* bn_seq_head;        /* host */
    /* Object masks applied on the device (heightmap form only), replacing the host products
     * `depth * mask[k]` / `depth * (mask[g] + mask[s])` of code/main.py:160,187: masks_dev holds n_masks arrays
     * [hm_size,hm_size] float64; stream s reads heightmap * (mask[stream_mask_a[s]] + mask[stream_mask_b[s]]), an
     * index of -1 meaning "no such term" (both -1: the plain heightmap).  NULL = no masking. */
    const double* masks_dev;
    int n_masks;
    const int* stream_mask_a;      /* host */
    const int* stream_mask_b;      /* host */
} smg_batch;

/* Forward: trunk `trunk_id` (0 suction_depth_trunk, 1 grasp_depth_trunk,
 * 2 gs_depth_trunk - layout order) and head `head_id` (0 suctionnet_val,
 * 1 graspnet_val, 2 gsnet_val).  q_out_dev: float32 [n_pairs][head_out][OH][OW]
 * (OH=OW=1 for S=640).  Keeps every activation needed by smg_backward until the next
 * forward on this engine.  Replaces reinforcement_net.forward / reactive_net.forward
 * (code/models.py:361-586, :72-296) for any of their branches.
 * NaN / inf: a non-finite BatchNorm batch statistic of a stream (pair) makes every Q value of the samples that use it NaN,
 * as it does in the reference (checked in every forward, with or without bn_seq_trunk / bn_seq_head). */
int smg_forward(smg_engine* e, const smg_net* net, int trunk_id, int head_id,
                const smg_batch* batch, float* q_out_dev, void* stream);

/* Loss on the device, replacing the python Huber of code/trainer.py:345-348
 * (mode 0: element [0,0,0] of each pair's output vs labels[pair]) and the weighted
 * cross entropy of code/trainer.py:296-299 + code/utils.py:306-313 (mode 1: 3 logits
 * vs integer class labels[pair], class weights {1,1,0}).  Writes loss_dev[n_pairs]
 * and dq_dev (same shape as q). */
int smg_loss(smg_engine* e, int mode, const float* q_dev, const float* labels_dev, int n_pairs,
             float* loss_dev, float* dq_dev, void* stream);

/* Whole-map loss for a dense Q map (inputs larger than S = 640: OH x OW values per pair), the per-pixel formulation of the Huber
 * of code/trainer.py:345-348; one-channel heads only (head_out != 1 returns -22 and launches nothing).  q, label, weight and dq are
 * [n_pairs][1][OH][OW]; weight_dev == NULL means all ones, a weight of exactly 0 masks its element.
 *     loss[j] = sum over the map of w * huber(q - label)        dq = w * huber'(q - label)
 * The call marks the saved forward "dense dq": the next smg_backward / smg_backward_phase(.., 0) of that forward runs the head's
 * value-convolution backward in its dense form (see "head_bwd" below).  smg_loss and every later smg_forward clear the mark. */
int smg_loss_map(smg_engine* e, const float* q_dev, const float* label_dev, const float* weight_dev, int n_pairs,
                 float* loss_dev, float* dq_dev, void* stream);

/* Whole-map cross entropy for the dense class maps of a 3-class head (reactive_net on inputs larger than S = 640): the reference's
 * CrossEntropyLoss2d (code/utils.py:306-313: NLLLoss2d(log_softmax(x, dim=1)), class weights {1, 1, 0}: code/trainer.py:38-60)
 * applied to the whole head output instead of the one pixel of code/trainer.py:296-299.  head_out != 3 returns -22 and launches
 * nothing.  q and dq are [n_pairs][3][OH][OW]; label is [n_pairs][1][OH][OW], float32 class indices as in smg_loss mode 1: 0 and 1
 * carry weight 1, anything else is class 2 ("no loss", weight 0) - the mask of the unlabelled pixels.  With P = OH * OW, per pair:
 *     nll_p   = logsumexp(q[:, p]) - q[y_p, p]          W = number of pixels of class 0 / 1
 *     loss[j] = (sum of nll_p over those pixels) / W     (torch's weighted-mean nll_loss; 0 when W == 0, not 0/0)
 *     dq[c,p] = (softmax(q[:, p])[c] - [c == y_p]) / W   (exactly 0 in all three channels of a class-2 pixel, whatever q holds)
 * Per pixel the arithmetic is smg_loss mode 1's: a map with exactly one labelled pixel reproduces its loss and dq bit for bit.
 * Like smg_loss_map the call marks the saved forward "dense dq" (see "head_bwd" below); smg_loss and every later smg_forward
 * clear the mark. */
int smg_loss_map_ce(smg_engine* e, const float* q_dev, const float* label_dev, int n_pairs,
                    float* loss_dev, float* dq_dev, void* stream);

/* ---- dense Q maps in the scene frame ----------------------------------------------------------------------------------------
 * A dense Q map lives in the ROTATED frame of its rotation, one value per 32 input pixels.  These entry points undo
 * F.affine_grid / F.grid_sample (code/models.py:372-382) and the head's 20x20 window geometry, so that a caller can read, pick and
 * train Q values at HEIGHTMAP pixels.  For a heightmap of side hm (code/trainer.py:165-173): pad = int((ceil(2 hm sqrt(2) / 32) * 32
 * - 2 hm) / 2), S = 2 hm + 2 pad (the engine's input size), OH = OW = S / 32 - 19 (the engine's).  Coordinates are (x = column,
 * y = row); all arithmetic is double:
 *   1. heightmap pixel (iy, ix) is the centre of its 2x2 replicated block of the padded input: x = 2 ix + 0.5 + pad, y likewise;
 *   2. normalised as align_corners=True does: u = 2 (x, y) / (S - 1) - 1;
 *   3. the forward computed rotated[p] = image[A p], A = the 2x2 part of the sample's theta (the six float32 numbers the forward
 *      used, widened to double): the scene point u is seen in that rotation at p = A^T u (the transpose, not a recomputed inverse);
 *   4. back to pixels: (px, py) = (p + 1) / 2 * (S - 1);
 *   5. map element (oy, ox) is the head's window over input pixels 32 ox .. 32 ox + 639, centre 32 ox + 319.5:
 *      qx = (px - 319.5) / 32, qy = (py - 319.5) / 32;
 *   6. the pixel is VALID in that rotation when 0 <= qx <= OW - 1 and 0 <= qy <= OH - 1; its value is the bilinear interpolation of
 *      the map at (qy, qx) - x0 = min(floor(qx), OW - 2), fx = qx - x0, the same in y,
 *      (1 - fy) ((1 - fx) Q[y0][x0] + fx Q[y0][x0 + 1]) + fy ((1 - fx) Q[y0 + 1][x0] + fx Q[y0 + 1][x0 + 1]) - rounded to float32 once;
 *   7. an invalid pixel has the value -inf: no window of the head is centred there.
 * affine_host: 6 float32 per map / pair, row-major 2x3 as in smg_batch.stream_affine; the translation column must be zero.
 * map_stride: element distance between consecutive maps in q_dev - OH * OW for the output of a one-channel head, 3 * OH * OW to
 * address one class plane of a [R][3][OH][OW] tensor.
 * All of them return -22 and launch nothing when hm_size does not pad to the engine's S, when the map is 1 x 1 (S = 640: no extent
 * to interpolate over), and for n_maps < 1 / K < 1 / n_pairs < 1. */

/* out_dev float32 [n_maps][hm_size][hm_size]: every map in the scene frame, -inf at invalid pixels. */
int smg_scene_maps(smg_engine* e, const float* q_dev, int64_t map_stride, int n_maps, const float* affine_host,
                   int hm_size, float* out_dev, void* stream);

/* The value of those scene-frame maps at K LISTED heightmap pixels per map, without writing the maps: pixels_dev int32
 * [n_maps][K][2] = (iy, ix), K points per map (only 4-byte alignment is assumed); out_dev float32 [n_maps][K].  out[m][k] is the
 * float smg_scene_maps stores at [m][iy][ix], bit for bit: steps 1-7 above in double, rounded to float32 once, -inf where no window
 * of the head is centred, NaN where a corner is NaN.  A point outside [0, hm_size)^2 is -inf; that is decided before the geometry
 * and no address is formed from it, so any int32 is legal there.  Any head width is accepted (map_stride = 3 OH OW addresses one
 * logit plane).  One thread per point, the four corners read from global memory; every element of out is written by every
 * successful call; no atomics, no scratch of the engine: two identical calls are bit-identical.
 * Returns -22 and launches nothing for a NULL pointer, n_maps < 1, K < 1, a negative map_stride, n_maps * K beyond int32 and the
 * geometry refusals above (hm_size, a 1 x 1 map, an affine with a translation). */
int smg_scene_values(smg_engine* e, const float* q_dev, int64_t map_stride, int n_maps, const float* affine_host,
                     int hm_size, int K, const int* pixels_dev, float* out_dev, void* stream);

/* The largest valid value of those scene-frame maps and its flattened index into [n_maps][hm_size][hm_size], without writing the
 * maps: idx_out_dev int32[1], val_out_dev float32[1].  The rules are smg_argmax's (lowest index on ties, a NaN wins) with invalid
 * pixels skipped; the result is bit-reproducible (per-workgroup partials in a scratch the engine owns, reduced by a second launch;
 * no atomics) and equals smg_argmax over smg_scene_maps' output.  Index -1, value -inf when no pixel is valid. */
int smg_scene_argmax(smg_engine* e, const float* q_dev, int64_t map_stride, int n_maps, const float* affine_host,
                     int hm_size, int* idx_out_dev, float* val_out_dev, void* stream);

/* smg_scene_argmax per OBJECT: every map restricted to the heightmap pixels its masks select, one result per group of maps, the
 * scene-frame maps never written.  Geometry, validity and values are steps 1-7 above, exactly smg_scene_maps' (a value rounded to
 * float32 once).
 * masks_dev float64 [n_masks][hm_size][hm_size] - the very tensor smg_batch.masks_dev was given for the forward: no second upload,
 * no conversion.  map_mask_a / map_mask_b (host, n_maps each): a pixel is SELECTED for map m when mask[map_mask_a[m]] or
 * mask[map_mask_b[m]] is not exactly 0 there; index -1 = no such term, both -1 = every pixel.  -0.0 does not select, a NaN does;
 * the values are never used arithmetically.  map_group (host, n_maps): map m competes for the result of group map_group[m]; the
 * maps of a group need not be contiguous.
 * idx_out_dev int32[n_groups], val_out_dev float32[n_groups]: per group the best selected valid pixel over the group's maps - the
 * flattened index into [n_maps][hm_size][hm_size] of the WHOLE call - by smg_argmax's rules (lowest index on ties, a NaN wins).  A
 * group with no map, or with no selected valid pixel, gets index -1, value -inf; every group's pair is written by every successful
 * call.  Per-workgroup partials in a scratch the engine owns, reduced by one workgroup per group; no atomics: two identical calls
 * are bit-identical, and a group's result equals smg_argmax over smg_scene_maps' output with the unselected pixels set to -inf.
 * Returns -22 and launches nothing for a NULL pointer, n_maps < 1, n_masks < 1, n_groups < 1, a negative map_stride, a mask index
 * outside [-1, n_masks), a group outside [0, n_groups), a flattened index that does not fit int32, and the geometry refusals above
 * (hm_size, a 1 x 1 map, an affine with a translation). */
int smg_scene_argmax_objects(smg_engine* e, const float* q_dev, int64_t map_stride, int n_maps, const float* affine_host,
                             int hm_size, const double* masks_dev, int n_masks, const int* map_mask_a, const int* map_mask_b,
                             const int* map_group, int n_groups, int* idx_out_dev, float* val_out_dev, void* stream);

/* The K best SEPARATED pixels per object: smg_scene_argmax_objects repeated greedily on the device, the scene-frame maps never
 * written.  Every argument of smg_scene_argmax_objects means what it means there, and geometry, validity, values, selection and
 * grouping are exactly that call's: steps 1-7 above, a value rounded to float32 once, selection by "not exactly 0" (-0.0 does not
 * select, a NaN does), the union of the two mask terms, groups that need not be contiguous, the flattened index into
 * [n_maps][hm_size][hm_size] of the whole call.
 * idx_out_dev int32 [n_groups][K], val_out_dev float32 [n_groups][K], rank-major per group:
 *   rank 0 of a group is smg_scene_argmax_objects' result for it, bit for bit;
 *   rank j >= 1 is the best pixel by smg_argmax's rules (a NaN wins, the lowest flattened index on ties) among the group's selected
 *     valid pixels that are not SUPPRESSED.  A candidate at heightmap pixel (iy, ix) - in ANY map of the group - is suppressed when
 *     for some earlier pick (py, px) of the same group (py, px = the pick's index % hm_size^2, decoded) (iy - py)^2 + (ix - px)^2
 *     <= radius^2, in integer arithmetic: a pick removes its disc in every rotation of its object.  radius = 0 removes only the
 *     picked pixel, in all the group's maps;
 *   when nothing is left, this rank and every later one are (-1, -inf).
 * Every element of both outputs is written by every successful call.  K rounds on the caller's stream, each the selected walk (a
 * pixel is tested against its group's earlier picks - read from idx_out_dev itself, no host round trip - before the geometry, so
 * a suppressed pixel costs no double-precision arithmetic) and the grouped reduce into slot [group][j]; per-workgroup partials in a
 * scratch the engine owns, no atomics: two identical calls are bit-identical, and the result equals the same greedy rule run on
 * smg_scene_maps' output with the unselected pixels set to -inf.
 * Returns -22 and launches nothing for every refusal of smg_scene_argmax_objects, for K < 1, K > 32 (kSceneTopK), radius < 0 and
 * n_groups * K beyond int32. */
int smg_scene_topk_objects(smg_engine* e, const float* q_dev, int64_t map_stride, int n_maps, const float* affine_host,
                           int hm_size, const double* masks_dev, int n_masks, const int* map_mask_a, const int* map_mask_b,
                           const int* map_group, int n_groups, int K, int radius, int* idx_out_dev, float* val_out_dev, void* stream);

/* EXPLORATION: n_draws Boltzmann draws per object - (map, pixel) drawn with probability proportional to exp(beta * Q) over the
 * object's selected valid pixels - on the device, the scene-frame maps never written.  Every argument shared with
 * smg_scene_argmax_objects means what it means there, and geometry, validity, values, selection, the union of the two mask terms,
 * groups that need not be contiguous and the flattened index into [n_maps][hm_size][hm_size] of the whole call are that call's.
 * beta = 1 / temperature: beta = 0 draws uniformly among the group's candidates, a large beta approaches the argmax.
 * The draw uses the Gumbel-max identity: argmax_i (beta v_i + G_i) with independent standard Gumbel noise G_i is a draw from
 * softmax(beta v).  The noise is a counter-based hash, so the call is a pure function of its arguments.  For a candidate with
 * flattened index i (i < 2^31), draw d >= 0 and the 64-bit seed, all integers mod 2^64:
 *     x = seed + (d << 32) + i
 *     mix(x): x += 0x9E3779B97F4A7C15; z = x
 *             z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9
 *             z = (z ^ z >> 27) * 0x94D049BB133111EB
 *             return z ^ z >> 31                         (the splitmix64 finaliser)
 *     h = mix(mix(x))
 *     u = ((h >> 12) + 0.5) * 2^-52                      (double, exact; strictly inside (0, 1), at most 1 - 2^-53)
 *     G = -log(-log(u))                                  (double; finite, in about [-3.61, 36.74])
 * and the SCORE of the candidate with map value v (the float32 smg_scene_maps stores there) is
 *     s = (float) fma(beta, (double) v, G)               (rounded to float32 once)
 * formed by one device function (scene_sample_score) wherever a kernel needs it.
 * idx_out_dev int32 [n_groups][n_draws], val_out_dev float32 [n_groups][n_draws], draw-major per group: for group g and draw d the
 * candidate with the best score among the group's selected valid pixels, by smg_argmax's rules applied to the SCORE (the lowest
 * flattened index on ties; a NaN value gives a NaN score and wins).  idx is its flattened index, val the float smg_scene_maps
 * stores there, bit for bit - the value, not the score.  A group without a map or without a candidate gets (-1, -inf) in every
 * draw; every element of both outputs is written by every successful call.  Draw d does not depend on n_draws, and the draws do
 * not depend on one another.
 * n_draws rounds on the caller's stream, each the selected walk (masks before geometry: only a selected valid pixel pays the
 * hash and the two logarithms) and the grouped reduce into slot [group][d]; the reduce recomputes the scores from (value, index),
 * so the outputs carry the running winner between launches of 32 maps and nothing beyond the engine's per-workgroup partials is
 * needed.  No atomics: two identical calls are bit-identical.
 * Returns -22 and launches nothing for every refusal of smg_scene_argmax_objects, for n_draws < 1, n_draws > 32 (kSceneDraws),
 * n_groups * n_draws beyond int32, and a beta that is negative, NaN or infinite. */
int smg_scene_sample_objects(smg_engine* e, const float* q_dev, int64_t map_stride, int n_maps, const float* affine_host,
                             int hm_size, const double* masks_dev, int n_masks, const int* map_mask_a, const int* map_mask_b,
                             const int* map_group, int n_groups, int n_draws, double beta, uint64_t seed,
                             int* idx_out_dev, float* val_out_dev, void* stream);

/* The NORMALISER of that policy: per object the log-sum-exp and the Boltzmann mean of its candidates, on the device, the
 * scene-frame maps never written.  Every argument shared with smg_scene_argmax_objects means what it means there, and geometry,
 * validity, values, selection, the union of the two mask terms and groups that need not be contiguous are that call's: the
 * CANDIDATES of group g are the selected valid pixels of its maps, each with the float32 value v smg_scene_maps stores there.
 * beta = 1 / temperature, as for smg_scene_sample_objects.
 * stats_out_dev float64 [n_groups][4], the row of group g = {count, vmax, lse, mean}:
 *     count = the number of candidates, exact
 *     vmax  = the largest candidate value M; as a float32 it is smg_scene_argmax_objects' val[g], bit for bit
 *     lse   = log sum_i exp(beta v_i) = fma(beta, M, log S)
 *     mean  = sum_i v_i exp(beta v_i) / sum_i exp(beta v_i) = T / S, the expectation of v under softmax(beta v)
 * so that log pi(i) = beta v_i - lse, the entropy is lse - beta mean, and mellowmax is (lse - log count) / beta.  A group without
 * a map or without a candidate gets (0, -inf, -inf, NaN); every element is written by every successful call.
 * The sums are kept as a streaming STATE (n, M, S, T) of a set of candidates: n = how many, M = the largest value,
 * S = sum exp(beta (v - M)) and T = sum v exp(beta (v - M)), both double; no exponent is ever positive, so nothing overflows
 * whatever beta and the offset of v.  The empty set is (0, -inf, 0, 0).
 *   ADD one candidate v to a state:
 *     the first candidate:  (1, v, 1, v)
 *     v <= M, or M a NaN:   e = exp(beta (v - M));  S += e;  T = fma(v, e, T)
 *     else (a NaN v too):   r = exp(beta (M - v));  S = fma(S, r, 1);  T = fma(T, r, v);  M = v
 *     then n += 1
 *   MERGE A (the earlier set) with B:
 *     an empty side yields the other side unchanged; else
 *     M = MA if MA > MB or MA is a NaN, else MB
 *     S = SA exp(beta (MA - M)) + SB exp(beta (MB - M)),  T likewise,  n = nA + nB      (one of the two factors is exp(0) = 1)
 * Order: a thread adds its pixels in ascending order; a fixed tree merges the 256 threads of a workgroup, whose state goes to a
 * scratch the engine owns; one workgroup per group merges that launch's slots of the group (thread t the slots t, t + 256, ...,
 * then the same tree).  Maps are launched 32 at a time: from the second launch on the reduce starts from the raw state the
 * earlier launches left in the group's row of stats_out_dev, and one last launch (one thread per group) turns the rows into
 * {count, vmax, lse, mean} in place.  No atomics: two identical calls are bit-identical.  Against float64 log-sum-exp over the
 * same float32 values the result differs by rounding only (tests/scene_softmax_ref.py derives the bound).
 * A NaN candidate is counted and makes vmax, lse and mean of its group NaN (a NaN wins, as for the argmax); other groups are
 * untouched.  Infinite values are outside the contract: the call does not fault and count stays exact.
 * Returns -22 and launches nothing for every refusal of smg_scene_argmax_objects (its outputs replaced by stats_out_dev), for a
 * beta that is negative, NaN or infinite, and for a stats_out_dev that is not 8-byte aligned. */
int smg_scene_softmax_objects(smg_engine* e, const float* q_dev, int64_t map_stride, int n_maps, const float* affine_host,
                              int hm_size, const double* masks_dev, int n_masks, const int* map_mask_a, const int* map_mask_b,
                              const int* map_group, int n_groups, double beta, double* stats_out_dev, void* stream);

/* The COLLAPSED map - the picture between "all the maps" and "one pick": per group of maps and heightmap pixel the best value over
 * the group's maps and which map gives it, the scene-frame maps never written.  q_dev, map_stride, n_maps, affine_host, hm_size,
 * masks_dev, n_masks, map_mask_a, map_mask_b, map_group and n_groups mean what they mean for smg_scene_argmax_objects (selection by
 * "not exactly 0": -0.0 does not select, a NaN does; the union of the two terms; both terms -1 = every pixel; groups that need not
 * be contiguous), with one addition: masks_dev == NULL with n_masks == 0 is allowed - every term must then be -1.  That is the sweep
 * form (one group, the R rotations of forward_dense), which has no masks tensor.
 * val_out_dev float32 [n_groups][hm_size][hm_size], arg_out_dev int32 [n_groups][hm_size][hm_size].  For group g and pixel i the
 * CANDIDATES are the maps m of the call with map_group[m] == g whose mask terms select i and in whose rotation i is valid (step 6):
 *   val[g][i] = the float smg_scene_maps stores at (m, i) for the best candidate - the same expression, so bit for bit equal;
 *   arg[g][i] = that m, an index into the call's maps (a caller turns it into a rotation with a table lookup);
 *   "best" by smg_argmax's rules with m as the index: the lowest m on ties, the first NaN wins - np.argmax over the group's maps
 *     in call order;
 *   with no candidate the pair is (-inf, -1).
 * Every element of both outputs is written by every successful call; a group without a map is (-inf, -1) everywhere.  Against
 * smg_scene_argmax_objects: the maximum of val[g] is that call's value for group g, bit for bit; where the maximum is attained
 * more than once the two calls may name different (map, pixel): the argmax orders by the flattened [m][pixel] index, this map is
 * read lowest pixel first, then lowest map.
 * One workgroup owns a tile of pixels of one group and visits the group's maps in ascending m, one map staged at a time; the masks
 * are read before the geometry, so an unselected pixel costs no double-precision arithmetic.  Maps are launched 32 at a time; a
 * launch after the first reads the outputs back as the running best, and leaves alone the groups it holds no map of.  No atomics,
 * no scratch of the engine: two identical calls are bit-identical.  16-byte stores per output when hm_size^2 is a multiple of 4
 * and that output is 16-byte aligned, else 4-byte ones.
 * Returns -22 and launches nothing for a NULL pointer (masks_dev aside), head_out != 1, n_maps < 1, a negative map_stride,
 * n_masks < 0, masks_dev NULL with n_masks > 0 or not NULL with n_masks == 0, a mask index outside [-1, n_masks), n_groups < 1, a
 * group outside [0, n_groups), n_groups * hm_size^2 beyond int32, and the geometry refusals above (hm_size, a 1 x 1 map, an affine
 * with a translation). */
int smg_scene_best_maps(smg_engine* e, const float* q_dev, int64_t map_stride, int n_maps, const float* affine_host, int hm_size,
                        const double* masks_dev, int n_masks, const int* map_mask_a, const int* map_mask_b, const int* map_group,
                        int n_groups, float* val_out_dev, int* arg_out_dev, void* stream);

/* Huber loss on K labelled heightmap pixels per pair, one-channel heads only (head_out != 1 returns -22): q and dq are
 * [n_pairs][1][OH][OW]; pixels_dev int32 [n_pairs][K][2] = (iy, ix); label_dev, weight_dev float32 [n_pairs][K] (weight_dev NULL =
 * all ones, a weight of exactly 0 masks its point).  With v_k the interpolated value of point k in its pair's rotation (double,
 * not rounded) and the Huber of code/trainer.py:345-348:
 *     loss[j] = sum_k w_k huber(v_k - label_k)
 *     dq[j][oy][ox] = sum_k w_k huber'(v_k - label_k) * (bilinear weight of (oy, ox) at point k)
 * accumulated in double in point order and rounded once; every element of dq is written, duplicate points add up, no atomics
 * (bit-identical between identical calls).  A point that is invalid in its pair's rotation contributes nothing (a caller refuses
 * it first).  Marks the saved forward "dense dq" exactly as smg_loss_map does. */
int smg_loss_scene(smg_engine* e, const float* q_dev, const float* affine_host, int hm_size, int n_pairs, int K,
                   const int* pixels_dev, const float* label_dev, const float* weight_dev,
                   float* loss_dev, float* dq_dev, void* stream);

/* smg_loss_scene with a whole label IMAGE per pair instead of K listed pixels, one-channel heads only (head_out != 1 returns -22):
 * q and dq are [n_pairs][1][OH][OW]; label_dev, weight_dev float32 [n_pairs][hm_size][hm_size] (weight_dev NULL = all ones).
 * Every heightmap pixel that is valid in its pair's rotation (step 6) and whose weight is not exactly 0 is a point, with v the
 * interpolated value there (double, not rounded) and smg_loss_scene's Huber:
 *     loss[j]       = sum over those pixels of w * huber(v - label)
 *     dq[j][oy][ox] = sum over those pixels of w * huber'(v - label) * (bilinear weight of (oy, ox) at that pixel)
 * A pixel that is invalid in the pair's rotation contributes nothing and is no error (a whole image always covers such pixels); a
 * weight of exactly 0 masks its pixel; the label of a masked or invalid pixel is never read into the arithmetic (a NaN there is
 * harmless), nor is the weight of an invalid pixel.  Like smg_loss_scene the call takes any 2x2 part (the box of an element is
 * found with the inverse of A^T; a matrix without a usable inverse makes every workgroup walk the whole heightmap: slow, same result).
 * Parallel over the map, not serial in the pixels: one workgroup per (pair, map
 * element) gathers the pixels of the heightmap box around that element in a fixed order and reduces by a fixed tree; the loss is
 * summed per element (each pixel counted at its corner element (y0, x0)) into a scratch the engine owns and reduced by a second
 * launch in fixed order.  Accumulated in double, rounded to float32 once, every element of dq written once (zeros included), no
 * atomics: identical calls are bit-identical, and a pair's result does not depend on the other pairs of the call.
 * Returns -22 and launches nothing for head_out != 1, the geometry refusals above, n_pairs < 1 and an affine with a translation.
 * Marks the saved forward "dense dq" exactly as smg_loss_scene does. */
int smg_loss_scene_map(smg_engine* e, const float* q_dev, const float* affine_host, int hm_size, int n_pairs,
                       const float* label_dev, const float* weight_dev, float* loss_dev, float* dq_dev, void* stream);

/* TRAINING the Boltzmann policy of smg_scene_sample_objects: per group of pairs the negative log-likelihood of an executed action
 * and the entropy of the policy, with their gradient on the maps.  One-channel heads only (head_out != 1 returns -22): q and dq are
 * [n_pairs][1][OH][OW].  masks_dev, n_masks, pair_mask_a, pair_mask_b, pair_group and n_groups mean what they mean for
 * smg_scene_argmax_objects, a "map" there being a pair here: selection by "not exactly 0" (-0.0 does not select, a NaN does), the
 * union of the two terms, both terms -1 = every pixel, groups that need not be contiguous, the same geometry and validity.  The
 * CANDIDATES of group g are the selected valid pixels of its pairs, each with the float32 v_i smg_scene_maps stores there, and
 * pi_i = exp(beta v_i - lse_g), beta = 1 / temperature.
 * action_dev int32 [n_groups]: the executed action of the group as a flattened index into [n_pairs][hm_size][hm_size], -1 = none.
 * weight_dev float64 [n_groups][2] = {w_nll, w_ent}; w_nll may be negative (an advantage).  Both are device pointers: the call
 * stays asynchronous.  With lse and mean of smg_scene_softmax_objects:
 *     H_g    = lse_g - beta mean_g                                    (the entropy of pi)
 *     loss_g = w_nll (lse_g - beta v_act) - w_ent H_g
 *     dloss_g/dv_i = pi_i (A + B (v_i - mean_g)) + C [i == act_g],    A = w_nll beta,  B = w_ent beta^2,  C = -w_nll beta
 *     dq[j][oy][ox] = sum over the candidates i of pair j of dloss/dv_i * (bilinear weight of (oy, ox) at pixel i)
 * The float32 rounding of v_i is treated as the identity in the gradient, so with w_nll = 1, w_ent = 0 the loss is the very number
 * the sampled forms report as -logp = -(beta v - lse).  With act_g == -1 the w_nll term and C are absent, and w_nll is ignored
 * whatever it holds (a NaN included).
 * Outputs: stats_out_dev float64 [n_groups][4] receives, bit for bit, what smg_scene_softmax_objects writes for the same arguments;
 * loss_dev float32 [n_groups]; dq_dev [n_pairs][1][OH][OW], every element written by every successful call.
 *   A group without a candidate: stats (0, -inf, -inf, NaN), loss 0 if act == -1 (else NaN), its pairs' dq exactly 0.
 *   An action that is not a candidate of its group - out of range, in a pair of another group, not selected, without a window -
 *     makes loss[g] NaN; the pi and entropy parts of that group's dq are still written.  No address is ever formed from the action
 *     (it is only compared with the indices of the pixels that are walked); a caller refuses such actions first.
 *   A NaN candidate makes its group's loss NaN and every element of its pairs' dq NaN; other groups are untouched, bit for bit.
 * Three phases on the caller's stream.  (1) The normaliser: smg_scene_softmax_objects' launches, unchanged, over all launches of
 * 32 pairs - every group's lse and mean are final before the gradient starts, so a group split by the 32-pair boundary needs no
 * care.  (2) The gather: one workgroup per (pair, map element), as smg_loss_scene_map; the masks are tested at the pixel, then
 * v = the very expression the walks store, pi = exp(fma(beta, v, -lse)); the element's sum is accumulated in double, reduced by a
 * fixed tree, rounded to float32 once and written once, zeros included.  The one thread that meets the action at its home element
 * (the corner (y0, x0) of its pixel) writes v_act: flattened indices are unique and a pixel has one home, so there is one writer.
 * (3) One thread per group forms loss_g in double and rounds once.  No atomics, no scratch of the engine beyond the normaliser's:
 * identical calls are bit-identical, and a pair's dq does not depend on which launch carries it.
 * Returns -22 and launches nothing for every refusal of smg_scene_argmax_objects (n_maps read as n_pairs), head_out != 1, a NULL
 * pointer, a beta that is negative, NaN or infinite, and a stats_out_dev or weight_dev that is not 8-byte aligned.
 * Marks the saved forward "dense dq" exactly as smg_loss_scene does. */
int smg_loss_scene_policy(smg_engine* e, const float* q_dev, const float* affine_host, int hm_size, int n_pairs,
                          const double* masks_dev, int n_masks, const int* pair_mask_a, const int* pair_mask_b,
                          const int* pair_group, int n_groups, double beta,
                          const int* action_dev,      /* int32 [n_groups], -1 = no action */
                          const double* weight_dev,   /* float64 [n_groups][2] = {w_nll, w_ent} */
                          double* stats_out_dev,      /* float64 [n_groups][4] = smg_scene_softmax_objects' row */
                          float* loss_dev,            /* float32 [n_groups] */
                          float* dq_dev,              /* [n_pairs][1][OH][OW], every element written */
                          void* stream);

/* ---- the reactive net's class maps in the scene frame --------------------------------------------------------------------------
 * The same services for a 3-class head (head_out != 3 returns -22 and launches nothing): q_dev is [n_maps][3][OH][OW], the
 * head output.  The geometry is steps 1-7 above, unchanged.  At a heightmap pixel that is valid in a map's rotation, in double:
 *     z_c = the bilinear interpolation of LOGIT plane c there (c = 0, 1, 2: the same corners and fractions for all three)
 *     P_c = exp(z_c - m) / sum_c' exp(z_c' - m),  m = max_c z_c,  rounded to float32 once.
 * The logits are interpolated and the softmax is taken at the scene pixel; probabilities are not interpolated.  The training loss
 * below is the cross entropy of those same interpolated logits, whose gradient is (softmax - onehot) x the four bilinear weights
 * (the dense-map form), so picking and training see one and the same function of the head output.  Nothing is special-cased: a
 * NaN, or an inf that produces inf - inf, in any of the twelve corner logits makes all three probabilities NaN, as torch.softmax
 * does in fp64.  An invalid pixel is -inf in every plane, so the argmax rules carry over unchanged.
 * All of them return -22 and launch nothing for the geometry refusals above, for n_maps < 1 / K < 1 / n_pairs < 1 and for cls out of range. */

/* out_dev float32: cls in {0,1,2} -> [n_maps][hm][hm] = P(class cls); cls == -1 -> [n_maps][3][hm][hm], all three.
 * q_dev is [n_maps][3][OH][OW] (the head output of a 3-class engine). */
int smg_scene_class_maps(smg_engine* e, const float* q_dev, int n_maps, const float* affine_host, int hm_size,
                         int cls, float* out_dev, void* stream);

/* smg_scene_values for the 3-class head: the class probabilities at K listed heightmap pixels per map, without writing the maps.
 * q_dev is [n_maps][3][OH][OW]; pixels_dev int32 [n_maps][K][2] = (iy, ix) as for smg_scene_values.  out_dev float32: cls in
 * {0,1,2} -> [n_maps][K] = P(class cls); cls == -1 -> [n_maps][3][K], all three.  Each value is the float smg_scene_class_maps
 * stores at that pixel, bit for bit (a NaN in any of the twelve corner logits makes it NaN); a point outside the heightmap or
 * invalid in the map's rotation is -inf in every plane.  Every element of out is written, no atomics, no scratch of the engine.
 * Returns -22 and launches nothing for a NULL pointer, head_out != 3, n_maps < 1, cls outside {-1,0,1,2}, K < 1, n_maps * K beyond
 * int32 and the geometry refusals above. */
int smg_scene_class_values(smg_engine* e, const float* q_dev, int n_maps, const float* affine_host, int hm_size, int cls,
                           int K, const int* pixels_dev, float* out_dev, void* stream);

/* Largest valid P(class cls), cls in {0,1,2}, and its flattened index into [n_maps][hm][hm], without writing the maps:
 * idx_out_dev int32[1], val_out_dev float32[1], smg_scene_argmax's rules and bit-reproducibility.  The value comes from the
 * expression smg_scene_class_maps stores: the result equals smg_argmax over plane cls of its output, bit for bit.  Index -1,
 * value -inf when no pixel is valid. */
int smg_scene_class_argmax(smg_engine* e, const float* q_dev, int n_maps, const float* affine_host, int hm_size,
                           int cls, int* idx_out_dev, float* val_out_dev, void* stream);

/* smg_scene_class_argmax per OBJECT - smg_scene_argmax_objects for the 3-class head: every map restricted to the heightmap pixels
 * its masks select, one result per group of maps, the value P(class cls) of the interpolated logits, cls in {0,1,2}; neither the
 * scene-frame maps nor the masked copies are written.  q_dev is [n_maps][3][OH][OW].  masks_dev, n_masks, map_mask_a, map_mask_b,
 * map_group, n_groups, idx_out_dev int32[n_groups] and val_out_dev float32[n_groups] mean what they mean for
 * smg_scene_argmax_objects, word for word: selection by "not exactly 0" on the float64 masks tensor of the forward (-0.0 does not
 * select, a NaN does), the union of the two terms, groups that need not be contiguous, every group's pair written, index -1 / value
 * -inf for a group with no map or no selected valid pixel, the flattened index into [n_maps][hm][hm] of the whole call, smg_argmax's
 * tie and NaN rules (a NaN in any corner logit of any plane makes the pixel's value NaN, and it wins its group).  The masks are
 * read before the geometry: an unselected pixel costs no double-precision arithmetic and no exponential.  No atomics: two identical
 * calls are bit-identical, the value comes from the expression smg_scene_class_maps stores, and a group's result equals smg_argmax
 * over plane cls of smg_scene_class_maps' output with the unselected pixels set to -inf, bit for bit.
 * Returns -22 and launches nothing for a NULL pointer, head_out != 3, cls outside {0,1,2}, n_maps < 1, n_masks < 1, n_groups < 1,
 * a mask index outside [-1, n_masks), a group outside [0, n_groups), a flattened index that does not fit int32, and the geometry
 * refusals above (hm_size, a 1 x 1 map, an affine with a translation). */
int smg_scene_class_argmax_objects(smg_engine* e, const float* q_dev, int n_maps, const float* affine_host, int hm_size, int cls,
                                   const double* masks_dev, int n_masks, const int* map_mask_a, const int* map_mask_b,
                                   const int* map_group, int n_groups, int* idx_out_dev, float* val_out_dev, void* stream);

/* smg_scene_topk_objects for the 3-class head - the K best separated pixels per object by P(class cls), cls in {0,1,2}: the
 * arguments of smg_scene_class_argmax_objects plus K and radius, idx_out_dev int32 [n_groups][K], val_out_dev float32 [n_groups][K].
 * The value of a pixel is scene_class_prob(c, cls), the expression smg_scene_class_maps stores; rank 0 of a group is
 * smg_scene_class_argmax_objects' result, bit for bit; ranks j >= 1, suppression (in heightmap pixels, across all the group's maps),
 * exhaustion (-1, -inf), "every element written", "no atomics, bit-identical between identical calls" are smg_scene_topk_objects',
 * word for word, and the result equals that greedy rule run on plane cls of smg_scene_class_maps' output with the unselected pixels
 * set to -inf.  A suppressed or unselected pixel costs no exponential.
 * Returns -22 and launches nothing for every refusal of smg_scene_class_argmax_objects, for K < 1, K > 32, radius < 0 and
 * n_groups * K beyond int32. */
int smg_scene_class_topk_objects(smg_engine* e, const float* q_dev, int n_maps, const float* affine_host, int hm_size, int cls,
                                 const double* masks_dev, int n_masks, const int* map_mask_a, const int* map_mask_b,
                                 const int* map_group, int n_groups, int K, int radius, int* idx_out_dev, float* val_out_dev,
                                 void* stream);

/* smg_scene_sample_objects for the 3-class head - n_draws Boltzmann draws per object by P(class cls), cls in {0,1,2}: the arguments
 * of smg_scene_class_argmax_objects plus n_draws, beta and seed, idx_out_dev int32 [n_groups][n_draws], val_out_dev float32
 * [n_groups][n_draws].  The value v of a candidate is scene_class_prob(c, cls), the expression smg_scene_class_maps stores; the
 * noise, the score, the rules, (-1, -inf), "every element written", "draw d does not depend on n_draws" and "no atomics,
 * bit-identical between identical calls" are smg_scene_sample_objects', word for word.  An unselected pixel costs no exponential.
 * Returns -22 and launches nothing for every refusal of smg_scene_class_argmax_objects, for n_draws < 1, n_draws > 32,
 * n_groups * n_draws beyond int32, and a beta that is negative, NaN or infinite. */
int smg_scene_class_sample_objects(smg_engine* e, const float* q_dev, int n_maps, const float* affine_host, int hm_size, int cls,
                                   const double* masks_dev, int n_masks, const int* map_mask_a, const int* map_mask_b,
                                   const int* map_group, int n_groups, int n_draws, double beta, uint64_t seed,
                                   int* idx_out_dev, float* val_out_dev, void* stream);

/* smg_scene_softmax_objects for the 3-class head - {count, vmax, lse, mean} per object of the policy proportional to
 * exp(beta P(class cls)), cls in {0,1,2}: the arguments of smg_scene_class_argmax_objects plus beta, stats_out_dev float64
 * [n_groups][4].  The value v of a candidate is scene_class_prob(c, cls), the expression smg_scene_class_maps stores; vmax as a
 * float32 is smg_scene_class_argmax_objects' val, bit for bit; the state, its update and merge, the order, the empty row, the
 * NaN rule, "every element written" and "no atomics, bit-identical between identical calls" are smg_scene_softmax_objects', word
 * for word.  An unselected pixel costs no exponential.
 * Returns -22 and launches nothing for every refusal of smg_scene_class_argmax_objects (its outputs replaced by stats_out_dev),
 * for a beta that is negative, NaN or infinite, and for a stats_out_dev that is not 8-byte aligned. */
int smg_scene_class_softmax_objects(smg_engine* e, const float* q_dev, int n_maps, const float* affine_host, int hm_size, int cls,
                                    const double* masks_dev, int n_masks, const int* map_mask_a, const int* map_mask_b,
                                    const int* map_group, int n_groups, double beta, double* stats_out_dev, void* stream);

/* smg_scene_best_maps for the 3-class head - per group and heightmap pixel the largest P(class cls), cls in {0,1,2}, over the
 * group's maps and the map that gives it: q_dev is [n_maps][3][OH][OW], every other argument, the candidates, the tie and NaN
 * rules, the empty pair (-inf, -1), "every element written", the carry between launches and "no atomics, bit-identical between
 * identical calls" are smg_scene_best_maps', word for word.  val[g][i] is the float smg_scene_class_maps(cls) stores at (m, i) for
 * the best candidate - scene_class_prob of the interpolated logits, the same expression, bit for bit (a NaN in any of the twelve
 * corner logits makes it NaN, and the first such map wins the pixel).  An unselected pixel costs no exponential.
 * Returns -22 and launches nothing for every refusal of smg_scene_best_maps with head_out != 3 in place of head_out != 1 and no
 * map_stride, and for cls outside {0,1,2}. */
int smg_scene_class_best_maps(smg_engine* e, const float* q_dev, int n_maps, const float* affine_host, int hm_size, int cls,
                              const double* masks_dev, int n_masks, const int* map_mask_a, const int* map_mask_b, const int* map_group,
                              int n_groups, float* val_out_dev, int* arg_out_dev, void* stream);

/* Cross entropy (CrossEntropyLoss2d, class weights {1,1,0}) on K labelled heightmap pixels per pair: q and dq are
 * [n_pairs][3][OH][OW]; pixels_dev int32 [n_pairs][K][2] = (iy, ix); label_dev float32 [n_pairs][K] class indices as in
 * smg_loss_map_ce (0 and 1 carry weight 1, anything else is class 2, "no loss").  W_j = the number of points of pair j whose class
 * is 0 or 1, which lie inside the heightmap and which are valid in the pair's rotation; every other point contributes nothing, is
 * not counted, and the logits under it are not read.  With z_k the three interpolated logits of point k (double, not rounded):
 *     nll_k   = logsumexp(z_k) - z_k[y_k]
 *     loss[j] = (sum_k nll_k) / W_j      (0 when W_j == 0, not 0/0)
 *     dq[j][c][oy][ox] = (1 / W_j) sum_k (softmax(z_k)[c] - [c == y_k]) * (bilinear weight of (oy, ox) at point k)
 * summed unnormalised in double in point order, divided by W_j once and rounded once; every element of dq is written, duplicate
 * points add up, no atomics (bit-identical between identical calls).  Also -22 when 24 OH OW bytes of accumulators exceed 48 KB
 * of LDS (maps beyond 45 x 45).  Marks the saved forward "dense dq" exactly as smg_loss_map_ce does. */
int smg_loss_scene_ce(smg_engine* e, const float* q_dev, const float* affine_host, int hm_size, int n_pairs, int K,
                      const int* pixels_dev, const float* label_dev, float* loss_dev, float* dq_dev, void* stream);

/* smg_loss_scene_ce with a whole class-label IMAGE per pair instead of K listed pixels: q and dq are [n_pairs][3][OH][OW];
 * label_dev float32 [n_pairs][hm_size][hm_size], class indices as in smg_loss_map_ce.  A heightmap pixel is a point of pair j when
 * it is valid in the pair's rotation (step 6) and its label is exactly 0 or 1; W_j = the number of points.  Every other pixel -
 * class 2, NaN, any other value - is "no loss": skipped before a logit is read, whatever the logits under it hold.  A pixel that
 * is invalid in the pair's rotation contributes nothing and is no error (a whole image always covers such pixels), and its label
 * is never read into the arithmetic.  With z the three interpolated logits of a point (double, not rounded), m = max z,
 * e_c = exp(z_c - m), s = e_0 + e_1 + e_2:
 *     nll     = (log(s) + m) - z_y
 *     loss[j] = (sum over the points of nll) / W_j      (0 when W_j == 0, not 0/0)
 *     dq[j][c][oy][ox] = (1 / W_j) sum over the points of (e_c / s - [c == y]) * (bilinear weight of (oy, ox) at the pixel)
 * summed unnormalised in double, divided by W_j once and rounded to float32 once; W_j == 0 gives dq exactly 0 everywhere.
 * Parallel over the map like smg_loss_scene_map, whose walk it shares: one workgroup per (pair, map element) gathers the pixels of
 * the heightmap box around that element in a fixed order (any 2x2 part; a matrix without a usable inverse walks the whole
 * heightmap) and reduces by a fixed tree; a pixel's nll and count go to its corner element (y0, x0) alone, its gradient share to
 * every element it touches.  The unnormalised per-element partials (three gradient sums, the loss sum, the count) go to a scratch
 * the engine owns; a second launch sums loss and count per pair in fixed order and writes loss and all of dq, every element once
 * (zeros included).  No atomics: identical calls are bit-identical, and a pair's result does not depend on the other pairs of the
 * call.  No accumulator of the map's size in LDS, so smg_loss_scene_ce's 45 x 45 limit does not apply.
 * Returns -22 and launches nothing for head_out != 3, the geometry refusals above, n_pairs < 1, n_pairs beyond the engine's
 * max_pairs and an affine with a translation.  Marks the saved forward "dense dq" exactly as smg_loss_scene_ce does. */
int smg_loss_scene_map_ce(smg_engine* e, const float* q_dev, const float* affine_host, int hm_size, int n_pairs,
                          const float* label_dev, float* loss_dev, float* dq_dev, void* stream);

/* Backward of the last smg_forward: accumulates (+=) d(sum of losses)/d(param) into
 * net->grads for the trunk and head that forward used.  Replaces loss.backward() at
 * code/trainer.py:350-351. */
int smg_backward(smg_engine* e, const smg_net* net, const float* dq_dev, void* stream);

/* The same backward in two halves, for a data-parallel caller that hides its gradient all-reduce under compute:
 * phase 0 runs the head and dense blocks 4, 3, 2; when it returns (in stream order) every gradient of the parameters from
 * smg_layout_trunk_split() to the end of the trunk range, and of the head range, is final - their all-reduce can start while
 * phase 1 (dense block 1, pool0, the stem: about a third of the backward) computes the rest, [trunk begin, split).
 * smg_backward == phase 0 followed by phase 1.
 * Phase 1 never reads or writes a gradient element of [split, trunk end) or of the head range (they may be in an in-place
 * all-reduce on another stream).  The order is enforced: phase 1 without phase 0 of the SAME forward, phase 0 twice, or
 * smg_backward between the two halves return -22 and launch nothing. */
int smg_backward_phase(smg_engine* e, const smg_net* net, const float* dq_dev, void* stream, int phase);
/* Element offset (params / grads) of the first parameter behind dense block 1 of trunk `trunk_id` (transition1.norm.weight). */
int smg_layout_trunk_split(int head_out, int trunk_id, int64_t* offset);

/* Precision mode of the engine (the reference runs apex O0 = fp32, code/trainer.py:101; modes 1 and 2 are BASELINE.json configs 3
 * and 5):
 *   0  (default) fp32 storage; fp32-class accuracy, what the parity suite gates: the dense layers' products as a scaled
 *      two-piece fp16 split per operand, three MFMA terms (scales per weight tensor, per BatchNorm operand and per gradient
 *      tensor and stream, maintained by the engine); the stem's, the transitions' and the head's gradient products as three
 *      bf16 pieces, six terms;
 *   1  bf16 STORAGE of activations and gradients (dense-block buffers, bottlenecks, G', the backward ring), one bf16 MFMA term
 *      per product;
 *   2  fp16 storage of activations with fp16 forward products; gradients stored and multiplied in bf16 (fp32 exponent range:
 *      no loss scaling).
 * In every mode parameters, their gradients, Adam, BN statistics, every accumulation, the input image, the stem plane and the
 * head's feature buffers stay fp32.  Takes effect with the next smg_forward (a saved forward of another mode is dropped).
 * A CHANGE of mode waits for the device and zeroes the mode-typed buffers: their padding rows are read as they lie and must not
 * hold the other storage type's words. */
int smg_engine_set_precision(smg_engine* e, int precision);

/* Engine switches by name.  "deterministic" (0 / 1): the 1x1-convolution weight gradients (conv1 of every dense layer,
 * the largest gradient tensors) are reduced from partial tiles in a fixed order instead of fp32 atomics, so the trunk's
 * convolution weight gradients of two identical calls are bit-identical like the reference's (code/trainer.py:350-351 on one
 * device); BatchNorm affine gradients and the head's value convolution (in its per-element form, see "head_bwd") keep their fp32 atomics.  (Since round 3 the fixed-order
 * path is also the default for batches of more than four streams whenever the partial tiles fit the workspace - it is the
 * faster one there; the option guarantees it for every batch: a launch whose partial tiles do not fit the workspace fails
 * with -12 instead of falling back to atomics.)
 * "head_bwd" (0 / 1 / 2): the form of the head's value-convolution backward.  1: the per-element form - every feature pixel walks the
 * output elements it feeds, skips zero dq and adds its share of the 20x20 weight gradient with fp32 atomics; right for the single
 * element smg_loss mode 0 sets.  2: the dense form - a data pass over the 400 taps and a weight pass that owns every element of
 * the weight gradient (no atomics, pairs in index order: bit-identical between identical calls); right for a whole map.
 * 0 (default): the dense form after smg_loss_map / smg_loss_map_ce / smg_loss_scene / smg_loss_scene_map / smg_loss_scene_ce / smg_loss_scene_map_ce, else the per-element form.  A 3-class head follows the same
 * rule as a one-channel head (its dense form loops over the three output channels).  smg_train_step_graph always runs the
 * per-element form (its loss is smg_loss).
 * "serialize" (0 / 1): every kernel on the caller's stream in issue order instead of two concurrent chains (profiling).
 * "debug_stop" (tests only; -1 = off): the next smg_backward returns behind the launches of dense layer (block, layer) =
 * (value / 100, value % 100), 0-based - or, with value % 100 == 50, in front of that block's first layer - with both streams
 * joined, so that smg_debug_read sees the ring slots, "dy2" and G' as that layer left them.  The forward's saved state is
 * consumed (run a new smg_forward before the next backward). */
int smg_engine_set_option(smg_engine* e, const char* name, int value);

/* Heightmap generation in front of the path (utils.get_heightmap, code/utils.py:38-68): the robot-frame height of every
 * camera pixel (get_pointcloud + cam_pose, :12-47) warped onto the table plane (cv2.warpPerspective, INTER_LINEAR,
 * constant 0 border, :62-66).  depth_img_dev float64 [h][w]; intrinsics row-major 3x3, cam_pose row-major 4x4 and the
 * INVERSE of cv2.getPerspectiveTransform(src, dst) row-major 3x3 in host memory; out_dev float64 [out_h][out_w]. */
int smg_heightmap(const double* depth_img_dev, int h, int w, const double* intrinsics3x3, const double* cam_pose4x4,
                  const double* inv_homography3x3, int out_w, int out_h, double* out_dev, void* stream);

/* Index and value of the largest of n float32 values (lowest index on ties, like np.argmax at
 * code/main.py:172-173,195), on the device: idx_out_dev int32[1], val_out_dev float32[1]. */
int smg_argmax(const float* values_dev, int n, int* idx_out_dev, float* val_out_dev, void* stream);

/* Adam over [offset, offset+count) of params/grads with moments m, v (same layout),
 * replacing torch.optim.Adam.step (code/trainer.py:99,383): lr 1e-4, betas
 * (0.9,0.999), eps 1e-8, no weight decay; `step` is the 1-based step count of this
 * segment. */
int smg_adam_step(float* params, const float* grads, float* m, float* v, int64_t offset, int64_t count,
                  int step, float lr, float beta1, float beta2, float eps, void* stream);

/* One training step - zero the (trunk, head) gradient ranges, smg_forward, smg_loss, smg_backward, Adam on both ranges - as ONE
 * replayable hipGraph: the reference's real call pattern is one (mask, rotation) sample per Trainer.backprop (code/main.py:338,
 * code/trainer.py:334-384), ~560 launches of 2-20 us, which an eager host enqueues no faster than the GPU runs them.  The first
 * call with a given set of pointers / shapes runs eagerly, the second is captured (stream capture across the engine's two
 * streams), later ones replay; what changes between steps without re-capture: the CONTENTS of the input images, masks and labels,
 * the batch description arrays of `batch` (rotations, pairings: same counts), and the Adam step counts.  Anything else
 * (pointers, counts, precision mode, options) re-captures.  Results are bit-identical to the four separate calls with
 * smg_adam_step(step) on the two ranges.  Asynchronous on `stream` like the calls it replaces. */
typedef struct {
    float* m; float* v;               /* Adam moments, flat, laid out like params */
    float lr, beta1, beta2, eps;
    int step_trunk, step_head;        /* 1-based step count of the trunk range / the head range for THIS step */
} smg_adam;
int smg_train_step_graph(smg_engine* e, const smg_net* net, int trunk_id, int head_id, const smg_batch* batch, int loss_mode,
                         const float* labels_dev, float* q_out_dev, float* loss_out_dev, float* dq_dev, const smg_adam* adam, void* stream);

/* Element range of params/grads used by (trunk_id) features or (head_id) head. */
int smg_layout_trunk_range(int head_out, int trunk_id, int64_t* offset, int64_t* count);
int smg_layout_head_range(int head_out, int head_id, int64_t* offset, int64_t* count);

/* ---- debug / test access (used by tests/ only) ------------------------------------ */
/* Copies an internal buffer to host as float32 (16-bit storage is widened).  name: "img", "stem", "x1".."x4",
 * "feat", "g1".."g4", "bt<block>_<layer>", "asc" ...; "fs_bt<block>_<layer>" / "fs_x<block>": the forward's fp64 sums of a
 * bottleneck / of a block buffer as raw doubles, [sum | sumsq][streams][128 | Ctot of the block] (the backward sums into another
 * arena: they are intact at a debug_stop); "bs_x<block>": the BACKWARD's fp64 sums s1 | s2 of a block buffer, [s1 | s2][streams][Ctot],
 * its replicas added up - behind a debug_stop the columns [cin, cin + 32) of the stopped layer hold what its GS was formed from.
 * Behind a debug_stop backward, in every precision mode:
 *   "gsnap"  G' of the stopped layer's block in front of that layer's 1x1 data gradients, in the mode's gradient storage;
 *   "dy2"    the raw 3x3 data gradient of the stopped layer, [streams][HWp of its block][128]: mode 0 reads the DY2 buffer (the
 *            layer the backward processed last, [streams][HWp of block 1][128] allocated); in modes 1 / 2 it lives in the layer's
 *            ring slot, which the norm2 backward overwrites in place - the stop copies the slot between the two kernels;
 *   "gs_<block>_<layer>" / "d2_<block>_<layer>"  that layer's ring slot: its finished output-slice gradient [streams][HWp][32] /
 *            bottleneck gradient [streams][HWp][128].  Mode 0: d2 rebuilt from its fp16 units and block scales - exactly the
 *            operand the consumers' MFMAs see.  Modes 1 / 2: plain bf16.  There gs_ holds the layer's gradient only where the
 *            walk MATERIALISED it - calls of more than 4 streams; with fewer the 3x3 kernels apply the BN backward on load and the
 *            slot keeps an earlier layer's words.  Rows [HW, HWp) of a slot are not written by the 16-bit kernels in either form.
 * A snapshot taken in one precision mode is refused (-22) in another.  Block / layer are 1-based.
 * Returns the element count or a negative error. */
int64_t smg_debug_read(smg_engine* e, const char* name, float* host_out, int64_t cap, void* stream);
/* Geometry of the engine: fills H (per block spatial size), HWp (padded rows). */
int smg_engine_geometry(const smg_engine* e, int H[6], int HWp[6]);
/* Per-kernel-class timing, measured with hipEvents recorded on the launch stream
 * around every launch while profiling is enabled (bench.py's roofline leg).
 * kind in [0, smg_profile_kinds()): the MFMA convolution classes, last = everything
 * else.  smg_profile_read drains pending events (synchronises) and returns the
 * accumulated milliseconds, launch count and executed FLOPs (2*M*N*K over valid
 * pixels) of one class since smg_profile_enable.  kind + smg_profile_kinds()*(1+b),
 * b in 0..3, reads the share of that class issued inside dense block b's layer loops. */
int smg_profile_enable(smg_engine* e, int on);
int smg_profile_kinds(void);
const char* smg_profile_kind_name(int kind);
int smg_profile_read(smg_engine* e, int kind, double* ms, int64_t* launches, double* flops);
/* Algorithmic HBM bytes of the same class (every operand read once, every result written once, fp32) - the
 * numerator of bench.py's HBM roofline.  Valid after smg_profile_read of that class. */
int smg_profile_read_bytes(smg_engine* e, int kind, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* SMG_HIP_H */
