// wgrad_plan.h - host-only planning of the backward's weight-gradient launches: how a launch is cut into tiles and pixel chunks, and
// who owns which range of the partial-tile workspace when (PartialTiles).  No HIP header and no HIP type: everything here is plain
// arithmetic, and a host program exercises it without a GPU.  The plain structs the kernels share with it (Plane, ReduceArgs, the
// column maps) live here and reach the kernels through gemm.cuh.
#pragma once
#include <cstdint>
#include <string>

#include "plan.h"

namespace smg {

struct Plane { int H, W, HW, HWp; };

enum { C_IDENT = 0, C_3x3 = 1, C_STEM = 2, C_STEM1 = 3 };                  // C_STEM1: column = tap, written to all three input channels

// Sum the partial weight-gradient tiles of one launch over its pixel chunks and add the
// result into the gradient array (reference layout).  Deterministic, no atomics.
//   value(tap, row, col) = sum_z part[tap*tap_stride + z*z_stride + row*ldp + col]
struct ReduceArgs {
    const float* part; int Z, taps, rows, cols, ldp; int64_t z_stride, tap_stride;
    float* dw; int ldw_out, cmap;
};
// The two tile layouts a weight-gradient launch leaves behind.
// Chunk-major tiles of rows_padded x ldp, taps outermost (the implicit-GEMM weight gradients and the wave-specialised 1x1 one):
static inline ReduceArgs reduce_chunk_major(const float* part, int n_chunks, int taps, int rows, int cols, int64_t rows_padded, int64_t ldp,
                                            float* dw, int ldw_out, int cmap) {
    ReduceArgs r{};
    r.part = part; r.Z = n_chunks; r.taps = taps; r.rows = rows; r.cols = cols; r.ldp = (int)ldp;
    r.z_stride = rows_padded * ldp; r.tap_stride = (int64_t)n_chunks * rows_padded * ldp;
    r.dw = dw; r.ldw_out = ldw_out; r.cmap = cmap;
    return r;
}
// Tap-inner tiles of 9 x 32 x 128 per (tile group, stream) (the halo 3x3 weight gradient):
static inline ReduceArgs reduce_tap_inner(const float* part, int n_tiles, float* dw) {
    ReduceArgs r{};
    r.part = part; r.Z = n_tiles; r.taps = 9; r.rows = kGrowth; r.cols = kBottleneck; r.ldp = kBottleneck;
    r.z_stride = (int64_t)9 * kGrowth * kBottleneck; r.tap_stride = (int64_t)kGrowth * kBottleneck;
    r.dw = dw; r.ldw_out = kBottleneck * 9; r.cmap = C_3x3;
    return r;
}
// ONE launch of reduce_partials_kernel serves up to two reductions (either may be empty: Z == 0); a workgroup sums 64 elements.
struct ReducePair {
    ReduceArgs a{}, b{};
    static int blocks(const ReduceArgs& r) { return r.Z ? (r.taps * r.rows * r.cols + 63) / 64 : 0; }
};

// Pixel-chunk size of a weight-gradient launch: enough workgroups to fill the chip
// (~768) but no more - every workgroup ends with one fp32 atomicAdd per output element.
// Chunks are sized over the plane's VALID rows: every chunk starts inside [0, HW), so every workgroup of the launch stores its
// partial tile (a chunk that starts in the plane's padding rows - up to 127 of them since make_plane pads the big planes to 128
// rows - would leave without storing, and reduce_partials_kernel would add whatever the workspace held there).  The last chunk
// may run into the padding (the kernels clamp its length to HWp; padding rows hold zero gradients).
static inline void pick_chunk(const Plane& pl, int n_planes, int tiles_per_chunk, int& chunk, int& cps, int target = 768) {
    const int want = (target + tiles_per_chunk - 1) / tiles_per_chunk;
    cps = (want + n_planes - 1) / n_planes;
    if (cps < 1) cps = 1;
    chunk = ((pl.HW + cps - 1) / cps + 63) / 64 * 64;
    cps = (pl.HW + chunk - 1) / chunk;
}

// Tile side of the LDS-halo 3x3 kernels for a plane: 16 where it tiles exactly, else 8 (ragged edges masked) - and 8
// as well when the launch would have fewer than 320 16x16 tiles (few streams per call; 80x80 planes of a 9-stream
// forward chain): four times the workgroups fill the chip (forward sweep 9.05 -> 8.77 ms, single-rotation forward
// 4.3 -> 3.6 ms).
static inline int halo_tile(const Plane& p, int n_streams = 1 << 20) {
    // (tiles that hang over the edge are masked: S = 1824's 456^2 / 228^2 / 114^2 planes take 16 x 16 tiles too - round 5)
    return (int64_t)((p.H + 15) / 16) * ((p.W + 15) / 16) * n_streams >= 200 ? 16 : 8;      // (round 5, 320 -> 200: a single-sample step's 160^2 planes and the 80^2 planes of
                                                                                            //  an 8-stream forward chain take 16 x 16 tiles - step 5.71 -> 5.63 ms, headline 16.0 both ways; 100: the 17-stream
                                                                                            //  40^2 planes would too, 16.05)
}

// Floats of the partial tiles a halo 3x3 weight-gradient launch leaves: 9 taps of 32 x 128 per (tile group, stream).
static inline int64_t w3_partial_floats(int groups, int n_streams) { return (int64_t)groups * n_streams * 9 * 32 * kBottleneck; }

// 3x3 weight-gradient halo kernel: tiles per workgroup.  The launch runs in rounds of 512 resident workgroups (2 per
// CU), each lasting tiles_per_wg tile-times plus a fixed prologue + 9-tap flush (~0.6 of a 16x16 tile-time, measured);
// take the run length with the shortest total (e.g. 100 tiles x 17 streams -> 7, 25 tiles -> 4), then lengthen it
// until the partial tiles fit the workspace.
static inline int w3_tiles_per_wg(int n_tiles, int ts, int n_streams, int64_t part_floats, double fix_scale = 1.0) {
    const double fix = (ts == 16 ? 0.6 : 2.4) * fix_scale;
    double best = 1e30;
    int tpw_best = 1;
    for (int tpw = 1; tpw <= n_tiles; ++tpw) {
        const int g = (n_tiles + tpw - 1) / tpw;
        const int rounds = (g * (kBottleneck / 32) * n_streams + 511) / 512;
        const double cost = rounds * (tpw + fix);
        if (cost < best - 1e-9) { best = cost; tpw_best = tpw; }
    }
    // (taking the LONGEST run length within 4-40 % of the shortest total - fewer partial tiles for the reduce to read back - measured
    //  17.3-17.4 against 17.27 ms per step: the partial-tile traffic is not what the side stream waits for)
    while (tpw_best < n_tiles && w3_partial_floats((n_tiles + tpw_best - 1) / tpw_best, n_streams) > part_floats) ++tpw_best;
    return tpw_best;
}

// The halo 3x3 weight gradient's cut of a plane: tiles of ts x 8 pixels, runs of tiles_per_wg tiles per workgroup.
constexpr int kW3TileH = 8;
struct W3Tiling { int ts, tiles_x, n_tiles, tiles_per_wg, groups; };
static inline W3Tiling w3_tiling(const Plane& pl, int ts, int n_streams, int64_t part_floats) {
    W3Tiling t;
    t.ts = ts;
    t.tiles_x = (pl.W + ts - 1) / ts; t.n_tiles = ((pl.H + kW3TileH - 1) / kW3TileH) * t.tiles_x;
    t.tiles_per_wg = w3_tiles_per_wg(t.n_tiles, ts, n_streams, part_floats, (double)ts / kW3TileH);
    t.groups = (t.n_tiles + t.tiles_per_wg - 1) / t.tiles_per_wg;
    return t;
}

// Column-tile widths of the two 1x1 weight-gradient kernels (WswGeo::BN, CfgW128x64::BN: asserted where they are launched).
constexpr int kW1WsTileN = 128, kW1TileN = 64;

// What a dense layer's two weight-gradient launches look like: a function of the plane, the layer's input channels and the call.
struct WgradPlan {
    // conv2 (3x3) with the activation halo in LDS (not filled under the generic3x3 crosscheck)
    W3Tiling w3; unsigned w3_grid;
    // conv1 (1x1): wave-specialised (128-column tiles) or generic (64-column tiles); nt column tiles, cps chunks of `chunk` pixels per stream
    bool w1_ws; int nt, chunk, cps;
};
// Does a dense layer's 1x1 weight gradient leave partial tiles (summed by reduce_partials_kernel in a fixed order) or add with fp32 atomics?
// Atomics save a few-stream call - which is host-launch-bound - the reduce launches, but each workgroup then sums its whole pixel chunk in
// ONE set of fp32 accumulators before it adds: on planes of more than 1600 pixels that is a chain of 800 - 2600 pixels per workgroup and
// 16 - 63 atomics per element, measured at 3.0 - 7.3x the error of a blocked fp32 reduction (S = 672, 3 streams, 168^2 / 84^2; the
// partial-tile form: 1.3 - 2.4x).  So few-stream calls keep the atomics on the small planes only - the ones whose GS the side stream
// materialises as well (backward.hip gs_on_side).
static inline bool w1_partial_tiles(const Plane& pl, int NS, bool deterministic) { return deterministic || NS > 4 || pl.HW > 1600; }

// split16: the walk's operand form of the dense layers (fp16-split units in D2), which the wave-specialised 1x1 kernel reads.
static inline WgradPlan plan_layer_wgrads(const Plane& pl, int cin, int NS, int prec, bool split16, bool deterministic, int64_t part_floats,
                                          bool generic3x3, bool generic_w1) {
    WgradPlan w{};
    if (!generic3x3) {
        w.w3 = w3_tiling(pl, halo_tile(pl, NS), NS, part_floats);
        w.w3_grid = (unsigned)(((w.w3.groups * NS + 7) / 8) * 8 * (kBottleneck / 32));      // (see the kernel: channel groups of a tile group share an XCD)
    }
    // conv1 weight gradient, wave-specialised (wsw.cuh): 128 x 128 tiles, 32-pixel k-tiles, loader + matrix waves - for the partial-tile
    // form (w1_partial_tiles) on layers of more than 64 input channels (a half-empty 128-column tile
    // costs block 1's first layer 77 -> 107 us; few-stream calls keep the generic kernel's 128 x 64 atomics: 7.3 -> 7.5 ms per single-sample step)
    const bool partial = w1_partial_tiles(pl, NS, deterministic);
    w.w1_ws = split16 && !generic_w1 && cin > 64 && partial;
    if (w.w1_ws) {
        w.nt = (cin + kW1WsTileN - 1) / kW1WsTileN;
        pick_chunk(pl, NS, w.nt, w.chunk, w.cps, 320);      // (256 / 512 / 768 workgroups: 16.45-16.62 / 16.64-16.67 / 16.73-16.82 ms per step against 16.47-16.53)
    } else {   // generic.  ~320 workgroups: it shares the chip with the data-gradient chain on the other stream
        // (256..384 measure the same, 512 / 768 / 1024 cost the step 0.15 / 0.35 / 0.75 ms)
        w.nt = (cin + kW1TileN - 1) / kW1TileN;
        // 16-bit storage: the k-loop is a third as long, the 128 x 64 atomics per workgroup are not - half as many workgroups
        // on many-stream batches (config 3: 28.9 -> 28.5 ms at 160; 120 / 80: 28.6 / 28.8; S = 1824 with 5 streams: 320 stays)
        // few-stream calls on the atomics form: 128 (every workgroup adds a 128 x 64 tile with fp32 atomics; single-sample step 5.9 -> 5.65 ms;
        // 64 / 192 / 320: 6.0 / 5.7 / 5.9)
        pick_chunk(pl, NS, w.nt, w.chunk, w.cps, (prec && NS >= 16) ? 160 : !partial ? 128 : 320);
    }
    return w;
}

// The partial-tile workspace of ONE backward call: `floats` floats, used by the side stream's weight-gradient launches and
// drained by reduce_partials_kernel launches on the same stream.  This type owns the cursor and the reductions that are still
// pending; the walk asks it where a launch's tiles go - always an offset in floats from the workspace's base, -1 = no partial tiles:
// the launch adds with fp32 atomics - and launches the ReducePairs it hands out, in the order it hands them out.  (The reductions
// themselves carry pointers: the walk builds them from the offset it was given.)  The rules:
//  * A launch outside the dense layers (head conv0, transition, stem - and the generic 3x3 crosscheck form) has the workspace to
//    itself from offset 0: whatever is pending is drained in front of it, and its own reduction follows it at once.
//  * A dense layer's halo 3x3 tiles start at offset 0 and its 1x1 tiles go behind them, so that ONE reduce launch serves both (if the
//    1x1 tiles do not fit behind, or the 1x1 takes atomics, the 3x3 reduction runs first and the 1x1 starts over at offset 0).
//    The 1x1 leaves partial tiles (reproducible; since reduce_partials splits the partials over four waves the fixed-order reduce
//    beats 128 x 64 fp32 atomics per workgroup) with more than four streams, under "deterministic" and on planes of more than 1600
//    pixels (w1_partial_tiles); a few streams are host-launch-bound, on the small planes atomics save the reduce launches.
//  * Layers whose 1x1 takes atomics (only the 3x3 leaves partial tiles): the reduce of layer l waits for layer l - 1's and
//    ONE launch serves both - the tiles alternate between the two halves of the workspace.  (The side stream is the longer one
//    in a single-sample step: 29 reduce launches of ~7.5 us less on it.)
//  * drain() before the side stream is joined.
// "deterministic" never loses its bit-reproducibility silently: a launch whose partial tiles do not fit is refused.
class PartialTiles {
public:
    enum Kind { ALONE, HALO3, HALO3_PAIRED, BEHIND3 };
    struct Slot {
        Kind kind; int64_t off;      // first float of the launch's partial tiles, or -1: atomics
        int64_t size;                // floats the tiles take
        ReducePair first;            // to launch in front of the weight-gradient launch (empty: nothing)
        bool refused;                // after `first`: the walk fails with code -12 and refusal()
    };
    PartialTiles(int64_t floats_, int n_streams, bool deterministic_) : floats(floats_), NS(n_streams), deterministic(deterministic_) {}

    Slot place_alone(int64_t need) {
        Slot s{ALONE, need <= floats ? 0 : -1, need, drain(), false};
        if (s.off < 0 && deterministic) s.refused = refuse(need, floats);
        return s;
    }
    // w1_partial: this layer's 1x1 leaves partial tiles behind the 3x3's (w1_partial_tiles)
    Slot place_halo3x3(int groups, bool w1_partial) {
        Slot s{HALO3, 0, w3_partial_floats(groups, NS), ReducePair{}, false};
        if (s.size > floats) { s.refused = refuse(-1, floats); return s; }
        if (!w1_partial && s.size * 2 <= floats) s.kind = HALO3_PAIRED;
        if (s.kind == HALO3) s.first = drain();
        else if (half) s.off = floats / 2;
        return s;
    }
    Slot place_behind3x3(int64_t need, bool partial) {
        Slot s{BEHIND3, cursor, need, ReducePair{}, false};
        if (held.Z && (!partial || s.off + need > floats)) { s.first.a = held; held.Z = 0; s.off = 0; }
        const int64_t have = floats - s.off;
        if (!partial || need > have) s.off = -1;
        if (partial && s.off < 0 && deterministic) s.refused = refuse(need, have);
        return s;
    }
    // The launch placed at `s` was issued and left `r` to reduce (Z == 0: it used atomics): the reduce launch that is due now.
    ReducePair launched(const Slot& s, const ReduceArgs& r) {
        ReducePair due;
        if (s.kind == ALONE) due.a = r;
        else if (s.kind == BEHIND3) { due.a = held; due.b = r; held.Z = 0; cursor = 0; }
        else if (s.kind == HALO3) { held = r; cursor = s.size; }
        else {       // this layer's reduce rides with the next layer's (or the final drain)
            if (carried.Z) { due.a = carried; due.b = r; carried.Z = 0; }
            else carried = r;
            half ^= 1;
        }
        return due;
    }
    // What must be reduced before the workspace is reused from its start, or the side stream joined.
    ReducePair drain() { ReducePair due; due.a = carried; carried.Z = 0; return due; }
    // The text of the last refusal (need < 0: a 3x3 launch whose tiles do not fit in any mode).
    std::string refusal() const {
        if (refusal_need < 0) return "partial-gradient workspace too small";
        return "deterministic: a weight-gradient launch needs " + std::to_string(refusal_need) + " partial-tile floats, the workspace holds " +
               std::to_string(refusal_have);
    }

private:
    bool refuse(int64_t need, int64_t have) { refusal_need = need; refusal_have = have; return true; }
    int64_t floats; int NS; bool deterministic;
    ReduceArgs carried{};      // a paired 3x3 reduction waiting for the next layer's
    ReduceArgs held{};         // this layer's 3x3 reduction, waiting for its 1x1's
    int64_t cursor = 0;        // ... and the floats its tiles occupy from offset 0
    int half = 0;              // the half of the workspace the next paired 3x3 launch takes
    int64_t refusal_need = 0, refusal_have = 0;
};

}  // namespace smg
