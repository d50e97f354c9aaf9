// backward.hip - the backward walk: replaces loss.backward() of Trainer.backprop (code/trainer.py:350-351).
#include "engine.h"

// ------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------
// phases: bit 0 = the head and dense blocks 4, 3, 2 (down to the gradient of block 1's buffer), bit 1 = dense block 1, pool0 and
// the stem.  Between the two halves every gradient of [transition1 .. norm5] and of the head is final on `st`: a data-parallel
// caller starts their all-reduce there and hides it under the second half (smg_backward_phase).
int do_backward(smg_engine* e, const smg_net* net, const float* dq, hipStream_t st, int phases, bool elem_head) {
    if (!e->have_fwd) return fail(-22, "smg_backward without a preceding smg_forward");
    if (!net->grads) return fail(-22, "net.grads is NULL");
    // phase bookkeeping: the second half continues the first half of the SAME forward (statistic arenas, ring position, G' buffers)
    if (phases == 2 && !e->bw_phase0_done)
        return fail(-22, "smg_backward_phase(1) must follow smg_backward_phase(0) of the same forward");
    if ((phases & 1) && e->bw_phase0_done)
        return fail(-22, "smg_backward / smg_backward_phase(0) while the second half of a two-phase backward is still due (run phase 1 or a new forward)");
    const Layout& L = *e->L;
    const TrunkRef& T = L.trunk[e->f_trunk];
    const HeadRef& Hd = L.head[e->f_head];
    const int NS = e->f_streams, NP = e->f_pairs;
    const float* P = net->params;
    float* Gr = net->grads;
    const Plane p4 = e->p_blk[3];
    const bool ph_a = phases & 1, ph_b = phases & 2;
    if (ph_a) {     // every replica (one 1-D fill each: the 2-D fill of the same bytes took 70 us per step)
        for (int r = 0; r < kStatRep; ++r) HIP_OK(hipMemsetAsync(e->bstat + (size_t)r * kStatRepStride, 0, 2 * e->bstat_span * sizeof(double), st));
    }
    const bool split16 = e->prec == 0 && kSplitOp == 3;      // the hot classes run on fp16-split operands: GS scaled by its recorded maximum,
                                                             // D2 written in unit form with per-block scales (bn_bwd_apply_split_kernel)
    if (ph_a && split16) HIP_OK(hipMemsetAsync(e->gamax, 0, (size_t)e->gamax_words * sizeof(unsigned), st));
    // Weight-gradient kernels only read what the data-gradient chain produces and write disjoint
    // gradient ranges, so they run on a second stream beside it (their MFMA/L2-bound phases overlap the
    // HBM-bound epilogues of the data-gradient kernels).  While profiling everything is serialised on
    // `st` so that per-kernel durations stay clean.
    // (a lowest-priority stream for the weight gradients gains 0.2 ms per step with one engine alive, and LOSES 10 ms as soon
    // as a second engine - two more streams - exists in the process: the streams then share hardware queues and serialise)
    const hipStream_t s2 = (e->prof || e->serialize) ? st : e->side;
    auto fork = [&](hipEvent_t ev) -> int {      // side stream continues after everything enqueued on st so far
        HIP_OK(hipEventRecord(ev, st));
        HIP_OK(hipStreamWaitEvent(s2, ev, 0));
        return 0;
    };
    // operand kind 3 needs the finished GS's recorded maximum (always materialised there); few streams: launch-bound, the fused form wins
    const bool gs_materialised = split16 || NS > 4;
    // ... and for calls of a few streams (the single-sample step of Trainer.backprop) the materialisation of the small planes (blocks 3-4,
    // precision mode 0) leaves the data-gradient CHAIN: the 3x3 data gradient applies the BN backward on load, scaled by its own halo's
    // maximum, and the side stream materialises GS (with the stream maximum its 3x3 weight gradient scales by) in front of the weight
    // gradients - one dependent 10-17 us launch less per layer on a chain that is all latency there (single-sample step 7.41-7.45 ->
    // 7.23-7.29 ms).  With 17 streams the side stream has no slack on those planes: the same move costs the headline step 0.15 ms
    // (16.44-16.50 -> 16.62-16.64 ms, alternating on one box), and on the big planes the two strided slice reads cost more than the launch.
    auto gs_on_side = [&](const Plane& pl) { return split16 && !e->generic3x3 && pl.HW <= 1600 && NS <= 4; };
    // The G' / X slices of dense layer d's 32 output channels with the BN backward applied on load: what the 3x3 kernels read in
    // the fused form, and what launch_gs_apply materialises (that one from the forward's table instead of the fp64 sums)
    auto fused_gsrc = [&](int b, const DenseLayerRef& d) {
        return grad_src(e, e->G[b], kBlockCtot[b], e->X[b], kBlockCtot[b], e->st_X[b], d.cin, nullptr);
    };
    auto launch_gs_apply = [&](int b, int i, hipStream_t cs, float* GSb, const GradSrc& fused) {
        const Plane pl = e->p_blk[b];
        BnBwdApplyArgs a{};
        a.src = fused; a.src.xtab = stat_table(e, e->sx_tab[b], e->max_streams, kBlockCtot[b], T.layers[b][i].cin);
        a.pl = pl; a.C = kGrowth;
        a.out = GSb; a.ldo = kGrowth; a.amax = split16 ? gamax_of(e, b, i, 0) : nullptr;
        PREC_DISPATCH(e, launch_kernel(e, bn_bwd_apply_kernel<PREC>, dim3((pl.HWp + bn_apply_rows(PREC) - 1) / bn_apply_rows(PREC), NS), dim3(256), 0, cs,
                                       K_OTHER, 0, ESZ(e) * NS * pl.HW * 3 * kGrowth, false, a));
    };

    // The two activation operands of dense layer (b, i) (ActSrc): X[b] through norm1, channels c0 on, with the forward's table - the
    // 1x1 weight gradient in both its forms (c0 = 0) and the per-layer 1x1 data gradient's mask (c0 = the group's lowest channel) read
    // it; Bt through norm2 - the 3x3 data gradient's mask and the 3x3 weight gradient (the generic 3x3 path leaves no table of the
    // bottleneck: the fp64 sums).  The transition kernels read no table: their operand takes the sums.
    auto norm1_src = [&](int b, int i, int c0) {
        const DenseLayerRef& d = T.layers[b][i];
        return act_src(e, e->X[b], kBlockCtot[b], e->st_X[b], c0, P + d.n1.w, P + d.n1.b, stat_table(e, e->sx_tab[b], e->max_streams, kBlockCtot[b]), asc_n1(e, b, i));
    };
    auto norm2_src = [&](int b, int i) {
        const DenseLayerRef& d = T.layers[b][i];
        return act_src(e, el(e, e->Bt, e->bt_off[b][i]), kBottleneck, e->st_Bt[b][i], 0, P + d.n2.w, P + d.n2.b,
                       !e->generic3x3 ? stat_table(e, e->sb_tab[b][i], e->max_streams, kBottleneck) : StatTab{}, asc_n2(e, b, i));
    };

    // the partial-tile workspace of this call and its pending reductions (wgrad_plan.h has the rules)
    PartialTiles tiles(e->part_floats, NS, e->deterministic);

    if (ph_a) {
    {   // value conv backward + relu1 + norm1 sums
        ValueBwdArgs a;
        a.h1 = head_norm1_src(e, Hd, P); a.p4 = p4; a.w2p = e->packed_f + e->pk_head1;
        a.dq = dq; a.out_ch = e->head_out; a.OH = e->OH; a.OW = e->OW; a.dh1 = e->DH1;
        a.st = stat_sink_bwd(e, e->st_H1, 0); a.aff = affine_sink(Gr, Hd.n1); a.dw2 = Gr + Hd.c1.w;
        // a dense dq (the mark of smg_loss_map / smg_loss_map_ce, or "head_bwd" = 2) takes the two-pass form without atomics on the weight
        // gradient, one-channel and 3-class heads alike
        const bool dense = !elem_head && (e->head_bwd == 2 || (e->head_bwd == 0 && e->f_dense_dq));
        if (!dense) {
            launch_kernel(e, value_bwd_kernel, dim3((p4.HW + 63) / 64, NP), dim3(256), 0, st, K_OTHER, 0, 0, false, a);
        } else {
            ValueWgradDenseArgs w;
            w.h1 = a.h1; w.p4 = p4;
            w.dq = dq; w.OH = e->OH; w.OW = e->OW; w.n_pairs = NP; w.dw2 = a.dw2;
            w.RC = std::min(e->OH, 64); w.OWp = (e->OW + 3) / 4 * 4; w.Wp = w.OWp + kVFrame;
            auto go = [&](auto oc) {
                constexpr int OC = decltype(oc)::value;
                // (3 classes on 38 x 38 maps: 78 528 B of dynamic LDS - launch_kernel raises the kernel's limit)
                launch_kernel(e, value_bwd_dense_kernel<OC>, dim3((p4.HW + 63) / 64, NP), dim3(256), value_bwd_dense_lds(OC, e->OH, e->OW), st, K_OTHER, 0, 0, false, a);
                launch_kernel(e, value_wgrad_dense_kernel<OC>, dim3(20, kHeadMid / 4, OC), dim3(256), value_wgrad_dense_lds(w), st, K_OTHER, 0, 0, false, w);
            };
            if (e->head_out == 1) go(std::integral_constant<int, 1>{});
            else go(std::integral_constant<int, 3>{});
        }
    }
    int chunk4, cps4;
    pick_chunk(p4, NP, 2 * kFeat / 64, chunk4, cps4);
    const GradSrc dh1 = grad_src(e, e->DH1, kHeadMid, e->H1, kHeadMid, e->st_H1, 0, P + Hd.n1.w);      // dy1 through norm1: both conv0 gradients read it
    const ActSrc f0 = act_src(e, e->F, 2 * kFeat, e->st_F, 0, P + Hd.n0.w, P + Hd.n0.b);                // F through the head's norm0: likewise
    {   // head conv0 weight gradient
        auto go = [&](auto ptag) -> int {
        BwdWeightP<CfgW64x64, W_ONE, C_IDENT, kPdWgrad, true, decltype(ptag)::value, true> p{};      // fp32 head buffers in every mode
        p.gs = dh1; p.pa = p4; p.MA = kHeadMid;
        p.bsrc = f0; p.pb = p4; p.NB = 2 * kFeat;
        p.chunk = chunk4; p.chunks_per_stream = cps4; p.n_chunks = NP * cps4;
        p.dw = Gr + Hd.c0.w; p.ldw_out = 2 * kFeat;
        if (fork(e->ev_misc)) return -5;
        const dim3 grid(1, 2 * kFeat / 64, NP * cps4);
        return launch_wgrad(e, s2, p, grid, K_HW0, 2.0 * NP * p4.HW * 2 * kFeat * kHeadMid,
                            4.0 * NP * p4.HW * (2 * kHeadMid + 2 * kFeat), 1, C_IDENT, tiles, tiles.place_alone(wgrad_partial_floats(p, grid)));
        };
        PREC_DISPATCH(e, if (int rc = go(PTAG)) return rc);
    }
    {   // head conv0 data gradient + relu0 + norm0 sums
        auto run = [&](auto tag, auto ptag) {
                using Cfg = decltype(tag);
                BwdDataP<Cfg, false, E_STORE, true, decltype(ptag)::value, true> p{};      // fp32 head buffers in every mode
        p.gs = dh1; p.pa = p4; p.KA = kHeadMid;
        p.wp = e->packed_u + e->pk_hd0; p.K8tot = kHeadMid / 8; p.ldn = 2 * kFeat; p.wcol0 = 0; p.N = 2 * kFeat;
        p.m = f0; p.pm = p4;
        p.dst = e->DF; p.ldd = 2 * kFeat; p.dcoff = 0;
        p.st = stat_sink_bwd(e, e->st_F, 0); p.aff = affine_sink(Gr, Hd.n0);
        launch_gemm(e, st, p, dim3(NP * p4.HWp / Cfg::BM, 2 * kFeat / Cfg::BN), K_HD0, 2.0 * NP * p4.HW * 2 * kFeat * kHeadMid,
                    4.0 * NP * p4.HW * (2 * kHeadMid + 2 * 2 * kFeat));
            };
            PREC_DISPATCH(e, if (p4.HWp % 128 == 0) run(CfgP128x128{}, PTAG); else run(CfgP64x128{}, PTAG));
    }
    {   // head norm0 backward + concat backward + norm5 backward -> G'_4
        Norm5BwdArgs a;
        a.df = grad_src(e, e->DF, 2 * kFeat, e->F, 2 * kFeat, e->st_F, 0, P + Hd.n0.w); a.p4 = p4;
        a.x4 = norm5_src(e, T, P);
        a.user_ptr = e->d_user_ptr; a.user_pair = e->d_user_pair; a.user_slot = e->d_user_slot;
        a.G4 = e->G[3]; a.st = stat_sink_bwd(e, e->st_X[3], 0); a.aff = affine_sink(Gr, T.norm5); a.chunk = 16;
        PREC_DISPATCH(e, launch_kernel(e, norm5_bwd_kernel<PREC>, dim3(4, NS, (p4.HW + 15) / 16), dim3(256), 0, st, K_OTHER, 0, 0, false, a));
    }
    }   // ph_a: head
    // Buffers of a dense layer's finished gradients (GS: its 32 output channels, D2: its bottleneck, D2S: D2's block scales): a ring of
    // kRing slots in backward order, which the side stream releases as its weight gradients finish.  The ring position of a layer is
    // static (a two-phase backward's second half continues where the first stopped).
    // (Measured and rejected in round 5: own buffers for the layers of blocks 3-4 and their weight gradients DEFERRED to the
    // bandwidth-bound kernels of block 2 - the idea being that a concurrent kernel stretches the 10-20 us chain kernels of the small
    // planes.  Same box, alternating: 16.44-16.66 ms per step without, 17.13-17.40 with four deferred layers per layer of block 2,
    // 17.37-17.50 with eight: the side stream's work on the small planes is what fills an otherwise idle chip.)
    struct LayerBuf { float* GS; float* D2; float* D2S; int ring; };
    auto buf_of = [&](int b, int i) -> LayerBuf {
        const int r = ring_pos(b, i);
        return LayerBuf{e->GS[r % kRing], e->D2[r % kRing], e->D2S[r % kRing], r};
    };
    // The two weight gradients of dense layer (b, i) and their reduce launches, on the side stream (which must already wait for the
    // layer's D2 / GS).
    auto issue_wgrads = [&](int b, int i) -> int {
        const Plane pl = e->p_blk[b];
        const DenseLayerRef& d = T.layers[b][i];
        const LayerBuf lb = buf_of(b, i);
        const WgradPlan w = plan_layer_wgrads(pl, d.cin, NS, e->prec, split16, e->deterministic, e->part_floats, e->generic3x3, e->generic_w1);
        GradSrc gsrc = fused_gsrc(b, d);
        if (gs_on_side(pl)) launch_gs_apply(b, i, s2, lb.GS, gsrc);
        if (gs_materialised) gsrc = grad_done(lb.GS, kGrowth, gamax_of(e, b, i, 0));
        if (!e->generic3x3) {
            // conv2 weight gradient with the activation halo resident in LDS (halo.cuh)
            const bool w1_partial = w1_partial_tiles(pl, NS, e->deterministic);
            const PartialTiles::Slot at = tiles.place_halo3x3(w.w3.groups, w1_partial);
            if (at.refused) return fail(-12, tiles.refusal());
            launch_reduce2(e, s2, at.first);
            Halo3x3WgradArgs a;
            a.g = gsrc; a.pl = pl; a.b = norm2_src(b, i); a.C = kBottleneck;
            a.tiles_x = w.w3.tiles_x; a.n_tiles = w.w3.n_tiles; a.tiles_per_wg = w.w3.tiles_per_wg;
            a.part = part_at(e, at);
            a.groups = w.w3.groups; a.streams = NS;
            const double flops = 2.0 * NS * pl.HW * 9 * kBottleneck * kGrowth, bytes = ESZ(e) * NS * pl.HW * (kGrowth + kBottleneck);
            if (w.w3.ts == 16) {
                PREC_DISPATCH(e, launch_kernel(e, conv3x3_halo_wgrad_kernel<16, PREC>, dim3(w.w3_grid), dim3(256), HaloWgradSGeo<16, PREC>::smem_bytes(), s2,
                                               K_W3, flops, bytes, false, a));
            } else {
                PREC_DISPATCH(e, launch_kernel(e, conv3x3_halo_wgrad_kernel<8, PREC>, dim3(w.w3_grid), dim3(256), HaloWgradSGeo<8, PREC>::smem_bytes(), s2,
                                               K_W3, flops, bytes, false, a));
            }
            launch_reduce2(e, s2, tiles.launched(at, reduce_tap_inner(a.part, w.w3.groups * NS, Gr + d.c2.w)));
        } else {   // conv2 weight gradient (generic implicit GEMM, one launch slice per tap)
            int chunk, cps;
            pick_chunk(pl, NS, 9, chunk, cps);      // (9 workgroups per chunk: one per tap)
            BwdWeightP<CfgW32x128, W_THREE, C_3x3, kPdWgrad, false> p{};
            p.gs = grad_done(lb.GS, kGrowth); p.pa = pl; p.MA = kGrowth;
            p.bsrc = norm2_src(b, i); p.pb = pl; p.NB = kBottleneck;
            p.chunk = chunk; p.chunks_per_stream = cps; p.n_chunks = NS * cps;
            p.dw = Gr + d.c2.w; p.ldw_out = kBottleneck * 9;
            const dim3 grid(1, 1, 9 * NS * cps);
            if (int rc = launch_wgrad(e, s2, p, grid, K_W3, 2.0 * NS * pl.HW * 9 * kBottleneck * kGrowth,
                                      ESZ(e) * NS * pl.HW * (kGrowth + kBottleneck), 9, C_3x3, tiles, tiles.place_alone(wgrad_partial_floats(p, grid)))) return rc;
        }
        if (w.w1_ws) {   // conv1 weight gradient, wave-specialised (wsw.cuh)
            using G = WswGeo;
            static_assert(G::BN == kW1WsTileN, "plan_layer_wgrads counts this kernel's column tiles");
            Wgrad1x1WsArgs a{};
            a.d2 = reinterpret_cast<const u32x4*>(lb.D2); a.binv = lb.D2S; a.b = norm1_src(b, i, 0); a.pl = pl; a.NB = d.cin;
            a.chunk = w.chunk; a.chunks_per_stream = w.cps; a.n_chunks = NS * w.cps;
            a.dw = Gr + d.c1.w; a.ldw_out = d.cin; a.ldp = w.nt * G::BN;
            const PartialTiles::Slot at = tiles.place_behind3x3((int64_t)a.n_chunks * G::BM * a.ldp, true);
            launch_reduce2(e, s2, at.first);
            if (at.refused) return fail(-12, tiles.refusal());
            a.part = part_at(e, at);
            a.tm = TileMap{a.n_chunks, w.nt, 0};
            launch_kernel(e, conv1x1_wgrad_ws_kernel, dim3(tile_grid(a.tm)), dim3(512), G::smem_bytes(w.chunk), s2, K_W1,
                          2.0 * NS * pl.HW * d.cin * kBottleneck, 4.0 * NS * pl.HW * (kBottleneck + d.cin), false, a);
            ReduceArgs red1{};
            if (a.part) red1 = reduce_chunk_major(a.part, a.n_chunks, 1, G::BM, d.cin, G::BM, a.ldp, a.dw, d.cin, C_IDENT);
            launch_reduce2(e, s2, tiles.launched(at, red1));
        } else {   // conv1 weight gradient, generic
            using Cfg = CfgW128x64;
            static_assert(Cfg::BN == kW1TileN, "plan_layer_wgrads counts this kernel's column tiles");
            auto go = [&](auto ptag) -> int {
                BwdWeightP<MC<Cfg, decltype(ptag)::value>, W_ONE, C_IDENT, kPdWgrad, false, decltype(ptag)::value> p{};
                p.gs = grad_done(lb.D2, kBottleneck); p.pa = pl; p.MA = kBottleneck; p.binv = lb.D2S;
                p.bsrc = norm1_src(b, i, 0); p.pb = pl; p.NB = d.cin;
                p.chunk = w.chunk; p.chunks_per_stream = w.cps; p.n_chunks = NS * w.cps;
                p.dw = Gr + d.c1.w; p.ldw_out = d.cin;
                const dim3 grid(1, w.nt, NS * w.cps);
                return launch_wgrad(e, s2, p, grid, K_W1, 2.0 * NS * pl.HW * d.cin * kBottleneck,
                                    ESZ(e) * NS * pl.HW * (kBottleneck + d.cin), 1, C_IDENT, tiles, tiles.place_behind3x3(wgrad_partial_floats(p, grid), w1_partial_tiles(pl, NS, e->deterministic)));
            };
            PREC_DISPATCH(e, if (int rc = go(PTAG)) return rc);
        }
        return 0;
    };
    // debug_stop (engine.h): leave the backward here - both streams joined, the forward's state consumed
    auto debug_stop = [&]() -> int {
        launch_reduce2(e, s2, tiles.drain());
        HIP_OK(hipEventRecord(e->ev_end, s2));
        HIP_OK(hipStreamWaitEvent(st, e->ev_end, 0));
        // the walk leaves in front of db_flush_kernel: drop what the layers so far left in the dbeta / dgamma scratch, or the next
        // backward's flush adds it to ITS norm1 / transition-norm gradients (the scratch is zero between calls: engine.h)
        HIP_OK(hipMemsetAsync(e->dbscr, 0, (size_t)kDbRep * e->db_total * sizeof(float), st));
        if (int rc = walk_status(e)) return rc;
        e->have_fwd = false; e->bw_phase0_done = false; e->prof_stage = -1;
        return 0;
    };
    // debug_stop only: a device-to-device copy of `elems` mode-typed elements of `src` on the chain stream, into a lazily grown debug buffer
    // (its capacity counts floats, so it holds the elements of every mode; n: the elements of THIS snapshot); smg_debug_read widens it by
    // the mode recorded here
    auto dbg_snapshot = [&](float*& buf, int64_t& cap, int64_t& n, const float* src, int64_t elems) -> int {
        if (cap < elems) {
            if (buf) (void)hipFree(buf);
            buf = nullptr; cap = 0;
            HIP_OK(hipMalloc((void**)&buf, (size_t)elems * sizeof(float)));
            cap = elems;
        }
        HIP_OK(hipMemcpyAsync(buf, src, (size_t)elems * (e->prec ? 2 : 4), hipMemcpyDeviceToDevice, st));
        e->dbg_snap_prec = e->prec; n = elems;
        return 0;
    };
    // pool0's backward and conv0's weight gradient at pooled resolution (elem.cuh: stem_tail_kernel; mode 0, one-channel stem) - like the
    // partial-tile form of the 1x1 weight gradient for calls of more than four streams or under "deterministic": a call of a few
    // streams is launch-bound on the side stream, where the moments and the combine are three launches more than the pair they
    // replace (single-sample step 5.34-5.57 ms with the stem-resolution pair, 5.65-6.20 with the pooled tail, alternating on one box)
    const bool pooled_tail = e->prec == 0 && e->f_stem1 && !e->stem_plane_tail && (NS > 4 || e->deterministic);
    for (int b = ph_a ? 3 : 0; b >= (ph_b ? 0 : 1); --b) {
        e->prof_stage = b;
        const Plane pl = e->p_blk[b];
        const int Ct = kBlockCtot[b];
        if (e->dbg_stop == b * 100 + 50) return debug_stop();
        if (b == 0 && pooled_tail) {      // the image moments R_n | S_n need the image only: on the side stream, under dense block 1's kernels
            StemMomArgs a;
            a.img = e->img4; a.pi = e->p_img; a.ps = e->p_stem; a.part = e->mom_part;
            a.tiles_x = stem_mom_tiles_x(e->p_stem); a.n_tiles = stem_mom_tiles(e->p_stem); a.tiles_per_wg = kMomTilesPerWg;
            if (fork(e->ev_misc)) return -5;
            e->prof_stage = -1;
            launch_kernel(e, stem_moments_kernel, dim3(e->mom_groups, NS), dim3(256), 0, s2, K_OTHER, 0, 0, false, a);
            launch_kernel(e, stem_moments_sum_kernel, dim3((kMomOut + 255) / 256, NS), dim3(256), 0, s2, K_OTHER, 0, 0, false,
                          (const float*)e->mom_part, e->mom_groups, e->mom);
            e->prof_stage = b;
        }
        for (int i = (int)T.layers[b].size() - 1; i >= 0; --i) {
            const DenseLayerRef& d = T.layers[b][i];
            float* bt = el(e, e->Bt, e->bt_off[b][i]);
            const ActSrc n2 = norm2_src(b, i);      // Bt through norm2: the 3x3 data gradient's mask (its weight gradient builds the same on the side stream)
            const StatSink n2st = stat_sink_bwd(e, e->st_Bt[b][i], 0);      // norm2's sums: the halo and the generic 3x3 data gradient add to them
            const LayerBuf lb = buf_of(b, i);
            float* GSb = lb.GS;
            float* D2b = lb.D2;
            // ring slots: at every third layer wait for the side stream's event of the LATEST of the next three slots' previous users
            // (ring position + 2 - kRing; the side stream is in order, so the two before it are done as well)
            static_assert(kRing % 3 == 0 && kRing > 3, "the sparse ring wait covers three slots at a time");
            if (lb.ring >= kRing && lb.ring % 3 == 0) HIP_OK(hipStreamWaitEvent(st, e->ev_side[(lb.ring + 2) % kRing], 0));
            // This layer's finished output-slice gradient GS = invstd*(G' - s1/n - xhat*s2/n), materialised once (dense
            // [px][32]) for the 3x3 data- and weight-gradient kernels.  They can also apply it while loading the G' / X
            // slices (GradSrc with x set): one launch less on the dependency chain, but measured 0.5 ms per step slower on
            // many-stream batches - two strided 128-B-per-pixel reads replace one dense one in both consumers.
            GradSrc gsrc = fused_gsrc(b, d);
            if (e->generic3x3 || (gs_materialised && !gs_on_side(pl))) {
                launch_gs_apply(b, i, st, GSb, gsrc);
                if (gs_materialised) gsrc = grad_done(GSb, kGrowth, gamax_of(e, b, i, 0));
            }
            if (!e->generic3x3) {
                // conv2 (3x3) data gradient with the gradient halo resident in LDS (halo.cuh)
                Halo3x3DgradArgs a;
                a.g = gsrc; a.pl = pl; a.C = kBottleneck; a.m = n2;
                a.dst = split16 ? e->DY2 : D2b; a.st = n2st;
                a.wu = e->packed_u + e->pk_hd[b][i];
                // (traced launches: dev stamps with SMG_TRACE_KIND=5)
                const double flops = 2.0 * NS * pl.HW * 9 * kBottleneck * kGrowth;
                const double bytes = ESZ(e) * NS * pl.HW * (kGrowth + 2 * kBottleneck);      // gradient in, mask source in, dy out
                if (halo_tile(pl, NS) == 16) {
                    a.tiles_x = (pl.W + 15) / 16; a.cg_per_wg = kBottleneck / 32;
                    if (pl.H % 16 || pl.W % 16) {      // tiles hang over the edge: the bounds-checked instantiation
                        PREC_DISPATCH(e, launch_kernel(e, conv3x3_halo_dgrad_kernel<16, PREC, true>, dim3(((pl.H + 15) / 16) * a.tiles_x, NS), dim3(256),
                                                       HaloDgradSGeo<16, PREC>::smem_bytes(kBottleneck), st, K_D3, flops, bytes, true, a));
                    } else {
                        PREC_DISPATCH(e, launch_kernel(e, conv3x3_halo_dgrad_kernel<16, PREC>, dim3((pl.H / 16) * a.tiles_x, NS), dim3(256),
                                                       HaloDgradSGeo<16, PREC>::smem_bytes(kBottleneck), st, K_D3, flops, bytes, true, a));
                    }
                } else {
                    a.tiles_x = (pl.W + 7) / 8; a.cg_per_wg = 1;      // small planes: one 64-channel group per workgroup
                    PREC_DISPATCH(e, launch_kernel(e, conv3x3_halo_dgrad_kernel<8, PREC>, dim3(((pl.H + 7) / 8) * a.tiles_x, NS, kBottleneck / 64), dim3(256),
                                                   HaloDgradSGeo<8, PREC>::smem_bytes(kBottleneck), st, K_D3, flops, bytes, true, a));
                }
            } else {   // conv2 (3x3) data gradient -> dy of relu2/norm2 (D2) + norm2 sums (generic implicit GEMM)
                auto run = [&](auto tag) {
                    using Cfg = decltype(tag);
                    BwdDataP<Cfg, true, E_STORE, false> p{};
                    p.gs = grad_done(GSb, kGrowth); p.pa = pl; p.KA = kGrowth;
                    p.wp = e->packed_u + e->pk_g3d[b][i]; p.K8tot = 9 * kGrowth / 8; p.ldn = kBottleneck; p.wcol0 = 0; p.N = kBottleneck;
                    p.m = n2; p.pm = pl;
                    p.dst = split16 ? e->DY2 : D2b; p.ldd = kBottleneck; p.dcoff = 0;
                    p.st = n2st; p.aff = affine_sink(Gr, d.n2);
                    launch_gemm(e, st, p, dim3(NS * pl.HWp / Cfg::BM, kBottleneck / Cfg::BN), K_D3, 2.0 * NS * pl.HW * 9 * kBottleneck * kGrowth,
                                ESZ(e) * NS * pl.HW * (kGrowth + 2 * kBottleneck));
                };
                if (pl.HWp % 128 == 0) run(CfgP128x128{}); else run(CfgP64x128{});
            }
            // dy through norm2 (the generic 3x3 path leaves no table of the bottleneck: the fp64 sums)
            const GradSrc dy2 = grad_src(e, split16 ? e->DY2 : D2b, kBottleneck, bt, kBottleneck, e->st_Bt[b][i], 0, P + d.n2.w,
                                         !e->generic3x3 ? stat_table(e, e->sb_tab[b][i], e->max_streams, kBottleneck) : StatTab{});
            if (split16) {   // norm2 backward applied once: D2 (unit form, per-block scales) <- gamma2*invstd*(dy - s1/n - xhat*s2/n)
                BnBwdApplySplitArgs a{};
                a.src = dy2; a.pl = pl; a.out = reinterpret_cast<u32x4*>(D2b); a.binv = lb.D2S;
                if (!e->generic3x3) a.aff = affine_sink(Gr, d.n2);      // the halo dgrad leaves these to us
                launch_kernel(e, bn_bwd_apply_split_kernel, dim3(pl.HWp / kScaleBlock, NS), dim3(256), 0, st, K_OTHER, 0, 4.0 * NS * pl.HW * 3 * kBottleneck, false, a);
            } else {   // 16-bit modes: norm2 backward applied once, in place: D2 <- gamma2*invstd*(dy - s1/n - xhat*s2/n)
                if (e->dbg_stop == b * 100 + i) {      // tests: the raw 3x3 data gradient, which the apply is about to overwrite ("dy2")
                    if (int rc = dbg_snapshot(e->dbg_dy2, e->dbg_dy2_floats, e->dbg_dy2_n, D2b, (int64_t)NS * pl.HWp * kBottleneck)) return rc;
                }
                BnBwdApplyArgs a{};
                a.src = dy2; a.pl = pl; a.C = kBottleneck; a.out = D2b; a.ldo = kBottleneck;
                if (!e->generic3x3) a.aff = affine_sink(Gr, d.n2);      // the halo dgrad leaves these to us
                PREC_DISPATCH(e, launch_kernel(e, bn_bwd_apply_kernel<PREC>, dim3((pl.HWp + bn_apply_rows(PREC) - 1) / bn_apply_rows(PREC), NS), dim3(256), 0, st,
                                               K_OTHER, 0, ESZ(e) * NS * pl.HW * 3 * kBottleneck, false, a));
            }
            // the layer's weight gradients: ONE fork per layer, behind the norm2 apply (GS and D2 are both final there)
            if (fork(e->ev_d2[lb.ring % kRing])) return -5;
            if (int rc = issue_wgrads(b, i)) return rc;
            HIP_OK(hipEventRecord(e->ev_side[lb.ring % kRing], s2));
            // conv1 (1x1) data gradient -> relu1/norm1 backward accumulated into G'.  Layers are grouped (kGroup,
            // from the top of the block): inside a group only the channels the group itself produced - needed by
            // the very next layer - are accumulated per layer; everything below the group's lowest layer is done
            // once for the whole group by BwdDataGroupP (gemm.cuh), which touches G' and x once instead of once
            // per layer.
            if (e->dbg_stop == b * 100 + i) {      // tests: G' of the block in front of this layer's 1x1 data gradients, in the mode's element size
                if (int rc = dbg_snapshot(e->dbg_gsnap, e->dbg_gsnap_floats, e->dbg_gsnap_n, e->G[b], (int64_t)NS * pl.HWp * Ct)) return rc;
            }
            const int L = (int)T.layers[b].size();
            const int g_lo = i - ((L - 1 - i) % kGroup == kGroup - 1 ? 0 : std::min(i, kGroup - 1 - (L - 1 - i) % kGroup));
            const int cs = T.layers[b][g_lo].cin;                       // channels below the group
            if (d.cin > cs) {                                           // [cs, cin): per-layer accumulate
                auto run = [&](auto tag, auto ptag) {
                    using Cfg = MC<decltype(tag), decltype(ptag)::value>;
                    BwdDataP<Cfg, false, E_ACCUM, false, decltype(ptag)::value> p{};
                    p.gs = grad_done(D2b, kBottleneck); p.pa = pl; p.KA = kBottleneck; p.binv = lb.D2S;
                    p.wp = e->packed_u + e->pk_d1[b][i]; p.K8tot = kBottleneck / 8; p.ldn = d.cin; p.wcol0 = cs; p.N = d.cin - cs;
                    p.m = norm1_src(b, i, cs); p.pm = pl;
                    p.dst = e->G[b]; p.ldd = Ct; p.dcoff = cs;
                    p.st = stat_sink_bwd(e, e->st_X[b], cs); p.aff = affine_sink_scr(e, e->db_off[b][i], d.cin, cs);
                    launch_gemm(e, st, p, dim3(NS * pl.HWp / Cfg::BM, (p.N + Cfg::BN - 1) / Cfg::BN), K_D1, 2.0 * NS * pl.HW * p.N * kBottleneck,
                                ESZ(e) * NS * pl.HW * (kBottleneck + 3.0 * p.N));          // dy in; x in, G' read + written
                };
                PREC_DISPATCH(e, if (pl.HWp % 128 == 0) run(CfgP128x64{}, PTAG); else run(CfgP64x64{}, PTAG));
            }
            if (i == g_lo) {                                            // [0, cs): the whole group at once
                auto run = [&](auto tag, auto ptag) {
                    using Cfg = MC<decltype(tag), decltype(ptag)::value>;
                    BwdDataGroupP<Cfg, decltype(ptag)::value> p{};
                    const int g_hi = L - 1 - ((L - 1 - g_lo) / kGroup) * kGroup;      // top layer of this group
                    p.nseg = g_hi - g_lo + 1;
                    for (int k = 0; k < p.nseg; ++k) {
                        const DenseLayerRef& dk = T.layers[b][g_lo + k];
                        const LayerBuf lk = buf_of(b, g_lo + k);
                        p.seg[k].g = lk.D2; p.seg[k].wp = e->packed_u + e->pk_d1[b][g_lo + k]; p.seg[k].ldn = dk.cin; p.seg[k].binv = lk.D2S;
                        p.seg[k].gamma = P + dk.n1.w; p.seg[k].beta = P + dk.n1.b;
                        p.seg[k].aff = affine_sink_scr(e, e->db_off[b][g_lo + k], dk.cin, 0);
                    }
                    p.ldg = kBottleneck; p.pa = pl; p.KA = kBottleneck; p.N = cs;
                    p.m = act_src(e, e->X[b], Ct, e->st_X[b], 0, nullptr, nullptr, stat_table(e, e->sx_tab[b], e->max_streams, Ct));      // (gamma / beta: per segment)
                    p.dst = e->G[b]; p.ldd = Ct;
                    p.st = stat_sink_bwd(e, e->st_X[b], 0);
                    launch_gemm(e, st, p, dim3(NS * pl.HWp / Cfg::BM, (cs + Cfg::BN - 1) / Cfg::BN), K_D1, 2.0 * NS * pl.HW * cs * kBottleneck * p.nseg,
                                ESZ(e) * NS * pl.HW * ((double)p.nseg * kBottleneck + 3.0 * cs));
                };
                // mode 0, 128-row tiles: 32-deep k-tiles with ONE tile of loads in flight - the staging registers of two 16-deep
                // tiles, half the barriers (k-loop 65k -> 50k cycles per workgroup, launches -7 %; same k16 order, same bits)
                // (MC doubles the depth in the 16-bit modes: 128 x 64 x 64 / 64 x 64 x 64)
                PREC_DISPATCH(e, if (pl.HWp % 128 == 0) run(GemmCfg<128, 64, 32, 2, 2, 1, true>{}, PTAG); else run(CfgP64x64{}, PTAG));
            }
            if (e->dbg_stop == b * 100 + i) return debug_stop();
        }
        if (b > 0) {   // transition b-1: X[b-1] (all channels) -> X[b][:, 0:C0]
            const Plane pp = e->p_blk[b - 1];
            const int Cp = kBlockCtot[b - 1], C0 = kBlockCin[b];
            const GradSrc gx = grad_src(e, e->G[b], Ct, e->X[b], Ct, e->st_X[b], 0, nullptr);      // the block's first C0 channels: both transition gradients read them
            const ActSrc xt = act_src(e, e->X[b - 1], Cp, e->st_X[b - 1], 0, P + T.tnorm[b - 1].w, P + T.tnorm[b - 1].b, StatTab{}, asc_trans(e, b - 1));      // X[b-1] through the transition norm: likewise
            {
                int chunk, cps;
                pick_chunk(pl, NS, (C0 / 128) * (Cp / 128), chunk, cps);
                auto go = [&](auto ptag) -> int {
                BwdWeightP<MC<CfgW128x128, decltype(ptag)::value>, W_POOL, C_IDENT, 1, true, decltype(ptag)::value> p{};      // (one k-tile in flight: the pooling fetch holds 4 float4 per slot, three tiles of them leave one workgroup per CU)
                p.gs = gx; p.pa = pl; p.MA = C0;
                p.bsrc = xt; p.pb = pp; p.NB = Cp;
                p.chunk = chunk; p.chunks_per_stream = cps; p.n_chunks = NS * cps;
                p.dw = Gr + T.tconv[b - 1].w; p.ldw_out = Cp;
                if (fork(e->ev_misc)) return -5;
                const dim3 grid(C0 / 128, Cp / 128, NS * cps);
                return launch_wgrad(e, s2, p, grid, K_TW, 2.0 * NS * pl.HW * Cp * C0,
                                    ESZ(e) * NS * (2.0 * pl.HW * C0 + (double)pp.HW * Cp), 1, C_IDENT, tiles, tiles.place_alone(wgrad_partial_floats(p, grid)));
                };
                PREC_DISPATCH(e, if (int rc = go(PTAG)) return rc);
            }
            if (pp.H != 2 * pl.H || pp.W != 2 * pl.W) {
                PREC_DISPATCH(e, launch_kernel(e, zero_uncovered_kernel<PREC>, dim3(256, NS), dim3(256), 0, st, K_OTHER, 0, 0, false,
                                               (void*)e->G[b - 1], Cp, pp, 2 * pl.H, 2 * pl.W, Cp));
            }
            {
                auto run = [&](auto tag, auto ptag) {
                using Cfg = MC<decltype(tag), decltype(ptag)::value>;
                BwdDataP<Cfg, false, E_UNPOOL, true, decltype(ptag)::value> p{};
                p.gs = gx; p.pa = pl; p.KA = C0;
                p.wp = e->packed_u + e->pk_td[b - 1]; p.K8tot = C0 / 8; p.ldn = Cp; p.wcol0 = 0; p.N = Cp;
                p.m = xt; p.pm = pp;
                p.dst = e->G[b - 1]; p.ldd = Cp; p.dcoff = 0;
                p.st = stat_sink_bwd(e, e->st_X[b - 1], 0); p.aff = affine_sink_scr(e, e->db_toff[b - 1], Cp, 0);
                launch_gemm(e, st, p, dim3(NS * pl.HWp / Cfg::BM, Cp / Cfg::BN), K_TD, 2.0 * NS * pl.HW * Cp * C0,
                            ESZ(e) * NS * (2.0 * pl.HW * C0 + 2.0 * pp.HW * Cp));
            };
            PREC_DISPATCH(e, run(CfgP64x128{}, PTAG));   // the 128-row variant of the unpool epilogue spills registers
            }
        }
    }
    e->prof_stage = -1;
    if (ph_b && pooled_tail) {   // pool0 / relu0 backward + norm0 sums + conv0 weight gradient from the pooled pixels
        const Plane p1 = e->p_blk[0];
        StemTailArgs a;
        a.g1 = grad_src(e, e->G[0], kBlockCtot[0], e->X[0], kBlockCtot[0], e->st_X[0], 0, nullptr); a.p1 = p1;
        a.argmax = e->argmax; a.stemv = e->stemv;
        a.stem = act_src(e, nullptr, 64, e->st_stem, 0, P + T.norm0.w, nullptr); a.ps = e->p_stem;      // (the stem plane is not read here)
        a.img = e->img4; a.pi = e->p_img;
        a.st = stat_sink_bwd(e, e->st_stem, 0);
        a.tiles_x = (p1.W + kTailTW - 1) / kTailTW; a.n_tiles = a.tiles_x * ((p1.H + kTailTH - 1) / kTailTH);
        // one 64 x 64 partial tile per workgroup.  Runs of 8 tiles or more: as long as it takes for ONE round of workgroups (three are
        // resident per CU) and for the partial tiles to fit the workspace
        a.tiles_per_wg = 8;
        auto groups = [&]() { return (a.n_tiles + a.tiles_per_wg - 1) / a.tiles_per_wg; };
        while (a.tiles_per_wg < a.n_tiles && ((int64_t)groups() * NS > 3 * e->n_cu || (int64_t)groups() * NS * 64 * 64 > e->part_floats)) ++a.tiles_per_wg;
        const int Z = groups() * NS;
        const PartialTiles::Slot at = tiles.place_alone((int64_t)Z * 64 * 64);
        launch_reduce2(e, s2, at.first);
        if (at.off < 0) return fail(-12, "partial-gradient workspace too small");
        a.part = part_at(e, at);
        // the kernel writes the workspace on `st`: behind everything the side stream still does there
        HIP_OK(hipEventRecord(e->ev_end, s2));
        HIP_OK(hipStreamWaitEvent(st, e->ev_end, 0));
        launch_kernel(e, stem_tail_kernel, dim3(groups(), NS), dim3(256), 0, st, K_SW, 2.0 * NS * p1.HW * 64 * 49,
                      4.0 * NS * ((double)p1.HW * (3 * 64 + 16) + (double)e->p_img.HW), false, a);
        if (fork(e->ev_misc)) return -5;
        launch_reduce2(e, s2, tiles.launched(at, reduce_chunk_major(a.part, Z, 1, 64, 49, 64, 64, Gr + T.conv0.w, 147, C_STEM1)));
        StemCombineArgs c;
        c.mom = e->mom; c.w0 = P + T.conv0.w; c.dy = grad_src(e, nullptr, 64, nullptr, 64, e->st_stem, 0, a.stem.gamma);      // (neither dy0 nor the stem plane exists here)
        c.HW = e->p_stem.HW; c.ns = NS; c.dw = Gr + T.conv0.w;
        launch_kernel(e, stem_combine_kernel, dim3(64), dim3(256), (size_t)(NS * kMomRows + 256) * sizeof(double), s2, K_OTHER, 0, 0, false, c);
    }
    if (ph_b && !pooled_tail) {
    {   // pool0 / relu0 backward + norm0 sums
        Pool0BwdArgs a;
        a.g1 = grad_src(e, e->G[0], kBlockCtot[0], e->X[0], kBlockCtot[0], e->st_X[0], 0, nullptr); a.p1 = e->p_blk[0];
        a.argmax = e->argmax; a.stem = act_src(e, e->stem, 64, e->st_stem, 0, P + T.norm0.w, P + T.norm0.b); a.ps = e->p_stem;
        a.DY0 = e->DY0; a.st = stat_sink_bwd(e, e->st_stem, 0); a.aff = affine_sink(Gr, T.norm0);
        if (e->p_stem.H % 8 || e->p_stem.W % 8) return fail(-22, "stem plane must tile by 8 (input_size multiple of 16)");
        a.tiles_per_wg = 8;          // 4..20 measure the same; 1 costs 0.7 ms per step in atomics
        const int n_t = (e->p_stem.H / 8) * (e->p_stem.W / 8);
        PREC_DISPATCH(e, launch_kernel(e, pool0_bwd_kernel<PREC>, dim3((n_t + a.tiles_per_wg - 1) / a.tiles_per_wg, NS), dim3(256), 0, st, K_OTHER, 0, 0, false, a));
    }
    {   // conv0 weight gradient (no data gradient: the image needs none)
        const Plane ps_ = e->p_stem;
        int chunk, cps;
        pick_chunk(ps_, NS, 1, chunk, cps);
        auto go = [&](auto ptag, auto mtag) -> int {
        constexpr int SM = decltype(mtag)::value;      // W_STEM (3-channel image, 196 columns) or W_STEM1 (one channel, 49 taps, replicated x3 at the flush)
        using WCfg = typename std::conditional<SM == W_STEM1, CfgW64x64, CfgW64x256>::type;
        BwdWeightP<WCfg, SM, SM == W_STEM1 ? C_STEM1 : C_STEM, kPdWgrad, true, decltype(ptag)::value> p{};      // (fp32 image / stem plane in every mode)
        p.gs = grad_src(e, e->DY0, 64, e->stem, 64, e->st_stem, 0, P + T.norm0.w); p.pa = ps_; p.MA = 64;
        p.bsrc.x = e->img4; p.bsrc.ldx = 4; p.pb = e->p_img; p.NB = SM == W_STEM1 ? 64 : 196;      // (the image: no BN in front of conv0)
        p.chunk = chunk; p.chunks_per_stream = cps; p.n_chunks = NS * cps;
        p.dw = Gr + T.conv0.w; p.ldw_out = 147;
        if (fork(e->ev_misc)) return -5;
        const dim3 grid(1, 1, NS * cps);
        return launch_wgrad(e, s2, p, grid, K_SW, 2.0 * NS * ps_.HW * 64 * 147,
                            4.0 * NS * (2.0 * ps_.HW * 64 + (double)e->p_img.HW * (SM == W_STEM1 ? 1 : 4)), 1, SM == W_STEM1 ? C_STEM1 : C_STEM,
                            tiles, tiles.place_alone(wgrad_partial_floats(p, grid)));
        };
        if (e->f_stem1) { PREC_DISPATCH(e, if (int rc = go(PTAG, std::integral_constant<int, W_STEM1>{})) return rc); }
        else { PREC_DISPATCH(e, if (int rc = go(PTAG, std::integral_constant<int, W_STEM>{})) return rc); }
    }
    }   // ph_b: pool0 + stem
    {   // the trunk's dbeta / dgamma: replicas -> gradient array (and zeroed for the next call).  Each half flushes ONLY the segments
        // it produced - the table holds dense block 1's 2 x 6 segments first, then blocks 2-4 and the transitions - because the
        // flush is a non-atomic read-modify-write of the gradient array: between the halves of a two-phase backward the ranges
        // [trunk split, end) + head are being all-reduced IN PLACE on another stream (parallel.OverlappedGradSync), and the second
        // half must not touch a single element of them (it would re-write a stale local value over the reduced one).
        const int first_b = 2 * kBlockLayers[0];
        const int seg0 = ph_b ? 0 : first_b, seg1 = ph_a ? e->n_dbseg : first_b;
        const GradSrc dy0 = grad_src(e, nullptr, 64, nullptr, 64, e->st_stem, 0, nullptr);      // norm0's sums: the statistics side alone
        launch_kernel(e, db_flush_kernel, dim3(4, seg1 - seg0 + 1), dim3(256), 0, st, K_OTHER, 0, 0, false,
                      reinterpret_cast<const DbSegD*>(e->d_dbseg + (size_t)e->f_trunk * e->n_dbseg) + seg0,
                      e->dbscr, e->db_total, kDbRep, Gr,
                      ph_b ? dy0.s1 : nullptr, ph_b ? dy0.s2 : nullptr, NS, Gr + T.norm0.b, Gr + T.norm0.w);
    }
    launch_reduce2(e, s2, tiles.drain());
    HIP_OK(hipEventRecord(e->ev_end, s2));          // join: everything after the backward (or this half of it) sees every gradient
    HIP_OK(hipStreamWaitEvent(st, e->ev_end, 0));
    if (int rc = walk_status(e)) return rc;
    e->bw_phase0_done = phases == 1;
    return 0;
}

