// host_sketch.inl -- part of lrge_hip.hip (one translation unit; included there, in this order): the sketch driver and the presketch of a streamed set on the side stream.  The driver: SketchReq (what is asked for), sk_entry_dispatch (entry kind -> kernel instantiation), GateWalk (the gates of an upload in flight), SketchRun (one function per form: wave, ranged, one_pass, two_pass_count, finish), sketch_launch (the order the forms are tried in), sketch_device (the entry point: decides `gated`).
// ------------------------------------------------------------------------------------------
// sketch driver
// ------------------------------------------------------------------------------------------
struct SketchOut {
    u64 *x = nullptr, *y = nullptr;   // pool memory (owned by the caller's Scratch)
    u32 *mz_off = nullptr;            // [n+1] per-read offsets
    u64 n = 0;
    // keep_slots (packed index entries, one-pass form): x stays null -- the entries still sit in the per-chunk slots of k_sketch_direct
    // (chunk c at slots[c * SK_CAP ...), offs[] = exclusive scan of the per-chunk counts) and the index sort's first pass reads them there
    u64 *slots = nullptr; u32 *offs = nullptr; u32 n_chunks = 0;
    bool segw = false;                // y holds a u32 ARRAY: SEGW entries (k_sketch.h, sketch_write_chunk PK == 2): x = word, y[i] = the two sort digits
    // wave-dense form (k_sketch.h: k_sketch_wave; SEGW entries only): x / y stay null -- wavefront v's entries sit, densely and in emission order,
    // at wave_x / wave_d [v * wave_cap ...), wave_cnt[v] of them; the index sort's first pass reads them there (k_prims.h: index_sort_seg, WaveSrc)
    u64 *wave_x = nullptr; u32 *wave_d = nullptr; u32 *wave_cnt = nullptr, *wave_offs = nullptr; u32 n_waves = 0, wave_cap = 0;      // wave_offs: exclusive scan of wave_cnt
};

// What the sketch is asked for.  An entry is one of four things (k_sketch.h): the (hash << 8 | span, y) pair of a query, the (hash, y) pair
// of an index, the packed 8-byte word of an index (pk_pos1 / pk_ybits: where read id and hash sit), or the SEGW word + digit pair.
enum class SkEntry { QUERY_PAIRS, INDEX_PAIRS, PACKED, SEGW };
struct SketchReq {
    SkEntry entry = SkEntry::QUERY_PAIRS;
    u32 pk_pos1 = 0, pk_ybits = 0;
    std::vector<u32> *h_mzoff = nullptr;          // the per-read offsets on the host as well (cleared by the wave-dense form, which has none)
    bool gated = false;                           // set by sketch_device: nobody has waited for the set's upload (seqset_ready) yet
    bool keep_slots = false;                      // PACKED: leave the entries in the per-chunk slots for the sort (SketchOut::slots)
    bool wave_ok = false;                         // the caller's sort reads the wave-dense form (SketchOut::wave_x)
};
static SkEntry sk_index_entry(u32 pk_ybits, bool segw) { return segw ? SkEntry::SEGW : pk_ybits ? SkEntry::PACKED : SkEntry::INDEX_PAIRS; }

// The one place that turns "what an entry is" into the template arguments (INDEX_KEYS, PK) of the sketch kernels: f(std::bool_constant, std::integral_constant<int>)
template <typename F>
static void sk_entry_dispatch(SkEntry e, F &&f) {
    if (e == SkEntry::QUERY_PAIRS) f(std::false_type{}, std::integral_constant<int, 0>{});
    else if (e == SkEntry::INDEX_PAIRS) f(std::true_type{}, std::integral_constant<int, 0>{});
    else if (e == SkEntry::PACKED) f(std::true_type{}, std::integral_constant<int, 1>{});
    else f(std::true_type{}, std::integral_constant<int, 2>{});
}
// k_sketch_compact over chunks [c0, c1) of slots indexed by chunk number; parts = SKC_X_ONLY / SKC_XY / SKC_X_U32
static int sk_compact_parts(SkEntry e) { return e == SkEntry::PACKED ? SKC_X_ONLY : e == SkEntry::SEGW ? SKC_X_U32 : SKC_XY; }
static void sketch_compact_launch(lrge_hip_ctx *ctx, int parts, const u64 *tx, const u64 *ty, const u32 *offs, const u32 *d_total, u32 c0, u32 c1,
                                  u64 *dx, u64 *dy, u32 out_cap = 0xFFFFFFFFu, u32 *ovf = nullptr) {
    const dim3 cgrid((u32)div_up(div_up(c1 - c0, 64), 4));
    if (parts == SKC_X_ONLY) hipLaunchKernelGGL(k_sketch_compact<SKC_X_ONLY>, cgrid, dim3(256), 0, ctx->stream, tx, ty, offs, d_total, c1, dx, dy, c0, out_cap, ovf);
    else if (parts == SKC_X_U32) hipLaunchKernelGGL(k_sketch_compact<SKC_X_U32>, cgrid, dim3(256), 0, ctx->stream, tx, ty, offs, d_total, c1, dx, dy, c0, out_cap, ovf);
    else hipLaunchKernelGGL(k_sketch_compact<SKC_XY>, cgrid, dim3(256), 0, ctx->stream, tx, ty, offs, d_total, c1, dx, dy, c0, out_cap, ovf);
}
// Do per-chunk slots of slot_bytes in all fit comfortably -- in a quarter of what the device and the pool have free?  (*mfree: what the device reports)
static bool sketch_slots_fit(lrge_hip_ctx *ctx, u64 slot_bytes, size_t *mfree = nullptr) {
    size_t mf = (size_t)64 << 30, mtot = 0;
    if (slot_bytes > ((u64)4 << 30)) (void)hipMemGetInfo(&mf, &mtot);       // (small sets: no need to ask)
    if (mfree) *mfree = mf;
    return slot_bytes < ((u64)mf + ctx->pool.idle()) / 4;
}
// entries a chunk's slot takes (option DEBUG_SK_CAP, tests: force the overflow fallback)
static u32 sketch_slot_cap(const lrge_hip_ctx *ctx) { const char *v = ctx->opt("DEBUG_SK_CAP"); return v ? (u32)std::min<u64>(strtoull(v, nullptr, 10), SK_CAP) : (u32)SK_CAP; }

// The walk over the gates of an upload that is still in flight (host-side pack, chunk after chunk: host_pack.h): gate j covers the words
// [.., gate_w1[j]) of the set's root, and the sketch chunks that lie wholly inside them may run behind it.
struct GateWalk {
    lrge_hip_ctx *ctx; const lrge_hip_seqset *s; u32 n_chunks; bool hpc, tile_form;
    std::shared_ptr<UploadJob> job;       // the job whose gates cover this set's words (a view: its root's); null: nothing to walk
    size_t g = 0;                         // gate cursor of wait_chunks
    GateWalk(lrge_hip_ctx *ctx_, const lrge_hip_seqset *s_, u32 n_chunks_, bool hpc_, bool tile_form_, bool gated)
        : ctx(ctx_), s(s_), n_chunks(n_chunks_), hpc(hpc_), tile_form(tile_form_) {
        if (!gated) return;
        const lrge_hip_seqset *root = s->is_view ? s->view_root : s;
        job = s->is_view ? s->view_job : s->job;
        if (!job || !root || root->job != job || job->gate_ev.empty()) job.reset();
    }
    // how far the sketch may go once the words [.., w1) (absolute offset) have arrived: every chunk that lies wholly inside them -- with HPC
    // only the chunks of reads that have arrived WHOLLY (a homopolymer-compressed step may run past its chunk, to the end of the read at most)
    u32 chunks_behind(u64 w1) const {
        if (w1 >= s->h_woff[s->n]) return n_chunks;
        if (w1 <= s->h_woff[0]) return 0;
        const u32 r = (u32)(std::upper_bound(s->h_woff.begin(), s->h_woff.end(), w1) - s->h_woff.begin()) - 1;
        if (hpc) return s->h_cs[r];
        u64 avail = w1 - s->h_woff[r];                            // words of read r that have arrived: 4 per 128-base chunk
        if (tile_form && avail) --avail;                          // (the tile form looks w steps past a chunk's end: one word more)
        return s->h_cs[r] + (u32)std::min<u64>(avail / (SK_CHUNK / 32), (u64)(s->h_cs[r + 1] - s->h_cs[r]));
    }
    // For each gate in turn: waits for it (on the host until its transfer has been queued, then on the device) and calls launch(c0, c1) for
    // the chunks that have arrived with it, c1 rounded down to a multiple of `align` unless it is the end.  *c_done: chunks [0, *c_done)
    // have been launched.  A failed job ends the walk early: the caller's seqset_ready reports it.
    template <typename F>
    int walk(u32 align, u32 *c_done, F &&launch) {
        *c_done = 0;
        for (size_t j = 0, ng = job ? job->gate_w1.size() : 0; j < ng && *c_done < n_chunks; ++j) {
            u32 c_end = chunks_behind(job->gate_w1[j]);
            if (c_end < n_chunks) c_end = c_end / align * align;
            if (c_end <= *c_done) continue;                                  // (a gate in front of this view, or inside one long read)
            if (!job->wait_gate((int)j)) break;
            HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, job->gate_ev[j], 0));
            launch(*c_done, c_end);
            KCHK(ctx);
            *c_done = c_end;
        }
        return LRGE_OK;
    }
    // waits for the first gate behind which chunks [.., c1) may be sketched; LRGE_ERR_DEVICE: the upload failed
    int wait_chunks(u32 c1) {
        if (!job) return LRGE_OK;
        size_t j = g;
        while (j + 1 < job->gate_w1.size() && chunks_behind(job->gate_w1[j]) < c1) ++j;
        if (!job->wait_gate((int)j)) return LRGE_ERR_DEVICE;       // (the job failed: seqset_ready reports it)
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, job->gate_ev[j], 0));
        g = j;
        return LRGE_OK;
    }
};

// One sketch of one set: the state the forms share, and one function per form.  A form function sets *done when the output is in `o`;
// otherwise the driver (sketch_launch) goes on to the next form.
template <int K, int W, bool HPC>
struct SketchRun {
    lrge_hip_ctx *ctx; Scratch &sc; const lrge_hip_seqset *s; SketchReq rq; SketchOut *o;
    u32 n_chunks; bool tile_form, pk, segw;
    u64 ebytes;                          // bytes per entry in the slots and in the output
    GateWalk gw; ChunkMap cm;
    u32 *d_cnt = nullptr, *d_total = nullptr, *d_mzoff = nullptr;       // per-chunk counts / offsets; [0] total, [1] overflow flag; per-read offsets
    // Option SKETCH_TILE_FORM: k_sketch_tile (k_sketch_tile.h: a lane per step, a workgroup per 16 chunks; + k_sketch_direct<REDO> for the HPC
    // tiles it marks) in place of k_sketch_direct (a lane per chunk) in the slot forms, into the same per-chunk slots.  Exact, and NOT the
    // default: measured at full-size C5 it is slower with HPC (index sketch 286 against 198 ms) and equal without.
    SketchRun(lrge_hip_ctx *ctx_, Scratch &sc_, const lrge_hip_seqset *s_, const SketchReq &rq_, SketchOut *o_)
        : ctx(ctx_), sc(sc_), s(s_), rq(rq_), o(o_), n_chunks((u32)s_->n_chunks),
          tile_form(ctx_->opt("SKETCH_TILE_FORM") != nullptr && rq_.entry != SkEntry::SEGW),      // (the tile form writes pairs or packed words only)
          pk(rq_.entry == SkEntry::PACKED), segw(rq_.entry == SkEntry::SEGW), ebytes(pk ? 8 : segw ? 12 : 16),
          gw(ctx_, s_, (u32)s_->n_chunks, HPC, tile_form, rq_.gated), cm{s_->d_cs, s_->n} {}
    u64 *get_y(size_t n_) { return segw ? (u64 *)sc.get<u32>(n_) : sc.get<u64>(n_); }      // the second member's array
    // the upload must be over from here on (a gated request that has not waited yet); nothing is left to walk behind it
    int ready() { if (!rq.gated) return LRGE_OK; rq.gated = false; gw.job.reset(); return seqset_ready(ctx, s); }

    // chunks [c0, c1) into the slots sx / sy (indexed by chunk number), counts to d_cnt, overflow flag at d_total + 1
    void launch_slots(u32 c0, u32 c1, u64 *sx, u64 *sy, u32 capv) {
        if (c1 <= c0) return;
        const dim3 gl((u32)div_up(c1 - c0, SK_THREADS)), gt((u32)div_up(c1 - c0, ST_G));
        StageTimer tk(ctx, LRGE_T_K_SKETCH);             // (timer level 2: the bench's roofline candidates)
        if (!tile_form) ctx->counters[LRGE_C_SKETCH_LAUNCHES] += 1;
        sk_entry_dispatch(rq.entry, [&](auto ik, auto pkc) {
            constexpr bool IK = decltype(ik)::value; constexpr int PK = decltype(pkc)::value;
            if constexpr (PK != 2) {
                if (tile_form) {
                    hipLaunchKernelGGL((k_sketch_tile<K, W, HPC, IK, PK != 0>), gt, dim3(ST_THREADS), 0, ctx->stream, s->d_pack, s->d_nmask, s->d_woff,
                                       s->d_len, cm, c1, d_cnt, d_total + 1, sx, sy, rq.pk_pos1, rq.pk_ybits, capv, c0);
                    if constexpr (HPC)
                        hipLaunchKernelGGL((k_sketch_direct<K, W, HPC, IK, PK, true>), gl, dim3(SK_THREADS), 0, ctx->stream, s->d_pack, s->d_nmask, s->d_woff,
                                           s->d_len, cm, c1, d_cnt, d_total + 1, sx, sy, rq.pk_pos1, rq.pk_ybits, capv, c0);
                    return;
                }
            }
            hipLaunchKernelGGL((k_sketch_direct<K, W, HPC, IK, PK>), gl, dim3(SK_THREADS), 0, ctx->stream, s->d_pack, s->d_nmask, s->d_woff,
                               s->d_len, cm, c1, d_cnt, d_total + 1, sx, sy, rq.pk_pos1, rq.pk_ybits, capv, c0);
        });
    }

    // ---- wave-dense form (round 6): index entries (SEGW, or packed words for the sort that reads slots) written densely per wavefront, no
    // compaction; see k_sketch_wave.  Behind the gates of an upload in flight, the wavefronts whose 64 chunks have arrived run gate by gate ----
    // (option NO_WAVE_SKETCH: the slot-per-chunk forms, rounds 2-5; WAVE_CAP: entries of room per wavefront, a multiple of 64, <= RS_TILE)
    int wave(bool *done) {
        if (!(rq.wave_ok && (segw || (pk && rq.keep_slots)) && n_chunks && !tile_form && !ctx->opt("DEBUG_SK_CAP") && !ctx->opt("NO_WAVE_SKETCH") &&
              !ctx->opt("SKETCH_TWO_PASS") && !ctx->opt("DEBUG_SK_RANGE_CHUNKS"))) return LRGE_OK;
        const u32 n_waves = (u32)div_up(n_chunks, 64);
        u32 capw = (u32)ctx->opt_u64("WAVE_CAP", HPC ? 2560 : 3328);
        capw = std::max<u32>(64, capw / 64 * 64);
        u64 *wx = sc.get<u64>((size_t)n_waves * capw + 8);
        u32 *wd = (wx && segw) ? sc.get<u32>((size_t)n_waves * capw + 8) : nullptr;      // (packed 8-byte entries have no digit member)
        u32 *wcnt = (wx && (wd || !segw)) ? sc.get<u32>((size_t)n_waves + 1) : nullptr, *woffs = wcnt ? sc.get<u32>((size_t)n_waves + 1) : nullptr;
        if (!(wx && (wd || !segw) && wcnt && woffs)) {
            if (wx) sc.drop(wx); if (wd) sc.drop(wd); if (wcnt) sc.drop(wcnt); if (woffs) sc.drop(woffs);
            (void)hipGetLastError(); ctx->err.clear();
            return LRGE_OK;
        }
        HIPCHK(ctx, hipMemsetAsync(d_total, 0, 8, ctx->stream));
        auto launch_wave = [&](u32 c0, u32 c1) {           // chunks [c0, c1), c0 a multiple of 64
            if (c1 <= c0) return;
            StageTimer tk(ctx, LRGE_T_K_SKETCH);
            ctx->counters[LRGE_C_SKETCH_WAVE_LAUNCHES] += 1;
            if (segw) hipLaunchKernelGGL((k_sketch_wave<K, W, HPC, 2>), dim3((u32)div_up(c1 - c0, SK_THREADS)), dim3(SK_THREADS), 0, ctx->stream, s->d_pack, s->d_nmask, s->d_woff,
                                         s->d_len, cm, c1, wcnt, d_total + 1, wx, wd, rq.pk_pos1, rq.pk_ybits, capw, c0);
            else hipLaunchKernelGGL((k_sketch_wave<K, W, HPC, 1>), dim3((u32)div_up(c1 - c0, SK_THREADS)), dim3(SK_THREADS), 0, ctx->stream, s->d_pack, s->d_nmask, s->d_woff,
                                    s->d_len, cm, c1, wcnt, d_total + 1, wx, (u32 *)nullptr, rq.pk_pos1, rq.pk_ybits, capw, c0);
        };
        u32 c_done = 0;
        int rc = gw.walk(64, &c_done, launch_wave); if (rc) return rc;
        rc = ready(); if (rc) return rc;
        launch_wave(c_done, n_chunks);
        KCHK(ctx);
        rc = scan_exclusive_u32(ctx, sc, wcnt, woffs, n_waves, d_total);
        if (rc) return rc;
        u32 tot_ovf[2] = {0, 0};
        HIPCHK(ctx, ctx->d2h(tot_ovf, d_total, 8, ctx->stream));
        HIPCHK(ctx, ctx->d2h_sync(ctx->stream));
        if (tot_ovf[1]) {          // a wavefront found more than its slot holds: the slot-per-chunk forms
            sc.drop(wx); if (wd) sc.drop(wd); sc.drop(wcnt); sc.drop(woffs);
            return LRGE_OK;
        }
        if (rq.h_mzoff) rq.h_mzoff->clear();
        sc.drop(d_cnt); sc.drop(d_total); sc.drop(d_mzoff);
        o->x = nullptr; o->y = nullptr; o->mz_off = nullptr; o->n = tot_ovf[0]; o->segw = segw;
        o->wave_x = wx; o->wave_d = wd; o->wave_cnt = wcnt; o->wave_offs = woffs; o->n_waves = n_waves; o->wave_cap = capw;
        *done = true;
        return LRGE_OK;
    }

    // ---- ranged one-pass form: the slots of the whole set do not fit, those of a range of its chunks do ----
    // Range after range: k_sketch_direct into the SAME slots, scan of the range's counts, compaction behind what the ranges before
    // left.  The output is sized by an estimate (the count is only known at the end); a set that beats the estimate, or a chunk
    // that overflows its slot, starts over in the two-pass form.  Full-size C5: index sketch of a 10-Gbase part and the
    // streamed views of the inverse strategy (two passes: 8.3 ps per base; one pass + compaction: 7.3).  Behind the gates of an upload
    // in flight every range waits for the gate that covers it.
    int ranged(size_t mfree, bool *done) {
        if (!n_chunks || ctx->opt("SKETCH_TWO_PASS") || ctx->opt("NO_RANGED_SKETCH") || ctx->opt("DEBUG_SK_CAP")) return LRGE_OK;
        const u64 per_chunk = (u64)SK_CAP * ebytes;
        const u64 avail = (u64)mfree + ctx->pool.idle();
        u64 R = std::min<u64>(avail / 8, (u64)24 << 30) / per_chunk / 256 * 256;
        R = ctx->opt_u64("DEBUG_SK_RANGE_CHUNKS", R);
        const u64 est = std::min<u64>((u64)s->total_bases + 1, (u64)((double)s->total_bases * 0.40) + 65536);
        if (!(R >= 256 && R < n_chunks && est < (1ULL << 32) && est * ebytes < avail / 2)) return LRGE_OK;
        if (!gw.job) { int rr = ready(); if (rr) return rr; }
        u64 *rx = sc.get<u64>((size_t)R * SK_CAP), *ry = pk ? nullptr : get_y((size_t)R * SK_CAP);
        u64 *dx = sc.get<u64>((size_t)est + 1), *dy = pk ? nullptr : get_y((size_t)est + 1);
        u32 *d_run = sc.get<u32>(2);                  // [0] output offset behind the ranges done, [1] the current range's count
        if (!(rx && (pk || ry) && dx && (pk || dy) && d_run)) {
            if (rx) sc.drop(rx); if (ry) sc.drop(ry); if (dx) sc.drop(dx); if (dy) sc.drop(dy); if (d_run) sc.drop(d_run);
            (void)hipGetLastError(); ctx->err.clear();
            return LRGE_OK;
        }
        HIPCHK(ctx, hipMemsetAsync(d_total, 0, 8, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_run, 0, 8, ctx->stream));
        for (u64 c0 = 0; c0 < n_chunks; c0 += R) {
            const u32 c1 = (u32)std::min<u64>(c0 + R, n_chunks), len = c1 - (u32)c0;
            if (gw.wait_chunks(c1) != LRGE_OK) { int rr = seqset_ready(ctx, s); return rr ? rr : LRGE_ERR_DEVICE; }   // this range's reads have arrived; the later ones may still travel
            u64 *sx = rx - c0 * SK_CAP, *sy = !ry ? nullptr : segw ? (u64 *)((u32 *)ry - c0 * SK_CAP) : ry - c0 * SK_CAP;      // (the kernels index slots by chunk number)
            launch_slots((u32)c0, c1, sx, sy, (u32)SK_CAP);
            KCHK(ctx);
            int rc = scan_exclusive_u32(ctx, sc, d_cnt + c0, d_cnt + c0, len, d_run + 1);
            if (rc) return rc;
            hipLaunchKernelGGL(k_add_base_u32, dim3((u32)div_up(len, 256)), dim3(256), 0, ctx->stream, d_cnt + c0, len, d_run);
            hipLaunchKernelGGL(k_bump_u32, dim3(1), dim3(1), 0, ctx->stream, d_run, d_run + 1, d_total + 1);
            KCHK(ctx);
            sketch_compact_launch(ctx, sk_compact_parts(rq.entry), sx, sy, d_cnt, d_run, (u32)c0, c1, dx, dy, (u32)est, d_total + 1);
            KCHK(ctx);
        }
        int rr = ready(); if (rr) return rr;
        hipLaunchKernelGGL(k_read_mz_offsets, dim3((u32)div_up((u64)s->n + 1, 256)), dim3(256), 0, ctx->stream, s->d_cs, d_cnt, s->n, n_chunks, d_run, d_mzoff);
        KCHK(ctx);
        u32 h_run = 0, h_ovf = 0;
        HIPCHK(ctx, ctx->d2h(&h_run, d_run, 4, ctx->stream));
        HIPCHK(ctx, ctx->d2h(&h_ovf, d_total + 1, 4, ctx->stream));
        int rc = fetch_mzoff(); if (rc) return rc;
        sc.drop(rx); if (ry) sc.drop(ry); sc.drop(d_run);
        if (h_ovf) { sc.drop(dx); if (dy) sc.drop(dy); return LRGE_OK; }          // beat the estimate, or a chunk overflowed its slot: two passes
        sc.drop(d_cnt); sc.drop(d_total);
        o->x = dx; o->y = dy; o->mz_off = d_mzoff; o->n = h_run; o->segw = segw;
        *done = true;
        return LRGE_OK;
    }
    // the per-read offsets to the host (if asked for) behind whatever else the caller has queued for it, and the one sync
    int fetch_mzoff() {
        if (rq.h_mzoff) {
            rq.h_mzoff->resize((size_t)s->n + 1);
            HIPCHK(ctx, ctx->d2h(rq.h_mzoff->data(), d_mzoff, ((size_t)s->n + 1) * 4, ctx->stream));
        }
        HIPCHK(ctx, ctx->d2h_sync(ctx->stream));
        return LRGE_OK;
    }
    // What the one-pass and the two-pass form share: chunk offsets from the counts; the per-read offsets follow from the chunk scan alone
    // and travel to the host with the total and the overflow flag, in the one sync
    int offsets_and_total(u32 tot_ovf[2]) {
        if (n_chunks) { int rc = scan_exclusive_u32(ctx, sc, d_cnt, d_cnt, n_chunks, d_total); if (rc) return rc; }
        hipLaunchKernelGGL(k_read_mz_offsets, dim3((u32)div_up((u64)s->n + 1, 256)), dim3(256), 0, ctx->stream, s->d_cs, d_cnt, s->n,
                           n_chunks, d_total, d_mzoff);
        KCHK(ctx);
        HIPCHK(ctx, ctx->d2h(tot_ovf, d_total, 8, ctx->stream));
        return fetch_mzoff();
    }
    // ---- one pass: k_sketch_direct into the per-chunk slots tx / ty of the whole set.  An upload still in flight (host-side pack, chunk
    // after chunk): the sketch chunks that lie wholly inside the words of upload chunk j run behind gate j, while the later chunks are
    // still being packed and sent.  tot_ovf[1]: a chunk held more than its slot ----
    int one_pass(u64 *tx, u64 *ty, u32 sk_cap, u32 tot_ovf[2]) {
        HIPCHK(ctx, hipMemsetAsync(d_total, 0, 8, ctx->stream));
        u32 c_done = 0;
        int rr = gw.walk(1, &c_done, [&](u32 c0, u32 c1) { launch_slots(c0, c1, tx, ty, sk_cap); }); if (rr) return rr;
        rr = ready(); if (rr) return rr;
        launch_slots(c_done, n_chunks, tx, ty, sk_cap);              // (everything, or whatever a failed / odd gate sequence left)
        KCHK(ctx);
        return offsets_and_total(tot_ovf);
    }
    // ---- two passes, first half: k_sketch_count (k_sketch_write follows in finish, once the output is allocated) ----
    int two_pass_count(u32 tot_ovf[2]) {
        HIPCHK(ctx, hipMemsetAsync(d_total, 0, 8, ctx->stream));
        if (n_chunks) {
            int rr = ready(); if (rr) return rr;
            hipLaunchKernelGGL((k_sketch_count<K, W, HPC>), dim3((u32)div_up(n_chunks, SK_THREADS)), dim3(SK_THREADS), 0, ctx->stream, s->d_pack, s->d_nmask,
                               s->d_woff, s->d_len, cm, n_chunks, d_cnt);
            KCHK(ctx);
        }
        return offsets_and_total(tot_ovf);
    }
    // The dense output of `total` entries: compacted out of the slots tx / ty (one pass), or written by k_sketch_write (two passes: tx null)
    int finish(u64 *tx, u64 *ty, u32 sk_cap, u32 total) {
        if (rq.keep_slots && pk && tx && n_chunks && sk_cap == (u32)SK_CAP) {
            // no compaction: the caller's sort reads the slots (k_prims.h: radix_sort_keys_first_pass_from_slots)
            sc.drop(d_total);
            o->x = nullptr; o->y = nullptr; o->mz_off = d_mzoff; o->n = total;
            o->slots = tx; o->offs = d_cnt; o->n_chunks = n_chunks;
            return LRGE_OK;
        }
        ALLOC_OR_FAIL(dx, sc, u64, (size_t)total + 1);
        u64 *dy = nullptr;
        if (!pk) { dy = get_y((size_t)total + 1); if (!dy) return LRGE_ERR_DEVICE; }
        if (n_chunks && tx) {
            sketch_compact_launch(ctx, sk_compact_parts(rq.entry), tx, ty, d_cnt, d_total, 0u, n_chunks, dx, dy);
            KCHK(ctx);
            sc.drop(tx); if (ty) sc.drop(ty);
        } else if (n_chunks) {
            sk_entry_dispatch(rq.entry, [&](auto ik, auto pkc) {
                hipLaunchKernelGGL((k_sketch_write<K, W, HPC, decltype(ik)::value, decltype(pkc)::value>), dim3((u32)div_up(n_chunks, SK_THREADS)), dim3(SK_THREADS), 0,
                                   ctx->stream, s->d_pack, s->d_nmask, s->d_woff, s->d_len, cm, n_chunks, d_cnt, dx, dy, rq.pk_pos1, rq.pk_ybits);
            });
            KCHK(ctx);
        }
        // (no sync: everything runs in order on ctx->stream; scratch is recycled in stream order)
        sc.drop(d_cnt); sc.drop(d_total);
        o->x = dx; o->y = dy; o->mz_off = d_mzoff; o->n = total; o->segw = segw;
        return LRGE_OK;
    }
};

// The forms in the order they are tried: wave-dense; then, with per-chunk slots, one pass when the slots of the whole set fit comfortably
// (the ranged form first when they do not); then two passes (count, scan, write) -- on request, when nothing else fits, or after a chunk
// overflowed its slot.  rq.gated: the caller has NOT waited for the set's upload (seqset_ready): the forms do, as late as they can --
// chunk range by chunk range behind the upload's gates where the form allows it.
template <int K, int W, bool HPC>
static int sketch_launch(lrge_hip_ctx *ctx, Scratch &sc, const lrge_hip_seqset *s, const SketchReq &rq, SketchOut *o) {
    if (s->n_chunks >= (1ULL << 32)) { LRGE_SET_ERR(ctx, "read set too large for one sketch launch"); return LRGE_ERR_TOO_MANY; }
    SketchRun<K, W, HPC> R(ctx, sc, s, rq, o);
    const u32 n_chunks = R.n_chunks;
    ALLOC_OR_FAIL(d_cnt, sc, u32, (size_t)n_chunks + 1);
    ALLOC_OR_FAIL(d_total, sc, u32, 2);
    ALLOC_OR_FAIL(d_mzoff, sc, u32, (size_t)s->n + 1);
    R.d_cnt = d_cnt; R.d_total = d_total; R.d_mzoff = d_mzoff;
    bool done = false;
    int rc = R.wave(&done);
    if (rc || done) return rc;
    size_t mfree = 0;
    const bool fit = sketch_slots_fit(ctx, (u64)n_chunks * SK_CAP * R.ebytes, &mfree);
    bool one_pass = n_chunks && !ctx->opt("SKETCH_TWO_PASS") && fit && !ctx->opt("DEBUG_SK_RANGE_CHUNKS");   // (tests: the ranged form)
    const u32 sk_cap = sketch_slot_cap(ctx);
    u64 *tx = nullptr, *ty = nullptr;
    if (one_pass) {
        tx = sc.get<u64>((size_t)n_chunks * SK_CAP);
        ty = R.pk ? nullptr : R.get_y((size_t)n_chunks * SK_CAP);
        if (!tx || (!R.pk && !ty)) { if (tx) sc.drop(tx); if (ty) sc.drop(ty); tx = ty = nullptr; one_pass = false; (void)hipGetLastError(); }
    }
    if (!one_pass) { rc = R.ranged(mfree, &done); if (rc || done) return rc; }
    u32 tot_ovf[2] = {0, 0};
    if (one_pass) {
        rc = R.one_pass(tx, ty, sk_cap, tot_ovf); if (rc) return rc;
        if (tot_ovf[1]) { sc.drop(tx); if (ty) sc.drop(ty); tx = ty = nullptr; one_pass = false; }      // a chunk held more than SK_CAP minimizers: redo in two passes
    }
    if (!one_pass) { rc = R.two_pass_count(tot_ovf); if (rc) return rc; }
    return R.finish(tx, ty, sk_cap, tot_ovf[0]);
}

// A set whose host-side pack is still running on the uploader thread (chunk gates: host_pack.h) is sketched chunk by chunk
// behind its transfer -- index sketches only (a streamed set's upload hides behind the index build anyway).  Since round 4 also
// VIEWS of such a set (the parts of a partitioned index: part 0 is sketched, sorted and tabled while parts 1.. still travel)
// and the HPC preset (whole reads only: an HPC step may read a homopolymer run past its chunk).  option NO_GATED_SKETCH: wait first.
static int sketch_device(lrge_hip_ctx *ctx, Scratch &sc, const lrge_hip_seqset *s, int preset, SketchReq rq, SketchOut *o) {
    const lrge_hip_seqset *root_ = s->is_view ? s->view_root : s;
    const std::shared_ptr<UploadJob> &job_ = s->is_view ? s->view_job : s->job;
    rq.gated = rq.entry != SkEntry::QUERY_PAIRS && root_ && root_->pending && job_ && root_->job == job_ && !job_->gate_ev.empty() && s->n_words != 0 &&
               (!s->is_view || s->view_gate >= 0) && !ctx->opt("NO_GATED_SKETCH") && s->n_chunks != 0 && s->n_chunks < (1ULL << 32);
    int rc = rq.gated ? LRGE_OK : seqset_ready(ctx, s);
    if (rc) return rc;
    StageTimer t(ctx, LRGE_T_SKETCH);
    rc = (preset == LRGE_PRESET_AVA_PB) ? sketch_launch<19, 5, true>(ctx, sc, s, rq, o) : sketch_launch<15, 5, false>(ctx, sc, s, rq, o);
    t.stop();
    return rc;
}

// ---- presketch: the streamed set's minimizers, computed on the side stream with no host round trip ----
// Two steps, because the device arena recycles blocks in the order of the MAIN stream: everything the side stream will touch
// is allocated where it forks (presketch_prepare: nothing released by the index build after that point can be handed to it),
// the kernels may be queued later (presketch_launch_prepared).
static int presketch_alloc(lrge_hip_ctx *ctx, const lrge_hip_seqset *s, PreSketch *p) {
    if (s->n_chunks >= (1ULL << 32) || s->total_bases + 1 >= (1ULL << 32)) return LRGE_ERR_TOO_MANY;
    Scratch &sc = *p->sc;
    const u64 nb = div_up(s->n_chunks, SCAN_TILE);
    if (nb > 8192) return LRGE_ERR_TOO_MANY;                   // (single-level scan with the caller's block sums)
    ALLOC_OR_FAIL(d_cnt, sc, u32, (size_t)s->n_chunks + 1);
    ALLOC_OR_FAIL(d_bs, sc, u32, (size_t)nb + 2);
    ALLOC_OR_FAIL(d_total, sc, u32, 1);
    ALLOC_OR_FAIL(d_mzoff, sc, u32, (size_t)s->n + 1);
    // the count is not known on the host when the write pass is queued: room for one minimizer per base
    ALLOC_OR_FAIL(dx, sc, u64, (size_t)s->total_bases + 1);
    ALLOC_OR_FAIL(dy, sc, u64, (size_t)s->total_bases + 1);
    p->cnt = d_cnt; p->bs = d_bs; p->x = dx; p->y = dy; p->mz_off = d_mzoff; p->d_total = d_total;
    return LRGE_OK;
}

template <int K, int W, bool HPC>
static int presketch_launch(lrge_hip_ctx *ctx, const lrge_hip_seqset *s, PreSketch *p, hipStream_t st) {
    Scratch &sc = *p->sc;
    const u32 n_chunks = (u32)s->n_chunks;
    ChunkMap cm{s->d_cs, s->n};
    const dim3 sgrid((u32)div_up(n_chunks, SK_THREADS));
    // Two passes here, not the one-pass form of sketch_launch: beside the index's memory-bound passes a second VALU-bound pass
    // overlaps where the one-pass form's streaming compaction competes.  Measured twice: beside the sort passes (round 2: the sort
    // loses what the sketch gains) and beside the table build, where this runs now (round 3: C4 step 32.7-32.8 ms with two passes,
    // 33.1-33.4 with slots + compaction on the same box).
    if (n_chunks) {
        hipLaunchKernelGGL((k_sketch_count<K, W, HPC>), sgrid, dim3(SK_THREADS), 0, st, s->d_pack, s->d_nmask, s->d_woff, s->d_len, cm, n_chunks, p->cnt);
        KCHK(ctx);
        int rc = scan_exclusive_u32(ctx, sc, p->cnt, p->cnt, n_chunks, p->d_total, st, true, p->bs);
        if (rc) return rc;
    } else {
        HIPCHK(ctx, hipMemsetAsync(p->d_total, 0, 4, st));
    }
    hipLaunchKernelGGL(k_read_mz_offsets, dim3((u32)div_up((u64)s->n + 1, 256)), dim3(256), 0, st, s->d_cs, p->cnt, s->n, n_chunks, p->d_total,
                       p->mz_off);
    KCHK(ctx);
    if (n_chunks) {
        hipLaunchKernelGGL((k_sketch_write<K, W, HPC, false, false>), sgrid, dim3(SK_THREADS), 0, st, s->d_pack, s->d_nmask, s->d_woff, s->d_len, cm,
                           n_chunks, p->cnt, p->x, p->y, 0u, 0u);
        KCHK(ctx);
    }
    return LRGE_OK;
}

static void presketch_drop_prepared(lrge_hip_ctx *ctx) {
    PreSketch *p = ctx->presk_prepared;
    if (!p) return;
    ctx->presk_prepared = nullptr; ctx->presk_prepared_set = nullptr;
    delete p->sc;                                        // (nothing has been queued on these blocks)
    ctx->event_pool.push_back(p->ev_start); ctx->event_pool.push_back(p->ev_done);
    delete p;
}

// Called by the index build right after its own sketch has been queued on ctx->stream: marks the point of the main stream
// the side stream starts from and takes the memory of the streamed set's sketch.
// indexed_bases: size of the set whose index build would hide the sketch.  A streamed set several times larger than the
// indexed one (the inverse strategy on a big job: 3 Gbases streamed against a 150 Mbase index) finds nothing to hide behind --
// the two VALU-bound sketches and the small sort just share the chip -- so the hint is ignored there and the overlap call
// sketches in line (C5/10 inverse: 95 -> 89 ms per step).
static int presketch_prepare(lrge_hip_ctx *ctx, u64 indexed_bases) {
    presketch_drop_prepared(ctx);
    lrge_hip_seqset *s = ctx->presk_pending;
    if (!s) return LRGE_OK;
    ctx->presk_pending = nullptr;
    if (s->total_bases > 2 * indexed_bases && !ctx->opt("PRESKETCH_ALWAYS")) return LRGE_OK;
    if (s->total_bases > ctx->opt_u64("STREAM_BASES", 4000000000ull)) return LRGE_OK;   // streamed in views: sketched per view
    if (s->presk) presketch_discard(s);
    PreSketch *p = new PreSketch();
    p->preset = ctx->presk_preset;
    p->sc = new Scratch(ctx);
    p->ev_start = ctx->get_event(); p->ev_done = ctx->get_event();
    ctx->presk_prepared = p; ctx->presk_prepared_set = s;
    // behind the index sketch (both are VALU-bound; the point is to run beside the passes that follow it)
    if (presketch_alloc(ctx, s, p) != LRGE_OK || hipEventRecord(ctx->ev_presk, ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        presketch_drop_prepared(ctx);                    // not fatal: the overlap call sketches the set itself
    }
    return LRGE_OK;
}

// Queues the prepared sketch on the side stream.  May block on the HOST until the set's upload job (host-side pack) is over,
// which is why the index build calls it only once it has nothing more of its own to queue that could run meanwhile.
static int presketch_launch_prepared(lrge_hip_ctx *ctx) {
    PreSketch *p = ctx->presk_prepared; lrge_hip_seqset *s = ctx->presk_prepared_set;
    if (!p) return LRGE_OK;
    hipError_t e = hipStreamWaitEvent(ctx->stream2, ctx->ev_presk, 0);
    // an upload of the set still in flight: only the side stream waits for it -- the main stream goes on with the index
    // (its own seqset_ready comes with the overlap call, which also returns the staging blocks to the pool)
    if (s->job && seqset_job_wait(ctx, s) != LRGE_OK) { presketch_drop_prepared(ctx); return LRGE_OK; }
    if (e == hipSuccess && s->pending) e = hipStreamWaitEvent(ctx->stream2, s->ev_ready, 0);
    if (e == hipSuccess) e = hipEventRecord(p->ev_start, ctx->stream2);
    int rc = LRGE_OK;
    if (e == hipSuccess) {
        rc = p->preset == LRGE_PRESET_AVA_PB ? presketch_launch<19, 5, true>(ctx, s, p, ctx->stream2)
                                             : presketch_launch<15, 5, false>(ctx, s, p, ctx->stream2);
        if (rc == LRGE_OK) e = hipEventRecord(p->ev_done, ctx->stream2);
    }
    if (e != hipSuccess || rc != LRGE_OK) {      // not fatal: the overlap call sketches the set itself
        (void)hipStreamSynchronize(ctx->stream2);
        (void)hipGetLastError();
        presketch_drop_prepared(ctx);
        return LRGE_OK;
    }
    ctx->presk_prepared = nullptr; ctx->presk_prepared_set = nullptr;
    s->presk = p;
    return LRGE_OK;
}

// may_block = false (one part of a partitioned index): a streamed set whose upload job is still running -- it is queued behind
// the targets' own on the uploader thread, i.e. behind parts that have not even arrived -- keeps its request for the next part's
// build instead of stalling the host (with this part's table passes unqueued) until the whole transfer is over
static int presketch_start_pending(lrge_hip_ctx *ctx, u64 indexed_bases, bool may_block = true) {
    if (!may_block && ctx->presk_pending && ctx->presk_pending->job && !ctx->presk_pending->job->is_done()) return LRGE_OK;
    int rc = presketch_prepare(ctx, indexed_bases);
    return rc ? rc : presketch_launch_prepared(ctx);
}

extern "C" int lrge_hip_seqset_presketch(lrge_hip_ctx *ctx, lrge_hip_seqset *s, int preset) {
    if (!ctx || !s || s->ctx != ctx) return LRGE_ERR_INVALID;
    if (preset != LRGE_PRESET_AVA_ONT && preset != LRGE_PRESET_AVA_PB) { LRGE_SET_ERR(ctx, "Preset not found: %d", preset); return LRGE_ERR_INVALID; }
    ctx->presk_pending = s; ctx->presk_preset = preset;
    return LRGE_OK;
}

extern "C" int lrge_hip_sketch_dump(lrge_hip_ctx *ctx, const lrge_hip_seqset *s, int preset, uint64_t *x, uint64_t *y,
                                    uint64_t cap, uint64_t *n_out) {
    if (!ctx || !s || !n_out) return LRGE_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->pin_items.clear(); ctx->pin_used = 0;      // reads an earlier, failed call may have left queued
    Scratch sc(ctx);
    SketchOut o;
    int rc = sketch_device(ctx, sc, s, preset, SketchReq(), &o);
    if (rc) return rc;
    *n_out = o.n;
    u64 m = o.n < cap ? o.n : cap;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // blocking copies below run on the null stream
    if (m && x) HIPCHK(ctx, hipMemcpy(x, o.x, m * 8, hipMemcpyDeviceToHost));
    if (m && y) HIPCHK(ctx, hipMemcpy(y, o.y, m * 8, hipMemcpyDeviceToHost));
    return LRGE_OK;
}
