// rtk_render_body.inc -- the body of the render kernels, included textually by both of them (rtk_trace.hip):
//   rtk_render_kernel      VIEWS = false: one camera, read through cam_ptr with scalar loads where it is used;
//   rtk_view_batch_kernel  VIEWS = true: `views` holds a camera and a hashed seed per view, the local tiles of `tmap` are
//                          [view][tile of a view's tiles_x x tiles_y grid], and every lane carries the byte offset of its view's record.
// Everything that differs sits behind `#if RTK_BODY_VIEWS`, which the including kernel defines as 0 or 1.  Textual inclusion and
// the preprocessor, not a shared function with a flag: through a forced-inline function, and even with `if constexpr` in this
// text, the plain kernels' scheduling and register allocation moved (tools/isa_diff.py); this way the compiler sees the plain
// kernel's tokens unchanged and its code is the same instruction for instruction.  The including kernel provides: real,
// FEAT_ALL, COUNT, IN_LDS; sc, cam_ptr or views, tmap, seed, partial, counters, tile_counter, tile_order, tile_cost, diag.
    extern __shared__ __align__(16) unsigned char lds_program[];
    if constexpr (IN_LDS) {
        // (lean MIXED kernel: byte pcs are used as LDS addresses, see rec_at) -- render nothing rather than garbage otherwise
        typedef const unsigned char __attribute__((address_space(3))) * lds_bytes_t;
        if (uint32_t(size_t((lds_bytes_t)lds_program)) != 0u) return;
    }
    constexpr bool BRACKET = (FEAT_ALL & F_SPHERE_MEDIA_ONLY) == 0;  // generic media (OP_MED_BEGIN / MID / END) may occur in the program
    // (measured and not done: also compiling get_lighting and the radiance registers out of the restricted variant -- 80 instead
    // of 96 B of scratch, and C5 34.6 instead of 32.0 ms at 32 spp)
    constexpr uint32_t FEAT = FEAT_ALL & ~uint32_t(F_LDS_BOXES | F_SPHERE_MEDIA_ONLY) & ~uint32_t(RTK_DEV_MASK_OFF);
    constexpr bool LDS_PART = (FEAT_ALL & F_LDS_BOXES) != 0;  // a program larger than LDS, part of it staged there
    static_assert(!LDS_PART || !IN_LDS, "F_LDS_BOXES: for programs that do not fit LDS");
    constexpr bool MIXED = (FEAT & F_F32_BOX) != 0;  // f32 culling boxes + exact primitives (f64 kernels, fast order): ...
    // ... the MIXED program of sphere-only scenes (32-byte units) or, for every other family, the COMPACT program (16-byte units)
    constexpr bool COMPACT = MIXED && (FEAT & ~uint32_t(F_F32_BOX | F_MATTE)) != kFeatLean;
    static_assert(!MIXED || sizeof(real) == 8, "F_F32_BOX: f64 kernels only");
    // ... which part depends on the layout.  Slot program (SPLIT): the box slots, the kind nibbles and a rank table.  COMPACT
    // program (COLD): the whole "hot" program -- f32 culling boxes, spheres, every rare record -- in which each run of quads
    // or triangles is ONE two-unit record {kind, count, first unit in the cold array}; the quads and triangles themselves
    // ("cold": 144 / 80 bytes each, tested a few times per sample) stay in memory (SceneView::program_cold).
    constexpr bool CH = MIXED && !COMPACT;  // the MIXED program's boxes are centre / half-extent records
    // ... which the kernel that stages that program copies from its host-built LDS image (MixedImg: the same values; every head
    // tells its kind in its first 16 bytes, a box's link sits beside its centre)
    constexpr bool IMG = CH && IN_LDS;
    constexpr bool CHE = COMPACT && kCompactChStatic<FEAT>;  // ... and so are the COMPACT programs' of the mesh family, with a per-ray slack
    constexpr bool CHE_RT = COMPACT && COUNT && !CHE;  // the counting kernel on any family's COMPACT program: asks the scene
    [[maybe_unused]] const bool che_rt = CHE_RT && sc.compact_ch != 0;
    constexpr int kCulling = CH ? 1 : (CHE ? 2 : (CHE_RT ? 3 : 0));
    constexpr bool SPLIT = LDS_PART && !COMPACT;
    constexpr bool COLD = LDS_PART && COMPACT;
    static_assert(!LDS_PART || !MIXED || COMPACT, "F_LDS_BOXES with f32 boxes: the COMPACT program");
    constexpr bool XF = (FEAT & F_XFORM) != 0;
    using ProgRec = std::conditional_t<COMPACT, Unit16, std::conditional_t<MIXED, std::conditional_t<IMG, MixedImg, MixedHead>, Slot<real>>>;  // what pc counts
    using CurRec = std::conditional_t<MIXED, std::conditional_t<IMG, MixedImg, MixedHead>, Slot<real>>;                                      // the record head a step holds in registers
    constexpr uint32_t kBoxUnits = COMPACT ? 2u : 1u, kSphereUnits = COMPACT ? 3u : (MIXED ? 2u : 1u), kQuadUnits = COMPACT ? 9u : 3u, kTriUnits = COMPACT ? 5u : 2u;
    const ProgRec* prog;
    if constexpr (COLD) prog = sc.program_hot;
    else if constexpr (COMPACT) prog = sc.program_compact;
    else if constexpr (IMG) prog = sc.program_mixed_lds;
    else if constexpr (MIXED) prog = sc.program_mixed;
    else prog = sc.program;
    const int n_records = COLD ? sc.n_hot_units : (COMPACT ? sc.n_units16 : (MIXED ? sc.n_units : sc.n_slots));  // units of sizeof(ProgRec)
    [[maybe_unused]] const Unit16* cold = nullptr;
    if constexpr (COLD) cold = sc.program_cold;
    const MaterialRec<real>* mats = sc.materials;
    if constexpr (IN_LDS || COLD) {  // program (COLD: its hot part), then the material table, both as 16-byte words
        const int n_prog16 = n_records * int(sizeof(ProgRec) / 16);
        const int n_mat16 = sc.n_materials * int(sizeof(MaterialRec<real>) / 16);
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(prog);
        const uint4* __restrict__ msrc = reinterpret_cast<const uint4*>(sc.materials);
        uint4* dst = reinterpret_cast<uint4*>(lds_program);
        for (int k = threadIdx.x; k < n_prog16; k += blockDim.x) dst[k] = src[k];
        for (int k = threadIdx.x; k < n_mat16; k += blockDim.x) dst[n_prog16 + k] = msrc[k];
        if constexpr (COLD && (FEAT & F_TEXTURE) != 0) {  // the Perlin tables as well when the launcher found room
            if (tmap.perlin_lds_offset > 0) {
                const int n16 = sc.n_perlins * int(sizeof(PerlinRec<real>) / 16);
                const uint4* __restrict__ psrc = reinterpret_cast<const uint4*>(sc.perlins);
                uint4* pdst = reinterpret_cast<uint4*>(lds_program + tmap.perlin_lds_offset);
                for (int k = threadIdx.x; k < n16; k += blockDim.x) pdst[k] = psrc[k];
                sc.perlins = reinterpret_cast<const PerlinRec<real>*>(lds_program + tmap.perlin_lds_offset);
            }
        }
        __syncthreads();
        prog = reinterpret_cast<const ProgRec*>(lds_program);
        mats = reinterpret_cast<const MaterialRec<real>*>(lds_program + size_t(n_prog16) * 16);
    }
    using BoxCacheRec = BoxRec<real>;  // what F_LDS_BOXES keeps per box
    [[maybe_unused]] const BoxCacheRec* lds_boxes = nullptr;
    [[maybe_unused]] const uint32_t* lds_kinds = nullptr;
    [[maybe_unused]] const uint2* lds_rank = nullptr;
    if constexpr (SPLIT) {
        const BoxCacheRec* cache = sc.box_cache;
        const uint32_t* kind_words = sc.kind_words;
        const uint2* box_rank = sc.box_rank;
        const int n_boxes = sc.n_cached_boxes, n_kind_words = sc.n_kind_words, n_rank_words = sc.n_rank_words;
        const size_t box_bytes = size_t(n_boxes) * sizeof(BoxCacheRec);  // a multiple of 8
        const uint2* __restrict__ src = reinterpret_cast<const uint2*>(cache);
        uint2* dst = reinterpret_cast<uint2*>(lds_program);
        for (int k = threadIdx.x; k < int(box_bytes / 8); k += blockDim.x) dst[k] = src[k];
        uint32_t* kdst = reinterpret_cast<uint32_t*>(lds_program + box_bytes);
        for (int k = threadIdx.x; k < n_kind_words; k += blockDim.x) kdst[k] = kind_words[k];
        uint2* rdst = reinterpret_cast<uint2*>(lds_program + box_bytes + ((size_t(n_kind_words) * 4 + 7) & ~size_t(7)));
        for (int k = threadIdx.x; k < n_rank_words; k += blockDim.x) rdst[k] = box_rank[k];
        // ... and the material table behind them when the launcher found room (tmap.mats_lds_offset > 0): every shade step reads it
        if (tmap.mats_lds_offset > 0) {
            const int n_mat16 = sc.n_materials * int(sizeof(MaterialRec<real>) / 16);
            const uint4* __restrict__ msrc = reinterpret_cast<const uint4*>(sc.materials);
            uint4* mdst = reinterpret_cast<uint4*>(lds_program + tmap.mats_lds_offset);
            for (int k = threadIdx.x; k < n_mat16; k += blockDim.x) mdst[k] = msrc[k];
            mats = reinterpret_cast<const MaterialRec<real>*>(lds_program + tmap.mats_lds_offset);
        }
        if constexpr ((FEAT & F_TEXTURE) != 0) {  // the Perlin tables too, when the launcher found room (tmap.perlin_lds_offset > 0)
            if (tmap.perlin_lds_offset > 0) {
                const int n16 = sc.n_perlins * int(sizeof(PerlinRec<real>) / 16);
                const uint4* __restrict__ psrc = reinterpret_cast<const uint4*>(sc.perlins);
                uint4* pdst = reinterpret_cast<uint4*>(lds_program + tmap.perlin_lds_offset);
                for (int k = threadIdx.x; k < n16; k += blockDim.x) pdst[k] = psrc[k];
                sc.perlins = reinterpret_cast<const PerlinRec<real>*>(lds_program + tmap.perlin_lds_offset);  // texture_value reads through sc
            }
        }
        __syncthreads();
        lds_boxes = reinterpret_cast<const BoxCacheRec*>(lds_program);
        lds_kinds = kdst;
        lds_rank = rdst;
    }
    // the head of the record that starts at pc, as a step holds it in registers
    // (COLD: a lane inside a run of cold primitives keeps its position in the run in the top byte of its pc)
    constexpr uint32_t kPcMask = COLD ? 0x00FFFFFFu : 0xFFFFFFFFu;
    constexpr uint32_t kPcUnit = CH ? kChPcUnit : 1u;  // what one unit of the program adds to a pc (CH: pcs count bytes)
    // the record that starts at pc
    auto rec_at = [&](uint32_t pc) -> const ProgRec* {
        if constexpr (CH && IN_LDS) {
            // The staged program starts at LDS address 0 -- this kernel declares no static LDS, so its dynamic segment does
            // (checked when the kernel starts, and on the code object by tests/test_abi_and_host.py) -- hence a byte pc IS
            // the LDS address: the box step's next read needs no address arithmetic at all (C2 19.35 -> 18.96 ms).
            typedef const unsigned char __attribute__((address_space(3))) * lds_bytes_t;
            return reinterpret_cast<const ProgRec*>((const unsigned char*)(lds_bytes_t)(size_t)pc);
        } else if constexpr (CH) return reinterpret_cast<const ProgRec*>(reinterpret_cast<const unsigned char*>(prog) + pc);
        else return prog + pc;
    };
    auto head_at = [&](uint32_t pc) -> CurRec {
        if constexpr (COMPACT) return *reinterpret_cast<const MixedHead*>(prog + (pc & kPcMask));
        else return *rec_at(pc);
    };
    // kind of the record that starts at pc; the box record at pc (SPLIT: from the LDS copies)
    auto kind_of = [&](uint32_t pc) -> uint32_t {
        if constexpr (SPLIT) return (lds_kinds[pc >> 3] >> ((pc & 7u) * 4u)) & 15u;
        else if constexpr (COMPACT) return prog[(pc & kPcMask) + 1].w[2] & 15u;
        else if constexpr (MIXED) return rec_at(pc)->kind();
        else return rec_at(pc)->kind_payload & 15u;
    };
    [[maybe_unused]] auto box_at = [&](uint32_t pc) -> CurRec {
        const uint2 e = lds_rank[pc >> 5];
        const uint32_t at = e.y + uint32_t(__builtin_popcount(e.x & ((1u << (pc & 31u)) - 1u)));
        if constexpr (MIXED) {
            return CurRec{};  // (the f32-box programs are only used when they fit LDS whole: no boxes-in-LDS kernel)
        } else {
            const BoxRec<real> b = lds_boxes[at];
            Slot<real> s;
            #pragma unroll
            for (int k = 0; k < 6; k++) s.v[k] = b.v[k];
            s.kind_payload = OP_BOX;
            s.aux = b.aux;
            return s;
        }
    };
    // The record a closest hit names (L.best_pc): a pc of the program, or -- COLD -- n_records + the unit of a cold primitive.
    auto record_of = [&](uint32_t id) -> const ProgRec* {
        if constexpr (COLD) return id < uint32_t(n_records) ? prog + id : reinterpret_cast<const ProgRec*>(cold + (id - uint32_t(n_records)));
        else return rec_at(id);
    };
    [[maybe_unused]] auto kind_of_hit = [&](uint32_t id) -> uint32_t {  // for the tie rule: the kind of the current winner
        if constexpr (COLD) return id < uint32_t(n_records) ? kind_of(id) : (cold[id - uint32_t(n_records) + 1].w[2] & 15u);
        else return kind_of(id);
    };
    // exact ties between primitives are resolved by the reference's ranks in the kernels that run re-grouped hierarchies
    // (the quad/box subset kernel serves the fast order without a flag of its own)
    // f64 kernels only: the float kernels are not bit-exact against the reference anyway (SURVEY 8(d)), and the lean one has no register to spare
    constexpr bool TIE = sizeof(real) == 8 && ((FEAT & (F_FMA_BOX | F_F32_BOX)) != 0 || (FEAT & ~uint32_t(F_MATTE)) == kFeatQuadBox);
    const TieCtx<TIE, decltype(kind_of_hit)> tie{TIE ? (COLD ? sc.tie_rank_hot : (MIXED ? sc.tie_rank : sc.tie_rank_slot)) : nullptr, kind_of_hit, CH ? 5u : 0u};
    // The hand-out order of the tiles (learned from the previous frame) is staged behind the program when the host
    // found room for it (tmap.order_in_lds): a lookup per work item from LDS instead of a cold global load.
    if constexpr ((FEAT & F_XFORM) != 0 && (IN_LDS || LDS_PART)) {
        if (tmap.chains_lds_offset > 0) {  // instance-transform chains (a few hundred bytes: word by word)
            const int n4 = sc.n_chains * int(sizeof(ChainRec<real>) / 4);
            const uint32_t* __restrict__ csrc = reinterpret_cast<const uint32_t*>(sc.chains);
            uint32_t* cdst = reinterpret_cast<uint32_t*>(lds_program + tmap.chains_lds_offset);
            for (int k = threadIdx.x; k < n4; k += blockDim.x) cdst[k] = csrc[k];
            __syncthreads();
            sc.chains = reinterpret_cast<const ChainRec<real>*>(lds_program + tmap.chains_lds_offset);
        }
    }
    const int32_t* lds_order = nullptr;
    if (tmap.order_in_lds && tile_order) {
        int32_t* dst_order = reinterpret_cast<int32_t*>(lds_program + tmap.order_lds_offset);
        for (int k = threadIdx.x; k < tmap.n_tiles_local; k += blockDim.x) dst_order[k] = tile_order[k];
        __syncthreads();
        lds_order = dst_order;
    }
    // The camera lives in device memory and is read with scalar loads where it is
    // used (once per sample); as a by-value argument it would sit in registers for
    // the whole kernel.
#if RTK_BODY_VIEWS
    const CameraRec<real>& cam = views->cam;  // what all views share -- width, height, spp -- is read from view 0; what a sample reads: RTK_LANE_CAM below
#else
    const CameraRec<real>& cam = *cam_ptr;
#endif
    const int lane = threadIdx.x & 63;
    const uint32_t seed_hash = pcg_hash(seed);
    const int n_tiles_total = tmap.tiles_x * tmap.tiles_y;
    const int width = cam.width, height = cam.height, spp = cam.spp;
    const uint32_t end_pc = uint32_t(n_records - (COMPACT ? 2 : 1)) * kPcUnit;  // OP_END: the last record (two units in the COMPACT layout)
    const float extent = sc.extent;
    Counters<COUNT> cnt;
    cnt.clear();

    // Wave-uniform hand-out state: pixels of work item `refill_item` from
    // `refill_next` on have not been given to a lane yet.
    const int n_positions = tmap.active_count ? int(__builtin_amdgcn_readfirstlane(*tmap.active_count)) : tmap.n_tiles_local;
    const int n_items = n_positions * tmap.n_chunks;
    int refill_item = 0, refill_next = 64;
    // The index of the NEXT work item is fetched one item ahead: the returning atomic is issued when an item is
    // taken and only waited for when its 64 pixels have been handed out, so its ~2 us round trip never stalls the wave.
    unsigned int prefetched_item = 0;
    if (lane == 0) prefetched_item = atomicAdd(tile_counter, 1u);
    bool exhausted = false;
    // tools/: A/B of the refill batch size through variant bits 14..16 (0 = default)
    constexpr int kRefillMinTable[8] = {4, 1, 4, 8, 16, 24, 32, 12};
    const int refill_min = kRefillMinTable[(diag >> 14) & 7];
    constexpr int kSphereMinTable[8] = {16, 65, 4, 8, 12, 16, 24, 32};  // variant bits 17..19; 65 = never (spheres only through the vote)
    const int sphere_sel = int(diag >> 17) & 7;
    // defaults per kernel family (tools/variant_sweep.py): MIXED 12 (24.5 vs 24.7 ms at 16); full-feature 4 (C5 297.3 -> 283.4 ms; 8: 285.7);
    // mesh subset 8 (C4 +1 %); 16 elsewhere
    constexpr uint32_t kFamily = FEAT & ~uint32_t(F_FMA_BOX | F_F32_BOX | F_MATTE);
    constexpr int kSphereMinDefault = (MIXED && !COMPACT) ? 12 : (kFamily == kFeatAll ? 4 : (kFamily == kFeatMesh ? 8 : 16));
    const int sphere_min = sphere_sel == 0 ? kSphereMinDefault : kSphereMinTable[sphere_sel];

    Lane<real> L;
    L.pc = end_pc;
    L.kind = OP_DEAD;                 // this lane owns no (pixel, chunk): it takes part in no vote and waits for a refill
    L.box_kind = OP_BOX;              // (never left undefined: the vote compares kind with it on every lane)
    L.sum = mk(real(0), real(0), real(0));
    L.s = 0;
    RTK_PROF_DECL
    int my_slot = 0, my_pix = 0, px_i = 0, px_j = 0, s_end = 0, cost_tile = -1;  // my_slot = chunk * n_tiles_local + local_tile: where the partial sum goes
#if RTK_BODY_VIEWS
    // The byte offset of the lane's view record in `views` (one register; re-deriving the view from my_slot would cost two integer
    // divisions per sample) and of the current work item's.  The camera and the hashed seed a sample reads are per-lane loads there.
    uint32_t my_view = 0, it_view = 0;
#define RTK_LANE_VIEW reinterpret_cast<const ViewRec<real>*>(reinterpret_cast<const unsigned char*>(views) + my_view)
#define RTK_LANE_CAM (RTK_LANE_VIEW->cam)
#define RTK_LANE_SEED_HASH (RTK_LANE_VIEW->seed_hash)
#else
#define RTK_LANE_CAM cam
#define RTK_LANE_SEED_HASH seed_hash
#endif

    // COLD: one primitive of the run the lane sits on.  The run record (hot, two units) = {kind, count | aux = first unit
    // in the cold array}; the lane's position in the run rides in the top byte of its pc.  A hit is recorded under the id
    // n_records + cold unit (record_of / the rank table understand it); after the last primitive the lane walks on in
    // the hot program.
    [[maybe_unused]] auto cold_step = [&](auto is_quad, uint32_t& k) {
        if constexpr (COLD) {
            constexpr bool QUAD = decltype(is_quad)::value;
            constexpr uint32_t units = QUAD ? 9u : 5u;
            const uint32_t hot = L.pc & kPcMask, sub = L.pc >> 24;
            const MixedHead run = head_at(hot);
            const uint32_t at = run.aux + sub * units;
            L.pc = uint32_t(n_records) + at;
            if constexpr (QUAD) {
                QuadRegs regs;
                const double* __restrict__ src = reinterpret_cast<const double*>(cold + at);
                #pragma unroll
                for (int e = 0; e < 18; e++) regs.q[e] = src[e];
                hit_quad<XF, MIXED>(L, &regs, 0u, cnt, tie);
            } else {
                hit_tri<XF, MIXED>(L, reinterpret_cast<const ProgRec*>(cold + at), 0u, cnt, tie);
            }
            const bool last = sub + 1u >= (run.kind_payload >> 4);
            L.pc = last ? hot + 2u : (hot | ((sub + 1u) << 24));
            k = last ? kind_of(L.pc) : uint32_t(QUAD ? OP_QUAD : OP_TRI);
            L.kind = k;
        }
    };
    // One refill round: idle lanes take the next pixels of the wave's current work item (a tile x a chunk of the
    // samples); when the item is used up the wave first pulls another one from the rank-wide counter.  A (pixel,
    // chunk) belongs to exactly one lane, which walks its samples in order.  Returns true when idle lanes remain that
    // were not offered a pixel (the item ran out first).  Everything that steers it is wave-uniform.
    // What is the same for all 64 pixels of a work item is computed when the item is taken, on the scalar unit: the
    // integer divisions that turn the item index into (tile, chunk, pixel origin) and the tile_order lookup used to be
    // redone -- and their latencies waited for -- in every refill round (~12 lanes each, 4.3 M rounds per C2 frame).
    int it_x0 = 0, it_y0 = 0, it_slot = 0, it_s_begin = 0, it_s_end = 0, it_cost_tile = -1;
    bool it_ok = false;
    auto hand_out = [&](unsigned long long m_idle) -> bool {
        if (refill_next >= 64) {
            const int t = int(__builtin_amdgcn_readfirstlane(prefetched_item));
            if (t >= n_items) {
                exhausted = true;
                RTK_PROF_QUEUE_EMPTY
                return false;
            }
            refill_item = t;
            refill_next = 0;
            if (lane == 0) prefetched_item = atomicAdd(tile_counter, 1u);
            // Items are handed out in `tile_order` when the host has one (most expensive tiles of the previous
            // frame first); which wave renders a tile, and when, never changes a pixel's value.
            const int position = t / tmap.n_chunks, chunk = t % tmap.n_chunks;
            int local_tile = position;
            if (tile_order) local_tile = lds_order ? int(__builtin_amdgcn_readfirstlane(lds_order[position])) : tile_order[position];
#if RTK_BODY_VIEWS
            const int tile = local_tile % n_tiles_total;  // local tiles are [view][tile]: view and tile derived once per item, here on the scalar unit
            it_view = uint32_t(local_tile / n_tiles_total) * uint32_t(sizeof(ViewRec<real>));
#else
            const int tile = local_tile * tmap.n_ranks + tmap.rank;
#endif
            it_slot = chunk * tmap.n_tiles_local + local_tile;
            it_x0 = (tile % tmap.tiles_x) * 8;
            it_y0 = (tile / tmap.tiles_x) * 8;
            it_s_begin = tmap.chunk_start[chunk];
            it_s_end = tmap.chunk_start[chunk + 1];
            it_cost_tile = chunk == 0 ? local_tile : -1;  // chunk 0 of every pixel reports the tile's cost
            it_ok = tile < n_tiles_total && it_s_begin < it_s_end;
        }
        const int avail = 64 - refill_next;
        const int rank_in_idle = int(__builtin_amdgcn_mbcnt_hi(uint32_t(m_idle >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m_idle), 0u)));
        if (L.kind == OP_DEAD && rank_in_idle < avail) {
            my_pix = refill_next + rank_in_idle;
            my_slot = it_slot;
#if RTK_BODY_VIEWS
            my_view = it_view;
#endif
            px_i = it_x0 + (my_pix & 7);
            px_j = it_y0 + (my_pix >> 3);
            s_end = it_s_end;
            if (it_ok && px_i < width && px_j < height) {
                L.sum = mk(real(0), real(0), real(0));
                L.s = it_s_begin;
                L.segs = 0;
                cost_tile = it_cost_tile;
                RTK_PROF_CHUNK_BEGIN
                begin_sample(L, RTK_LANE_CAM, px_i, px_j, RTK_LANE_SEED_HASH, cnt);
                if (L.depth > 0) begin_segment<(FEAT & F_XFORM) != 0, MIXED, kCulling>(L, cnt, extent);
                else L.pc = end_pc;  // max_depth == 0: ray_color returns black at once (Camera.txt:205-206)
                L.kind = kind_of(L.pc);
            }
        }
        const int n_idle = popcount64(m_idle);
        refill_next += n_idle < avail ? n_idle : avail;
        return n_idle > avail;
    };

    for (;;) {
        // ---- regeneration at pixel granularity, BATCHED: handing out one pixel costs a full begin_sample +
        // begin_segment (hashes, RNG draws, the lens rejection loop, three f64 divisions) executed by the whole wave,
        // so idle lanes wait until `refill_min` of them can be served at once (or nobody has work left).  Which lane
        // renders a pixel, and when, never changes its value.  At most two rounds: the rest of the current item,
        // then the head of the next one.
        {
            const unsigned long long m_idle = __ballot(L.kind == OP_DEAD);
            const int n_idle = popcount64(m_idle);
            if (uniform(!exhausted && (n_idle >= refill_min || n_idle == 64))) {
                RTK_PROF_MARK(0, 0, 0)
                if (uniform(hand_out(m_idle))) hand_out(__ballot(L.kind == OP_DEAD));
                RTK_PROF_MARK(4, 1, n_idle)  // profile build: refills are booked under "other op" (phase 4)
            }
        }

        // ---- vote (registers and scalar unit only).  A lane's record kind IS its vote; OP_DEAD lanes have none.
        const uint32_t kind = L.kind;
        const unsigned long long m_box = __ballot(kind == L.box_kind);  // irregular rays' boxes count as "other"
        const unsigned long long m_sph = __ballot(kind == OP_SPHERE);
        const unsigned long long m_shd = __ballot(kind == OP_END);
        const unsigned long long m_quad = (FEAT & F_QUAD) ? __ballot(kind == OP_QUAD) : 0ull;
        const unsigned long long m_tri = (FEAT & F_TRI) ? __ballot(kind == OP_TRI) : 0ull;
        const unsigned long long m_oth = __ballot(kind != OP_DEAD) & ~(m_box | m_sph | m_shd | m_quad | m_tri);
        if ((m_box | m_sph | m_oth | m_shd | m_quad | m_tri) == 0ull) {
            if (exhausted) break;
            continue;
        }
        const int n_box = popcount64(m_box), n_sph = popcount64(m_sph), n_oth = popcount64(m_oth), n_shd = popcount64(m_shd);
        const int n_quad = popcount64(m_quad), n_tri = popcount64(m_tri);
        RTK_PROF_MARK(0, 1, n_box + n_sph + n_oth + n_shd + n_quad + n_tri)
        // The kind with the most ready lanes wins; ties go to the cheaper kind (order of the tests).  Written as
        // nested comparisons on purpose: a running "pick/most" update chain compiled to a 9 % slower kernel
        // (tools/ab/run_ab.sh A/B on the same box: 78.5 ms vs 70.2 ms per C2 frame).
        // (round 3: a shortcut for the common case -- 32 or more lanes on box records are a majority, so the other five ballots need
        // not be counted -- left the pick unchanged and the lean kernel with 128 VGPRs + 28 B of scratch instead of 110 + 0
        // (compile-only, tools/kernel_resources.py): not built.  The vote's cost is the wait for the lanes' record kinds, not its
        // thirty instructions.)
        int pick;
        if (n_box >= n_sph && n_box >= n_quad && n_box >= n_tri && n_box >= n_shd && n_box >= n_oth) pick = W_BOX;
        else if (n_sph >= n_quad && n_sph >= n_tri && n_sph >= n_shd && n_sph >= n_oth) pick = W_SPHERE;
        else if (n_quad >= n_tri && n_quad >= n_shd && n_quad >= n_oth) pick = W_QUAD;
        else if (n_tri >= n_shd && n_tri >= n_oth) pick = W_TRI;
        else if (n_shd >= n_oth) pick = W_SHADE;
        else pick = W_OTHER;
        if (pick == W_BOX) {
          if constexpr (IMG) {
            // The box loop on the LDS image (the loop of every other kernel follows, with the measurements behind its shape).  A
            // step holds the record at L.pc as its two 16-byte halves: `a` = centre and link -- or any other head's first half,
            // whose word 3 tells the kind as kind ^ 1, so a box's link is usable as read -- and `b` = half-extent, or a sphere's
            // y and z.  `k` is that code; lanes get their kind back when the loop ends.
            const int sel = int(diag >> 8) & 7;  // tools/: A/B of the loop-exit threshold, as below
            const int frac = (n_box * (sel == 0 ? 2 : sel)) >> 3;
            const int keep = frac > 8 ? frac : 8;
            typedef const rtk_u32x4 __attribute__((address_space(3))) * lds_uint4_t;
            rtk_u32x4 a, b;
            uint32_t k = kind ^ kImageKindXor;
            auto fetch = [&]() {
                a = *(lds_uint4_t)(size_t)L.pc;
                b = *(lds_uint4_t)(size_t)(L.pc + 16u);
                k = a.w & 15u;
            };
            a = *(lds_uint4_t)(size_t)L.pc;
            b = *(lds_uint4_t)(size_t)(L.pc + 16u);
            const uint32_t box_code = L.box_kind ^ kImageKindXor;  // a lane with an irregular ray matches nothing here
            constexpr uint32_t sphere_code = uint32_t(OP_SPHERE) ^ kImageKindXor;
            int remaining;
            __builtin_amdgcn_s_setprio(kBoxLoopPrio);
            do {
                #pragma unroll
                for (int step = 0; step < kUnrollMixed; step++) {
                    if (k == box_code) {
                        step_box_img(L, a, b, cnt);
                        fetch();
                    }
                }
                if ([[maybe_unused]] const int n_ride = popcount64(__ballot(k == sphere_code)); n_ride >= sphere_min) {  // sphere tests ride along
                    if (k == sphere_code) {
                        step_sphere_img<kPcUnit>(L, a, b, rec_at(L.pc), cnt, tie, extent);
                        fetch();
                    }
                    RTK_PROF_MARK(2, 1, n_ride)
                }
                remaining = popcount64(__ballot(k == box_code));
                RTK_PROF_MARK(1, 1, remaining)
            } while (remaining >= keep);
            __builtin_amdgcn_s_setprio(0);
            L.kind = k ^ kImageKindXor;
          } else {
            // Box tests dominate (about 100 per sample against a dozen sphere tests), so
            // the vote is amortised: keep stepping boxes -- one ballot and one branch per
            // step -- until fewer than `keep` lanes are still sitting on a box record.  A low
            // threshold wins: leaving the loop costs a vote plus an exposed LDS round trip,
            // which is worth more than the lanes that idle for a few extra steps.
            const int sel = int(diag >> 8) & 7;  // tools/: A/B of the loop-exit threshold, in eighths of the starters (0 = default)
            const int eighths = sel == 0 ? (kFamily == kFeatMesh ? 3 : 2) : sel;  // mesh subset: 3/8 (C4 42.4 -> 41.1 ms)  // measured on C2 (votes now cost ~2 box steps, spheres ride along): 2/8 of the starters 30.9 ms, 3/8 31.8, 4/8 32.4
            const int frac = (n_box * eighths) >> 3;
            const int keep = frac > 8 ? frac : 8;
            // box steps per trip around the loop's scalar checks: the per-family table above the kernel
            constexpr int kBoxUnroll = COLD ? kUnrollCold : SPLIT ? kUnrollSplit
                                       : (((MIXED && !COMPACT) || FEAT == (kFeatLean | uint32_t(F_FMA_BOX))) ? kUnrollMixed
                                          : (kFamily == kFeatAll ? 2 : (kFamily == kFeatQuadBox ? (COMPACT ? kUnrollCompactQuadBox : kUnrollQuadBox)
                                                                       : (kFamily == kFeatMesh ? (COMPACT ? kUnrollCompactMesh : kUnrollMesh) : kUnrollLean))));
            CurRec cur;  // the record at L.pc (its first 32 bytes in the MIXED / COMPACT layouts), held in registers: one LDS round trip per step
            uint32_t k = kind;
            // the record at L.pc -> cur, its kind -> k.  SPLIT: the kind comes from the LDS nibble table and only boxes are
            // fetched (from the LDS copy); a primitive's record is read from memory by the step that tests it
            // (tried on C5: requesting a sphere's record from memory already here, when a lane lands on it -- 770 vs 839 Msamples/s:
            // `cur` is one set of registers for the whole wave, so the next box step waits for that load all the same)
            auto fetch = [&]() {
                if constexpr (SPLIT) {
                    k = kind_of(L.pc);
                    if (k == OP_BOX) cur = box_at(L.pc);
                } else {
                    cur = head_at(L.pc);
                    k = cur.kind_payload & 15u;  // (a header word that IS the kind, read without the mask: the allocator answers with 14 moves per step, 21.9 vs 19.4 ms)
                }
            };
            if constexpr (SPLIT) {
                if (k == OP_BOX) cur = box_at(L.pc);
            } else {
                cur = head_at(L.pc);
            }
            const uint32_t box_kind = L.box_kind;  // a lane with an irregular ray matches nothing here: it never steps in this loop
            int remaining;
            [[maybe_unused]] SignMasks signs;
            if constexpr (MIXED && !CH && !CHE) {  // per-lane direction signs as wave masks; rays do not change inside this loop
                signs.x = __ballot(L.inv32.x < 0.0f);
                signs.y = __ballot(L.inv32.y < 0.0f);
                signs.z = __ballot(L.inv32.z < 0.0f);
            }
            __builtin_amdgcn_s_setprio(kBoxLoopPrio);
            // Sphere tests ride along: whenever `sphere_min` lanes of the wave sit on a sphere record, they are
            // stepped here, inside the box loop, instead of waiting for the loop to drain and a vote to pick
            // them (a vote round costs about two box steps).  Those lanes then return to box records, which
            // also keeps the loop populated for longer.
            do {
                if (k == box_kind) {
                    if constexpr (CH) step_box32_ch(L, cur, cnt);
                    else if constexpr (CHE) step_box32_che(L, cur, cnt);
                    else if constexpr (CHE_RT) {
                        if (che_rt) step_box32_che(L, cur, cnt);
                        else step_box32<kBoxUnits>(L, cur, cnt, signs);
                    }
                    else if constexpr (MIXED) step_box32<kBoxUnits>(L, cur, cnt, signs);
                    else step_box<false, XF, (FEAT & F_FMA_BOX) != 0>(L, cur, cnt);
                    fetch();
                    L.kind = k;
                }
                #pragma unroll
                for (int extra = 1; extra < kBoxUnroll; extra++) {
                    // further box steps before the loop's scalar checks (vote / sphere / exit): the checks are a
                    // dependent v_cmp -> s_bcnt1 -> s_cmp -> branch chain per step, and the kernel is latency-bound
                    if (k == box_kind) {
                        if constexpr (CH) step_box32_ch(L, cur, cnt);
                    else if constexpr (CHE) step_box32_che(L, cur, cnt);
                    else if constexpr (CHE_RT) {
                        if (che_rt) step_box32_che(L, cur, cnt);
                        else step_box32<kBoxUnits>(L, cur, cnt, signs);
                    }
                    else if constexpr (MIXED) step_box32<kBoxUnits>(L, cur, cnt, signs);
                        else step_box<false, XF, (FEAT & F_FMA_BOX) != 0>(L, cur, cnt);
                        fetch();
                        L.kind = k;
                    }
                }
                if ([[maybe_unused]] const int n_ride = popcount64(__ballot(k == OP_SPHERE)); n_ride >= sphere_min) {
                    if (k == OP_SPHERE) {
                        if constexpr (SPLIT) cur = head_at(L.pc);
                        if constexpr (COMPACT) step_sphere_compact<XF>(L, cur, prog + L.pc, cnt, tie);
                        else if constexpr (MIXED) step_sphere_mixed<kPcUnit>(L, cur, rec_at(L.pc), cnt, tie, extent);
                        else step_sphere<XF>(L, cur, cnt, tie);
                        fetch();
                        L.kind = k;
                    }
                    RTK_PROF_MARK(2, 1, n_ride)
                }
                if constexpr ((FEAT & F_TRI) != 0) {
                    // triangle tests ride along as well (mesh scenes: a bvh leaf is a box and one or two triangles):
                    // C4 47.8 -> 42.5 ms at 16 lanes (8: 42.8, 24: 43.6)
                    if (popcount64(__ballot(k == OP_TRI)) >= kTriRide) {
                        if (k == OP_TRI) {
                            if constexpr (COLD) {
                                cold_step(std::false_type{}, k);
                                cur = head_at(L.pc);
                            } else {
                                hit_tri<XF, MIXED>(L, prog + L.pc, kTriUnits, cnt, tie);
                                fetch();
                                L.kind = k;
                            }
                        }
                    }
                }
                // ... and quad tests in the quad/box subset kernels (C3 31.9 -> 30.4 ms at 16 lanes, 30.8 at 24); the
                // full-feature kernel has no registers for it (C5 298 -> 316 ms)
                if constexpr ((FEAT & ~uint32_t(F_FMA_BOX | F_F32_BOX | F_MATTE)) == kFeatQuadBox) {
                    if (popcount64(__ballot(k == OP_QUAD)) >= kQuadRide) {
                        if (k == OP_QUAD) {
                            hit_quad<XF, MIXED>(L, prog + L.pc, kQuadUnits, cnt, tie);
                            fetch();
                            L.kind = k;
                        }
                    }
                }
                remaining = popcount64(__ballot(k == box_kind));
                RTK_PROF_MARK(1, 1, remaining)
            } while (remaining >= keep);
            __builtin_amdgcn_s_setprio(0);
          }
        } else if (pick == W_SPHERE) {
            // A bvh leaf usually holds two spheres in a row: same amortisation, half the starters.
            const int ssel = int(diag >> 11) & 7;  // tools/: same for the sphere loop (0 = default)
            const int sfrac = (n_sph * (ssel == 0 ? 4 : ssel)) >> 3;
            const int keep = sfrac > 8 ? sfrac : 8;
            CurRec cur = head_at(L.pc);
            uint32_t k = kind;
            int remaining;
            __builtin_amdgcn_s_setprio(kSphereLoopPrio);
            do {
                if (k == OP_SPHERE) {
                    if constexpr (COMPACT) step_sphere_compact<XF>(L, cur, prog + L.pc, cnt, tie);
                    else if constexpr (MIXED) step_sphere_mixed<kPcUnit>(L, cur, rec_at(L.pc), cnt, tie, extent);
                    else step_sphere<XF>(L, cur, cnt, tie);
                    if constexpr (SPLIT) {
                        k = kind_of(L.pc);
                        if (k == OP_SPHERE) cur = head_at(L.pc);
                    } else {
                        cur = head_at(L.pc);
                        if constexpr (IMG) k = cur.kind();
                        else k = cur.kind_payload & 15u;
                    }
                    L.kind = k;
                }
                remaining = popcount64(__ballot(k == OP_SPHERE));
                RTK_PROF_MARK(2, 1, remaining)
            } while (remaining >= keep);
            __builtin_amdgcn_s_setprio(0);
        } else if ((FEAT & F_QUAD) && pick == W_QUAD) {
          if constexpr ((FEAT & F_QUAD) != 0) {
            // quad::hit.  A box() is six quads in a row (quad.h:86-108): stay while at least half the starters do.
            const int keep = (n_quad >> 1) > 8 ? (n_quad >> 1) : 8;
            uint32_t k = kind;
            int remaining;
            __builtin_amdgcn_s_setprio(kPrimLoopPrio);
            do {
                if (k == OP_QUAD) {
                    if constexpr (COLD) {
                        cold_step(std::true_type{}, k);
                    } else {
                        hit_quad<XF, MIXED>(L, prog + L.pc, kQuadUnits, cnt, tie);
                        k = kind_of(L.pc);
                        L.kind = k;
                    }
                }
                remaining = popcount64(__ballot(k == OP_QUAD));
                RTK_PROF_MARK(5, 1, remaining)
            } while (remaining >= keep);
            __builtin_amdgcn_s_setprio(0);
          }
        } else if ((FEAT & F_TRI) && pick == W_TRI) {
          if constexpr ((FEAT & F_TRI) != 0) {
            // triangle::hit; a bvh leaf holds one or two triangles.
            const int keep = (n_tri >> 1) > 8 ? (n_tri >> 1) : 8;
            uint32_t k = kind;
            int remaining;
            __builtin_amdgcn_s_setprio(kPrimLoopPrio);
            do {
                if (k == OP_TRI) {
                    if constexpr (COLD) {
                        cold_step(std::false_type{}, k);
                    } else {
                        hit_tri<XF, MIXED>(L, prog + L.pc, kTriUnits, cnt, tie);
                        k = kind_of(L.pc);
                        L.kind = k;
                    }
                }
                remaining = popcount64(__ballot(k == OP_TRI));
                RTK_PROF_MARK(5, 1, remaining)
            } while (remaining >= keep);
            __builtin_amdgcn_s_setprio(0);
          }
        } else if (pick == W_SHADE) {
            // 1. the body of ray_color for the lanes whose segment ended; a finished (pixel, chunk) is written out
            // (round 3, measured and removed: lanes whose closest hit carries a noise or image texture parked without a vote until
            // 4 - 16 of them had gathered -- C5 34.1 - 34.3 vs 31.9 ms at 32 spp for every threshold: the textures are 9 % of that
            // frame (tools/knockout.py), the gathering saved none of it and the extra ballot and spills cost 7 %.)
            bool finished = false, next_sample = false, alive = false;
            RTK_PROF_MARK(8, 1, 0)   // profile build: from the vote to here (marks sit outside divergent code: the profile registers are lane 0's)
            if (kind == OP_END) {
                alive = true;
                const bool ended = L.depth <= 0 || shade<real, FEAT, COUNT>(L, record_of(L.best_pc), sc, mats, RTK_LANE_CAM, cnt RTK_SHADE_PROF_ARG);
                if (ended) {  // pixel_color += ray_color(...) (Camera.txt:72)
                    if constexpr (!kNoRadianceState<FEAT>) L.sum = L.sum + L.radiance;
                    L.s += 1;
                    if (L.s < s_end) {
                        next_sample = true;
                    } else {
                        finished = true;
                        alive = false;
                        L.kind = OP_DEAD;
                        RTK_PROF_CHUNK_END
                        store_partial(partial, my_slot, my_pix, L.sum);
                        if (tile_cost && cost_tile >= 0) atomicAdd(&tile_cost[cost_tile], L.segs);  // no return value: fire and forget
                    }
                }
            }
            RTK_PROF_MARK(3, 1, n_shd)   // profile build: the shade step in three parts -- ray_color's body, begin_sample, begin_segment
            // 2. lanes that just finished take the next pixels of the wave's current work item right here, so that
            // their begin_sample / begin_segment is the code the continuing lanes execute anyway; a separate refill
            // round costs as much as a shade step and serves a dozen lanes.  Only what the current item still holds:
            // fetching the next item stays with the batched refill at the top of the loop.
            // (Not in the glossy quad/box subset kernel, which is short of registers: A/B on C3 34.5 vs 35.4 ms; its matte
            // variant has room: 32.3 -> 31.9.  C2 24.4 -> 23.0.)
            constexpr bool kRefillInShade = (FEAT & ~uint32_t(F_FMA_BOX | F_F32_BOX | F_MATTE)) != kFeatQuadBox || (FEAT & F_MATTE) != 0;
            const unsigned long long m_fin = kRefillInShade ? __ballot(finished) : 0ull;
            if (uniform(m_fin != 0ull && refill_next < 64)) {
                const int avail = 64 - refill_next;
                const int rank_in_fin = int(__builtin_amdgcn_mbcnt_hi(uint32_t(m_fin >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m_fin), 0u)));
                if (finished && rank_in_fin < avail) {
                    my_pix = refill_next + rank_in_fin;
                    my_slot = it_slot;
#if RTK_BODY_VIEWS
                    my_view = it_view;
#endif
                    px_i = it_x0 + (my_pix & 7);
                    px_j = it_y0 + (my_pix >> 3);
                    s_end = it_s_end;
                    if (it_ok && px_i < width && px_j < height) {
                        L.sum = mk(real(0), real(0), real(0));
                        L.s = it_s_begin;
                        L.segs = 0;
                        cost_tile = it_cost_tile;
                        RTK_PROF_CHUNK_BEGIN
                        alive = true;
                        next_sample = true;
                    }
                }
                const int n_fin = popcount64(m_fin);
                refill_next += n_fin < avail ? n_fin : avail;
            }
            // 3. the next sample of the same or of the new pixel, then the next segment
            if (next_sample) begin_sample(L, RTK_LANE_CAM, px_i, px_j, RTK_LANE_SEED_HASH, cnt);
            RTK_PROF_MARK(6, 1, popcount64(__ballot(next_sample)))
            if (alive) {
                if (L.depth > 0) begin_segment<(FEAT & F_XFORM) != 0, MIXED, kCulling>(L, cnt, extent);
                else L.pc = end_pc;
                L.kind = kind_of(L.pc);
            }
            RTK_PROF_MARK(7, 1, popcount64(__ballot(alive)))
        } else {
            // (A short loop here -- stay while at least half of the starters still sit on a rare record: book 2's two media are
            // neighbours in the program, an instance is entered and left through two chain switches -- was measured and
            // removed in round 3: C5 42.55 vs 42.10 ms at 32 spp, C4 15.47 vs 15.38, and the quad/box kernel lost 27 % to it,
            // C3 33.6 vs 26.3 ms at 100 spp.)
            // (Also measured and removed in round 3: the two sphere-bounded media of book 2 -- neighbours in the program, met by
            // every segment -- evaluated side by side in ONE branch-free step so that their two chains of dependent f64
            // operations interleave, B's random number drawn speculatively from the state A leaves: same image, same
            // counters, C5 42.9 vs 41.9 ms at 32 spp.)
            if (m_oth >> lane & 1ull) {
                if constexpr (MIXED && !COMPACT) step_other_mixed<kPcUnit>(L, rec_at(L.pc), cnt, tie, extent);
                else step_other<real, FEAT, BRACKET>(L, prog + L.pc, sc, cnt, tie, extent);
                L.kind = kind_of(L.pc);
            }
            RTK_PROF_MARK(4, 1, n_oth)
        }
    }
    RTK_PROF_FLUSH
    if constexpr (COUNT) {
        #pragma unroll
        for (int k = 0; k < C_COUNT; k++) {
            unsigned long long v = cnt.c[k];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0 && v) atomicAdd(&counters[k], v);
        }
    }
#undef RTK_LANE_CAM
#undef RTK_LANE_SEED_HASH
#if RTK_BODY_VIEWS
#undef RTK_LANE_VIEW
#endif
