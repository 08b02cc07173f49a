// tables.hip — the planner options behind the ABI, the plan hash, and build_device: the tables tables_host.cpp builds from the planner's
// output (particle state, tile descriptors and constraint streams, global colours, halo lists, the peer mailbox), uploaded
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree); the exported functions are the
// [BUILDER-DEFINED] boundary of SURVEY.md §8b (include/softbody*.h).
#include "solver_internal.hpp"
#include "launch_shape.hpp"

namespace sbi {

sbp::Input make_input(const float *rest, int32_t n, const int32_t *d, int64_t md, const int32_t *v, int64_t mv,
                      const int32_t *b, int64_t mb) {
    sbp::Input in;
    in.rest = rest; in.n = n; in.dist_ij = d; in.m_d = md; in.vol = v; in.m_v = mv; in.bend = b; in.m_b = mb;
    return in;
}

// The planner options behind the ABI's fields: ONE rule for sb_finalize and sb_plan_build, so the CPU schedule a host builds
// with sb_plan_build is the one the GPU solver of the same mesh runs.
sbp::Domain to_domain(const sb_domain &d) {
    sbp::Domain D;
    D.set = true; D.n_global = d.n_global; D.ell = d.spacing; D.fill = d.fill > 0 && d.fill <= 1 ? d.fill : 1.0;
    for (int a = 0; a < 3; ++a) { D.lo[a] = d.lo[a]; D.hi[a] = d.hi[a]; }
    return D;
}
sbp::Opts plan_opts(int rank, int world, const int32_t dims[3], int32_t tile_particles, int32_t partition, uint32_t plan_flags,
                    int64_t m_v, int64_t m_b, const sb_domain *domain) {
    sbp::Opts o;
    if (domain) {       // sharded: the automatic tile size follows the WHOLE mesh, which only the domain knows
        o.domain = to_domain(*domain);
        if (domain->four_vertex_constraints) m_v += 1;
    }
    o.rank = rank; o.world = world <= 0 ? 1 : world;
    for (int a = 0; a < 3; ++a) o.dims[a] = dims ? dims[a] : 0;
    // automatic tile size: 512 particles for spring meshes (bandwidth-bound: the fewest rim tiles that still fill the chip),
    // 256 when tets or hinges are present (latency-bound: shorter programs per tile, more tiles in flight)
    o.tile_particles = tile_particles != 0 ? tile_particles : (m_v + m_b > 0 ? 256 : 512);
    o.partition = partition;
    o.third_tiling = !(plan_flags & SB_PLAN_NO_T2);
    o.third_list = !(plan_flags & SB_PLAN_NO_THIRD_LIST);
    o.cluster_layers = !(plan_flags & SB_PLAN_NO_CLUSTER_LAYERS);
    o.mixed_groups = !(plan_flags & SB_PLAN_NO_MIXED_GROUPS);
    o.bank_aware_lanes = !(plan_flags & SB_PLAN_NO_BANK_ORDER);
    o.merge_tiles = !(plan_flags & SB_PLAN_NO_TILE_MERGE);
    if ((plan_flags >> 8) & 3u) o.balanced_lists = (int)((plan_flags >> 8) & 3u);
    return o;
}

// 64-bit FNV-1a over everything the ranks of a partitioned solver must agree on: the published orders, who owns which
// particle, the phase list with its halo slots, and the options that shaped them. (The halo lists are functions of these.)
uint64_t hash_plan(const sbp::Plan &P) {
    uint64_t h = sbt::kFnvBasis;
    auto mix = [&](const void *p, size_t bytes) {
        const uint8_t *b = static_cast<const uint8_t *>(p);
        // 8 bytes at a time (the arrays are tens of MB at 256^3), tail bytewise
        size_t k = 0;
        for (; k + 8 <= bytes; k += 8) { uint64_t w; std::memcpy(&w, b + k, 8); h = sbt::fnv1a(h, w); }
        for (; k < bytes; ++k) h = sbt::fnv1a(h, b[k]);
    };
    const int32_t head[8] = {P.n, P.opts.world, P.opts.tile_particles, P.partition,
                             (int32_t)((P.opts.third_tiling ? 0 : 1) | (P.opts.third_list ? 0 : 2) | (P.opts.cluster_layers ? 0 : 4) |
                                       (P.opts.mixed_groups ? 0 : 8) | (P.opts.bank_aware_lanes ? 0 : 16) | (P.opts.merge_tiles ? 0 : 32) | (P.opts.balanced_lists << 8)),
                             P.dims[0], P.dims[1], P.dims[2]};
    mix(head, sizeof(head));
    mix(P.m, sizeof(P.m));
    for (int p = 0; p < 2; ++p) {
        mix(P.order_type[p].data(), P.order_type[p].size());
        mix(P.order_id[p].data(), P.order_id[p].size() * sizeof(int32_t));
        for (const sbp::Phase &ph : P.phases[p]) {
            const int64_t rec[6] = {ph.kind, ph.tiling, ph.halo_slot, ph.layer, ph.order_begin, ph.order_end};
            mix(rec, sizeof(rec));
        }
    }
    mix(P.owner_of_old.data(), P.owner_of_old.size() * sizeof(int32_t));
    return h;
}

// the peer mailbox of this rank: allocated, zeroed, its header written
static void alloc_mailbox(sb_solver *s, sbt::HostMailbox &M) {
    auto &PS = s->peer;
    const int W = s->plan->local.world;
    PS.n_slots = M.n_slots; PS.off_table = M.off_table; PS.data_off_words = M.data_off_words; PS.bytes = M.bytes;
    PS.my_off = std::move(M.my_off);
    void *mb = nullptr;
    // (SB_TUNE_PEER_COARSE: an ordinary cached allocation -- timing experiments on ONE device only; between devices the flags and
    // segments must be uncached for the stores of one agent to reach the loads of another without cache maintenance)
    if (!(s->tune_flags & SB_TUNE_PEER_COARSE) && hipExtMallocWithFlags(&mb, PS.bytes, hipDeviceMallocFinegrained) == hipSuccess) PS.fine_grained = true;
    else { (void)hipGetLastError(); HIP_CHECK(hipMalloc(&mb, PS.bytes)); }
    PS.mailbox = (uint32_t *)mb;
    s->dev_bytes += (int64_t)PS.bytes;
    HIP_CHECK(hipMemset(PS.mailbox, 0, PS.bytes));
    HIP_CHECK(hipMemcpy(PS.mailbox, M.header.data(), M.header.size() * 4, hipMemcpyHostToDevice));
    int64_t unaccounted = 0;       // (sb_stats.device_bytes counts the mailbox, not these 32 bytes per slot)
    PS.local.alloc((size_t)PS.n_slots * 8, unaccounted);
    HIP_CHECK(hipMemset(PS.local.p, 0, (size_t)PS.n_slots * 8 * sizeof(uint32_t)));
    PS.h_error.alloc(1, /*mapped=*/true);
    *PS.h_error.p = 0;
    PS.remote.assign((size_t)W, nullptr);
    PS.opened.assign((size_t)W, 0);
    PS.remote[(size_t)s->plan->local.rank] = PS.mailbox;
}

// Builds the host tables stage by stage (tables_host.cpp) and uploads each stage before the next is built, so that the host never
// holds more than one tiling's tables. The order of the allocations is part of the behaviour: sb_stats reports dev_bytes, and
// placement experiments (sb_tuning.prev_offset_bytes) depend on what is allocated before what.
void build_device(sb_solver *s) {
    const sbp::LocalPlan &L = s->plan->local;
    const AuthoredMesh &M = *s->mesh;
    const sbt::TableInput in{&s->plan->plan, &L, M.pos.data(), M.vel.data(), M.invm.data(), M.kind[0].rest.data(), M.kind[1].rest.data(),
                             M.kind[2].rest.data(), (int64_t)M.kind[1].rest.size(), (int64_t)M.kind[2].rest.size()};
    sbt::TableOptions opt;
    opt.tune_flags = s->tune_flags; opt.tile_lanes = s->tile_lanes; opt.quad_lanes = s->quad_lanes; opt.narrow_min_tiles = s->narrow_min_tiles;
    opt.pack_tiles = s->pack_tiles; opt.win_dwords_cap = s->win_dwords_cap;
    opt.split_launches = s->overlap_halo || s->calib.state == 1;
    opt.peer_enabled = s->peer.enabled; opt.sharded = s->sharded; opt.plan_hash = s->plan_hash;
    opt.plan_shape = opt.peer_enabled && L.world > 1 ? plan_shape(s) : 0u;
    sbt::HostTables H;
    sbt::build_state(in, opt, H);
    s->n_owned = H.n_owned; s->n_local = H.n_local;
    s->w_palette = H.w_palette; s->w_uniform = H.w_uniform;
    s->d_pos3.upload(H.pos3, s->dev_bytes);
    s->d_wf.upload(H.wf, s->dev_bytes);
    if (H.w_palette) s->d_w8.upload(H.w8, s->dev_bytes);
    s->d_wpal.upload(H.wpal, s->dev_bytes);
    s->d_vel.upload(H.vel, s->dev_bytes);
    for (std::vector<float> *v : {&H.pos3, &H.wf, &H.vel}) std::vector<float>().swap(*v);
    std::vector<uint8_t>().swap(H.w8);
    s->d_prev.alloc((size_t)s->n_local * 3, s->dev_bytes, (size_t)s->prev_offset_bytes / sizeof(float));
    HIP_CHECK(hipMemset(s->d_prev.p, 0, (size_t)s->n_local * 3 * sizeof(float)));
    s->d_tp.alloc(1, s->dev_bytes);
    for (int tl = 0; tl < 3; ++tl) {
        sbt::build_tiling(in, opt, tl, H);
        sbt::HostTiling &T = H.T[tl];
        DevTiling &D = s->tiling[tl];
        static_cast<sbt::TilingScalars &>(D) = T;
        D.tiles.upload(T.tiles, s->dev_bytes); D.runs_overflow.upload(T.runs_overflow, s->dev_bytes);
        D.stream.upload(T.stream, s->dev_bytes);
        D.gather.upload(T.gather, s->dev_bytes);
        T.release_arrays();       // (later stages read the scalars)
    }
    s->t2_layer_range = H.t2_layer_range;
    sbt::build_gcolours(in, H);
    for (const sbt::HostGColour &G : H.gcolours) {
        auto D = std::make_unique<DevGColour>();
        D->type = G.type; D->count = G.count;
        if (G.type == 0) { D->ij.upload(G.ij, s->dev_bytes); D->rest.upload(G.rest, s->dev_bytes); }
        else { D->quad.upload(G.quad, s->dev_bytes); D->rest2.upload(G.rest2, s->dev_bytes); }
        s->gcolours.push_back(std::move(D));
    }
    sbt::build_halos(in, opt, H);
    for (sbt::HostHalo &G : H.halos) {
        auto D = std::make_unique<DevHalo>();
        D->send_idx.upload(G.send_idx, s->dev_bytes); D->recv_idx.upload(G.recv_idx, s->dev_bytes);
        D->peers = std::move(G.peers); D->send_off = std::move(G.send_off); D->recv_off = std::move(G.recv_off);
        s->halos.push_back(std::move(D));
    }
    s->d_sendbuf.alloc(H.send_floats, s->dev_bytes);
    s->d_recvbuf.alloc(H.recv_floats, s->dev_bytes);
    if (H.recv_floats) HIP_CHECK(hipMemset(s->d_recvbuf.p, 0, H.recv_floats * sizeof(float)));
    s->fused_unpack = H.fused_unpack;
    if (s->peer.enabled && L.world > 1) alloc_mailbox(s, H.mailbox);
    // previous positions as 8-byte codes between the tile kernels: for the whole solver or not at all (launch_shape.hpp)
    sbt::PrevCodeInputs pc;
    pc.world = s->desc.world; pc.tile_lanes = s->tile_lanes; pc.w_palette = s->w_palette; pc.n_local = s->n_local;
    pc.halo_slots = s->loopback ? 1 : 0;
    for (const auto &D : s->halos) if (D->active()) ++pc.halo_slots;
    pc.steps_between_tiles = (int)s->t2_layer_range.size() + (int)s->gcolours.size();
    s->prev_codes = sbt::use_prev_codes(s->tiling[0], s->tiling[1], pc);
    s->lean_coded = sbt::use_lean_coded(s->tiling[0], s->tiling[1], pc);
    if (s->prev_codes) {
        s->d_prev_code.alloc((size_t)s->n_local, s->dev_bytes);
        HIP_CHECK(hipMemset(s->d_prev_code.p, 0, (size_t)s->n_local * sizeof(uint2)));
    }
}

}  // namespace sbi
