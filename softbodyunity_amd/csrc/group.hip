// group.hip — sb_group_*: ONE process (a Unity player) driving several MI355X behind one Softbody component (include/softbody_group.h).
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree); [BUILDER-DEFINED] from BASELINE.json:5 and
// SURVEY.md §1 L1' ("one process x 8 devices"), §8b (`device_count`).
//
// A group is N ordinary solvers (sb_desc.rank = r, world = N, device = devices[r]) plus what a single host needs around them: the whole
// mesh authored once (cut into windows here when the partition is the block grid), the transport connected inside the process, one
// call per tick, state gathered in the caller's numbering, one render snapshot gathered on one device (what happens to it there is
// render.hpp's state and stage, the same as a single solver's). Two host models (softbody_group.h):
// a thread per rank (default) or the calling thread walking the tick program step by step across the ranks (SB_GROUP_WALK).
#include "solver_internal.hpp"

#include <condition_variable>
#include <thread>

using namespace sbi;

namespace {

// One host thread per rank: run(f) executes f(r) on every rank's thread and returns when all are done.
class RankThreads {
public:
    explicit RankThreads(int n) : results_((size_t)n, 0), errors_((size_t)n) {
        for (int r = 0; r < n; ++r) threads_.emplace_back([this, r] { loop(r); });
    }
    ~RankThreads() {
        { std::lock_guard<std::mutex> l(mu_); stop_ = true; ++generation_; }
        cv_go_.notify_all();
        for (auto &t : threads_) t.join();
    }
    // returns the first non-zero status (its message becomes the caller's sb_last_error)
    int run(const std::function<int(int)> &f) {
        {
            std::lock_guard<std::mutex> l(mu_);
            job_ = &f; pending_ = (int)threads_.size(); ++generation_;
        }
        cv_go_.notify_all();
        std::unique_lock<std::mutex> l(mu_);
        cv_done_.wait(l, [this] { return pending_ == 0; });
        job_ = nullptr;
        for (size_t r = 0; r < results_.size(); ++r)
            if (results_[r] != SB_OK) return fail(results_[r], "rank " + std::to_string(r) + ": " + errors_[r]);
        return SB_OK;
    }
private:
    void loop(int r) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<int(int)> *job;
            {
                std::unique_lock<std::mutex> l(mu_);
                cv_go_.wait(l, [&] { return generation_ != seen; });
                seen = generation_;
                if (stop_) return;
                job = job_;
            }
            int rc = SB_OK;
            try { rc = (*job)(r); }
            catch (const std::exception &e) { rc = fail(SB_ERR_INVALID_ARG, e.what()); }
            {
                std::lock_guard<std::mutex> l(mu_);
                results_[(size_t)r] = rc;
                errors_[(size_t)r] = rc ? last_error_text() : "";       // (the error text is thread-local to this worker)
                if (--pending_ == 0) cv_done_.notify_all();
            }
        }
    }
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_go_, cv_done_;
    const std::function<int(int)> *job_ = nullptr;
    uint64_t generation_ = 0;
    int pending_ = 0;
    bool stop_ = false;
    std::vector<int> results_;
    std::vector<std::string> errors_;
};

}  // namespace

struct sb_group {
    sb_desc desc{};
    uint32_t flags = 0;
    int W = 0;
    std::vector<int> devices;
    std::vector<sb_solver *> ranks;
    std::unique_ptr<RankThreads> threads;       // null in walk mode (and for a single rank)
    bool finalized = false, sharded = false;
    // the mesh, authored once (authoring.hpp): the ranks are handed windows cut from it, or share it
    std::shared_ptr<AuthoredMesh> mesh = std::make_shared<AuthoredMesh>();
    // kinematic scratch per rank (ids in the rank's numbering)
    std::vector<std::vector<int32_t>> kin_ids;
    std::vector<std::vector<float>> kin_pos;
    std::vector<int32_t> owner;                  // [n] caller numbering -> owning rank (after finalize)
    std::vector<int32_t> index_in_rank;          // [n] caller numbering -> index in the owner's numbering
    // ---- render readback, gathered on the render device (rank 0's): render.pos[k] is the buffer every rank snapshots into; with an
    // embedding (SPEC.md 6b) the cage is in the whole mesh's numbering ----
    RenderState render;
    struct RankRender {                          // per rank, on the rank's device
        DevBuf<int32_t> d_target_of_local;       // owned particle l -> caller id (full snapshots)
        DevBuf<int32_t> d_rs_ids, d_rs_local;    // the render particles (or, with an embedding, the cage particles) the rank owns: caller id, device index
        std::vector<int32_t> rs_local;
        Event ev_snap[kSnapSlots];
        int64_t acct = 0;
    };
    std::vector<RankRender> rr;
    int64_t dev_bytes = 0;
    bool heightfield_set = false;                // sb_group_set_heightfield left a table on every rank (SPEC.md 2h)
    bool distance_field_set[SB_DISTANCE_FIELD_SLOTS] = {};      // sb_group_set_distance_field left a table in this slot on every rank (SPEC.md 2i)
    int32_t reaction_count = 0;                  // the list length of the last sb_group_collide_reactions call (SPEC.md 2g): what a fetch returns

    int device_of(int r) const { return devices[(size_t)r]; }
    // f(r) for every rank: on the ranks' threads, or one after the other on the calling thread
    int for_ranks(const std::function<int(int)> &f) {
        if (threads) return threads->run(f);
        for (int r = 0; r < W; ++r) { const int rc = f(r); if (rc) return fail(rc, "rank " + std::to_string(r) + ": " + last_error_text()); }
        return SB_OK;
    }
    // The destructor holds only what is ORDER (and which device is current); the handles give themselves back.
    ~sb_group() {
        // 1. the rank threads are joined: nobody else drives a device from here on
        threads.reset();
        // 2. EVERY rank quiescent before ANY rank, mailbox or gather buffer goes away: neighbours push into each other's mailboxes and the
        //    snapshot kernels of every rank write into the render device's gather buffers
        for (sb_solver *s : ranks) if (s && s->finalized) (void)sb_synchronize(s);
        // 3. the render copy stream drained before its buffers go
        if (!devices.empty()) (void)hipSetDevice(devices[0]);
        if (render.copy_stream) (void)hipStreamSynchronize(render.copy_stream);
        // 4. every resource is destroyed with its own device current: the per-rank entries here, one device after the other, ...
        for (size_t r = 0; r < rr.size(); ++r) {
            (void)hipSetDevice(devices[r]);
            rr[r] = RankRender{};
        }
        for (sb_solver *s : ranks) if (s) (void)sb_destroy(s);       // (sets the rank's device itself)
        // ... and `render`, a member that dies after this body, on the render device: so that device is the body's last word
        if (!devices.empty()) (void)hipSetDevice(devices[0]);
    }
};

namespace {

bool walk_mode(const sb_group *g) { return (g->flags & SB_GROUP_WALK) != 0 || g->W == 1; }

// The mesh to rank r: its window of the whole mesh under sharded authoring (the particles whose rest position lies in its box, the
// constraints among them; their whole-mesh ids, domain and `sharded` as sb_set_domain sets them), else the group's mesh itself.
int author_rank(sb_group *g, int r, const sb_domain *dom) {
    sb_solver *s = g->ranks[(size_t)r];
    if (!dom) { s->mesh = g->mesh; return SB_OK; }
    sb_plan_opts o{};
    o.rank = r; o.world = g->W;
    for (int a = 0; a < 3; ++a) o.part_dims[a] = g->desc.part_dims[a];
    // (the automatic tile size must be resolved the way plan_opts resolves it for the whole mesh)
    o.tile_particles = g->desc.tile_particles;
    double lo[3], hi[3];
    if (sb_domain_window(dom, &o, lo, hi) != SB_OK) throw std::runtime_error(std::string("sb_group_finalize: ") + last_error_text());
    Window w = cut_window(*g->mesh, lo, hi);
    if (w.gid.empty()) return fail(SB_ERR_INVALID_ARG, "sb_group_finalize: a rank's window of the mesh is empty (fewer occupied cells than ranks?)");
    s->mesh = std::make_shared<AuthoredMesh>(std::move(w.mesh));
    s->domain = *dom;
    s->global_id = std::move(w.gid);
    s->sharded = true;
    return SB_OK;
}

// per rank: the rank's numbering -> the caller's (sharded authoring: window index -> whole-mesh id; null = identity)
const int32_t *id_map(const sb_group *g, int r) { const sb_solver *s = g->ranks[(size_t)r]; return s->global_id.empty() ? nullptr : s->global_id.data(); }

// ---- walk mode: the calling thread takes the tick apart --------------------------------------------------------------------------------
// One exchange step for every rank: pack kernels, then the sends and receives of ALL ranks inside one RCCL group, then the unpack
// kernels. `fork`: the overlapped schedule's form -- the exchange travels on each rank's second stream between two events.
void walk_exchange(sb_group *g, const TickStep &st) {
    const bool fork = st.kind == StepKind::ForkExchange;
    bool rccl_needed = false;
    for (int r = 0; r < g->W; ++r) {
        sb_solver *s = g->ranks[(size_t)r];
        HIP_CHECK(hipSetDevice(g->device_of(r)));
        hipStream_t stream = fork ? s->comm_stream : s->stream;
        if (fork) {
            HIP_CHECK(hipEventRecord(s->ev_boundary, s->stream));
            HIP_CHECK(hipStreamWaitEvent(s->comm_stream, s->ev_boundary, 0));
        }
        if (s->xtimer.enabled) s->xtimer.mark(stream);
        if (!s->peer.enabled) halo_exchange_pre(s, st.index, stream);
        if (s->xtimer.enabled) s->xtimer.mark(stream);
        if (s->peer.enabled) halo_exchange_pre(s, st.index, stream);
        rccl_needed = rccl_needed || (!s->peer.enabled && halo_slot_active(s, st.index));
    }
    if (rccl_needed) {
        NCCL_CHECK(rccl().GroupStart());
        try {
            for (int r = 0; r < g->W; ++r) {
                sb_solver *s = g->ranks[(size_t)r];
                HIP_CHECK(hipSetDevice(g->device_of(r)));
                halo_exchange_calls(s, st.index, fork ? s->comm_stream : s->stream);
            }
        } catch (...) {
            (void)rccl().GroupEnd();      // never leave the group open behind an error
            throw;
        }
        NCCL_CHECK(rccl().GroupEnd());
    }
    for (int r = 0; r < g->W; ++r) {
        sb_solver *s = g->ranks[(size_t)r];
        HIP_CHECK(hipSetDevice(g->device_of(r)));
        hipStream_t stream = fork ? s->comm_stream : s->stream;
        halo_exchange_post(s, st.index, stream);
        if (s->xtimer.enabled) s->xtimer.mark(stream);
        if (fork) HIP_CHECK(hipEventRecord(s->ev_halo, s->comm_stream));
    }
}

int walk_step(sb_group *g, float dt, int substeps) {
    if (g->W == 1) return sb_step(g->ranks[0], dt, substeps);
    return guarded([&]() -> int {
        std::vector<TickShape> shape((size_t)g->W);
        for (int r = 0; r < g->W; ++r) {
            HIP_CHECK(hipSetDevice(g->device_of(r)));
            shape[(size_t)r] = begin_tick(g->ranks[(size_t)r], dt, substeps);
        }
        // Every rank writes down its own program. They have the same steps in the same order -- the phases are a property of the plan, the
        // schedule is the same on every rank -- and differ only in what the FIRST tile step is: a rank whose previous tick still holds its
        // last kernel back starts with the fused mid-tick kernel (with or without kinematic targets: a rank that owns no pin has none), a
        // rank whose tick was completed by a read (ranks peek from a tile count on: one may have peeked where another flushed) starts with
        // the tick's plain first kernel. Whether the tick's own last kernel is held back depends on the arguments only, hence agrees.
        std::vector<std::vector<TickStep>> prog((size_t)g->W);
        for (int r = 0; r < g->W; ++r) {
            const TickShape &t = shape[(size_t)r];
            prog[(size_t)r] = tick_program(g->ranks[(size_t)r], substeps, t.fuse, t.defer_last, t.kin);
            bool same = prog[(size_t)r].size() == prog[0].size();
            for (size_t i = 0; same && i < prog[0].size(); ++i) same = prog[(size_t)r][i].kind == prog[0][i].kind && prog[(size_t)r][i].index == prog[0][i].index;
            if (!same) throw HipError(SB_ERR_STATE, "sb_group_step: the ranks' tick programs differ (different schedules or plans on the ranks of one group?)");
        }
        for (size_t i = 0; i < prog[0].size(); ++i) {
            const TickStep &st0 = prog[0][i];
            if (st0.kind == StepKind::Exchange || st0.kind == StepKind::ForkExchange) { walk_exchange(g, st0); continue; }
            for (int r = 0; r < g->W; ++r) {
                HIP_CHECK(hipSetDevice(g->device_of(r)));
                run_step(g->ranks[(size_t)r], prog[(size_t)r][i], nullptr);
            }
        }
        for (int r = 0; r < g->W; ++r) {
            HIP_CHECK(hipSetDevice(g->device_of(r)));
            HIP_CHECK(hipGetLastError());
            end_tick(g->ranks[(size_t)r], shape[(size_t)r]);
        }
        return SB_OK;
    });
}

// The communicators of a walk-mode group: all ranks of one thread, created together inside one RCCL group.
int walk_comm_init(sb_group *g) {
    return guarded([&]() -> int {
        const bool loopback = (g->desc.debug_flags & SB_DEBUG_LOOPBACK) != 0;
        std::vector<ncclUniqueId> ids((size_t)(loopback ? g->W : 1));
        for (auto &id : ids) NCCL_CHECK(rccl().GetUniqueId(&id));
        NCCL_CHECK(rccl().GroupStart());
        try {
            for (int r = 0; r < g->W; ++r) {
                sb_solver *s = g->ranks[(size_t)r];
                HIP_CHECK(hipSetDevice(g->device_of(r)));
                // SB_DEBUG_LOOPBACK (one-device pipeline tests): every rank a communicator of size 1 of its own, every peer the rank itself
                if (loopback) NCCL_CHECK(rccl().CommInitRank(&s->comm, 1, ids[(size_t)r], 0));
                else NCCL_CHECK(rccl().CommInitRank(&s->comm, g->W, ids[0], r));
            }
        } catch (...) {
            (void)rccl().GroupEnd();
            for (sb_solver *s : g->ranks) s->comm = nullptr;      // (whatever the failed group left behind is not a communicator to destroy)
            throw;
        }
        const ncclResult_t r = rccl().GroupEnd();
        if (r != ncclSuccess) {
            for (sb_solver *s : g->ranks) s->comm = nullptr;
            throw HipError(SB_ERR_RCCL, std::string("ncclGroupEnd (communicators of the group's ranks): ") + rccl().GetErrorString(r));
        }
        return SB_OK;
    });
}

// Peer access between the ranks' devices (pointers of one rank dereferenced by kernels of another: mailboxes, the render gather).
void enable_peer_access(sb_group *g) {
    for (int a = 0; a < g->W; ++a)
        for (int b = 0; b < g->W; ++b) {
            const int da = g->device_of(a), db = g->device_of(b);
            if (da == db) continue;
            HIP_CHECK(hipSetDevice(da));
            int can = 0;
            HIP_CHECK(hipDeviceCanAccessPeer(&can, da, db));
            if (!can) throw HipError(SB_ERR_UNSUPPORTED, "sb_group_finalize: device " + std::to_string(da) + " cannot access device " + std::to_string(db) + " (no peer access)");
            const hipError_t e = hipDeviceEnablePeerAccess(db, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) throw HipError(SB_ERR_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
            (void)hipGetLastError();
        }
}

int check_group(const sb_group *g, bool finalized, const char *who) {
    if (!g) return fail(SB_ERR_INVALID_ARG, std::string(who) + ": null group");
    if (finalized && !g->finalized) return fail(SB_ERR_STATE, std::string(who) + " before sb_group_finalize");
    if (!finalized && g->finalized) return fail(SB_ERR_STATE, std::string(who) + " after sb_group_finalize");
    return SB_OK;
}

}  // namespace

extern "C" {

int sb_group_create(const sb_desc *desc, const int32_t *devices, int32_t n_devices, uint32_t flags, sb_group **out) {
    if (!desc || !out) return fail(SB_ERR_INVALID_ARG, "sb_group_create: null argument");
    *out = nullptr;
    if (n_devices < 1 || n_devices > 64) return fail(SB_ERR_INVALID_ARG, "sb_group_create: n_devices must be 1 .. 64");
    if (flags & ~(SB_GROUP_WALK | SB_GROUP_WHOLE_MESH)) return fail(SB_ERR_INVALID_ARG, "sb_group_create: unknown bit in flags");
    if ((flags & SB_GROUP_WALK) && n_devices > 1) {
        if (desc->halo_schedule == SB_SCHEDULE_SERIAL_GRAPH || desc->halo_schedule == SB_SCHEDULE_OVERLAP_GRAPH)
            return fail(SB_ERR_UNSUPPORTED, "sb_group_create: SB_GROUP_WALK runs the eager schedules only (a capture spanning several devices' streams is not built)");
    }
    return guarded([&]() -> int {
        auto g = std::make_unique<sb_group>();
        g->desc = *desc; g->flags = flags; g->W = n_devices;
        for (int r = 0; r < n_devices; ++r) g->devices.push_back(devices ? devices[r] : r);
        g->ranks.assign((size_t)n_devices, nullptr);
        g->mesh->group = true;
        g->kin_ids.resize((size_t)n_devices); g->kin_pos.resize((size_t)n_devices);
        for (int r = 0; r < n_devices; ++r) {
            sb_desc d = *desc;
            d.device = g->devices[(size_t)r]; d.rank = r; d.world = n_devices;
            if (n_devices == 1) { d.halo_transport = SB_TRANSPORT_RCCL; d.halo_schedule = SB_SCHEDULE_AUTO; d.debug_flags = 0; }
            const int rc = sb_create(&d, &g->ranks[(size_t)r]);
            if (rc) return rc;
            g->ranks[(size_t)r]->group_walk = walk_mode(g.get()) && n_devices > 1;
        }
        if (!walk_mode(g.get())) g->threads = std::make_unique<RankThreads>(n_devices);
        *out = g.release();
        return SB_OK;
    });
}

int sb_group_destroy(sb_group *g) {
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_destroy: null group");
    delete g;
    return SB_OK;
}

int sb_group_set_particles(sb_group *g, const float *pos, const float *vel, const float *inv_mass, int32_t n) {
    if (int rc = check_group(g, false, "sb_group_set_particles")) return rc;
    return guarded([&]() -> int { return report(g->mesh->set_particles("sb_group_set_particles", pos, vel, inv_mass, n)); });
}

int sb_group_set_rest_positions(sb_group *g, const float *rest, int32_t n) {
    if (int rc = check_group(g, false, "sb_group_set_rest_positions")) return rc;
    return guarded([&]() -> int { return report(g->mesh->set_rest_positions("sb_group_set_rest_positions", rest, n)); });
}

static int group_set_cons(sb_group *g, const char *who, int type, const int32_t *idx, const float *rest, int32_t m, float compliance) {
    if (int rc = check_group(g, false, who)) return rc;
    return guarded([&]() -> int { return report(g->mesh->set_constraints(type, who, idx, rest, m, compliance)); });
}
int sb_group_set_distance_constraints(sb_group *g, const int32_t *ij, const float *rest_len, int32_t m, float compliance) {
    return group_set_cons(g, "sb_group_set_distance_constraints", 0, ij, rest_len, m, compliance);
}
int sb_group_set_volume_constraints(sb_group *g, const int32_t *ijkl, const float *rest_vol, int32_t m, float compliance) {
    return group_set_cons(g, "sb_group_set_volume_constraints", 1, ijkl, rest_vol, m, compliance);
}
int sb_group_set_bending_constraints(sb_group *g, const int32_t *ijkl, const float *rest_cs, int32_t m, float compliance) {
    return group_set_cons(g, "sb_group_set_bending_constraints", 2, ijkl, rest_cs, m, compliance);
}

int sb_group_set_ground_plane(sb_group *g, float nx, float ny, float nz, float d, int32_t enabled) {
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_set_ground_plane: null group");
    if (int rc = report(g->mesh->set_ground_plane("sb_group_set_ground_plane", nx, ny, nz, d, enabled))) return rc;
    if (g->finalized) for (sb_solver *s : g->ranks) { const int rc = sb_set_ground_plane(s, nx, ny, nz, d, enabled); if (rc) return rc; }
    return SB_OK;
}

int sb_group_finalize(sb_group *g) {
    if (int rc = check_group(g, false, "sb_group_finalize")) return rc;
    if (g->mesh->n <= 0) return fail(SB_ERR_STATE, "sb_group_finalize before sb_group_set_particles");
    const int W = g->W;
    const bool peer = W > 1 && g->desc.halo_transport == SB_TRANSPORT_PEER;
    const bool no_comm = (g->desc.debug_flags & SB_DEBUG_NO_COMM) != 0;
    const bool use_rccl = W > 1 && !peer && !no_comm;
    int rc = guarded([&]() -> int {
        // ---- the mesh to every rank: its window under the block partition (sharded authoring), else the whole mesh ----
        sb_domain dom{};
        // Windows (sharded authoring) where they are known to reproduce the whole-mesh plan: a lattice-like body (distance constraints only,
        // filling its bounding box -- colours, tiles and leftovers of such a mesh are local to a window; a tet mesh's or a cloth's are not:
        // tests/fuzz/fuzz_parity.py found every such mesh refused by the ranks' agreement check) under the block partition -- asked for
        // (SB_PARTITION_BLOCKS), or SB_PARTITION_AUTO on a LARGE mesh (the block grid is what AUTO takes for it anyway, and eight whole-mesh
        // plans of 16.8 M particles are 26 GB of host memory and 8 x 4.9 s of planning against 8 x 0.6 s on windows).
        constexpr int32_t kAutoShardParticles = 1 << 21;
        const bool may_shard = W > 1 && !(g->flags & SB_GROUP_WHOLE_MESH) && g->desc.tile_particles >= 0 && g->mesh->count(1) == 0 && g->mesh->count(2) == 0 &&
                               (g->desc.partition == SB_PARTITION_BLOCKS || (g->desc.partition == SB_PARTITION_AUTO && g->mesh->n >= kAutoShardParticles));
        g->sharded = false;
        if (may_shard) {
            dom = domain_of(make_input(*g->mesh));
            g->sharded = dom.fill >= 1.0;
        }
        if (W > 1) enable_peer_access(g);
        int rc1 = g->for_ranks([&](int r) { return guarded([&]() -> int { return author_rank(g, r, g->sharded ? &dom : nullptr); }); });
        if (rc1) return rc1;
        // ---- the transport ----
        if (use_rccl) {
            if (walk_mode(g)) { if ((rc1 = walk_comm_init(g))) return rc1; }
            else {
                const bool loopback = (g->desc.debug_flags & SB_DEBUG_LOOPBACK) != 0;
                std::vector<std::array<uint8_t, SB_UNIQUE_ID_BYTES>> ids((size_t)(loopback ? W : 1));
                for (auto &id : ids) if ((rc1 = sb_comm_unique_id(id.data()))) return rc1;
                // every rank's thread joins the communicator (the rendezvous of ncclCommInitRank blocks until all have called)
                if ((rc1 = g->for_ranks([&](int r) { return sb_comm_init(g->ranks[(size_t)r], ids[(size_t)(loopback ? r : 0)].data()); }))) return rc1;
            }
        }
        // ---- plan on every rank (host work, side by side), agreement, tables on every device ----
        // All ranks live in this process: their plans are compared right here (the records sb_finalize all-gathers across processes).
        // Windows that do not reproduce the whole-mesh plan -- the fill / constraint-type rule above lets through e.g. a cloud of particles on
        // a line joined by nearest-neighbour springs -- are found by exactly that comparison: the ranks are then handed the whole mesh and plan again.
        // (ranks' own threads where the group has them, else helper threads)
        auto on_every_rank = [&](const std::function<int(int)> &f) -> int {
            if (g->threads) return g->for_ranks(f);
            std::vector<int> lrc((size_t)W, 0);
            std::vector<std::string> lerr((size_t)W);
            {
                std::vector<std::thread> th;
                for (int r = 0; r < W; ++r) th.emplace_back([&, r] {
                    lrc[(size_t)r] = guarded([&]() -> int { return f(r); });
                    if (lrc[(size_t)r]) lerr[(size_t)r] = last_error_text();
                });
                for (auto &t : th) t.join();
            }
            for (int r = 0; r < W; ++r) if (lrc[(size_t)r]) return fail(lrc[(size_t)r], "rank " + std::to_string(r) + ": " + lerr[(size_t)r]);
            return SB_OK;
        };
        auto plan_and_compare = [&]() -> int {
            int rcp = on_every_rank([&](int r) { return guarded([&]() -> int { return finalize_plan(g->ranks[(size_t)r]); }); });
            if (rcp) return rcp;
            if (W > 1 && !(g->desc.debug_flags & SB_DEBUG_LOOPBACK)) {
                std::vector<uint64_t> all;
                for (int r = 0; r < W; ++r) { const auto rec = agreement_record(g->ranks[(size_t)r], false); all.insert(all.end(), rec.begin(), rec.end()); }
                return check_agreement(all, W, -1);
            }
            return SB_OK;
        };
        rc1 = plan_and_compare();
        if (rc1 == SB_ERR_STATE && g->sharded) {
            g->sharded = false;
            for (int r = 0; r < W; ++r) reset_authoring(g->ranks[(size_t)r]);
            if ((rc1 = g->for_ranks([&](int r) { return guarded([&]() -> int { return author_rank(g, r, nullptr); }); }))) return rc1;
            rc1 = plan_and_compare();
        }
        if (rc1) return rc1;
        if ((rc1 = on_every_rank([&](int r) { return guarded([&]() -> int { return finalize_device(g->ranks[(size_t)r]); }); }))) return rc1;
        if ((rc1 = on_every_rank([&](int r) { return finalize_link(g->ranks[(size_t)r]); }))) return rc1;
        // ---- peer transport inside one process: the mailboxes by plain pointer ----
        if (peer && !(g->desc.debug_flags & SB_DEBUG_LOOPBACK)) {
            for (int a = 0; a < W; ++a)
                for (int b = 0; b < W; ++b) {
                    if (a == b) continue;
                    bool needed = false;
                    for (const auto &H : g->ranks[(size_t)a]->halos) for (int pr : H->peers) needed |= pr == b;
                    if (!needed || g->ranks[(size_t)a]->peer.remote[(size_t)b]) continue;
                    if ((rc1 = sb_peer_connect(g->ranks[(size_t)a], b, nullptr, g->ranks[(size_t)b]))) return rc1;
                }
            // (links -- and with them the neighbours' plan / pair hashes -- are checked now, not at the first tick)
            if ((rc1 = g->for_ranks([&](int r) { return guarded([&]() -> int { int rcd = set_device(g->ranks[(size_t)r]); if (rcd) return rcd; peer_link(g->ranks[(size_t)r]); return SB_OK; }); }))) return rc1;
        }
        // ---- who owns what, in the caller's numbering ----
        g->owner.assign((size_t)g->mesh->n, -1); g->index_in_rank.assign((size_t)g->mesh->n, -1);
        for (int r = 0; r < W; ++r) {
            sb_solver *s = g->ranks[(size_t)r];
            const std::vector<int32_t> &own = s->plan->plan.owner_of_old;
            const int32_t *map = id_map(g, r);
            for (int32_t o = 0; o < s->mesh->n; ++o)
                if (own[(size_t)o] == r) {
                    const int32_t c = map ? map[o] : o;
                    if (g->owner[(size_t)c] >= 0) return fail(SB_ERR_STATE, "sb_group_finalize: internal: a particle is owned by two ranks");
                    g->owner[(size_t)c] = r; g->index_in_rank[(size_t)c] = o;
                }
        }
        for (int32_t c = 0; c < g->mesh->n; ++c) if (g->owner[(size_t)c] < 0) return fail(SB_ERR_STATE, "sb_group_finalize: internal: a particle is owned by no rank");
        g->mesh->release_bulk();       // (the ranks hold their own by now)
        g->finalized = true;
        return SB_OK;
    });
    return rc;
}

int sb_group_step(sb_group *g, float dt, int32_t substeps) {
    if (int rc = check_group(g, true, "sb_group_step")) return rc;
    if (!(dt > 0.0f) || substeps <= 0) return fail(SB_ERR_INVALID_ARG, "sb_group_step: dt and substeps must be positive");
    if (walk_mode(g)) return walk_step(g, dt, substeps);
    return g->for_ranks([&](int r) { return sb_step(g->ranks[(size_t)r], dt, substeps); });
}

static int group_get_state(sb_group *g, float *out, int32_t n, bool velocity, const char *who) {
    if (int rc = check_group(g, true, who)) return rc;
    if (!out || n != g->mesh->n) return fail(SB_ERR_INVALID_ARG, std::string(who) + ": bad argument (n differs from sb_group_set_particles?)");
    if (g->W == 1) return velocity ? sb_get_velocities(g->ranks[0], out, n) : sb_get_positions(g->ranks[0], out, n);      // (the permutation runs on the GPU)
    // every rank writes the entries it owns (disjoint), the ranks side by side
    return g->for_ranks([&](int r) { return guarded([&]() -> int { return get_state_owned(g->ranks[(size_t)r], out, velocity, id_map(g, r)); }); });
}
int sb_group_get_positions(sb_group *g, float *out, int32_t n) { return group_get_state(g, out, n, false, "sb_group_get_positions"); }
int sb_group_get_velocities(sb_group *g, float *out, int32_t n) { return group_get_state(g, out, n, true, "sb_group_get_velocities"); }

int sb_group_set_state(sb_group *g, const float *pos, const float *vel, int32_t n) {
    if (int rc = check_group(g, true, "sb_group_set_state")) return rc;
    if (!pos || !vel || n != g->mesh->n) return fail(SB_ERR_INVALID_ARG, "sb_group_set_state: bad argument");
    return g->for_ranks([&](int r) { return guarded([&]() -> int { return set_state_from(g->ranks[(size_t)r], pos, vel, id_map(g, r)); }); });
}

int sb_group_set_kinematic_positions(sb_group *g, const int32_t *ids, const float *pos, int32_t count) {
    if (int rc = check_group(g, true, "sb_group_set_kinematic_positions")) return rc;
    if (count < 0 || (count > 0 && (!ids || !pos))) return fail(SB_ERR_INVALID_ARG, "sb_group_set_kinematic_positions: bad argument");
    if (count == 0) return SB_OK;
    return guarded([&]() -> int {
        // validate the whole call first (nothing is changed on an error), then hand every rank the entries it owns, in its numbering
        for (auto &v : g->kin_ids) v.clear();
        for (auto &v : g->kin_pos) v.clear();
        for (int32_t k = 0; k < count; ++k) {
            if (ids[k] < 0 || ids[k] >= g->mesh->n) return fail(SB_ERR_INVALID_ARG, "sb_set_kinematic_positions: particle index out of range");
            if (g->mesh->invm[(size_t)ids[k]] != 0.0f)
                return fail(SB_ERR_INVALID_ARG, "sb_set_kinematic_positions: particle " + std::to_string(ids[k]) + " has a non-zero inverse mass (only pinned particles are kinematic)");
            for (int c = 0; c < 3; ++c) if (!(pos[3 * (size_t)k + c] == pos[3 * (size_t)k + c])) return fail(SB_ERR_INVALID_ARG, "sb_set_kinematic_positions: NaN");
            const int r = g->owner[(size_t)ids[k]];
            g->kin_ids[(size_t)r].push_back(g->index_in_rank[(size_t)ids[k]]);
            for (int c = 0; c < 3; ++c) g->kin_pos[(size_t)r].push_back(pos[3 * (size_t)k + c]);
        }
        // two moves without a tick between them: the earlier one takes effect first, which completes the held-back tick -- on EVERY rank
        // alike, so that the ranks stay in the same tick state (an id given twice in one call is found by the rank that owns it)
        bool pending = false;
        for (sb_solver *s : g->ranks) pending = pending || s->kin_pending >= 0;
        return g->for_ranks([&](int r) {
            sb_solver *s = g->ranks[(size_t)r];
            if (pending) { const int rcf = guarded([&]() -> int { int rcd = set_device(s); if (rcd) return rcd; flush_deferred(s); return SB_OK; }); if (rcf) return rcf; }
            if (g->kin_ids[(size_t)r].empty()) return (int)SB_OK;
            return guarded([&]() -> int { return set_kinematic(s, g->kin_ids[(size_t)r].data(), g->kin_pos[(size_t)r].data(), (int32_t)g->kin_ids[(size_t)r].size()); });
        });
    });
}

int sb_group_apply_impulses(sb_group *g, const sb_impulse *items, int32_t count) {
    if (!g || count < 0 || (count > 0 && !items)) return fail(SB_ERR_INVALID_ARG, "sb_group_apply_impulses: bad argument (null handle, null items or negative count)");
    if (int rc = check_group(g, true, "sb_group_apply_impulses")) return rc;
    if (count == 0) return SB_OK;
    return guarded([&]() -> int {
        if (int rc = validate_impulses("sb_group_apply_impulses", items, count, g->mesh->n, impulse_triangles_in_force(g->render), false)) return rc;
        // SURFACE items expanded here (a triangle's particles, a vertex' cage, may belong to several ranks), then every rank its entries in
        // list order and in its own numbering; an explosion reaches the particles of every rank
        std::vector<sb_impulse> flat;
        expand_impulses(g->render, items, count, flat);
        std::vector<std::vector<sb_impulse>> per_rank((size_t)g->W);
        for (const sb_impulse &it : flat) {
            if (it.kind == SB_IMPULSE_RADIAL) { for (auto &v : per_rank) v.push_back(it); continue; }
            sb_impulse e = it;
            e.index = g->index_in_rank[(size_t)it.index];
            per_rank[(size_t)g->owner[(size_t)it.index]].push_back(e);
        }
        // (a rank with nothing to apply still completes its tick: the ranks stay in the same tick state, as under sb_group_set_state)
        return g->for_ranks([&](int r) {
            return guarded([&]() -> int { return apply_impulses_validated(g->ranks[(size_t)r], per_rank[(size_t)r].data(), (int32_t)per_rank[(size_t)r].size()); });
        });
    });
}

int sb_group_apply_surface_forces(sb_group *g, const sb_surface_force *f) {
    // null and record checks before the group is touched: refused the same way on a machine without a device
    if (!g || !f) return fail(SB_ERR_INVALID_ARG, "sb_group_apply_surface_forces: null argument");
    if (int rc = validate_surface_force("sb_group_apply_surface_forces", f)) return rc;
    if (int rc = check_group(g, true, "sb_group_apply_surface_forces")) return rc;
    if (g->W > 1)
        return fail(SB_ERR_UNSUPPORTED, "sb_group_apply_surface_forces: a group of more than one rank (a triangle needs positions and velocities of corners that "
                    "another rank owns, and no rank holds those at a tick's end)");
    if (g->render.emb.m > 0)
        return fail(SB_ERR_UNSUPPORTED, "sb_group_apply_surface_forces: a render embedding is in force (its triangles index skinned vertices, which have no velocities of their own)");
    if (g->render.tri.empty()) return fail(SB_ERR_STATE, "sb_group_apply_surface_forces: no render triangles are set (sb_group_set_render_triangles comes first)");
    return guarded([&]() -> int {
        // the one rank holds the whole body; the triangles are the group's, handed over in the rank's numbering while its tables are not built
        sb_solver *s = g->ranks[0];
        std::vector<int32_t> tri;
        if (!surface_tables_built(s)) {
            tri.resize(g->render.tri.size());
            for (size_t c = 0; c < tri.size(); ++c) tri[c] = g->index_in_rank[(size_t)g->render.tri[c]];
        }
        return apply_surface_forces_validated(s, *f, tri.data(), (int64_t)(g->render.tri.size() / 3));
    });
}

int sb_group_place(sb_group *g, const sb_placement *p) {
    // null and struct checks before the group is touched: refused the same way on a machine without a device
    if (!g || !p) return fail(SB_ERR_INVALID_ARG, "sb_group_place: null argument");
    if (int rc = validate_placement("sb_group_place", p)) return rc;
    if (int rc = check_group(g, true, "sb_group_place")) return rc;
    // the same struct to every rank: each maps what it holds, ghosts included, and completes its tick (an identity map too: the ranks
    // stay in the same tick state). The render device takes no part.
    const sb_placement P = *p;
    return g->for_ranks([&](int r) { return guarded([&]() -> int { return place_validated(g->ranks[(size_t)r], P); }); });
}

int sb_group_collide(sb_group *g, const sb_collider *colliders, int32_t count) {
    // null and list checks before the group is touched: refused the same way on a machine without a device
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_collide: null group");
    if (int rc = validate_colliders("sb_group_collide", colliders, count)) return rc;
    if (int rc = check_group(g, true, "sb_group_collide")) return rc;
    if (count == 0) return SB_OK;      // nothing at all: no rank completes its tick
    // the same list to every rank: each walks what it holds, ghosts included, and completes its tick (a list that touches nothing too: the
    // ranks stay in the same tick state). The render device takes no part.
    const std::vector<sb_collider> list(colliders, colliders + count);
    return g->for_ranks([&](int r) { return guarded([&]() -> int { return collide_validated(g->ranks[(size_t)r], list.data(), count); }); });
}

int sb_group_collide_reactions(sb_group *g, const sb_collider *colliders, int32_t count) {
    // sb_group_collide's checks in its order, then the one of its own
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_collide_reactions: null group");
    if (int rc = validate_colliders("sb_group_collide_reactions", colliders, count)) return rc;
    if (count > SB_COLLIDE_REACTIONS_MAX) return fail(SB_ERR_INVALID_ARG, "sb_group_collide_reactions: more than SB_COLLIDE_REACTIONS_MAX colliders");
    if (int rc = check_group(g, true, "sb_group_collide_reactions")) return rc;
    g->reaction_count = 0;             // the stored records are replaced, by nothing if the call fails
    if (count == 0) return SB_OK;      // nothing at all to the state: no rank completes its tick
    const std::vector<sb_collider> list(colliders, colliders + count);
    const int rc = g->for_ranks([&](int r) { return guarded([&]() -> int { return collide_reactions_validated(g->ranks[(size_t)r], list.data(), count); }); });
    if (rc) return rc;
    g->reaction_count = count;
    return SB_OK;
}

int sb_group_get_collider_reactions(sb_group *g, sb_collider_reaction *out, int32_t capacity, int32_t *count_out) {
    if (!g || !count_out) return fail(SB_ERR_INVALID_ARG, "sb_group_get_collider_reactions: null argument");
    if (capacity < 0) return fail(SB_ERR_INVALID_ARG, "sb_group_get_collider_reactions: negative capacity");
    if (capacity > 0 && !out) return fail(SB_ERR_INVALID_ARG, "sb_group_get_collider_reactions: null out");
    if (int rc = check_group(g, true, "sb_group_get_collider_reactions")) return rc;
    const int32_t count = g->reaction_count, m = std::min(count, capacity);
    *count_out = count;
    if (m == 0) return SB_OK;
    // every rank waits for its own event and hands over its first m records (64 bytes each); the ranks' records are added in rank order,
    // so the same state and list give the same bits (SPEC.md 2g)
    std::vector<std::vector<sb_collider_reaction>> part((size_t)g->W, std::vector<sb_collider_reaction>((size_t)m));
    const int rc = g->for_ranks([&](int r) { return guarded([&]() -> int { return get_collider_reactions_owned(g->ranks[(size_t)r], part[(size_t)r].data(), m); }); });
    if (rc) return rc;
    for (int32_t k = 0; k < m; ++k) {
        sb_collider_reaction t = part[0][(size_t)k];
        for (int r = 1; r < g->W; ++r) {
            const sb_collider_reaction &q = part[(size_t)r][(size_t)k];
            for (int c = 0; c < 3; ++c) { t.impulse[c] += q.impulse[c]; t.angular_impulse[c] += q.angular_impulse[c]; }
            t.contact_mass += q.contact_mass;
            t.n_contacts += q.n_contacts;
        }
        out[k] = t;
    }
    return SB_OK;
}

int sb_group_set_heightfield(sb_group *g, const sb_heightfield *desc, const float *heights) {
    // null and table checks before the group is touched: refused the same way on a machine without a device
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_set_heightfield: null group");
    if (desc)
        if (int rc = validate_heightfield("sb_group_set_heightfield", desc, heights)) return rc;
    if (int rc = check_group(g, true, "sb_group_set_heightfield")) return rc;
    // no rank completes its tick: the table has a lifetime of its own, and a held-back last kernel still fuses with the next tick
    if (!desc) {
        if (!g->heightfield_set) return SB_OK;
        g->heightfield_set = false;
        return g->for_ranks([&](int r) { return guarded([&]() -> int { return clear_heightfield(g->ranks[(size_t)r]); }); });
    }
    const sb_heightfield D = *desc;
    const float top = heightfield_top(heights, (int64_t)D.nx * D.nz);
    g->heightfield_set = false;        // (set again once every rank has its table: a failure half way leaves no table in force)
    const int rc = g->for_ranks([&](int r) { return guarded([&]() -> int { return set_heightfield_validated(g->ranks[(size_t)r], D, heights, top); }); });
    if (rc) return rc;
    g->heightfield_set = true;
    return SB_OK;
}

int sb_group_collide_heightfield(sb_group *g, float friction, float restitution) {
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_collide_heightfield: null group");
    if (int rc = validate_heightfield_call("sb_group_collide_heightfield", friction, restitution)) return rc;
    if (int rc = check_group(g, true, "sb_group_collide_heightfield")) return rc;
    if (!g->heightfield_set) return SB_OK;      // nothing at all: no rank completes its tick (sb_group_collide's count == 0)
    // every rank walks what it holds, ghosts included, and completes its tick (a table that touches nothing too: the ranks stay in the same
    // tick state). The render device takes no part.
    return g->for_ranks([&](int r) { return guarded([&]() -> int { return collide_heightfield_validated(g->ranks[(size_t)r], friction, restitution); }); });
}

int sb_group_set_distance_field(sb_group *g, int32_t slot, const sb_distance_field *desc, const float *samples) {
    // null, slot and table checks before the group is touched: refused the same way on a machine without a device
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_set_distance_field: null group");
    if (int rc = validate_distance_field("sb_group_set_distance_field", slot, desc, samples)) return rc;
    if (int rc = check_group(g, true, "sb_group_set_distance_field")) return rc;
    // no rank completes its tick: a table has a lifetime of its own, and a held-back last kernel still fuses with the next tick
    if (!desc) {
        if (!g->distance_field_set[slot]) return SB_OK;
        g->distance_field_set[slot] = false;
        return g->for_ranks([&](int r) { return guarded([&]() -> int { return clear_distance_field(g->ranks[(size_t)r], slot); }); });
    }
    const sb_distance_field D = *desc;
    g->distance_field_set[slot] = false;      // (set again once every rank has its table: a failure half way leaves no table in force)
    const int rc = g->for_ranks([&](int r) { return guarded([&]() -> int { return set_distance_field_validated(g->ranks[(size_t)r], slot, D, samples); }); });
    if (rc) return rc;
    g->distance_field_set[slot] = true;
    return SB_OK;
}

int sb_group_collide_distance_field(sb_group *g, int32_t slot, const sb_distance_field_pose *pose) {
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_collide_distance_field: null group");
    if (int rc = validate_distance_field_pose("sb_group_collide_distance_field", slot, pose)) return rc;
    if (int rc = check_group(g, true, "sb_group_collide_distance_field")) return rc;
    if (!g->distance_field_set[slot]) return SB_OK;      // nothing at all: no rank completes its tick (sb_group_collide's count == 0)
    // every rank walks what it holds, ghosts included, and completes its tick (a pose that touches nothing too: the ranks stay in the same
    // tick state). The render device takes no part.
    const sb_distance_field_pose P = *pose;
    return g->for_ranks([&](int r) { return guarded([&]() -> int { return collide_distance_field_validated(g->ranks[(size_t)r], slot, P); }); });
}

/* ---- render readback, gathered on the render device ------------------------------------------------------------------------------------- */

int sb_group_set_render_triangles(sb_group *g, const int32_t *tri, int32_t m) {
    if (!g || m < 0 || (m > 0 && !tri)) return fail(SB_ERR_INVALID_ARG, "sb_group_set_render_triangles: bad argument");
    if (g->mesh->n <= 0) return fail(SB_ERR_STATE, "sb_group_set_render_triangles before sb_group_set_particles");
    if (g->render.pending) return fail(SB_ERR_STATE, "sb_group_set_render_triangles while a readback is pending");
    if (m > 0 && g->render.emb.m > 0)
        return fail(SB_ERR_STATE, "sb_group_set_render_triangles: a render embedding is set (switch it off first: sb_group_set_render_embedding with m_vertices = 0)");
    return guarded([&]() -> int {
        if (g->render.copy_stream) HIP_CHECK(hipSetDevice(g->device_of(0)));
        const int rc = set_render_triangles("sb_group_set_render_triangles", g->render, g->mesh->n, tri, m);
        if (rc == SB_OK) for (sb_solver *s : g->ranks) if (s) release_surface_tables(s);       // (the surface forces' tables of the old list; only a single rank has any)
        return rc;
    });
}

int sb_group_set_render_embedding(sb_group *g, const int32_t *cage_ijkl, const float *weights4, int32_t m_vertices, const int32_t *tri_abc, int32_t m_tri) {
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_set_render_embedding: null group");
    if (g->mesh->n <= 0) return fail(SB_ERR_STATE, "sb_group_set_render_embedding before sb_group_set_particles");
    if (g->render.pending) return fail(SB_ERR_STATE, "sb_group_set_render_embedding while a readback is pending");
    if (m_vertices > 0 && !g->render.tri.empty())
        return fail(SB_ERR_STATE, "sb_group_set_render_embedding: render triangles are set (switch them off first: sb_group_set_render_triangles with m = 0)");
    return guarded([&]() -> int {
        if (g->render.copy_stream) HIP_CHECK(hipSetDevice(g->device_of(0)));
        const bool was_on = g->render.emb.m > 0;
        const int rc = set_render_embedding("sb_group_set_render_embedding", g->render, g->mesh->n, cage_ijkl, weights4, m_vertices, tri_abc, m_tri);
        if (rc == SB_OK && (was_on || m_vertices > 0)) for (sb_solver *s : g->ranks) if (s) s->n_peek_tiles = -1;
        return rc;
    });
}

int sb_group_set_render_uvs(sb_group *g, const float *uv, int32_t count) {
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_set_render_uvs: null group");
    return guarded([&]() -> int {
        if (g->render.copy_stream) HIP_CHECK(hipSetDevice(g->device_of(0)));
        return set_render_uvs("sb_group_set_render_uvs", g->render, g->mesh->n, uv, count);
    });
}

int sb_group_set_readback_render_set_only(sb_group *g, int32_t on) {
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_set_readback_render_set_only: null group");
    return set_readback_render_set_only("sb_group_set_readback_render_set_only", g->render, on);
}

}  // extern "C"

namespace {

// The render particles (or, with an embedding, the distinct cage particles), split by owner: caller id and device index, on each rank's device.
void upload_rank_subsets(sb_group *g, const std::vector<int32_t> &particles) {
    std::vector<std::vector<int32_t>> ids((size_t)g->W), loc((size_t)g->W);
    for (int32_t c : particles) {
        const int r = g->owner[(size_t)c];
        ids[(size_t)r].push_back(c);
        loc[(size_t)r].push_back(local_of_old(g->ranks[(size_t)r])[(size_t)g->index_in_rank[(size_t)c]]);
    }
    for (int r = 0; r < g->W; ++r) {
        HIP_CHECK(hipSetDevice(g->device_of(r)));
        auto &Q = g->rr[(size_t)r];
        Q.d_rs_ids.upload(ids[(size_t)r], Q.acct); Q.d_rs_local.upload(loc[(size_t)r], Q.acct);
        Q.rs_local = loc[(size_t)r];
        g->ranks[(size_t)r]->n_peek_tiles = -1;        // the peek's tile subset follows these particles
    }
    HIP_CHECK(hipSetDevice(g->device_of(0)));
}

// Every rank: tick-end positions (peek or completed tick) of what it owns -- all of it, or its part of the subset -- straight into the
// gather buffer of slot k on the render device, whose copy stream then waits for all of them.
int gather_snapshots(sb_group *g, int k, bool subset) {
    float *dst = g->render.pos[k].d.p;
    const int rc = g->for_ranks([&](int r) {
        return guarded([&]() -> int {
            sb_solver *s = g->ranks[(size_t)r];
            int rcd = set_device(s); if (rcd) return rcd;
            auto &Q = g->rr[(size_t)r];
            const float *src = tick_end_positions(s, subset, Q.rs_local);
            if (subset) launch_snapshot_subset(s, src, Q.d_rs_ids.p, Q.d_rs_local.p, (int)Q.rs_local.size(), dst);
            else launch_snapshot_all(s, src, Q.d_target_of_local.p, dst);
            HIP_CHECK(hipEventRecord(Q.ev_snap[k], s->stream));
            return SB_OK;
        });
    });
    if (rc) return rc;
    HIP_CHECK(hipSetDevice(g->device_of(0)));
    for (int r = 0; r < g->W; ++r) HIP_CHECK(hipStreamWaitEvent(g->render.copy_stream, g->rr[(size_t)r].ev_snap[k], 0));
    return SB_OK;
}

}  // namespace

extern "C" {

int sb_group_readback_begin(sb_group *g) {
    if (int rc = check_group(g, true, "sb_group_readback_begin")) return rc;
    if (g->render.pending == 2) return fail(SB_ERR_STATE, "sb_group_readback_begin: two snapshots already pending, call sb_group_readback_end");
    return guarded([&]() -> int {
        RenderState &R = g->render;
        const int W = g->W, dev0 = g->device_of(0);
        const size_t n3 = (size_t)g->mesh->n * 3;
        HIP_CHECK(hipSetDevice(dev0));
        // first use, keyed on what it creates last (the last rank's last event); every step before it can simply be done again
        if (g->rr.empty() || !g->rr.back().ev_snap[kSnapSlots - 1]) {
            R.copy_stream.create();
            g->rr.resize((size_t)W);
            for (int k = 0; k < kSnapSlots; ++k) {
                R.pos[k].d.alloc(n3, g->dev_bytes);       // (its pinned twin: with the first full snapshot of the slot)
                HIP_CHECK(hipMemset(R.pos[k].d.p, 0, n3 * sizeof(float)));
                R.ev_copied[k].create(hipEventDisableTiming);
            }
            for (int r = 0; r < W; ++r) {      // owned particle -> caller id, on the rank's device
                sb_solver *s = g->ranks[(size_t)r];
                HIP_CHECK(hipSetDevice(g->device_of(r)));
                const sbp::LocalPlan &L = s->plan->local;
                const int32_t *map = id_map(g, r);
                std::vector<int32_t> target((size_t)s->n_owned);
                for (int64_t l = 0; l < s->n_owned; ++l) { const int32_t o = L.local_to_old[(size_t)l]; target[(size_t)l] = map ? map[o] : o; }
                g->rr[(size_t)r].d_target_of_local.upload(target, g->rr[(size_t)r].acct);
                for (int k = 0; k < kSnapSlots; ++k) g->rr[(size_t)r].ev_snap[k].create(hipEventDisableTiming);
            }
            HIP_CHECK(hipSetDevice(dev0));
        }
        const bool compact = R.set_only && !R.tri.empty();
        if (!R.tri.empty() && R.dirty) {     // the incident-triangle lists, the render set and who owns which of its particles
            HIP_CHECK(hipStreamSynchronize(R.copy_stream));
            const std::vector<int32_t> off = R.topo.upload(R.tri, g->mesh->n, g->dev_bytes);
            R.set.clear();
            for (int32_t v = 0; v < g->mesh->n; ++v) if (off[(size_t)v + 1] > off[v]) R.set.push_back(v);
            R.d_set.upload(R.set, g->dev_bytes);
            upload_rank_subsets(g, R.set);
            R.dirty = false;
        }
        const int k = R.next_slot();
        R.slot[k] = RenderState::Slot{};
        R.tan.snap_has[k] = false;
        if (R.emb.m > 0) {
            // Embedded render vertices: every rank snapshots the cage particles it owns into the gather buffer (whole-mesh numbering),
            // then the render device skins the visual mesh from it, computes the normals of the skinned array and copies both out.
            RenderEmbedding &E = R.emb;
            if (E.dirty) {
                HIP_CHECK(hipStreamSynchronize(R.copy_stream));
                std::vector<int4> cage((size_t)E.m);
                std::vector<uint8_t> seen((size_t)g->mesh->n, 0);
                std::vector<int32_t> distinct;
                for (int32_t v = 0; v < E.m; ++v) {
                    const int32_t *c = &E.cage[4 * (size_t)v];
                    cage[(size_t)v] = make_int4(c[0], c[1], c[2], c[3]);
                    for (int j = 0; j < 4; ++j) if (!seen[(size_t)c[j]]) { seen[(size_t)c[j]] = 1; distinct.push_back(c[j]); }
                }
                upload_rank_subsets(g, distinct);
                E.upload(cage, g->dev_bytes);      // (last: it clears E.dirty, the key of this block)
            }
            if (int rc = gather_snapshots(g, k, /*subset=*/true)) return rc;
            launch_skin(R.copy_stream, R.pos[k].d.p, E.d_cage.p, E.d_w.p, E.pos[k].d.p, (int)E.m);
            E.pos[k].copy_out(R.copy_stream, (size_t)E.m * 3);
            R.slot[k].embedded = true;
            if (!E.tri.empty()) launch_normals_stage(R.copy_stream, R, k, E.pos[k].d.p, (int)E.m, false, (size_t)E.m, g->dev_bytes);
            launch_bounds_stage(R.copy_stream, R.bnd, k, E.pos[k].d.p, nullptr, E.m, g->dev_bytes);      // SPEC.md 6d on the skinned vertices
        } else {
            const int count = compact ? (int)R.set.size() : (int)g->mesh->n;
            // this slot's buffers, by what it will carry (they only grow)
            if (!compact && !R.pos[k].h.p) R.pos[k].pin();
            if (!R.tri.empty()) {
                if (R.nrm[k].d.count < (size_t)count * 3) R.nrm[k].alloc((size_t)count * 3, g->dev_bytes);
                if (compact && R.cpos[k].d.count < (size_t)count * 3) R.cpos[k].alloc((size_t)count * 3, g->dev_bytes);
            }
            if (int rc = gather_snapshots(g, k, compact)) return rc;
            if (!compact) R.pos[k].copy_out(R.copy_stream, n3);
            R.slot[k].compact = compact;
            if (!R.tri.empty()) {
                launch_normals_stage(R.copy_stream, R, k, R.pos[k].d.p, count, compact, (size_t)count, g->dev_bytes);
                R.slot[k].has_render_set = true;
            }
            // SPEC.md 6d on the delivered array: every rank's rows are in the gather buffer by now
            launch_bounds_stage(R.copy_stream, R.bnd, k, compact ? R.cpos[k].d.p : R.pos[k].d.p, nullptr, count, g->dev_bytes);
        }
        HIP_CHECK(hipEventRecord(R.ev_copied[k], R.copy_stream));
        ++R.pending;
        return SB_OK;
    });
}

int sb_group_readback_end(sb_group *g, const float **pos_xyz_out) {
    if (!g || !pos_xyz_out) return fail(SB_ERR_INVALID_ARG, "sb_group_readback_end: null argument");
    if (g->render.pending == 0) return fail(SB_ERR_STATE, "sb_group_readback_end without a pending sb_group_readback_begin");
    return guarded([&]() -> int {
        HIP_CHECK(hipSetDevice(g->device_of(0)));
        HIP_CHECK(hipEventSynchronize(g->render.ev_copied[g->render.head]));
        for (sb_solver *s : g->ranks) check_peer_error(s);
        *pos_xyz_out = end_slot(g->render);
        return SB_OK;
    });
}

int sb_group_readback_get_normals(sb_group *g, const float **out) {
    if (!g || !out) return fail(SB_ERR_INVALID_ARG, "sb_group_readback_get_normals: null argument");
    return readback_get_normals("sb_group_readback_get_normals", g->render, out);
}

int sb_group_readback_get_tangents(sb_group *g, const float **out) {
    if (!g || !out) return fail(SB_ERR_INVALID_ARG, "sb_group_readback_get_tangents: null argument");
    return readback_get_tangents("sb_group_readback_get_tangents", g->render, out);
}

int sb_group_set_readback_bounds(sb_group *g, int32_t enabled) {
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_set_readback_bounds: null group");
    return set_readback_bounds("sb_group_set_readback_bounds", g->render, enabled);
}

int sb_group_readback_get_bounds(sb_group *g, float lo_xyz[3], float hi_xyz[3]) {
    if (!g || !lo_xyz || !hi_xyz) return fail(SB_ERR_INVALID_ARG, "sb_group_readback_get_bounds: null argument");
    return readback_get_bounds("sb_group_readback_get_bounds", "sb_group_set_readback_bounds", g->render, lo_xyz, hi_xyz);
}

int sb_group_get_bounds(sb_group *g, float lo_xyz[3], float hi_xyz[3]) {
    if (!g || !lo_xyz || !hi_xyz) return fail(SB_ERR_INVALID_ARG, "sb_group_get_bounds: null argument");
    if (int rc = check_group(g, true, "sb_group_get_bounds")) return rc;
    // every rank reduces what it owns on its own device (32 bytes each to the host); min and max compose exactly (SPEC.md 6d)
    std::vector<std::array<float, 6>> box((size_t)g->W);
    const int rc = g->for_ranks([&](int r) { return guarded([&]() -> int { return get_bounds_owned(g->ranks[(size_t)r], &box[(size_t)r][0], &box[(size_t)r][3]); }); });
    if (rc) return rc;
    for (int c = 0; c < 3; ++c) {
        float lo = std::numeric_limits<float>::infinity(), hi = -lo;
        for (int r = 0; r < g->W; ++r) {
            if (box[(size_t)r][(size_t)c] < lo) lo = box[(size_t)r][(size_t)c];
            if (box[(size_t)r][(size_t)c + 3] > hi) hi = box[(size_t)r][(size_t)c + 3];
        }
        lo_xyz[c] = lo + 0.0f; hi_xyz[c] = hi + 0.0f;
    }
    return SB_OK;
}

int sb_group_get_body_state(sb_group *g, uint32_t what, sb_body_state *out) {
    if (!g || !out) return fail(SB_ERR_INVALID_ARG, "sb_group_get_body_state: null argument");
    if (what == 0 || (what & ~(SB_BODY_POSE | SB_BODY_MOTION))) return fail(SB_ERR_INVALID_ARG, "sb_group_get_body_state: `what` must be SB_BODY_POSE, SB_BODY_MOTION or both");
    if (int rc = check_group(g, true, "sb_group_get_body_state")) return rc;
    // every rank reduces what it owns on its own device (272 bytes each to the host); the ranks' sums are added in rank order, so the
    // same state gives the same bits (SPEC.md 6f), and everything else is derived from the totals
    std::vector<std::array<double, 32>> sums((size_t)g->W);
    std::vector<std::array<int64_t, 2>> counts((size_t)g->W);
    const int rc = g->for_ranks([&](int r) { return guarded([&]() -> int { return get_body_sums_owned(g->ranks[(size_t)r], what, sums[(size_t)r].data(), counts[(size_t)r].data()); }); });
    if (rc) return rc;
    std::array<double, 32> total = sums[0];
    int64_t n_dynamic = counts[0][0], n_pinned = counts[0][1];
    for (int r = 1; r < g->W; ++r) {
        for (size_t k = 0; k < 32; ++k) total[k] += sums[(size_t)r][k];
        n_dynamic += counts[(size_t)r][0]; n_pinned += counts[(size_t)r][1];
    }
    body_state_derive(total.data(), n_dynamic, n_pinned, what, out);
    return SB_OK;
}

int sb_group_readback_raycast(sb_group *g, const float *rays, int32_t count, sb_ray_hit *hits_out) {
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_readback_raycast: null group");
    return guarded([&]() -> int {
        if (g->render.copy_stream) HIP_CHECK(hipSetDevice(g->device_of(0)));       // the render device, in both host models: the ranks take no part
        return readback_raycast("sb_group_readback_raycast", g->render, rays, count, hits_out, g->dev_bytes);
    });
}

int sb_group_readback_closest_points(sb_group *g, const float *queries, int32_t count, sb_closest_hit *hits_out) {
    if (!g) return fail(SB_ERR_INVALID_ARG, "sb_group_readback_closest_points: null group");
    return guarded([&]() -> int {
        if (g->render.copy_stream) HIP_CHECK(hipSetDevice(g->device_of(0)));       // the render device, in both host models: the ranks take no part
        return readback_closest_points("sb_group_readback_closest_points", g->render, queries, count, hits_out, g->dev_bytes);
    });
}

int sb_group_readback_get_render_set(sb_group *g, const int32_t **ids, int32_t *count) {
    if (!g || !ids || !count) return fail(SB_ERR_INVALID_ARG, "sb_group_readback_get_render_set: null argument");
    return readback_get_render_set("sb_group_readback_get_render_set", g->render, ids, count);
}

int sb_group_synchronize(sb_group *g) {
    if (int rc = check_group(g, true, "sb_group_synchronize")) return rc;
    return g->for_ranks([&](int r) { return sb_synchronize(g->ranks[(size_t)r]); });
}

int32_t sb_group_rank_count(const sb_group *g) { return g ? g->W : -1; }

int sb_group_get_rank(sb_group *g, int32_t rank, sb_solver **out) {
    if (!g || !out) return fail(SB_ERR_INVALID_ARG, "sb_group_get_rank: null argument");
    if (rank < 0 || rank >= g->W) return fail(SB_ERR_INVALID_ARG, "sb_group_get_rank: no such rank");
    *out = g->ranks[(size_t)rank];
    return SB_OK;
}

}  // extern "C"
