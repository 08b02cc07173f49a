// solver_internal.hpp — what the translation units of libsoftbody_mi355x.so share: error plumbing, the run-time RCCL binding, the
// solver object (what owns its device resources: device_handles.hpp). Nothing declared here is exported (exports.map keeps the dynamic symbol table to sb_*).
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree).
// Units: device_handles.hpp (the owning handle types, the table ring, the first-use rule), binding.hip (errors, RCCL / HIP runtime binding), tables_host.cpp (plan -> host tables, no HIP), stream_codec.hpp (the bit layout of the tile constraint stream: the builder's encoders, the kernels' and the validator's decoders), tables.hip (their upload), launch_shape.hpp (which tile_kernel
// instantiation a launch runs: a pure host function), schedule.hip (launches, ghost exchange, the tick), readback.hip (state reads / writes, where the tick-end positions are, kinematic targets), body_state.hip (mass centre, momenta, best-fit rotation: the reduction and the host derivation), impulse.hip (impulses between two ticks), surface_force.hip (wind, air drag and pressure on the render triangles between two ticks), placement.hip (placement between two ticks: one affine map over the whole body), collide.hip (collider contacts between two ticks: spheres, capsules, boxes against every particle), render.hip (render readback: the stage and the entry-point bodies a solver
// and a group share -- render.hpp -- and the solver's entry points), authoring.cpp (the authored mesh behind sb_set_* and sb_group_set_*, the
// window cut; no HIP), validate.hip (table validator), abi.hip (lifecycle, authoring, finalize,
// stats), plan_abi.hip (host-only planner inspection), group.hip (one process driving several devices).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>      // types and prototypes only: the library itself is bound at run time (RcclApi below)
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <type_traits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/softbody.h"
#include "../../include/softbody_plan.h"
#include "../../include/softbody_debug.h"
#include "../../include/softbody_group.h"
#include "kernel_types.hpp"
#include "plan.hpp"
#include "tables_host.hpp"
#include "authoring.hpp"

namespace sbi {

int fail(int code, const std::string &msg);      // records the thread's last error (sb_last_error) and returns code
inline int report(const Status &st) { return st.code == SB_OK ? (int)SB_OK : fail(st.code, st.text); }      // what authoring.cpp answered
const char *last_error_text();

struct HipError : std::runtime_error {
    int code;
    HipError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
#define HIP_CHECK(expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            throw HipError(SB_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)
// RCCL is NOT a link-time dependency. A world == 1 host never loads it (the library is 570 MB); a world > 1 host binds, on
// first use, the librccl.so.1 that is ALREADY in the process when there is one -- a host that imported PyTorch first brought
// PyTorch's own RCCL together with PyTorch's own HIP runtime, which this plugin's libamdhip64.so.7 dependency resolved to as
// well, and a second ROCm stack in one process is the one thing that must not happen -- and the system's otherwise (the
// plugin's RUNPATH: /opt/rocm/lib). What was bound is reported by sb_runtime_info and decides which schedules are admitted.
struct RcclApi {
    void *handle = nullptr;
    bool was_resident = false;
    int version = 0;
    std::string path, error;
    decltype(&ncclGetVersion) GetVersion = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    bool ok() const { return handle != nullptr; }
};
RcclApi &rccl(bool required = true);
#define NCCL_CHECK(expr)                                                                                  \
    do {                                                                                                  \
        ncclResult_t r_ = (expr);                                                                         \
        if (r_ != ncclSuccess)                                                                            \
            throw HipError(SB_ERR_RCCL, std::string(#expr) + ": " + rccl().GetErrorString(r_));          \
    } while (0)

int hip_runtime_version();
bool capture_overlap_ok();      // see binding.hip

}  // namespace sbi

#include "device_handles.hpp"      // Event, Stream, DevBuf, HostBuf, Mirror, TableRing, GraphCache (need HIP_CHECK)
#include "render.hpp"      // the render readback's state (needs them)

namespace sbi {

struct DevHalo {                 // one halo slot: who we talk to and which particles travel
    std::vector<int> peers;
    std::vector<int32_t> send_off, recv_off;  // per peer (+1), in particles
    DevBuf<int32_t> send_idx, recv_idx;
    bool active() const { return !peers.empty(); }
};

struct DevTiling : sbt::TilingScalars {
    DevBuf<sbk::TileDesc> tiles;
    DevBuf<int2> runs_overflow;
    DevBuf<uint32_t> stream;     // per tile: [round words][rest-length dictionary][round data], see stream_codec.hpp
    DevBuf<int32_t> gather;      // T2: particle lists of the tiles (local numbering)
};

// Surface forces (sb_group_apply_surface_forces, surface_force.hip; SPEC.md 2e): the render triangles in device numbering, the render particles
// with their incident-triangle lists (ascending t, one entry per corner slot) and one float4 of scratch per triangle. Built at the first
// call after the triangles changed, released when they change; `bytes` is their share of sb_stats.device_bytes (0 = not built).
struct SurfaceForceTables {
    DevBuf<int32_t> d_tri, d_part, d_off, d_adj;
    DevBuf<float4> d_J;
    int64_t m = 0, n_part = 0, bytes = 0;
};

struct DevGColour {
    int type = 0;
    int32_t count = 0;
    DevBuf<int2> ij;
    DevBuf<int4> quad;
    DevBuf<float> rest;
    DevBuf<float2> rest2;
};

}  // namespace sbi

namespace sbi {

// The tick as a program (schedule.hip tick_program): launches and exchanges in order, tile ranges by name.
enum class StepKind : uint8_t { Tile, T2Layer, GColour, Exchange, ForkExchange, JoinExchange };
enum class TileRange : uint8_t { All, T0Boundary, T0Interior, T1Interior, T1Boundary };
struct TickStep {
    StepKind kind;
    TileRange range;        // Tile: which of the rank's tiles
    bool kin;               // Tile: the fused first kernel carries kinematic targets (tile_kernel kKindMidKinematic)
    int it, substeps;       // Tile: kernel K_it of a tick of `substeps` substeps
    int index;              // T2Layer: layer; GColour: colour; *Exchange: halo slot
};
struct TickShape { int substeps; bool fuse, defer_last, kin; };

// sb_debug_exchange_timing: three events per exchange (start, after the pack / push kernel, end) on the stream it runs on
struct ExchangeTimer {
    bool enabled = false;
    std::vector<Event> pending, join_pending, free_list;      // join_pending: pairs around the compute stream's wait for an overlapped exchange
    void mark(hipStream_t st, bool join = false);
    void recycle();         // everything pending -> free_list
};

}  // namespace sbi

using sbi::DevBuf; using sbi::DevGColour; using sbi::DevHalo; using sbi::DevTiling;

struct sb_plan {
    sbp::Plan plan;
    sbp::LocalPlan local;
    // keep inputs needed by inspection calls
    bool owns_local = true;
};

struct sb_solver {
    sb_desc desc;
    bool finalized = false;
    sbi::Stream stream;
    sbi::Event ev0, ev1;
    ncclComm_t comm = nullptr;
    bool loopback = false;           // SB_DEBUG_LOOPBACK: every peer is this rank itself (1-GPU pipeline test)
    int schedule = SB_SCHEDULE_SERIAL_EAGER;   // world > 1: what desc.halo_schedule resolved to (sb_finalize)
    uint64_t plan_hash = 0;          // hash of the published orders, ownership and plan options (equal on every rank)
    sbi::Stream comm_stream;
    sbi::Event ev_boundary, ev_halo;
    bool overlap_halo = false;       // T0 boundary tiles first, ghost exchange on comm_stream beside the interior
    // What was authored (authoring.hpp): the solver's own, its window of a group's mesh, or -- only read, until finalize_link leaves this
    // rank a copy of what it needs afterwards -- the whole mesh the ranks of a group share with the group
    std::shared_ptr<sbi::AuthoredMesh> mesh = std::make_shared<sbi::AuthoredMesh>();
    bool sharded = false;            // sb_set_domain: the mesh is this rank's window of a larger one
    sb_domain domain{};
    std::vector<int32_t> global_id;  // [n] ids of the window's particles in the whole mesh (sharded only)
    // plan
    std::unique_ptr<sb_plan> plan;
    // device state
    int64_t dev_bytes = 0;
    int64_t n_owned = 0, n_local = 0;
    DevBuf<float> d_pos3;            // packed xyz per local particle
    DevBuf<float> d_wf;              // inverse mass per local particle (static)
    DevBuf<uint8_t> d_w8;            // palette index of the inverse mass (when <= 64 distinct values)
    DevBuf<float> d_wpal;
    bool w_palette = false;
    bool w_uniform = false;          // one distinct inverse mass: the tile kernels skip the per-particle index read
    sbk::PosView pos_view() const { return sbk::PosView{d_pos3.p, d_wf.p}; }
    DevBuf<float> d_prev, d_vel;
    // Previous positions as 8-byte codes against x (prev_code.hpp), decided once at sb_finalize (launch_shape.hpp use_prev_codes): the tile
    // kernels then hand d_prev_code to each other and d_prev holds only the particles whose code does not fit. Nothing else reads either.
    bool prev_codes = false;
    bool lean_coded = false;         // ... and every tile of both tilings is lane-packed: the coded launches run the lean kernels (launch_shape.hpp use_lean_coded)
    DevBuf<uint2> d_prev_code;       // one per local particle
    DevBuf<sbk::TickParams> d_tp;
    DevBuf<float> d_sendbuf, d_recvbuf;   // 3 (slot 1: 6) floats per ghost, peers back to back
    DevTiling tiling[3];             // T0, T1, and the sparse T2 tiles (all layers; see t2_layer_range)
    std::vector<std::pair<int32_t, int32_t>> t2_layer_range;   // device-tile ranges of tiling[2], one per T2 layer
    std::vector<std::unique_ptr<DevGColour>> gcolours;
    std::vector<std::unique_ptr<DevHalo>> halos;   // indexed by halo slot
    sbk::TickParams tp_host{};
    bool tp_valid = false;
    sbi::GraphCache graphs;          // sb_step's executables; key = substeps * 8 + (1: tick starts with the fused kernel) + (2: last kernel deferred) + (4: that kernel carries kinematic targets)
    // Lazy tick boundary: the last kernel of a tick (rounds + collide + velocity write) is deferred; if the next tick
    // has the same parameters it is FUSED with that tick's first kernel into one ordinary mid-tick kernel, otherwise
    // (or whenever state is read or written) it is flushed first. Results are identical either way.
    bool deferred = false;
    int deferred_substeps = 0;
    // Tuning (sb_set_tuning of softbody_debug.h: A/B measurements; the plugin reads no environment variable for any of this)
    uint32_t tune_flags = 0;         // SB_TUNE_* as given; the fields below are what they resolve to
    int win_dwords_cap = 0;          // sb_tuning.win_dwords (0 = the tiling's own window)
    int prev_offset_bytes = 0;       // sb_tuning.prev_offset_bytes: the previous-position array starts this far into its allocation (placement experiment)
    bool lazy_tick = true;           // !SB_TUNE_NO_LAZY_TICK
    int tile_lanes = 0;              // sb_tuning.tile_lanes = 128|256|512 forces the workgroup width of small tiles (0 = by launch size)
    int quad_lanes = 512;            // sb_tuning.quad_lanes = 256|512: workgroup width of tiles that hold tets / hinges (8 waves: every group of the
                                     // 100 k surrogate fits one row of wave slots; 1.99 against 2.11 ms per tick with 4 waves)
    int store_through_max_tiles = 6144;   // sb_tuning.store_through_max_tiles: launches of at most this many tiles store their state through the L2
                                          // (measured: 96^3 -18 %, 128^3 = 4096 tiles -3 %, 160^3 = 8000 tiles +2 %, 256^3 +4 %)
    int store_through_large = 0;          // sb_tuning.store_through_large = mask: the same for larger launches (experiments; bit 0 previous positions, bit 1 positions)
    int narrow_min_tiles = 10240;    // sb_tuning.narrow_min_tiles; measured crossover: 160^3 (8000 tiles) ties, 192^3 (13824) +4 % narrow
    size_t lds_pad = 0;              // sb_tuning.lds_pad_bytes of unused LDS per workgroup (occupancy experiments)
    bool pack_tiles = true;          // !SB_TUNE_NO_PACK: under-full tiles share a workgroup (build_device)
    bool fused_unpack = false;       // the T1 kernels read ghosts from the receive buffer: no unpack launch behind the slot-1 exchange
    bool graph_rccl = false;         // a multi-rank tick, exchange included, is captured in the hipGraph (SB_SCHEDULE_*_GRAPH)
    std::vector<float> h_stage;
    // SB_SCHEDULE_AUTO measured on the devices at hand (schedule.hip calibrate_*): ticks 0 / 1 warm the two eager schedules up (first use of
    // the communicator, of the second stream), ticks 2 .. 5 alternate serialised / overlapped under HIP events, the 7th sb_step decides.
    struct AutoSchedule {
        int state = 0;                       // 0 off, 1 calibrating, 2 decided
        int tick = 0;                        // sb_step calls so far
        sbi::Event ev[8];                    // start / end of the four timed ticks
        int n[2] = {0, 0};                   // ticks timed per schedule
        double decided_ms[2] = {0, 0};       // per tick, slowest rank: [0] serialised, [1] overlapped
    } calib;
    bool group_walk = false;         // a rank of a group whose host thread walks the tick across the ranks (group.hip): exchanges are issued there
    bool capturing = false;          // sb_step is recording the tick into a hipGraph right now
    sbi::ExchangeTimer xtimer;       // sb_debug_exchange_timing
    // peer-store halo transport (SB_HALO_TRANSPORT=peer; aux_kernels.hip.hpp): one mailbox per rank = [header words | ghost segments]
    struct PeerState {
        bool enabled = false, linked = false, fine_grained = false;
        uint32_t *mailbox = nullptr;            // header: words 0-1 = the rank's plan hash, 2 = sharded?, 4 .. 4+2W = its pair hashes; per slot: data flags[world], ack flags[world], epoch, 2 counters; then the offset table
        size_t bytes = 0, data_off_words = 0, off_table = 0;
        int n_slots = 0;
        std::vector<uint32_t *> remote;         // [world]: the ranks' mailboxes as this process sees them (own pointer for itself)
        std::vector<uint8_t> opened;            // remote[r] was mapped with hipIpcOpenMemHandle
        std::vector<std::vector<uint32_t>> my_off;   // [slot][rank]: first word (from the mailbox start) of rank's segment in MY mailbox
        std::vector<sbk::PeerSlot> slots;
        DevBuf<uint32_t> local;                 // 8 ordinary (cached) words per slot: epoch, workgroup counters, go words
        sbi::HostBuf<uint32_t> h_error;         // pinned host word the kernels set when a wait gives up: the host reads it without a copy
        size_t slot_base(int slot, int world) const { return sbt::mailbox_slot_base(slot, world); }
        // ORDER: the mappings of the neighbours' mailboxes are closed before this rank's own mailbox is freed (tables.hip alloc_mailbox made it)
        ~PeerState() {
            for (size_t r = 0; r < remote.size(); ++r) if (opened[r] && remote[r]) (void)hipIpcCloseMemHandle(remote[r]);
            if (mailbox) (void)hipFree(mailbox);
        }
    } peer;
    // asynchronous render readback (sb_readback_begin / sb_readback_end; render.hpp): what a group's render device keeps too ...
    sbi::RenderState render;
    // ... and what is this rank's own: the snapshot runs on the compute stream, in device numbering
    sbi::Event ev_snap[sbi::kSnapSlots];
    DevBuf<int32_t> d_local_to_old;
    DevBuf<float> d_get_scratch;           // caller-numbered staging of the blocking sb_get_* calls (world == 1)
    DevBuf<int32_t> d_render_local;
    std::vector<int32_t> render_local;     // device numbering of render.set's particles
    std::vector<int32_t> cage_local;       // the distinct cage particles of render.emb, device numbering: what a peek has to cover
    // kinematic targets (sb_set_kinematic_positions): a ring of mapped pinned tables the scatter / fill kernels read in place, one table per
    // call: [int32 device particle x count][pad to 16 bytes][float xyz x count] (kin_table_pos_at)
    sbi::TableRing<4> kin_ring;
    std::vector<uint32_t> kin_seen; uint32_t kin_stamp = 0;     // duplicate-id check of sb_set_kinematic_positions
    std::vector<int32_t> local_of_old;     // the rank's numbering -> device numbering (-1: not held), built at first use (readback.hip)
    // Targets are PENDING until the next tick starts: if that tick's first kernel also finishes the tick before (lazy tick boundary),
    // they travel into it (tile_kernel kKindMidKinematic applies them between the old tick's velocity and the new tick's integrate) and the
    // fusion is kept; any other way across the boundary (state read or written, parameters changed, first tick) completes the old
    // tick and scatters them onto the positions (materialise_kinematic).
    int kin_pending = -1, kin_pending_count = 0;      // ring slot that holds them, or -1
    static size_t kin_table_pos_at(int count) { return ((size_t)count * sizeof(int32_t) + 15) / 16 * 16; }      // where the targets start in a table of `count`
    DevBuf<int32_t> d_kin_map;             // per local particle: slot of a pinned particle, -1 for a free one (built at the first use)
    DevBuf<float> d_kin_target;            // 3 floats per pinned particle: pending target or NaN
    int64_t n_kin_fused = 0;               // ticks whose fused first kernel carried targets
    bool kin_fuse = true;                  // !SB_TUNE_NO_KIN_FUSE (A/B: pending targets always complete the previous tick first)
    // impulses (sb_apply_impulses, impulse.hip): the sparse kernels' tables travel like the kinematic targets, one table per call
    sbi::TableRing<4> imp_ring;
    // surface forces (sb_group_apply_surface_forces, surface_force.hip): nothing before the first call
    sbi::SurfaceForceTables surf;
    // Peek (world == 1): a position read while the tick's last kernel is deferred runs tile_kernel<kKindPeek> -- the same rounds + collide on
    // the same inputs, written to d_peek instead of the state -- so the deferred kernel can still be fused with the next tick's first
    // one. A render-set-only readback peeks only at the T0 tiles that hold a render particle (peek_tiles: copies of their descriptors).
    DevBuf<float> d_peek;                  // packed xyz per local particle; only the peeked tiles' entries are ever written or read
    DevBuf<sbk::TileDesc> peek_tiles;
    int32_t n_peek_tiles = -1;             // -1: not built for the current render set
    bool peek_enabled = true;              // !SB_TUNE_NO_PEEK
    // A peek is one more launch; what it saves is the difference between a fused first kernel and a separate last + first kernel. That
    // pays where launches are bandwidth-bound (256^3 render-set readback: 3.49 -> 3.35 ms per tick) and costs where a launch is a fixed
    // latency whatever it covers (every tile resident at once -- 100 k tet mesh: +15 us per tick, 64^3: +2 us; profiles/
    // r03s2_soak_peek.jsonl): peek only from this many T0 workgroups on (sb_tuning.peek_min_tiles).
    int peek_min_tiles = 2048;
    int64_t n_peeks = 0;                   // launches so far (sb_stats.readback_peeks)
    int64_t n_fused = 0;                   // ticks that started with the fused kernel (sb_stats.ticks_fused)
    // Body state (sb_group_get_body_state, body_state.hip; SPEC.md 6f): the reference pose of the owned particles in device order -- kept on
    // the host by sb_finalize (12 bytes per owned particle) and moved to the device by the first POSE query --, the workgroups' rows and
    // the mapped pinned row the final kernel writes (32 sums, 2 counts), both from the first query on
    std::vector<float> ref_pose;
    DevBuf<float> d_ref_pose;
    DevBuf<double> d_body_partials;
    sbi::HostBuf<double> h_body;
    // Placement (sb_group_place, placement.hip; SPEC.md 2d): SB_PLACE_FROM_REFERENCE reads the reference pose of EVERY local particle. The
    // ghosts' part is kept on the host by sb_finalize beside ref_pose (12 bytes per ghost); the first such call puts both on the device
    DevBuf<float> d_place_ref;             // packed xyz per local particle, device order
    std::vector<float> ref_pose_ghost;
    // Reactions (sb_group_collide_reactions, collide.hip; SPEC.md 2g), nothing before the first such call: the workgroups' rows of the pass
    // and their masks, the rows and masks of the first final level, the mapped pinned records the last level writes
    // (SB_COLLIDE_REACTIONS_MAX of 8 words each) and the event recorded behind the last batch, which is all a fetch waits for
    DevBuf<double> d_react_rows, d_react_rows1;
    DevBuf<uint32_t> d_react_masks, d_react_masks1;
    sbi::Event ev_react;
    sbi::HostBuf<double> h_react;
    // Heightfield (sb_group_set_heightfield, heightfield.hip; SPEC.md 2h), nothing before the first set: the rank's copy of the heights, the
    // descriptor they came with, the cull height made of them, and the event recorded behind the last pass that read the table -- what a
    // later set or clear waits for before the memory is written or released
    DevBuf<float> d_hf;
    sb_heightfield hf_desc{};
    float hf_top = 0.0f;
    bool hf_set = false, hf_in_flight = false;
    sbi::Event ev_hf_read;
    // Signed-distance volumes (sb_group_set_distance_field, distance_field.hip; SPEC.md 2i), nothing before the first set: per slot the
    // rank's copy of the samples, the descriptor they came with, and the event recorded behind the last pass that read the slot -- what a
    // later set or clear of that slot waits for before the memory is written or released. The pose is the call's, never kept.
    struct DistanceFieldTable {
        DevBuf<float> d;
        sb_distance_field desc{};
        bool set = false, in_flight = false;
        sbi::Event ev_read;
    };
    DistanceFieldTable df[SB_DISTANCE_FIELD_SLOTS];

    // The destructor holds only what is ORDER; every handle above gives itself back afterwards (members, in reverse order of declaration,
    // none of which depends on another once the device is idle). sb_destroy has made the solver's device current.
    ~sb_solver() {
        // 1. everything the device may still be running for this solver: compute, exchange and render copy stream
        if (stream) (void)hipStreamSynchronize(stream);
        if (comm_stream) (void)hipStreamSynchronize(comm_stream);
        if (render.copy_stream) (void)hipStreamSynchronize(render.copy_stream);
        // 2. the graph executables before the communicator: captured RCCL launches hold references into it
        graphs.clear();
        // 3. the communicator before the streams it was used on (members: they go after this body)
        if (comm) (void)sbi::rccl(false).CommDestroy(comm);
        // (4. IPC mappings before the mailbox: ~PeerState)
    }
};

namespace sbi {

// ---- tables.hip: plan -> device tables (built by tables_host.cpp) ---------------------------------------------------------------------------------------------
sbp::Input make_input(const float *rest, int32_t n, const int32_t *d, int64_t md, const int32_t *v, int64_t mv, const int32_t *b, int64_t mb);
sbp::Domain to_domain(const sb_domain &d);
sb_domain domain_of(const sbp::Input &in);       // abi.hip: what sb_domain_from_mesh measures
// The planner options behind the ABI's fields: ONE rule for sb_finalize and sb_plan_build
sbp::Opts plan_opts(int rank, int world, const int32_t dims[3], int32_t tile_particles, int32_t partition, uint32_t plan_flags,
                    int64_t m_v, int64_t m_b, const sb_domain *domain = nullptr);
constexpr uint32_t kPlanFlagsAll = SB_PLAN_NO_T2 | SB_PLAN_NO_THIRD_LIST | SB_PLAN_NO_CLUSTER_LAYERS | SB_PLAN_NO_MIXED_GROUPS | SB_PLAN_NO_BANK_ORDER | SB_PLAN_NO_TILE_MERGE | SB_PLAN_BALANCED_LISTS(3);
uint64_t hash_plan(const sbp::Plan &P);
void build_device(sb_solver *s);

// ---- schedule.hip: launches, ghost exchange, the tick -----------------------------------------------------------------------------------
sbk::TickParams tick_params(const sb_solver *s, float dt, int substeps);
void upload_tick_params(sb_solver *s, float dt, int substeps);
void peer_link(sb_solver *s);
void halo_exchange(sb_solver *s, int slot, hipStream_t st = nullptr);
bool halo_slot_active(const sb_solver *s, int slot);
void halo_exchange_pre(sb_solver *s, int slot, hipStream_t st);       // the three parts of an exchange, for a host thread that drives several ranks
void halo_exchange_calls(sb_solver *s, int slot, hipStream_t st);
void halo_exchange_post(sb_solver *s, int slot, hipStream_t st);
std::vector<TickStep> tick_program(const sb_solver *s, int substeps, bool fused_first, bool defer_last, bool kin);
struct LaunchTimer;
void run_step(sb_solver *s, const TickStep &st, LaunchTimer *lt);
TickShape begin_tick(sb_solver *s, float dt, int substeps);
void end_tick(sb_solver *s, const TickShape &t);
void flush_deferred(sb_solver *s);
void scatter_kinematic(sb_solver *s, float *dst);
bool can_peek(const sb_solver *s);
void build_peek_subset(sb_solver *s, const std::vector<int32_t> &wanted);
void peek_positions(sb_solver *s, bool subset);
void check_peer_error(sb_solver *s);

// ---- readback.hip -----------------------------------------------------------------------------------------------------------------------
const std::vector<int32_t> &local_of_old(sb_solver *s);
int get_state_owned(sb_solver *s, float *out, bool velocity, const int32_t *id_map);
int set_state_from(sb_solver *s, const float *pos, const float *vel, const int32_t *id_map);
int set_kinematic(sb_solver *s, const int32_t *ids, const float *pos, int32_t count);
// where the tick-end positions are, made valid on the solver's stream (the caller synchronises): a peek while the last kernel is held back
const float *tick_end_positions(sb_solver *s, bool subset = false, const std::vector<int32_t> &wanted_local = {});
// sb_get_bounds: the box of the particles this rank owns, on what sb_get_positions would return now (peeks where that peeks)
int get_bounds_owned(sb_solver *s, float lo[3], float hi[3]);

// ---- body_state.hip: mass centre, momenta, best-fit rotation (SPEC.md 6f) ------------------------------------------------------------------
// the 32 sums over the particles this rank owns (what = SB_BODY_POSE | SB_BODY_MOTION bits; counts = dynamic, pinned): POSE alone peeks
// where get_bounds_owned peeks, MOTION completes the tick's held-back last kernel as a velocity read does
int get_body_sums_owned(sb_solver *s, uint32_t what, double sums[32], int64_t counts[2]);
// every field of *out from the sums (pure host arithmetic; the arguments are valid)
void body_state_derive(const double sums[32], int64_t n_dynamic, int64_t n_pinned, uint32_t what, sb_body_state *out);

// ---- impulse.hip: impulses between two ticks (SPEC.md 2c) ----------------------------------------------------------------------------------
int64_t impulse_triangles_in_force(const RenderState &R);       // triangles of the render mode in force, -1 = none
int validate_impulses(const char *who, const sb_impulse *items, int32_t count, int32_t n, int64_t m_tri, bool rank);
void expand_impulses(const RenderState &R, const sb_impulse *items, int32_t count, std::vector<sb_impulse> &out);      // SURFACE -> PARTICLE-like entries
int apply_impulses_validated(sb_solver *s, const sb_impulse *items, int32_t count);      // PARTICLE / RADIAL, the rank's numbering, owned particles

// ---- surface_force.hip: wind, air drag and pressure on the render triangles between two ticks (SPEC.md 2e) ----------------------------------
int validate_surface_force(const char *who, const sb_surface_force *f);      // the record alone: needs neither a solver nor a device
bool surface_tables_built(const sb_solver *s);                               // false: the next call reads its triangle list
// world == 1; tri: m render triangles in the rank's numbering (read only while the tables are not built); asynchronous on s->stream
int apply_surface_forces_validated(sb_solver *s, const sb_surface_force &f, const int32_t *tri, int64_t m);
void release_surface_tables(sb_solver *s);                                   // the render triangles changed

// ---- placement.hip: placement between two ticks (SPEC.md 2d) -------------------------------------------------------------------------------
int validate_placement(const char *who, const sb_placement *p);      // the struct alone: needs neither a group nor a device
int place_validated(sb_solver *s, const sb_placement &p);            // every local particle, ghosts included; asynchronous on s->stream

// ---- collide.hip: collider contacts between two ticks (SPEC.md 2f) -------------------------------------------------------------------------
int validate_colliders(const char *who, const sb_collider *colliders, int32_t count);      // the list alone: needs neither a group nor a device
int collide_validated(sb_solver *s, const sb_collider *colliders, int32_t count);         // count > 0; every local particle, ghosts included; asynchronous on s->stream
// SPEC.md 2g: the same state, and what the owned particles give back to each collider; 0 < count <= SB_COLLIDE_REACTIONS_MAX; asynchronous
int collide_reactions_validated(sb_solver *s, const sb_collider *colliders, int32_t count);
int get_collider_reactions_owned(sb_solver *s, sb_collider_reaction *out, int32_t count);   // waits for the last call above alone; this rank's `count` records

// ---- heightfield.hip: contacts with a terrain heightfield between two ticks (SPEC.md 2h) ---------------------------------------------------
int validate_heightfield(const char *who, const sb_heightfield *d, const float *heights);      // descriptor and heights alone: needs neither a group nor a device
int validate_heightfield_call(const char *who, float friction, float restitution);
float heightfield_top(const float *heights, int64_t count);                                     // no rounded height of the table exceeds it
int set_heightfield_validated(sb_solver *s, const sb_heightfield &d, const float *heights, float top);      // copies; leaves the tick's stream alone
int clear_heightfield(sb_solver *s);
int collide_heightfield_validated(sb_solver *s, float friction, float restitution);            // every local particle, ghosts included; asynchronous on s->stream

// ---- distance_field.hip: contacts with signed-distance volumes between two ticks (SPEC.md 2i) ----------------------------------------------
int validate_distance_field(const char *who, int32_t slot, const sb_distance_field *d, const float *samples);      // slot, descriptor and samples alone (d may be null: a clear); needs neither a group nor a device
int validate_distance_field_pose(const char *who, int32_t slot, const sb_distance_field_pose *p);
int set_distance_field_validated(sb_solver *s, int32_t slot, const sb_distance_field &d, const float *samples);    // copies; leaves the tick's stream alone
int clear_distance_field(sb_solver *s, int32_t slot);
int collide_distance_field_validated(sb_solver *s, int32_t slot, const sb_distance_field_pose &p);                 // every local particle, ghosts included; asynchronous on s->stream

// ---- abi.hip: the phases of sb_finalize (a group runs them itself) ----------------------------------------------------------------------
int finalize_local(sb_solver *s);                       // plan + tables, this rank alone (= finalize_plan, then finalize_device)
int finalize_plan(sb_solver *s);                        //   host work only: schedule, plan, plan hash
int finalize_device(sb_solver *s);                      //   device tables, streams
void reset_authoring(sb_solver *s);                     // forget a window (sb_set_domain) and the plan made from it
std::vector<uint64_t> agreement_record(const sb_solver *s, bool failed);
uint32_t plan_shape(const sb_solver *s);                // the tick program's shape: tiling on / off, leftover (T2) layers, global colours (= halo slots)
int check_agreement(const std::vector<uint64_t> &all, int W, int me);
int finalize_agree(sb_solver *s, int local_rc);         // RCCL all-gather of the agreement records (entered by a failed rank too)
int finalize_link(sb_solver *s);                        // peer mailboxes over the communicator, bookkeeping
template <class F>
int guarded(F &&f) {
    try {
        return f();
    } catch (const HipError &e) {
        return fail(e.code, e.what());
    } catch (const std::bad_alloc &) {
        return fail(SB_ERR_NOMEM, "out of host memory");
    } catch (const std::exception &e) {
        return fail(SB_ERR_INVALID_ARG, e.what());
    }
}

int set_device(const sb_solver *s);

}  // namespace sbi
