/*
 * softbody_group.h — ONE process driving SEVERAL MI355X behind one `Softbody : MonoBehaviour` component.
 *
 * A Unity player is one process. The per-rank entry points of softbody.h (sb_desc.rank / world, sb_comm_init) are the form a
 * one-process-per-GPU job uses (bench.py under torch.distributed.run); a component in a player uses this header instead: one handle
 * that owns one solver per device, authored ONCE with the whole mesh, stepped with ONE call, read back gathered in the caller's
 * numbering -- csharp/Softbody.cs `deviceCount`.
 *
 * Reference interface replaced: NONE EXISTS (/root/reference/README.md:1 is the whole reference tree). [BUILDER-DEFINED] from
 * BASELINE.json:5 ("keeping the reference's Softbody component / MonoBehaviour update API surface ... the mesh is spatially partitioned
 * across the 8 GPUs of one node with RCCL halo exchange") and SURVEY.md §1 L1' ("one process x 8 devices"), §8b (`device_count`).
 *
 * How a tick runs. Two host models (sb_group_create flags), same results:
 *   default        ONE HOST THREAD PER RANK, owned by the group: sb_group_step hands the tick to the ranks' threads, each enqueues its own
 *                  rank's launches and exchanges (exactly what a one-process-per-GPU job does, hipGraph replay and captured schedules included)
 *                  and the call returns when all have ENQUEUED -- the host cost of a tick is that of one rank, whatever the number of GPUs.
 *                  A tick of 256^3 on 8 ranks is ~30 launches + 10 exchanges per rank and ~0.7 ms of GPU time: one thread issuing all of it for
 *                  8 devices would be the bottleneck (measured on one device: profiles/r04_group_host_models.txt).
 *   SB_GROUP_WALK  no thread of the plugin's own: the CALLING thread walks the tick LAUNCH BY LAUNCH across the ranks (every rank's tile
 *                  kernel K_it, then every rank's next launch, ...), never rank by rank, so the launches of one step run side by side on the
 *                  devices; a ghost exchange is issued for all ranks together: pack kernels on every rank's stream, then the sends and receives
 *                  of ALL ranks inside ONE ncclGroupStart / ncclGroupEnd (a single thread that posted one rank's receive outside a group would
 *                  wait for a send it has not posted yet), then the unpack kernels (none where the T1 kernels read the receive buffer
 *                  themselves). The communicators are created together inside one ncclGroupStart / ncclGroupEnd. Eager schedules only, and
 *                  SB_SCHEDULE_AUTO is the serialised one here (its measurement of the two eager schedules runs on the ranks' own threads).
 * Transports (sb_desc.halo_transport): SB_TRANSPORT_RCCL as above; SB_TRANSPORT_PEER = the mailbox transport of softbody.h with the mailboxes
 * connected by plain pointer (sb_group_finalize enables peer access between the devices): push and unpack kernels only, nothing on the host.
 * The lazy tick boundary, the peek, kinematic targets and the render readback work as for a single solver; results are bit-identical to a
 * single-device solver of the same mesh (same published order: the plan does not depend on the partition).
 *
 * UNVERIFIED BETWEEN TWO DEVICES: the build and test boxes have one GPU. Everything here is verified with all ranks on ONE device
 * (tests/test_gpu_group.py: bitwise against the CPU oracle); several ranks on one device need a hardware queue each for the PEER transport
 * (environment GPU_MAX_HW_QUEUES >= ranks); RCCL refuses two ranks on one device, so its legs run as self-exchanges there (SB_DEBUG_LOOPBACK).
 */
#ifndef SOFTBODY_MI355X_GROUP_H
#define SOFTBODY_MI355X_GROUP_H

#include "softbody.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SB_GROUP_WALK 1u               /* sb_group_create flags: no plugin threads, the calling thread walks the tick across the ranks (see above) */
#define SB_GROUP_WHOLE_MESH 2u         /* never cut windows: every rank is handed (and plans) the whole mesh, whatever the partition (see sb_group_finalize) */

typedef struct sb_group sb_group;      /* opaque, plugin-owned */

/* ---- lifecycle ------------------------------------------------------------------------------------------------------------------------- */
/* desc: the settings of EVERY rank (gravity, damping, tile_particles, partition, part_dims, plan_flags, halo_transport, halo_schedule,
 * debug_flags); its device / rank / world fields are ignored. devices: n_devices HIP ordinals, rank r runs on devices[r] (NULL = 0, 1, ...,
 * n_devices - 1); an ordinal may repeat (several ranks on one device: tests). n_devices = 1 is a plain single-device solver behind the same
 * entry points, so a component needs only this header. The ranks' solvers exist from here on (sb_group_get_rank: sb_set_tuning).
 * Calling convention: calls on ONE group must not overlap in time (a component calls from Unity's main thread; the group's own threads
 * are an implementation detail behind each call); different groups are independent. A call that fails changes nothing it can avoid
 * changing, with one exception: after a failed sb_group_finalize (or a failed sb_group_step: a rank's device or transport error) the group
 * is good for sb_group_destroy only -- its ranks may no longer be in the same tick state. */
int sb_group_create(const sb_desc *desc, const int32_t *devices, int32_t n_devices, uint32_t flags, sb_group **out);
int sb_group_destroy(sb_group *g);

/* ---- authoring: the whole mesh, once (same arguments as the sb_set_* of softbody.h) ------------------------------------------------------- */
int sb_group_set_particles(sb_group *g, const float *pos_xyz, const float *vel_xyz /* may be NULL = 0 */, const float *inv_mass, int32_t n);
int sb_group_set_rest_positions(sb_group *g, const float *rest_xyz, int32_t n);
int sb_group_set_distance_constraints(sb_group *g, const int32_t *ij, const float *rest_len, int32_t m, float compliance);
int sb_group_set_volume_constraints(sb_group *g, const int32_t *ijkl, const float *rest_vol, int32_t m, float compliance);
int sb_group_set_bending_constraints(sb_group *g, const int32_t *ijkl, const float *rest_cs, int32_t m, float compliance);
int sb_group_set_ground_plane(sb_group *g, float nx, float ny, float nz, float d, int32_t enabled);
/* Plan, partition, upload on every device (the ranks plan side by side on host threads), connect the transport, verify that the ranks
 * planned consistently (plan hash + pair hashes, as sb_finalize does across processes).
 * Sharded authoring: every rank is handed only ITS WINDOW of the mesh (cut here from the one copy the group holds) instead of the whole
 * mesh where that is known to reproduce the whole-mesh plan -- a LATTICE-LIKE body: distance constraints only, filling its bounding box
 * (sb_domain.fill = 1) -- and the partition is the block grid: sb_desc.partition = SB_PARTITION_BLOCKS, or SB_PARTITION_AUTO on at least
 * 2 M particles (for which AUTO takes the block grid anyway; below that, eight whole-mesh plans cost less than they save). Every other mesh
 * (tets, hinges, a body that fills its box unevenly: their colouring and leftover layers are not local to a window) is planned whole on
 * every rank, under whatever partition was asked for (SB_PARTITION_AUTO may then choose RCB). SB_GROUP_WHOLE_MESH forces that for any mesh.
 * The rule is a filter, not the guarantee: the ranks' plans are compared before anything is uploaded, and where windows did NOT reproduce the
 * whole-mesh plan (e.g. particles on a line joined by nearest-neighbour springs pass the filter) every rank is handed the whole mesh and
 * plans again -- sb_group_finalize succeeds either way, only slower. */
int sb_group_finalize(sb_group *g);

/* ---- the hot path (FixedUpdate) ---------------------------------------------------------------------------------------------------------- */
int sb_group_step(sb_group *g, float dt, int32_t substeps);

/* ---- state, gathered in the caller's numbering --------------------------------------------------------------------------------------------- */
/* What these do to a tick whose last kernel is held back (softbody.h, sb_step), on every rank alike: sb_group_get_positions peeks where
 * sb_get_positions peeks (the tick stays fusable, pending kinematic targets show and stay pending) and completes the tick elsewhere;
 * sb_group_get_velocities and sb_group_set_state complete it and land pending kinematic targets: the next sb_group_step starts unfused. */
int sb_group_get_positions(sb_group *g, float *pos_xyz_out, int32_t n);      /* every entry written: each rank delivers what it owns */
int sb_group_get_velocities(sb_group *g, float *vel_xyz_out, int32_t n);
int sb_group_set_state(sb_group *g, const float *pos_xyz, const float *vel_xyz, int32_t n);
/* Kinematic targets (sb_set_kinematic_positions): ids in the caller's numbering, each at most once; every rank takes the ones it owns.
 * The call leaves a held-back tick held back, and the move rides the next tick's fused first kernel -- unless targets of an earlier call
 * are still pending on any rank (two moves without a tick between them): the earlier one takes effect first, which completes the tick on
 * EVERY rank, also on one that owns none of either call's targets, so that the ranks stay in the same tick state. */
int sb_group_set_kinematic_positions(sb_group *g, const int32_t *ids, const float *pos_xyz, int32_t count);
/* Impulses between two ticks (sb_apply_impulses, SPEC.md 2c), same contract, in the whole mesh's numbering: the list is validated once,
 * SURFACE items are expanded on the host from the group's own copies of the triangles and the embedding (a cage may straddle ranks),
 * every rank is handed its entries in order and in its numbering, RADIAL items go to every rank unchanged. Every rank completes its
 * tick's held-back last kernel, so the ranks stay in the same tick state. Both host models. */
int sb_group_apply_impulses(sb_group *g, const sb_impulse *items, int32_t count);
/* Surface forces between two ticks (SPEC.md 2e): wind, air drag and internal pressure on the render triangles of
 * sb_group_set_render_triangles -- a cloth that flutters, a shell the air slows down, a closed skin that is inflated. One call applies one
 * record to every triangle, from the tick-end positions and velocities, in binary32 without FMA. Per triangle with unit normal n (right-hand
 * rule of its winding), area A, velocity vt = the mean of its corners' and u = wind - vt:
 *     F = A * (normal * (u.n) n + tangential * (u - (u.n) n)) + pressure * A * n
 * and every corner takes a third of the impulse dt * F, times its inverse mass. The force is linear in u (plain drag): normal > tangential
 * makes a sail, wind = 0 is still-air drag, pressure pushes along n. Every triangle is evaluated on the state as it was before the call;
 * a particle then adds its incident triangles' shares in ascending triangle order, once per corner slot that names it. A triangle whose
 * doubled area squared is below 2^-96, infinite or NaN is skipped. A pinned particle (inverse mass 0), a particle in no triangle and a
 * particle in skipped triangles only keep their velocity's bits; positions never change. A velocity component that comes out NaN is stored
 * as the quiet NaN 0x7fc00000 (SPEC.md 2c).
 * The scheme is explicit: a particle overshoots once inverse mass * dt * max(normal, tangential) * (incident area / 3) exceeds 1 -- the
 * caller's choice of coefficients.
 * Errors, all before anything changes (the record is checked before the group is touched): SB_ERR_INVALID_ARG for a null argument, a
 * non-zero flag or reserved field, a NaN or infinite wind, normal, tangential, pressure or dt, normal < 0, tangential < 0, dt <= 0;
 * SB_ERR_STATE before sb_group_finalize and while no render triangles are set; SB_ERR_UNSUPPORTED while a render embedding is in force (its
 * triangles index skinned vertices, which have no velocities of their own) and on a group of more than one rank (a partitioned body's
 * triangle needs positions and velocities of corners that another rank owns, and no rank holds those at a tick's end --
 * sb_readback_get_normals is unsupported on a rank for the same reason). Neither limit has a host fallback. A refused call leaves every bit
 * of the state as it was, and the tick's last kernel held back.
 * Asynchronous like sb_group_step (two kernels on the rank's stream). Velocities exist only once a tick is complete, so the call completes
 * the tick's held-back last kernel (and lands pending kinematic targets) first: THE NEXT sb_group_step STARTS UNFUSED, as after
 * sb_group_apply_impulses. The tables (triangles in device numbering, incident lists, 16 bytes of scratch per triangle) are built at the
 * first call after sb_group_set_render_triangles and released by the next sb_group_set_render_triangles; they count in the rank's
 * sb_stats.device_bytes. Nothing is allocated before the first call. */
typedef struct {                 /* 44 bytes */
    float    wind[3];            /* air velocity, world space */
    float    normal, tangential; /* drag coefficients along and across the triangle's normal, >= 0 */
    float    pressure;           /* along the winding's right-hand normal; negative deflates */
    float    dt;                 /* > 0: the time the force acts for (the tick's dt) */
    uint32_t flags;              /* none defined: must be 0 */
    int32_t  reserved[3];        /* must be 0 */
} sb_surface_force;
int sb_group_apply_surface_forces(sb_group *g, const sb_surface_force *force);

/* ---- render readback (same contract as sb_readback_* / sb_set_render_triangles of softbody.h) -------------------------------------------- */
/* Every rank snapshots the particles it owns (peeking while its tick's last kernel is held back) straight into ONE buffer on the render device
 * (rank 0's; peer stores), whole array or render set; the vertex normals are computed there on the gathered snapshot, then one copy to pinned
 * host memory. */
int sb_group_set_render_triangles(sb_group *g, const int32_t *tri_abc, int32_t m);
int sb_group_set_readback_render_set_only(sb_group *g, int32_t render_set_only);
/* Embedded render vertices (sb_set_render_embedding; cage indices in the whole mesh's numbering): every rank snapshots the cage particles it
 * owns into the gather buffer (its peek covers only the tiles that hold one), the render device skins the visual mesh from it and computes
 * the normals of the skinned array; sb_group_readback_end / sb_group_readback_get_normals then deliver m_vertices*3 floats. Same
 * validation, same exclusion against sb_group_set_render_triangles. */
int sb_group_set_render_embedding(sb_group *g, const int32_t *cage_ijkl, const float *weights4, int32_t m_vertices,
                                  const int32_t *tri_abc, int32_t m_tri);
/* Render tangents (sb_set_render_uvs / sb_readback_get_tangents, SPEC.md 6c; UVs indexed by whole-mesh particle, or by render vertex of the
 * embedding): the same contract on the gathered snapshot -- the render device computes normals and tangents in one kernel after the gather, in
 * all three modes (full, render-set-only, embedded). Nothing changes on the ranks. */
int sb_group_set_render_uvs(sb_group *g, const float *uv /* 2 floats per vertex */, int32_t count);
int sb_group_readback_begin(sb_group *g);
int sb_group_readback_end(sb_group *g, const float **pos_xyz_out);
int sb_group_readback_get_normals(sb_group *g, const float **normal_xyz_out);
int sb_group_readback_get_tangents(sb_group *g, const float **tangent_xyzw_out);
int sb_group_readback_get_render_set(sb_group *g, const int32_t **ids_out, int32_t *count_out);
/* Bounding box (sb_set_readback_bounds / sb_readback_get_bounds / sb_get_bounds, SPEC.md 6d), same contract. The readback box is computed on the
 * render device on the array the group delivers -- the gathered snapshot, the compact render set or the skinned vertices -- after the gather.
 * sb_group_get_bounds asks every rank for the box of what it owns (each peeks or completes its tick as sb_group_get_positions would make it; 32
 * bytes per rank) in both host models and combines the answers on the host: component-wise min / max, then + 0.0f. */
int sb_group_set_readback_bounds(sb_group *g, int32_t enabled);
int sb_group_readback_get_bounds(sb_group *g, float lo_xyz[3], float hi_xyz[3]);
int sb_group_get_bounds(sb_group *g, float lo_xyz[3], float hi_xyz[3]);
/* Ray casts (sb_readback_raycast, SPEC.md 6e), same contract, against the snapshot the last sb_group_readback_end returned: on the render
 * device, on the gathered snapshot (whole array or render set) or the skinned vertices, in both host models -- the ranks take no part. */
int sb_group_readback_raycast(sb_group *g, const float *rays /* 8 floats per ray */, int32_t count, sb_ray_hit *hits_out);
/* Closest points (SPEC.md 6g): what Collider.ClosestPoint, Physics.CheckSphere and Physics.OverlapSphere are to a rigid body, for the deformed
 * render mesh -- the ray cast's twin. For each query (x, y, z, max_distance), world space, the nearest point on the triangles of the snapshot
 * the last sb_group_readback_end returned: the render triangles over the gathered snapshot (whole array or render set), or the embedding's
 * triangles over the skinned vertices. Brute force over every triangle on the render device, two launches per batch of 256 queries and no
 * atomics; per triangle the closest point by its Voronoi regions (vertex, edge, face), in binary32 without FMA, bit for bit SPEC.md 6g.
 *  - hits_out[r] = {triangle, distance, u, v}: point = (1 - u - v) p[a] + u p[b] + v p[c] with (a, b, c) the triangle's corners, exactly
 *    what sb_ray_hit's (u, v) mean, so triangle, u, v go into an SB_IMPULSE_SURFACE item unchanged (penetration of a sphere of radius r:
 *    r - distance; INTEGRATION.md has the loop). Among equally near triangles the lowest index. Nothing within max_distance: -1, 0, 0, 0.
 *  - The limit is compared squared: a triangle is a candidate iff dd <= max_distance * max_distance (and dd is finite), dd the squared
 *    distance in binary32; distance = sqrtf(dd) of the winner. max_distance = 0 finds only points on the surface (dd == 0); +inf is allowed.
 *  - A triangle with a NaN or infinite corner is never returned and removes nothing else. Known limitation: a triangle whose deciding
 *    region divides 0 by 0 -- a repeated corner, some collinear corners -- is no candidate either, although it has a nearest point.
 *  - Synchronous, on the ray cast's stream and in its buffers (4 MB, allocated at the first cast or query and counted from then on; larger
 *    counts walk in batches). It answers for the snapshot ended last whatever has been stepped or begun since, waits for no pending
 *    snapshot, does not peek and leaves the tick's held-back last kernel alone: sb_stats.ticks_fused and readback_peeks do not change.
 *  - SB_ERR_INVALID_ARG, nothing written to hits_out: a null group, count < 0, a null queries or hits_out with count > 0, a NaN or infinite
 *    coordinate, a max_distance that is NaN or negative. SB_ERR_STATE exactly where sb_group_readback_raycast returns it: no readback has
 *    ended, or the snapshot ended last has no triangles (taken without them, or the render mode was set again since). count = 0 returns
 *    SB_OK once the state checks pass.
 * The entry point is the group's only (a group of one rank is the plain solver, as for sb_group_place). Both host models; the ranks take no part. */
typedef struct { int32_t triangle; float distance, u, v; } sb_closest_hit;      /* 16 bytes, the layout of sb_ray_hit; triangle = -1: nothing within max_distance */
int sb_group_readback_closest_points(sb_group *g, const float *queries /* 4 floats per query: x, y, z, max_distance */, int32_t count, sb_closest_hit *hits_out);

/* ---- body state: where the body is and how it moves (SPEC.md 6f) ------------------------------------------------------------------------- */
/* What Rigidbody.worldCenterOfMass / .velocity / .angularVelocity and transform.position / rotation are to a rigid body, for a soft one:
 * mass centre, momenta, kinetic energy and the rigid frame that fits the deformed body best -- a few hundred bytes instead of the state.
 * Every rank reduces the DYNAMIC particles it owns (inverse mass > 0; pinned ones are only counted) to 32 mass-weighted sums in binary64 on
 * its own device, two launches and no atomics; the host adds the ranks' sums in rank order and derives the fields below from the totals.
 * The sums depend on the device order of the particles, so SPEC.md 6f gives them an error bound and run-to-run determinism, not bits:
 * two calls on the same state return the same bits. Non-finite inputs propagate by IEEE rules.
 * sums[]: 0 mass; 1..3 sum m x; 4..6 sum m q; 7..12 sum m x x^T (xx, yy, zz, xy, xz, yz); 13..21 sum m x q^T (row = component of x);
 * 22..24 sum m v; 25..27 sum m (x cross v); 28 sum m |v|^2; 29..31 zero -- x, v the tick-end state, q the reference pose (what
 * sb_group_set_rest_positions gave, else the positions of sb_group_set_particles), all about the world origin. A slot and a field that
 * `what` did not ask for are 0, the rotation then identity. POSE gives slots 0..21, MOTION 0..3, 7..12 and 22..28. */
#define SB_BODY_POSE   1u   /* positions only: peeks where sb_group_get_bounds peeks; the tick stays fusable */
#define SB_BODY_MOTION 2u   /* needs velocities: completes the tick's held-back last kernel, as sb_group_get_velocities does */
/* sb_body_state.flags */
#define SB_BODY_NO_MASS            1u   /* no dynamic particle: every field 0, rotation identity */
#define SB_BODY_DEGENERATE_POSE    2u   /* apq has rank below 2 (sigma_2 <= 1e-12 sigma_1: one particle, collinear poses): rotation identity */
#define SB_BODY_DEGENERATE_INERTIA 4u   /* inertia tensor with lambda_min <= 1e-12 lambda_max (collinear particles, fewer than 3): angular_velocity 0 */

typedef struct {
    int64_t n_dynamic, n_pinned;
    uint32_t what, flags;
    double sums[32];
    double mass, com[3], ref_com[3], second_moment[6], apq[9], rotation[4];     /* second_moment about com, in the order of slots 7..12;
                                                                                    apq = sum m (x - com)(q - ref_com)^T, row-major;
                                                                                    rotation: unit quaternion (x, y, z, w), w >= 0, of the
                                                                                    polar factor of apq with det = +1 (reference -> world) */
    double momentum[3], velocity[3], angular_momentum[3], angular_velocity[3], kinetic_energy;    /* angular_momentum about com;
                                                                                    angular_velocity = I^-1 L, I = tr(C) 1 - C */
} sb_body_state;

/* Synchronous, like sb_group_get_bounds, in both host models. SB_ERR_INVALID_ARG (null argument, what == 0, an unknown bit) leaves *out
 * untouched; SB_ERR_STATE before sb_group_finalize. The first POSE query uploads the reference pose (12 bytes per owned particle) and the
 * first query of any kind allocates the workgroups' rows; until then sb_stats.device_bytes is what it was. */
int sb_group_get_body_state(sb_group *g, uint32_t what, sb_body_state *out);
/* Pure: no group, no GPU. A host adds the sums[] of several bodies (and their counts) and derives the compound body's state; slots `what`
 * does not cover are ignored. SB_ERR_INVALID_ARG as above, or for a negative count. */
int sb_group_body_state_from_sums(const double sums[32], int64_t n_dynamic, int64_t n_pinned, uint32_t what, sb_body_state *out);

/* ---- placement: move, rotate, respawn between two ticks (SPEC.md 2d) --------------------------------------------------------------------- */
/* What transform.position = ..., Rigidbody.MovePosition / MoveRotation and a respawn are to a rigid body: ONE affine map over positions and
 * velocities of the whole body, on the devices -- one streaming pass per rank over every particle it holds, ghosts included (the same
 * arithmetic on a ghost gives its owner's bits: no exchange) -- instead of sb_group_get_positions + sb_group_get_velocities + a host loop +
 * sb_group_set_state. Per particle, in binary32 without FMA (SPEC.md 2d has the parentheses):
 *     x' = m (src - from) + to,   src = x, or the reference pose q (SPEC.md 6f) under SB_PLACE_FROM_REFERENCE
 *     v' = m v                    for inverse mass > 0 (a rotated body keeps flying, rotated), or
 *     v' = lin + ang x (x' - to)  under SB_PLACE_SET_VELOCITY and always under SB_PLACE_FROM_REFERENCE (lin = ang = 0: at rest)
 * A pinned particle moves with the body (no spring to a pin is stretched) and keeps its velocity's bits; SB_PLACE_KEEP_PINNED leaves it
 * entirely alone (a body hanging from a world anchor). m is any finite row-major 3x3 matrix; rest lengths do not scale with it. A written
 * component that comes out NaN is stored as 0x7fc00000. Asynchronous; completes every rank's held-back last kernel first, as
 * sb_group_apply_impulses does, which lands pending kinematic targets (old frame) before they are mapped like every other position. The
 * ground plane, the render snapshot delivered last and the render device take no part. */
#define SB_PLACE_FROM_REFERENCE 1u
#define SB_PLACE_SET_VELOCITY   2u
#define SB_PLACE_KEEP_PINNED    4u
typedef struct {
    uint32_t flags, reserved;      /* SB_PLACE_*; reserved = 0 */
    float m[9], from[3], to[3], lin[3], ang[3];
} sb_placement;                    /* 92 bytes */
/* SB_ERR_INVALID_ARG (null argument, unknown flag bit, reserved != 0, a NaN or infinite field: all checked before the group is touched),
 * SB_ERR_STATE before sb_group_finalize; a refused call changes nothing. The first SB_PLACE_FROM_REFERENCE call uploads the reference pose
 * of every particle a rank holds (12 bytes each); until then sb_stats.device_bytes is what it was. Both host models. */
int sb_group_place(sb_group *g, const sb_placement *p);

/* ---- collider contacts: spheres, capsules and boxes between two ticks (SPEC.md 2f) ------------------------------------------------------- */
/* What a scene's SphereCollider, CapsuleCollider and BoxCollider are to a rigid body: the body rests on them, slides off them and is shoved
 * by them. ONE streaming pass per rank over every particle it holds, ghosts included (the same arithmetic on a ghost gives its owner's
 * bits: no exchange), instead of a closest-point query, a penetration test and a SURFACE impulse per collider and frame. Per particle with
 * inverse mass > 0 the list is walked in order -- the position and velocity after collider k are the input of collider k + 1 -- in binary32
 * without FMA (SPEC.md 2f has the parentheses):
 *     SPHERE  (a, radius)        hit iff |x - a|^2 < radius^2;      n = (x - a) / |x - a| ((0, 1, 0) at the centre), depth = radius - |x - a|
 *     CAPSULE (a, b, radius)     the sphere's rule about the closest point of the segment a b
 *     BOX     (a, rot, half)     q_k = (x - a) . rot[3k..3k+2]; hit iff |q_k| < half[k] for k = 0, 1, 2; the exit face is the one with the
 *                                smallest half[k] - |q_k| (ties: the lowest k), n = +-row k. rot: three orthonormal world-space axes, not checked
 *     x' = x + depth n           vc = lin + ang x (x' - a), u = v - vc, un = u . n
 *     un < 0 (approaching):      v' = vc + (ut' + restitution (-un) n), ut' the tangential part of u shortened by friction (-un) (Coulomb;
 *                                removed when shorter than that: stick). Otherwise the velocity is not written.
 * A particle with inverse mass 0 is left entirely alone, and a particle that no collider touches keeps every bit of its position and
 * velocity: a call that touches nothing changes nothing. A NaN or infinite position is never hit. A written component that comes out NaN
 * is stored as 0x7fc00000. Contacts are resolved once per call (per tick, not per substep); particles collide, not triangles (a collider
 * thinner than the particle spacing passes between them); this call reports nothing back to the collider (sb_group_collide_reactions below
 * does); there is no self-collision. Asynchronous;
 * completes every rank's held-back last kernel first, as sb_group_place does, which lands pending kinematic targets; the next tick starts
 * unfused. The ground plane, the render snapshot delivered last, the render device and a render embedding take no part. */
#define SB_COLLIDER_SPHERE  0u
#define SB_COLLIDER_CAPSULE 1u
#define SB_COLLIDER_BOX     2u
typedef struct {
    uint32_t shape, flags;         /* SB_COLLIDER_*; flags = 0 */
    float a[3], b[3];              /* SPHERE: centre a. CAPSULE: segment a b. BOX: centre a. a is also the pivot of ang */
    float rot[9], half[3];         /* BOX: the axes as rows, the half extents along them */
    float radius;                  /* SPHERE, CAPSULE */
    float lin[3], ang[3];          /* the collider's velocity at a and its angular velocity (radians per second) */
    float friction, restitution;   /* Coulomb coefficient >= 0; restitution in [0, 1] */
    int32_t reserved[3];           /* 0 */
} sb_collider;                     /* 128 bytes */
/* count colliders in list order; calls apply in call order. count == 0 passes the checks and does nothing at all (the tick stays held
 * back). SB_ERR_INVALID_ARG (null group, count < 0, null colliders with count > 0, an unknown shape, flags or a reserved word != 0, a NaN
 * or infinite field -- of any shape's, used or not --, radius < 0, a negative half, friction < 0, restitution outside [0, 1]: all checked
 * before the group is touched), SB_ERR_STATE before sb_group_finalize; a refused call changes nothing. The list is copied before the call
 * returns. No device memory is allocated. Both host models, any number of ranks. */
int sb_group_collide(sb_group *g, const sb_collider *colliders, int32_t count);

/* ---- reactions: the impulse and torque the body gives back to each collider (SPEC.md 2g) ------------------------------------------------ */
/* sb_group_collide leaves the colliders alone; this pair reports what Newton's third law owes them, so that the host can apply it to its
 * rigid bodies (the plugin never moves a collider). sb_group_collide_reactions does to positions and velocities EXACTLY what
 * sb_group_collide does with the same list -- the same bits, the same ordering rules (completes the held-back kernel, the next tick starts
 * unfused, count == 0 does nothing to the state, asynchronous), the same refusals and count > SB_COLLIDE_REACTIONS_MAX on top -- and in the
 * same pass adds up, per collider k of the list, over the particles a rank OWNS (a ghost is its owner's to count) that collider k hit
 * (inverse mass w > 0, position written), with the state as collider k found it and left it, in binary64 on the binary32 values:
 *     m = 1 / w,   dv = v_before - v_after (v_after = v_before's bits where the velocity was not written: a separating particle adds
 *     exactly 0, a non-finite velocity propagates by IEEE rules),   p = x' - a (the binary32 difference of 2f)
 *     impulse = sum m dv      angular_impulse = sum p x (m dv)      contact_mass = sum m      n_contacts = how many
 * The position push carries no impulse: only the velocity change is reported. Contraction and the order of additions are free, so the
 * sums come with an error bound instead of bits (SPEC.md 2g derives it): |sum - exact| <= (n_contacts + 16) 2^-52 A, A the sum of the
 * absolute values of the elementary products. The same state and list give the same bits (fixed merge order, no atomics); a sum that is
 * not finite is NaN, +inf or -inf as the exact evaluation is. The first call allocates the workgroups' rows (about 1 byte per particle a
 * rank holds, counted in sb_stats.device_bytes) and a pinned result of SB_COLLIDE_REACTIONS_MAX records per rank; later calls allocate
 * nothing, and sb_group_collide never does. */
typedef struct {
    double  impulse[3];            /* on the collider, simulation space:  sum m (v_before - v_after) */
    double  angular_impulse[3];    /* about the collider's point a:       sum p x m (v_before - v_after) */
    double  contact_mass;          /* sum m over the particles this collider hit */
    int64_t n_contacts;            /* how many it hit */
} sb_collider_reaction;            /* 64 bytes */
#define SB_COLLIDE_REACTIONS_MAX 1024
int sb_group_collide_reactions(sb_group *g, const sb_collider *colliders, int32_t count);
/* The records of the LAST sb_group_collide_reactions call, the ranks' rows added in rank order: writes min(count, capacity) records and
 * the list's count (0 before any such call and after one with count == 0). Waits for that call alone -- an event recorded behind its
 * launches, no device-wide synchronise: a tick launched after it keeps running and keeps its fused boundary. May be called any number
 * of times and returns the same bits each time; sb_group_collide, a tick or any other call leaves the stored records alone, the next
 * reactions call replaces them. SB_ERR_INVALID_ARG (null g or count_out, capacity < 0, null out with capacity > 0), SB_ERR_STATE before
 * sb_group_finalize. */
int sb_group_get_collider_reactions(sb_group *g, sb_collider_reaction *out, int32_t capacity, int32_t *count_out);

/* ---- heightfield contacts: a terrain between two ticks (SPEC.md 2h) --------------------------------------------------------------------- */
/* What a scene's Terrain is to a rigid body: ground that is not flat. A height map of nx * nz samples, h[iz * nx + ix] in simulation units
 * along `up`, stands in a frame of its own -- sample (0, 0) at height 0 is the point a; ix grows along row 0 of rot, `up` is row 1, iz
 * grows along row 2 (orthonormal, not checked) -- with the spacing cell[0] along row 0 and cell[1] along row 2. Every cell is two
 * triangles, cut along the diagonal from sample (ix + 1, iz) to (ix, iz + 1). sb_group_set_heightfield COPIES descriptor and heights (the
 * caller may free both on return) into a table on every rank's device -- 4 nx nz bytes, counted in sb_stats.device_bytes, given back when
 * the table is cleared (desc == NULL), replaced (a table of the same size reuses the memory) or the group destroyed. It does not complete
 * a held-back tick: a set between two ticks leaves their fusion alone. A pass of the table before still in flight is waited for (its
 * own event, never the device) before its memory is written or released, so that pass reads the table it was given.
 *
 * sb_group_collide_heightfield is ONE streaming pass per rank over every particle it holds, ghosts included (the same arithmetic on a
 * ghost gives its owner's bits: no exchange). Per particle with inverse mass > 0, in binary32 without FMA (SPEC.md 2h has the parentheses):
 *     q = rot (x - a);   fx = q_0 / cell[0], fz = q_2 / cell[1];   over the grid iff 0 <= fx <= nx - 1 and 0 <= fz <= nz - 1
 *     height = the cell's triangle under (fx, fz), interpolated;   gap = height - q_1;   m = the triangle's unit normal in the frame
 *     depth = gap m_1;   hit iff gap > 0 and depth < thickness;    n = m in simulation space
 * and for a hit 2f's response against a collider at rest with the call's friction and restitution: x' = x + depth n, and the velocity is
 * written only when the particle approaches. A particle further below the surface than `thickness` (along the normal) is left alone, as
 * are pinned particles, particles beside the grid and particles above it: they keep every bit. A written component that comes out NaN is
 * stored as 0x7fc00000. The push goes along the normal of the one triangle under the particle (in a concave crease a particle may land
 * under the neighbouring triangle until the next call); contacts are resolved once per call, not per substep; particles collide, not
 * triangles; the terrain is static and gets no reactions. Asynchronous; completes every rank's held-back last kernel first, which lands
 * pending kinematic targets; the next tick starts unfused. With no heightfield set the call returns SB_OK and does nothing at all (the
 * tick stays held back). It allocates nothing. Both host models, any number of ranks. */
#define SB_HEIGHTFIELD_MAX_SAMPLES 4097
typedef struct {
    float a[3];                    /* sample (0, 0) at height 0, simulation space */
    float rot[9];                  /* rows: the axis ix grows along, up, the axis iz grows along */
    float cell[2];                 /* the spacing along rows 0 and 2, > 0 */
    int32_t nx, nz;                /* samples along rows 0 and 2: 2 .. SB_HEIGHTFIELD_MAX_SAMPLES */
    float thickness;               /* > 0: how far under the surface, along the normal, a particle is still pushed out */
    uint32_t flags;                /* 0 */
    int32_t reserved[2];           /* 0 */
} sb_heightfield;                  /* 80 bytes */
/* desc == NULL clears and releases (heights is then not read). SB_ERR_INVALID_ARG (null group; null heights; nx or nz out of range;
 * flags or a reserved word != 0; a NaN or infinite float of the descriptor; cell <= 0; thickness <= 0; a NaN or infinite height --
 * sb_last_error names the first such sample's index --: all checked before the group is touched), SB_ERR_STATE before
 * sb_group_finalize; a refused call changes nothing and keeps the table set before. */
int sb_group_set_heightfield(sb_group *g, const sb_heightfield *desc, const float *heights);
/* SB_ERR_INVALID_ARG (null group, friction < 0 or NaN or infinite, restitution outside [0, 1]), SB_ERR_STATE before sb_group_finalize; a
 * refused call changes nothing. */
int sb_group_collide_heightfield(sb_group *g, float friction, float restitution);

/* ---- signed-distance volumes: moving props of any shape between two ticks (SPEC.md 2i) ------------------------------------------------------ */
/* What a scene's MeshCollider is to a rigid body: a bowl, a staircase, a cave with overhangs, a turning gear. The prop is baked once into a
 * table of nx * ny * nz signed distances (negative inside, simulation units), s[(iz * ny + iy) * nx + ix], on a regular grid with the
 * spacing cell[k] along axis k. The table holds the SHAPE and goes to a slot (SB_DISTANCE_FIELD_SLOTS of them); where it stands and how
 * it moves -- the POSE -- comes with every call, so a prop moves and turns every tick with nothing uploaded, and one slot may be used at
 * several poses in one frame (instances of one prop). sb_group_set_distance_field COPIES descriptor and samples (the caller may free both
 * on return) into a table on every rank's device -- 4 nx ny nz bytes, counted in sb_stats.device_bytes, given back when the slot is
 * cleared (desc == NULL), replaced (a table of the same size reuses the memory) or the group destroyed. It does not complete a held-back
 * tick. A pass of that slot still in flight is waited for (its own event, never the device) before the slot's memory is written or
 * released, so that pass reads the table it was given.
 *
 * sb_group_collide_distance_field is ONE streaming pass per rank over every particle it holds, ghosts included (the same arithmetic on a
 * ghost gives its owner's bits: no exchange). Per particle with inverse mass > 0, in binary32 without FMA (SPEC.md 2i has the parentheses):
 *     q = rot (x - a);   f_k = q_k / cell[k];   in the volume iff 0 <= f_k <= n_k - 1 for k = 0, 1, 2
 *     phi = the trilinear interpolation of the cell's eight samples, G = its analytic gradient in the frame
 *     gap = offset - phi;   hit iff gap > 0, gap < thickness and |G| > 0;   n = rot^T G / |G|;   depth = gap
 * and for a hit 2f's response against a collider with the pose's a, lin, ang, friction and restitution: x' = x + depth n, and the velocity
 * is written only when the particle approaches. Pinned particles, particles outside the volume, particles on or outside the contact
 * surface phi = offset and particles deeper under it than `thickness` keep every bit; a call that touches nothing is a bit-identity. A
 * written component that comes out NaN is stored as 0x7fc00000. Asynchronous; completes every rank's held-back last kernel first, which
 * lands pending kinematic targets; the next tick starts unfused. With nothing set in `slot` the call returns SB_OK and does nothing at all
 * (the tick stays held back). It allocates nothing. Both host models, any number of ranks. Several props are several calls, applied in
 * call order.
 * NOT DONE: contacts are resolved once per call, not per substep; particles collide, not triangles; the prop gets no reactions; there
 * is no brick-level cull (every particle inside the footprint gathers its eight samples); a trilinear field rounds off features thinner
 * than a cell. */
#define SB_DISTANCE_FIELD_SLOTS        4          /* tables a group can hold at once */
#define SB_DISTANCE_FIELD_MAX_DIM      1024       /* samples along one axis: 2 .. this */
#define SB_DISTANCE_FIELD_MAX_SAMPLES  (1 << 27)  /* nx*ny*nz: 512 MiB of float; the flat index fits an int32 */
typedef struct {
    int32_t nx, ny, nz;        /* samples along the frame's rows 0, 1, 2; s[(iz*ny + iy)*nx + ix] */
    float   cell[3];           /* spacing along the rows, > 0 */
    float   offset;            /* >= 0: the contact surface is the level set phi = offset (a skin round the baked surface) */
    float   thickness;         /* > 0: a particle deeper than this under the contact surface is left alone */
    uint32_t flags;            /* 0 */
    int32_t reserved[3];       /* 0 */
} sb_distance_field;           /* 48 bytes */
typedef struct {
    float a[3];                /* where sample (0,0,0) is, simulation space; also the pivot of ang */
    float rot[9];              /* rows: the axes ix, iy, iz grow along (orthonormal, not checked) */
    float lin[3], ang[3];      /* the prop's velocity at a and its angular velocity */
    float friction, restitution;
    int32_t reserved[2];       /* 0 */
} sb_distance_field_pose;      /* 88 bytes */
/* desc == NULL clears the slot and releases its memory (samples is then not read). SB_ERR_INVALID_ARG (null group; slot outside
 * 0 .. SB_DISTANCE_FIELD_SLOTS - 1; null samples; a dimension out of range or nx ny nz over SB_DISTANCE_FIELD_MAX_SAMPLES; flags or a
 * reserved word != 0; a NaN or infinite float of the descriptor; cell <= 0; offset < 0; thickness <= 0; a NaN or infinite sample --
 * sb_last_error names the first such sample's index --: all checked before the group is touched), SB_ERR_STATE before
 * sb_group_finalize; a refused call changes nothing and keeps the table set before. */
int sb_group_set_distance_field(sb_group *g, int32_t slot, const sb_distance_field *desc, const float *samples);
/* SB_ERR_INVALID_ARG (a null argument; slot out of range; a NaN or infinite field of the pose; friction < 0; restitution outside [0, 1];
 * a reserved word != 0: all checked before the group is touched), SB_ERR_STATE before sb_group_finalize; a refused call changes nothing. */
int sb_group_collide_distance_field(sb_group *g, int32_t slot, const sb_distance_field_pose *pose);

/* ---- synchronisation, inspection ------------------------------------------------------------------------------------------------------------ */
int sb_group_synchronize(sb_group *g);
int32_t sb_group_rank_count(const sb_group *g);
/* Borrowed handle of rank r (valid until sb_group_destroy) for sb_get_stats, sb_get_owner, sb_debug_validate, sb_get_plan: inspection only
 * -- stepping or reading state through it desynchronises the group. */
int sb_group_get_rank(sb_group *g, int32_t rank, sb_solver **out);

#ifdef __cplusplus
}
#endif
#endif /* SOFTBODY_MI355X_GROUP_H */
