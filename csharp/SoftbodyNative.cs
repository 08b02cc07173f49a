// SoftbodyNative.cs — P/Invoke layer over libsoftbody_mi355x.so (include/softbody.h + softbody_group.h / softbody_plan.h / softbody_debug.h, ABI version 8).
//
// One [DllImport] per exported function, same name and argument order as the header; the Python twin
// used by the test-suite is softbodyunity_amd/native.py (tests/test_abi.py keeps the three in sync).
// The reference repository holds no C# to mirror (/root/reference/README.md:1 is its only line), so
// this file is the builder-defined binding SURVEY.md §8b calls for.
//
// NOT COMPILED IN THIS ENVIRONMENT: no C# toolchain (dotnet/mono/mcs/csc) and no UnityEngine.dll exist
// in the build image; see INTEGRATION.md.
using System;
using System.Runtime.InteropServices;

namespace SoftbodyMI355X
{
    [StructLayout(LayoutKind.Sequential)]
    public struct SbDesc
    {
        public int device;
        public int rank;
        public int world;
        public int partDimX, partDimY, partDimZ;
        public float gravityX, gravityY, gravityZ;
        public float damping;
        public int tileParticles;
        public int useGraph;
        public int partition;        // SoftbodyNative.Partition*
        public uint planFlags;       // SoftbodyNative.PlanNo*: every rank the same (checked across the ranks at sb_finalize)
        public int haloTransport;    // SoftbodyNative.Transport*
        public int haloSchedule;     // SoftbodyNative.Schedule*
        public uint debugFlags;      // test-only, leave 0
        public int reserved0, reserved1, reserved2;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SbStats
    {
        public long nParticlesOwned, nParticlesLocal;
        public long nDistanceLocal, nVolumeLocal, nBendingLocal;
        public int nTilings, nGlobalColours;
        public long nTilesT0, nTilesT1, tileConstraintsT0, tileConstraintsT1;
        public long constraintsInTiles, constraintsInGlobal;
        public long haloParticlesT1, haloParticlesGlobal, deviceBytes;
        public long nT2Layers, nT2Tiles, t2Constraints;
        // compulsory HBM bytes of one launch: mid-tick on T0 / T1, first, last kernel of a tick, all T2 layers of a substep
        public long launchBytesMidT0, launchBytesMidT1, launchBytesFirst, launchBytesLast, launchBytesT2;
        // partition (world > 1)
        public int partition, haloPeers;
        public long partitionCost, partitionCostMax, partitionCostTotal;
        public long haloParticlesRecv;
        public ulong planHash;
        public int haloSchedule, haloUnpackFused;
        public long readbackPeeks, readbackPeekTiles, ticksFused, ticksFusedKinematic;
        public long lanePackedTilesT0, lanePackedTilesT1;
        public int haloAutoState, haloAutoTicks;          // SB_SCHEDULE_AUTO's calibration: 0 none, 1 measuring, 2 decided; ticks timed
        public double haloAutoMsSerial, haloAutoMsOverlap; // per tick, slowest rank
          // workgroups whose spring slots are lane-packed (16 B per lane)   // position reads served by a peek; T0 workgroups of one render-set peek (-1: none set up)
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SbValidateReport
    {
        public long tilesChecked, groupsChecked, constraintsChecked;
        // 0 index out of range, 1 a particle twice in one group / colour, 2 a particle staged by two tiles of one launch,
        // 3 a group's data leaves the tile's stream, 4 malformed run table / particle list, 5 wave items disagree with the group words
        public long errors0, errors1, errors2, errors3, errors4, errors5;
        public int firstStage, firstTile, firstGroup, firstKind;   // -1 = no error
    }

    [StructLayout(LayoutKind.Sequential, CharSet = CharSet.Ansi)]
    public struct SbRuntimeInfo
    {
        public int hipRuntimeVersion, hipDriverVersion, rcclVersion, rcclHeaderVersion;
        public int rcclWasResident, captureSerialOk, captureOverlapOk, reserved;
        [MarshalAs(UnmanagedType.ByValTStr, SizeConst = 256)] public string hipLibrary;
        [MarshalAs(UnmanagedType.ByValTStr, SizeConst = 256)] public string rcclLibrary;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SbPlanOpts
    {
        public int rank, world;
        public int partDimX, partDimY, partDimZ;
        public int tileParticles;
        public int partition;
        public uint planFlags;
        public IntPtr domain;        // SbDomain* (sharded authoring: the input is this rank's window of a larger mesh) or IntPtr.Zero
        public IntPtr globalId;      // int* ids of the window's particles in the whole mesh, ascending, or IntPtr.Zero
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SbDomain
    {
        public long nGlobal;
        public double loX, loY, loZ, hiX, hiY, hiZ;
        public double spacing;
        public double fill;          // fraction of the bounding box the mesh occupies (1 for a lattice)
        public int fourVertexConstraints, reserved;
    }

    // include/softbody_debug.h: A/B measurement switches (a product host never sets them) and exchange timing
    [StructLayout(LayoutKind.Sequential)]
    public struct SbTuning
    {
        public uint flags;           // SoftbodyNative.Tune*
        public int tileLanes, quadLanes, narrowMinTiles, storeThroughMaxTiles, storeThroughLarge, peekMinTiles, ldsPadBytes, winDwords, prevOffsetBytes;
        public int reserved0, reserved1, reserved2, reserved3, reserved4, reserved5;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SbExchangeTiming
    {
        public long exchanges;
        public double packMs, transportMs, totalMs, exposedWaitMs;
    }

    /// <summary>sb_ray_hit (16 bytes): the nearest hit of one ray; triangle = -1 where nothing is hit. t in units of the direction's length,
    /// (u, v) barycentric: point = (1 - u - v) p[a] + u p[b] + v p[c].</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SbRayHit
    {
        public int triangle;
        public float t, u, v;
    }

    /// <summary>sb_closest_hit (16 bytes, the layout of SbRayHit): the nearest point of the render mesh to one query (SPEC.md 6g); triangle = -1
    /// where nothing lies within max_distance. (u, v) barycentric as in SbRayHit: point = (1 - u - v) p[a] + u p[b] + v p[c].</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SbClosestHit
    {
        public int triangle;
        public float distance, u, v;
    }

    /// <summary>sb_impulse (48 bytes): one item of sb_apply_impulses / sb_group_apply_impulses (SPEC.md 2c). kind = SoftbodyNative.SB_IMPULSE_PARTICLE / _SURFACE / _RADIAL, flags = SB_IMPULSE_VELOCITY_CHANGE | SB_IMPULSE_LINEAR_FALLOFF;
    /// PARTICLE: index = particle, vec = J; SURFACE: index = triangle (-1 skips the item), (u, v) as SbRayHit gives them, vec = J;
    /// RADIAL: vec = centre, radius, strength. reserved stays 0.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SbImpulse
    {
        public int kind;
        public uint flags;
        public int index;
        public float u, v;
        public float vecX, vecY, vecZ;
        public float radius, strength;
        public int reserved0, reserved1;
    }

    /// <summary>sb_surface_force (44 bytes): the record of sb_group_apply_surface_forces (SPEC.md 2e). wind: air velocity in
    /// simulation space; normal, tangential: drag coefficients along and across a triangle's normal (>= 0); pressure: along the winding's right-hand
    /// normal; dt: the time the force acts for (> 0). flags and reserved stay 0.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SbSurfaceForce
    {
        public float windX, windY, windZ;
        public float normal, tangential, pressure, dt;
        public uint flags;
        public int reserved0, reserved1, reserved2;
    }

    /// <summary>sb_body_state (592 bytes): what sb_group_get_body_state / sb_group_body_state_from_sums fill (SPEC.md 6f). what = SoftbodyNative.BodyPose |
    /// BodyMotion as asked, flags = BodyNoMass | BodyDegeneratePose | BodyDegenerateInertia. sums: the 32 mass-weighted sums in binary64 (the header lists the slots);
    /// secondMoment about com (xx, yy, zz, xy, xz, yz); apq row-major; rotation: unit quaternion (x, y, z, w), w >= 0, reference pose -> simulation space;
    /// angularMomentum about com. Fields that were not asked for are 0, the rotation then identity.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SbBodyState
    {
        public long nDynamic, nPinned;
        public uint what, flags;
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 32)] public double[] sums;
        public double mass;
        public double comX, comY, comZ;
        public double refComX, refComY, refComZ;
        public double secondMomentXX, secondMomentYY, secondMomentZZ, secondMomentXY, secondMomentXZ, secondMomentYZ;
        public double apq00, apq01, apq02, apq10, apq11, apq12, apq20, apq21, apq22;
        public double rotationX, rotationY, rotationZ, rotationW;
        public double momentumX, momentumY, momentumZ;
        public double velocityX, velocityY, velocityZ;
        public double angularMomentumX, angularMomentumY, angularMomentumZ;
        public double angularVelocityX, angularVelocityY, angularVelocityZ;
        public double kineticEnergy;
    }

    /// <summary>sb_placement (92 bytes): what sb_group_place takes (SPEC.md 2d). x' = m (src - from) + to, m row-major, src the positions or -- under
    /// SB_PLACE_FROM_REFERENCE -- the reference pose; velocities turn with m, or become lin + ang x (x' - to) under SB_PLACE_SET_VELOCITY and always
    /// under SB_PLACE_FROM_REFERENCE; SB_PLACE_KEEP_PINNED leaves pinned particles alone. reserved stays 0.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SbPlacement
    {
        public uint flags, reserved;
        public float m00, m01, m02, m10, m11, m12, m20, m21, m22;
        public float fromX, fromY, fromZ;
        public float toX, toY, toZ;
        public float linX, linY, linZ;
        public float angX, angY, angZ;
    }

    /// <summary>sb_collider (128 bytes): one entry of sb_group_collide's list (SPEC.md 2f). shape = SB_COLLIDER_*; a: the centre (SPHERE, BOX) or one
    /// end of the segment a b (CAPSULE), and the pivot of ang; rot: the box's three world-space axes as rows, half its half extents along them; lin: the
    /// collider's velocity at a, ang its angular velocity in radians per second; friction >= 0, restitution in [0, 1]; flags and reserved stay 0.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SbCollider
    {
        public uint shape, flags;
        public float aX, aY, aZ;
        public float bX, bY, bZ;
        public float rot00, rot01, rot02, rot10, rot11, rot12, rot20, rot21, rot22;
        public float halfX, halfY, halfZ;
        public float radius;
        public float linX, linY, linZ;
        public float angX, angY, angZ;
        public float friction, restitution;
        public int reserved0, reserved1, reserved2;
    }

    /// <summary>sb_collider_reaction (64 bytes): what the body gave back to one collider of sb_group_collide_reactions' list (SPEC.md 2g), in simulation
    /// space: the impulse, the angular impulse about the collider's point a, the mass and the number of the particles it hit.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SbColliderReaction
    {
        public double impulseX, impulseY, impulseZ;
        public double angularImpulseX, angularImpulseY, angularImpulseZ;
        public double contactMass;
        public long contacts;
    }

    /// <summary>sb_heightfield (80 bytes): the frame of sb_group_set_heightfield's height map (SPEC.md 2h). a: sample (0, 0) at height 0, simulation
    /// space; rot: rows = the axis ix grows along, up, the axis iz grows along; cellX / cellZ: the spacing along rows 0 and 2; heights are
    /// h[iz * nx + ix] along up; thickness > 0: how far under the surface a particle is still pushed out; flags and reserved stay 0.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SbHeightfield
    {
        public float aX, aY, aZ;
        public float rot00, rot01, rot02, rot10, rot11, rot12, rot20, rot21, rot22;
        public float cellX, cellZ;
        public int nx, nz;
        public float thickness;
        public uint flags;
        public int reserved0, reserved1;
    }

    /// <summary>sb_distance_field (48 bytes): the shape of sb_group_set_distance_field's table (SPEC.md 2i). nx, ny, nz: samples along the
    /// frame's rows 0, 1, 2, s[(iz * ny + iy) * nx + ix], signed distances in simulation units, negative inside; cellX/Y/Z: the spacing along
    /// the rows; offset >= 0: the contact surface is phi = offset; thickness > 0: how deep under it a particle is still pushed out; flags and
    /// reserved stay 0.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SbDistanceField
    {
        public int nx, ny, nz;
        public float cellX, cellY, cellZ;
        public float offset, thickness;
        public uint flags;
        public int reserved0, reserved1, reserved2;
    }

    /// <summary>sb_distance_field_pose (88 bytes): where a slot's table stands and how it moves, per call (SPEC.md 2i). a: sample (0, 0, 0),
    /// simulation space, and the pivot of ang; rot: rows = the axes ix, iy, iz grow along; lin / ang: the prop's velocity at a and its angular
    /// velocity; reserved stays 0.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SbDistanceFieldPose
    {
        public float aX, aY, aZ;
        public float rot00, rot01, rot02, rot10, rot11, rot12, rot20, rot21, rot22;
        public float linX, linY, linZ, angX, angY, angZ;
        public float friction, restitution;
        public int reserved0, reserved1;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SbPhaseInfo
    {
        public int kind, type, tiling, haloSlot;
        public long orderBegin, orderEnd, taskBegin, taskEnd;
    }

    public static class SoftbodyNative
    {
        const string Lib = "softbody_mi355x";
        const CallingConvention CC = CallingConvention.Cdecl;
        public const int UniqueIdBytes = 128;
        public const int PartitionAuto = 0, PartitionBlocks = 1, PartitionRcb = 2;
        public const uint PlanNoT2 = 1, PlanNoThirdList = 2, PlanNoClusterLayers = 4, PlanNoMixedGroups = 8, PlanNoBankOrder = 16, PlanNoTileMerge = 32;
        public static uint PlanBalancedLists(int n) => (uint)n << 8;   // irregular meshes: 1..3 balanced extra lists; 0 = default (2)
        public const int TransportRccl = 0, TransportPeer = 1;
        public const int ScheduleAuto = 0, ScheduleSerialEager = 1, ScheduleSerialGraph = 2, ScheduleOverlapEager = 3, ScheduleOverlapGraph = 4;
        public const uint GroupWalk = 1;       // sb_group_create flags: no plugin threads, the calling thread walks the tick across the ranks
        public const uint GroupWholeMesh = 2;  // never cut windows: every rank plans the whole mesh (sb_group_finalize)
        // sb_group_get_body_state (SPEC.md 6f): what to ask for, and sb_body_state.flags
        public const uint BodyPose = 1;        // positions only: peeks, the tick stays fusable
        public const uint BodyMotion = 2;      // needs velocities: completes the tick's held-back last kernel
        public const uint BodyNoMass = 1, BodyDegeneratePose = 2, BodyDegenerateInertia = 4;
        // sb_impulse (SPEC.md 2c), named as in include/softbody.h
        public const int SB_IMPULSE_PARTICLE = 0, SB_IMPULSE_SURFACE = 1, SB_IMPULSE_RADIAL = 2;      // SbImpulse.kind
        public const uint SB_IMPULSE_VELOCITY_CHANGE = 1, SB_IMPULSE_LINEAR_FALLOFF = 2;               // SbImpulse.flags (LINEAR_FALLOFF: RADIAL only)

        // sb_placement.flags (SPEC.md 2d), named as in include/softbody_group.h
        public const uint SB_PLACE_FROM_REFERENCE = 1, SB_PLACE_SET_VELOCITY = 2, SB_PLACE_KEEP_PINNED = 4;

        // sb_collider.shape (SPEC.md 2f), named as in include/softbody_group.h
        public const uint SB_COLLIDER_SPHERE = 0, SB_COLLIDER_CAPSULE = 1, SB_COLLIDER_BOX = 2;

        [DllImport(Lib, CallingConvention = CC)] public static extern void sb_desc_default(ref SbDesc d);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_create(ref SbDesc desc, out IntPtr solver);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_destroy(IntPtr s);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_particles(IntPtr s, IntPtr posXyz, IntPtr velXyz, IntPtr invMass, int n);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_rest_positions(IntPtr s, IntPtr restXyz, int n);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_distance_constraints(IntPtr s, IntPtr ij, IntPtr restLen, int m, float compliance);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_volume_constraints(IntPtr s, IntPtr ijkl, IntPtr restVol, int m, float compliance);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_bending_constraints(IntPtr s, IntPtr ijkl, IntPtr restCosSin, int m, float compliance);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_ground_plane(IntPtr s, float nx, float ny, float nz, float d, int enabled);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_domain(IntPtr s, ref SbDomain domain, IntPtr globalId, int n);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_domain_from_mesh(IntPtr restXyz, int n, IntPtr distIj, int mD, IntPtr volIjkl, int mV, IntPtr bendIjkl, int mB, out SbDomain domain);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_domain_window(ref SbDomain domain, ref SbPlanOpts opts, double[] lo3, double[] hi3);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_finalize(IntPtr s);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_comm_unique_id(IntPtr outId128);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_comm_init(IntPtr s, IntPtr id128);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_step(IntPtr s, float dt, int substeps);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_get_positions(IntPtr s, IntPtr posXyzOut, int n);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_get_velocities(IntPtr s, IntPtr velXyzOut, int n);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_state(IntPtr s, IntPtr posXyz, IntPtr velXyz, int n);
        // kinematic particles (attachments): move particles with inverse mass 0 between two ticks (SPEC.md 2); a rank applies the ones it owns
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_kinematic_positions(IntPtr s, IntPtr ids, IntPtr posXyz, int count);
        // impulses between two ticks (SPEC.md 2c): velocities only; the next sb_step starts unfused
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_apply_impulses(IntPtr s, SbImpulse[] items, int count);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_readback_begin(IntPtr s);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_readback_end(IntPtr s, out IntPtr posXyz);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_render_triangles(IntPtr s, int[] triAbc, int m);
        // embedded render vertices (SPEC.md 6b): cageIjkl 4 particle indices and weights4 4 floats per render vertex, triAbc over RENDER VERTICES (may be null with mTri = 0)
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_render_embedding(IntPtr s, int[] cageIjkl, float[] weights4, int mVertices, int[] triAbc, int mTri);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_readback_get_normals(IntPtr s, out IntPtr normalXyz);
        // render tangents (SPEC.md 6c): uv = 2 floats per vertex of the render mode in force (a pinned Vector2[]); tangents = Vector4 per row (xyz, handedness)
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_render_uvs(IntPtr s, IntPtr uv, int count);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_readback_get_tangents(IntPtr s, out IntPtr tangentXyzw);
        // bounding box (SPEC.md 6d): lo / hi are float[3], filled by the call
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_readback_bounds(IntPtr s, int enabled);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_readback_get_bounds(IntPtr s, [Out] float[] loXyz, [Out] float[] hiXyz);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_get_bounds(IntPtr s, [Out] float[] loXyz, [Out] float[] hiXyz);
        // rays: 8 floats each = origin xyz, t_max, direction xyz, 0 (SPEC.md 6e)
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_readback_raycast(IntPtr s, float[] rays, int count, [Out] SbRayHit[] hits);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_readback_render_set_only(IntPtr s, int renderSetOnly);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_readback_get_render_set(IntPtr s, out IntPtr ids, out int count);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_get_owner(IntPtr s, IntPtr ownerRankOut, int n);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_profile_begin(IntPtr s);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_profile_end(IntPtr s, out float elapsedMs);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_synchronize(IntPtr s);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_step_profiled(IntPtr s, float dt, int substeps, IntPtr slotMsOut, IntPtr slotLaunchesOut, int nSlots);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_debug_launch(IntPtr s, float dt, int substeps, int it, int gcolour);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_debug_halo_pack(IntPtr s, int slot, IntPtr hostOut, long capacityFloats, out long countFloats);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_debug_halo_unpack(IntPtr s, int slot, IntPtr hostIn, long countFloats);
        // table validator ("race detector"): a GPU kernel re-reads every table the tile kernels read and counts violations (softbody.h)
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_debug_validate(IntPtr s, int injectFault, out SbValidateReport report);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_get_stats(IntPtr s, out SbStats stats);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_runtime_info(out SbRuntimeInfo info);
        // opt-in peer-store halo transport (SbDesc.haloTransport = TransportPeer): see softbody.h
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_peer_mailbox_handle(IntPtr s, byte[] handle64);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_peer_connect(IntPtr s, int rank, byte[] handle64, IntPtr sameProcessPeer);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_build(IntPtr restXyz, int n, IntPtr distIj, int mD, IntPtr volIjkl, int mV, IntPtr bendIjkl, int mB, ref SbPlanOpts opts, out IntPtr plan);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_destroy(IntPtr plan);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_get_plan(IntPtr s, out IntPtr plan);
        [DllImport(Lib, CallingConvention = CC)] public static extern long sb_plan_order_count(IntPtr plan);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_get_order(IntPtr plan, int parity, IntPtr typeOut, IntPtr idOut);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_phase_count(IntPtr plan, int parity);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_get_phases(IntPtr plan, int parity, [Out] SbPhaseInfo[] phases);
        [DllImport(Lib, CallingConvention = CC)] public static extern long sb_plan_task_count(IntPtr plan, int parity);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_get_tasks(IntPtr plan, int parity, IntPtr taskOffOut);
        [DllImport(Lib, CallingConvention = CC)] public static extern long sb_plan_group_count(IntPtr plan, int parity);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_get_groups(IntPtr plan, int parity, IntPtr groupOffOut);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_get_owner(IntPtr plan, IntPtr ownerRankOut);
        [DllImport(Lib, CallingConvention = CC)] public static extern long sb_plan_local_count(IntPtr plan, out long owned);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_get_local_particles(IntPtr plan, IntPtr globalIdOut);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_halo_slot_count(IntPtr plan);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_halo_counts(IntPtr plan, int slot, IntPtr sendCountPerRank, IntPtr recvCountPerRank);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_get_halo(IntPtr plan, int slot, int peer, IntPtr sendIds, IntPtr recvIds);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_get_pair_hashes(IntPtr plan, IntPtr outPerRank);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_plan_get_local_order_mask(IntPtr plan, int parity, IntPtr maskOut);
        // ---- one process, several GPUs (include/softbody_group.h): what Softbody.cs calls when deviceCount > 1 ----
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_create(ref SbDesc desc, int[] devices, int nDevices, uint flags, out IntPtr group);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_destroy(IntPtr g);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_particles(IntPtr g, IntPtr posXyz, IntPtr velXyz, IntPtr invMass, int n);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_rest_positions(IntPtr g, IntPtr restXyz, int n);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_distance_constraints(IntPtr g, IntPtr ij, IntPtr restLen, int m, float compliance);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_volume_constraints(IntPtr g, IntPtr ijkl, IntPtr restVol, int m, float compliance);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_bending_constraints(IntPtr g, IntPtr ijkl, IntPtr restCosSin, int m, float compliance);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_ground_plane(IntPtr g, float nx, float ny, float nz, float d, int enabled);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_finalize(IntPtr g);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_step(IntPtr g, float dt, int substeps);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_get_positions(IntPtr g, IntPtr posXyzOut, int n);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_get_velocities(IntPtr g, IntPtr velXyzOut, int n);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_state(IntPtr g, IntPtr posXyz, IntPtr velXyz, int n);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_kinematic_positions(IntPtr g, IntPtr ids, IntPtr posXyz, int count);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_apply_impulses(IntPtr g, SbImpulse[] items, int count);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_apply_surface_forces(IntPtr g, ref SbSurfaceForce force);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_render_triangles(IntPtr g, int[] triAbc, int m);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_render_embedding(IntPtr g, int[] cageIjkl, float[] weights4, int mVertices, int[] triAbc, int mTri);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_render_uvs(IntPtr g, IntPtr uv, int count);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_readback_render_set_only(IntPtr g, int renderSetOnly);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_readback_begin(IntPtr g);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_readback_end(IntPtr g, out IntPtr posXyz);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_readback_get_normals(IntPtr g, out IntPtr normalXyz);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_readback_get_tangents(IntPtr g, out IntPtr tangentXyzw);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_readback_get_render_set(IntPtr g, out IntPtr ids, out int count);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_readback_bounds(IntPtr g, int enabled);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_readback_get_bounds(IntPtr g, [Out] float[] loXyz, [Out] float[] hiXyz);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_get_bounds(IntPtr g, [Out] float[] loXyz, [Out] float[] hiXyz);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_readback_raycast(IntPtr g, float[] rays, int count, [Out] SbRayHit[] hits);
        // queries: 4 floats each = x, y, z, max_distance (SPEC.md 6g)
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_readback_closest_points(IntPtr g, float[] queries, int count, [Out] SbClosestHit[] hits);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_place(IntPtr g, ref SbPlacement placement);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_collide(IntPtr g, SbCollider[] colliders, int count);
        public const int SB_COLLIDE_REACTIONS_MAX = 1024;
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_collide_reactions(IntPtr g, SbCollider[] colliders, int count);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_get_collider_reactions(IntPtr g, [Out] SbColliderReaction[] reactions, int capacity, out int count);
        public const int SB_HEIGHTFIELD_MAX_SAMPLES = 4097;
        // copies descriptor and heights (nx * nz floats); ClearHeightfield is the same entry point with desc == NULL (clear and release)
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_heightfield(IntPtr g, ref SbHeightfield desc, float[] heights);
        [DllImport(Lib, CallingConvention = CC, EntryPoint = "sb_group_set_heightfield")] public static extern int ClearHeightfield(IntPtr g, IntPtr nullDesc, IntPtr nullHeights);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_collide_heightfield(IntPtr g, float friction, float restitution);
        public const int SB_DISTANCE_FIELD_SLOTS = 4, SB_DISTANCE_FIELD_MAX_DIM = 1024, SB_DISTANCE_FIELD_MAX_SAMPLES = 1 << 27;
        // copies descriptor and samples (nx * ny * nz floats) into the slot; ClearDistanceField is the same entry point with desc == NULL (clear and release)
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_set_distance_field(IntPtr g, int slot, ref SbDistanceField desc, float[] samples);
        [DllImport(Lib, CallingConvention = CC, EntryPoint = "sb_group_set_distance_field")] public static extern int ClearDistanceField(IntPtr g, int slot, IntPtr nullDesc, IntPtr nullSamples);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_collide_distance_field(IntPtr g, int slot, ref SbDistanceFieldPose pose);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_get_body_state(IntPtr g, uint what, out SbBodyState state);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_body_state_from_sums(double[] sums32, long nDynamic, long nPinned, uint what, out SbBodyState state);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_synchronize(IntPtr g);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_rank_count(IntPtr g);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_group_get_rank(IntPtr g, int rank, out IntPtr solver);
        // ---- include/softbody_debug.h: measurement harnesses only ----
        [DllImport(Lib, CallingConvention = CC)] public static extern void sb_tuning_default(ref SbTuning t);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_set_tuning(IntPtr s, ref SbTuning t);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_debug_exchange_timing(IntPtr s, int enabled);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_debug_exchange_timing_read(IntPtr s, out SbExchangeTiming t);
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_debug_last_words(int fd, byte[] text, long len, int exitCode);
        [DllImport(Lib, CallingConvention = CC)] public static extern IntPtr sb_last_error();
        [DllImport(Lib, CallingConvention = CC)] public static extern int sb_abi_version();

        public static string LastError() => Marshal.PtrToStringAnsi(sb_last_error());

        public static void Check(int rc, string what)
        {
            if (rc != 0) throw new InvalidOperationException($"{what} failed ({rc}): {LastError()}");
        }
    }
}
