// aic_trace.hip -- hand-written CDNA4 (gfx950) kernels of the voxel raytracer: the image kernel and its launchers. The ONE device translation
// unit of the trace side: what it is made of lives in headers by subject, included below and compiled with it (DESIGN.md 4 has the reason --
// compiling the small kernels on their own changes the image kernels' register allocation):
//   aic_tunables.h       the numeric build-time tunables (AIC_*)
//   aic_raycast.h        the Raycaster restated (lvl_init, lvl_next, lvl_first_masks, intersection_point)
//   aic_colour.h         f32 colour arithmetic, the powf / expf tables
//   aic_light_bounce.h   light lookup, LightingOption::Bounce's secondary rays
//   aic_scene_kernels.h  scatter_cubes, tag_cubes, order_tiles, assemble_strips and their launchers
//   aic_probe_kernels.h  the probe kernels and their launchers
//   aic_launch.h         every launcher of this translation unit as the host code sees it
//
// Replaces, behind the C ABI of include/aic_hip.h, the reference's per-image hot loop:
//   trace_scene_to_image_impl / RtScene::trace_patch / trace_ray_through_layers
//       and the draw_rgba encoder (all-is-cubes-render/src/raytracer/renderer.rs:282-308, 424-478, 516-556)
//   SpaceRaytracer::trace_ray_impl + TracingState (raytracer/sr.rs:135-238, 595-769)
//   SurfaceIter / VoxelSurfaceIter / DepthIter (raytracer/surface.rs:251-491)
//   Raycaster (all-is-cubes-base/src/raycast.rs:63-832)
//   ColorBuf / apply_transmittance (all-is-cubes/src/raytracer_components.rs:20-258)
//   Camera::project_ndc_into_world / post_process_color, Rgba::to_srgb8.
//
// Design (MI355X-first, not a translation of the reference's iterator stack). The kernel is bound by instruction issue, not memory:
//  * persistent waves: the grid is what is resident at the kernel's occupancy -- the production variants 4 waves per SIMD (128 VGPRs, no scratch,
//    four workgroups of 256 threads per CU), the recording (DIAG) and Bounce variants 2. Each wave pulls 8x8-pixel tiles (one wave-full), macro tile
//    by macro tile, from the tile queue of the XCD it runs on -- one queue per XCD, each ordered costliest macro tiles of the previous frame first
//    (order_tiles_kernel); it helps the next XCD's queue when its own is empty -- and refills idle lanes one by one.
//  * every lane is a state machine. ONE predicated, straight-line Amanatides-Woo step serves both DDA levels (cube grid and a block's voxels share
//    the lookup pool, the registers and the code): a stepping trip is up to AIC_STEP_REPS full passes, each preceded by up to AIC_FAST_STEPS
//    bookkeeping-free fast steps. The expensive, divergent work -- shading a surface, entering a block, finishing / starting a ray -- is parked per
//    lane as an event and run kind by kind when enough lanes wait; ENTER and NEWRAY take the first lookup of the level they set up themselves.
//  * hot state in registers, cold state (what only events touch) in an LDS column that belongs to the ray, not to the lane.
//  * lane exchange (the XC variants, chosen at run time by the frame's size): the waves of a workgroup share a pool of parked rays in LDS; before a
//    round a wave trades lanes that would idle for parked rays of the kind it is about to run, and parks such lanes while slots are free, so that
//    the workgroup holds more rays than lanes. Nothing waits for another wave; frames are bit-identical for any pool size or policy.
//  * DDA arithmetic is f64 in the reference's exact operation order (bit-exact hit cubes/voxels/faces/t); built with -ffp-contract=off. Colour
//    arithmetic is f32 in the reference's order; powf and expf follow the C library's algorithms, evaluated in f64. The per-lane order of
//    operations is the reference's, so results are bit-identical to the sequential formulation (hit cubes, t values, step counts).
//  * no MFMA: the path is branchy integer/f64 traversal and gather loads, not a contraction.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstddef>
#include <cstdlib>

#include "aic_device.h"
#include "aic_encode.h"
#include "aic_lightmath.h"
#include "aic_launch.h"
#include "aic_tunables.h"
#include "aic_raycast.h"
#include "aic_colour.h"
#include "aic_light_bounce.h"
#include "aic_scene_kernels.h"
#include "aic_probe_kernels.h"

namespace aic {

// ---- the image kernel's own helpers, constants and structs

// population count of a wave mask as a 32-bit scalar (the compiler widens __popcll's result and then compares it on the VALU)
AIC_DEV uint32_t wave_popc(unsigned long long m) {
    uint32_t n;
    asm volatile("s_bcnt1_i32_b64 %0, %1" : "=s"(n) : "s"(m) : "scc");
    return n;
}
// a float literal that is materialised where it is used (as KC, aic_colour.h, for a VGPR)
AIC_DEV float KF(float v) { asm volatile("" : "+v"(v)); return v; }

struct Diag {
    uint32_t n_outer, n_inner, n_hits, n_light;
    uint32_t layer;  // layer of that first hit: 0 world, 1 UI (its block_index is an index into THAT layer's block table)
    int hit;  // first Hit carrying a Position
    int cube[3], voxel[3], res, face, block;
    double t;
};
struct SurfDiag {  // DIAG only: identity of a pending surface
    uint32_t nlight;
    int cube[3], voxel[3], res, face, block;
};

// camera (camera_struct.rs:238-257; euclid Transform3D::transform_point3d)
template <class MatP>
AIC_DEV void unproject(MatP m, double x, double y, double z, double out[3]) {
    const double px = x * m[0] + y * m[4] + z * m[8] + m[12];
    const double py = x * m[1] + y * m[5] + z * m[9] + m[13];
    const double pz = x * m[2] + y * m[6] + z * m[10] + m[14];
    const double pw = x * m[3] + y * m[7] + z * m[11] + m[15];
    if (pw > 0.0) {
        // Three quotients by one divisor: the generic division's reciprocal (v_rcp_f64 and its two refinement steps) made once, then each quotient's
        // multiply and two residual steps -- the generic sequence's own operations when nothing needs scaling, which the exponent window guarantees
        // (see div_known_recip above); 21 instructions for the three instead of 33. Lanes outside the window divide generically.
        const bool fast = ((int)f64_exp_in_768_1280(pw) & (int)f64_exp_in_768_1280(px) & (int)f64_exp_in_768_1280(py) & (int)f64_exp_in_768_1280(pz)) != 0;
        double r = __builtin_amdgcn_rcp(pw);
        double e = fma(-pw, r, 1.0);
        r = fma(r, e, r);
        e = fma(-pw, r, 1.0);
        r = fma(r, e, r);
        const double qx = px * r, qy = py * r, qz = pz * r;
        out[0] = fma(fma(-pw, qx, px), r, qx); out[1] = fma(fma(-pw, qy, py), r, qy); out[2] = fma(fma(-pw, qz, pz), r, qz);
        if (__builtin_amdgcn_ballot_w64(!fast) != 0ull) {
            AIC_RARE_PATH();
            if (!fast) { out[0] = px / pw; out[1] = py / pw; out[2] = pz / pw; }
        }
    } else {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        out[0] = out[1] = out[2] = nan;
    }
}

constexpr float NO_WORLD_TO_SHOW = 0.5028865f;  // palette.rs:76 #BCBCBC decoded to linear

// viewport.rs:104-113
AIC_DEV double fb_x_edge(uint32_t w, uint32_t x) { return ((double)x) / (double)w * 2.0 - 1.0; }
AIC_DEV double fb_y_edge(uint32_t h, uint32_t y) { return -(((double)y) / (double)h * 2.0 - 1.0); }


// lane event word (ev): what the lane needs next. Values below 4 mean "stepping" (the wave scheduler's test), with
//   1  EV_FRESH   the first cube of a level was emitted by the event that set the level up: look it up without stepping
//   2  EV_DEAD    the current level's Raycaster has ended: it cannot step any further
// and the parked kinds (EV_DEAD may ride along with SHADE / ENTER: the event still needs the ended level's state)
constexpr uint32_t EV_FRESH = 1u, EV_DEAD = 2u, EV_SHADE = 4u, EV_ENTER = 8u, EV_FINISH = 16u, EV_NEWRAY = 32u, EV_DONE = 64u,
                   EV_TAKE = 128u;  // with NEWRAY: take a new pixel first
// lane state bits (st):
//   9-13   flags below;  14-15 the antialiasing sample being traced
//   16-18  the suspended outer level's Face while inside a block; 21 ST_OUTER_ALIVE: that level can go on stepping
//   24-26  sign bits of the ray direction (x: 26, y: 25, z: 24; set = component >= 0) = the sky octant
//   22     ST_DIR_FAST: RayDir::fast of the ray's direction (divisions by it may use t_delta: div_known_recip)
constexpr uint32_t ST_IN_BLOCK = 1u << 9, ST_HAS_LAST = 1u << 10, ST_OPAQUE = 1u << 12, ST_TRACED = 1u << 13, ST_OUTER_ALIVE = 1u << 21, ST_DIR_FAST = 1u << 22;

// Waits for a lookup issued into a register (`raw`, in the stepping trip) by an earlier asm statement. The loaded register goes in as a plain INPUT and the code comes
// out in a fresh register, copied AFTER the wait: every later use depends on this statement. (Until round 4 this was
// `asm("s_waitcnt vmcnt(0)" : "+v"(raw))`: a tied operand, for which the compiler may place a register copy in front of the
// statement -- i.e. read the destination of a load still in flight. Register allocation happened never to need one; the first
// change that gave `raw` another live range -- the speculative lookups -- made it appear, in front of the full pass's wait.)
#define AIC_WAIT_LOOKUP(reg_) { const uint32_t in_flight_ = reg_; asm volatile("s_waitcnt vmcnt(0)\n\tv_mov_b32 %0, %1" : "=&v"(reg_) : "v"(in_flight_)); }
#define AIC_WAIT_RAW() AIC_WAIT_LOOKUP(raw)
// The first lookup of a level, issued by the event that set it up as soon as `boff` exists: under the eligible lanes (a wave mask), so that the event's
// remaining assignments run under its latency. AIC_WAIT_LOOKUP(reg_) ends it.
#define AIC_ISSUE_FIRST_LOOKUP(elig_, reg_)                                                                                                            \
    {                                                                                                                                              \
        const unsigned long long m_first_ = __builtin_amdgcn_ballot_w64(elig_);                                                                    \
        unsigned long long sv_first_;                                                                                                              \
        asm volatile("s_mov_b64 %[sv], exec\n\t"                                                                                                   \
                     "s_mov_b64 exec, %[m]\n\t"                                                                                                    \
                     "global_load_ushort %[raw], %[bo], %[pool]\n\t"                                                                               \
                     "s_mov_b64 exec, %[sv]\n\t"                                                                                                   \
                     : [raw] "+v"(reg_), [sv] "=&s"(sv_first_)                                                                                     \
                     : [bo] "v"(boff), [pool] "s"(pool_bits), [m] "s"(m_first_)                                                                    \
                     : "memory");                                                                                                                  \
    }
// ---- Lane exchange between the waves of a workgroup ("regime-sorted waves"; DESIGN.md 4.2, tools/wave_sim) ----
// A wave runs ONE kind of work per scheduler round (a stepping trip, or one kind of event) and the lanes of the other kinds idle: every phase
// ran at 25-39 of 64 lanes (profiles/r04_phase_cycles.txt) on a kernel bound by instruction issue. The production variants therefore share a POOL
// of parked rays per workgroup, in LDS: before a round the wave trades lanes that would idle for parked rays of the kind it is about to run
// (compare-and-swap on a slot's tag, then a plain exchange of the ray's 40 hot dwords; the cold state stays in the ray's LDS column, whose index
// travels with the ray), and while the pool has free slots it parks such lanes and starts new pixels in them, so that the workgroup holds more rays
// than lanes (the reservoir the sorting needs). Nothing ever waits for another wave: a claim that fails is simply not made. A ray is a pure
// function of its own state, which moves as a whole, so frames are bit-identical for any pool size or policy.
constexpr uint32_t TAG_FREE = 0u, TAG_STEP = 1u, TAG_SHADE = 2u, TAG_ENTER = 3u, TAG_RAY = 4u, TAG_BUSY = 7u;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// How a DDA level is held in registers by the image kernel (both levels -- the cube grid and a block's
// voxel volume -- use the same registers and the same stepping code):
//   t[3]   t_max, exactly the reference's (raycast.rs:99-121)
//   td[3]  t_delta = 1/|d|, a per-ray constant shared by both levels (a sub-ray keeps its direction)
//   r[3]   steps the ray can still take along each axis before it leaves the level's bounds, MINUS ONE: for a
//          coordinate c relative to the level's lower corner, r = size - 1 - c going up, c going down
//          (direction sign = the octant bit). Stepping decrements it; the decrement's borrow (r was 0) <=> the
//          include_exit step. The coordinate is recovered when an event needs it: c = size - 1 - r or r.
//   boff   BYTE offset of the current cube's / voxel's u16 in the pool; ss[3] the signed byte strides.
//          Stepping adds ss[axis]: no index arithmetic in the loop, and the lookup is a
//          scalar-base + 32-bit-offset load (the pool is at most 4 GiB: aic_upload_space checks).
//   thr    a looked-up code >= thr is a visible surface (voxels: the block's first visible palette code;
//          cubes with tag bits: 0x8000, i.e. tag >= kCubeTagVisible)
// The axis to step along is recomputed from t[] at every step (two v_min_f64, two compares) instead of being
// carried in the state: it is a pure function of t[], which nothing modifies between steps.

template <bool VOL, int LMODE, bool DIAG, bool BIG, bool XC>
__global__ __launch_bounds__((XC && !DIAG && LMODE != 3) ? AIC_XWG_THREADS : AIC_WG_THREADS, (DIAG || LMODE == 3) ? 2 : AIC_MIN_WAVES) void trace_image_kernel(const DevFrame F) {
    // XCHG: the production variants -- lanes are exchanged between the workgroup's waves through a pool of parked rays, and the part of a ray's
    // cold state that only ENTER / SHADE / FINISH touch (origin, direction, antialiasing sums) lives in global memory to make room for it.
    // The aux-recording and Bounce variants (more per-lane state, built for 2 waves per SIMD) keep everything in LDS and exchange nothing.
    // (XC: the production variants exist with and without the exchange; the launcher picks by the frame's size -- DevFrame::exchange)
    constexpr bool XCHG = XC && !DIAG && LMODE != 3;
    constexpr uint32_t WGT = XCHG ? (uint32_t)AIC_XWG_THREADS : (uint32_t)AIC_WG_THREADS;  // threads per workgroup
    constexpr uint32_t NPOOL = XCHG ? (uint32_t)AIC_POOL : 0u;                            // pool slots
    constexpr uint32_t NCOL = WGT + NPOOL;                                                // LDS columns: one per lane and one per slot
    static_assert(NPOOL <= 192u, "three tags per lane are scanned");
    // ---- persistent waves: each wave pulls 8x8-pixel tiles from a global counter until the
    // image is exhausted, so cheap (sky) and expensive (geometry) tiles balance dynamically ----
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t tile_x0 = 0, tile_y0 = 0;  // wave-uniform: pixel origin of the tile the refill is drawing from
    // small decode tables live in LDS for the life of the persistent workgroup
    __shared__ float s_lut[256];     // PackedLight scalar decode (light/data.rs:301-354)
    __shared__ double s_pow[64];     // powf tables (powf_table)
    pow_tables_to_lds(s_pow, threadIdx.x, WGT);
    for (uint32_t i = threadIdx.x; i < 256u; i += WGT) s_lut[i] = F.light_lut[i];
    __syncthreads();
    const float *lut = s_lut;
    // Kernel arguments and the persistent loop. The stepping phase needs three scalars of them (the pool pointer and the cube
    // grid's two byte strides, below); everything else is wanted by events only. Left as plain uses of `F`, the compiler
    // fetches all ~250 dwords of DevFrame before the loop, keeps what fits in SGPRs and parks the rest in VGPR lanes
    // (v_writelane / v_readlane + hazard nops: round 2's 92 spilled SGPRs and two VGPRs lost to them). Instead every event
    // phase reads the arguments it needs through an OPAQUE pointer to the kernel-argument segment (see the event phase):
    // scalar loads that hit the constant cache, issued where they are used, holding no register across the loop.
    const int ostx = 2 * F.layer.size[1] * F.layer.size[2], osty = 2 * F.layer.size[2];  // byte strides of the cube grid (z: 2)
    const uint32_t hit_layer_s = F.hit_layer;  // (DIAG builds: the stepping phase labels first hits with their layer)
    // cube grid at offset 0, then every block's voxel volume. The pointer is laundered through an
    // s_mov so that it is a computed SGPR pair rather than a re-loadable kernel argument: under SGPR
    // pressure the compiler would otherwise re-fetch it (s_load + wait) in front of every lookup.
    unsigned long long pool_bits = (unsigned long long)F.layer.pool;
    asm volatile("s_mov_b64 %0, %1" : "=s"(pool_bits) : "s"(pool_bits));
    // BIG: block tables past 16384 entries -- plain 16-bit indices in the grid, classes from L.cls
    const uint32_t idx_mask = BIG ? 0xffffu : kCubeIndexMask;
    const uint32_t outer_thr = BIG ? 0x10000u : (kCubeTagVisible << kCubeClassShift);

    // ---- per-lane state, hot: lives in registers across the stepping loop ----
    double tx = 0, ty = 0, tz = 0, last_t = 0;   // t_max of the current level, t of the step that entered the current cube
    double tdx = 0, tdy = 0, tdz = 0;            // t_delta
    uint32_t rx = 0, ry = 0, rz = 0;             // steps left before leaving the bounds, minus one, per axis
    uint32_t boff = 0;                           // byte offset of the current cube / voxel in the pool
    int ssx = 0, ssy = 0, ssz = 0;               // signed byte strides of the current level
    uint32_t thr = outer_thr;                    // codes >= thr are visible surfaces
    uint32_t raw = 0;                            // the code looked up last (read by the event it raised)
    uint32_t lax = 8u;                           // axis last stepped along (0..2), or 8 | Face set by an event (FACE_TABLE applied late)
    uint32_t st = 0u;
    uint32_t count = 0;
    ColorBuf acc;
    acc.l0 = acc.l1 = acc.l2 = 0.f; acc.t = 1.0f;
    // DepthIter.last_surface, already shaded: its premultiplied light and transmittance
    float pend0 = 0.f, pend1 = 0.f, pend2 = 0.f, pend_tr = 1.f;
    // the block the lane is inside: palette offset; log2(resolution) << 24 | stored-volume lower corner; stored-volume size
    uint32_t blk_pal_off = 0, blk_geo = 0, blk_vsz = 0;
    // LightingOption::Bounce (LMODE 3 only; dead code elsewhere): the ray's SmallRng (sr.rs:165-178) and what its secondary rays traced
    BounceRng brng{0ull, 0ull, 0ull, 0ull};
    uint32_t sec_steps = 0;
    // ---- per-lane state, cold: only events touch it, so it lives in LDS (one column per thread: conflict-free
    //      ds_read/ds_write), not in registers -- that is what lets the kernel run at 3-4 waves per SIMD ----
    //      A column belongs to a RAY, not to a lane: it travels with the ray when lanes are exchanged (`col`), and every pool slot holds a spare one.
    //      The exchanging variants hold the rows up to C_DZ / K_PXY only (80 bytes per column): they re-derive a ray's origin from its pixel where ENTER
    //      needs it (`ray_of_pixel`, the code NEWRAY runs: the same bits) and keep the antialiasing sums in global memory (DevFrame::ray_cold; antialiased frames only).
    //      (The suspended level's last t is not kept: a level that is resumed steps -- and sets it -- before anything reads it, or the ray is over.)
    enum { C_STX, C_STY, C_STZ,                     // the suspended outer level while inside a block: t_max
           C_TABS,                                  // |direction| (sr.rs:146)
           C_DX, C_DY, C_DZ,                        // ray direction (sanitised: Parameters::new, raycast.rs:749-771)
           C_OX, C_OY, C_OZ, N_C64_ALL };           // ray origin
    enum { K_SRX, K_SRY, K_SRZ, K_SBOFF,            // the suspended outer level: steps left, byte offset
           K_TVIEW, K_PXY,                          // |direction| / view distance; pixel x | row << 16
           K_BLK, K_S0, K_S1, K_S2, K_ST, N_C32_ALL };  // block index (aux records); ColorBuf::mean accumulators (antialiasing)
    constexpr int N_C64 = XCHG ? (int)C_OX : (int)N_C64_ALL, N_C32 = XCHG ? (int)K_BLK : (int)N_C32_ALL;
    __shared__ double c64[N_C64][NCOL];
    __shared__ uint32_t c32[N_C32][NCOL];
    __shared__ uint32_t s_steps[WGT];               // per thread: steps of the rays it finished (RaytraceInfo)
    // the pool of parked rays (XCHG): per slot the ray's 40 hot dwords (or, free, just the spare column in word 38), and its tag
    __shared__ u32x4 s_pool[NPOOL ? NPOOL : 1u][10];
    constexpr uint32_t NTAG = NPOOL > 128u ? 192u : (NPOOL > 64u ? 128u : 64u);
    __shared__ uint32_t s_tag[NTAG];                // (padded to a multiple of 64: one to three tags per lane are read; the entries past the pool stay BUSY)
    __shared__ u32x4 s_census;                      // parked rays by kind: STEP, SHADE, ENTER, RAY (advisory: read without a claim)
    __shared__ uint8_t s_pick[WGT / 64u][2][64];    // per wave: the slots a round's givers are paired with (wanted kind; free)
    const uint32_t tid = threadIdx.x;
    uint32_t col = tid;  // the LDS column holding this lane's ray
    s_steps[tid] = 0u;
    if (!XCHG) c32[XCHG ? 0 : (int)K_BLK][tid] = 0u;
    c32[K_PXY][tid] = 0u;
    if (XCHG) {
        for (uint32_t i = tid; i < NTAG; i += WGT) s_tag[i] = i < NPOOL ? TAG_FREE : TAG_BUSY;
        for (uint32_t i = tid; i < NPOOL; i += WGT) {
            s_pool[i][9] = u32x4{0u, 0u, WGT + i, 0u};  // the slot's spare column
            c32[K_PXY][WGT + i] = 0u;
        }
        if (tid == 0u) s_census = u32x4{0u, 0u, 0u, 0u};
        __syncthreads();
    }
    uint32_t dry = 0u;                              // wave-uniform, 0 / 1: this wave has seen the tile queue exhausted (a word, not a bool: a bool that the compiler
                                                    // cannot prove uniform is kept as a lane mask, and every read of it costs six instructions)
    // The tile queue this wave takes from (DevFrame::n_queues > 1): its XCD's own to begin with, the next one's when that is empty. How many queues it has
    // seen empty is a word of LDS per wave, read once per tile -- kept in a scalar register for the life of the wave it cost the production variant
    // four spilled VGPRs (12 bytes of scratch per lane, 1.2 GB of scratch written back per C3 frame: profiles/r04_experiments.txt K).
    __shared__ uint32_t s_queues_tried[WGT / 64u];
    __shared__ uint32_t s_tile_state[WGT / 64u][4];  // (XCHG) the wave's tile_x0, tile_y0, next_idx between its RAY phases (registers elsewhere)
    __shared__ uint32_t s_idle_spins[WGT / 64u];  // (XCHG) rounds in which the wave found only rays in transit: bounded, so that nothing can hang
    if (lane == 0u) { s_queues_tried[threadIdx.x >> 6] = 0u; s_idle_spins[threadIdx.x >> 6] = 0u; }
    SurfDiag pend_d;
    double pend_t = 0.0;
    bool pend_visible = false;
    if (DIAG) {
        pend_d.nlight = 0; pend_d.res = pend_d.face = pend_d.block = 0;
        for (int a = 0; a < 3; a++) pend_d.cube[a] = pend_d.voxel[a] = 0;
    }
    // pixel bookkeeping: in LDS (K_PXY, K_S*); the antialiasing sample being traced rides in st bits 14-15
    uint32_t px_steps = 0, px_steps_prev = 0;          // DIAG: steps of this pixel
    Diag dg;
    if (DIAG) {
        dg.n_outer = dg.n_inner = dg.n_hits = dg.n_light = 0; dg.layer = 0; dg.hit = 0; dg.res = dg.face = dg.block = 0; dg.t = 0.0;
        for (int a = 0; a < 3; a++) dg.cube[a] = dg.voxel[a] = 0;
    }
    uint32_t tot_outer = 0, tot_inner = 0, tot_hits = 0, tot_light = 0;
    // DIAG: the Split accumulator's depth and layer (raytrace_to_texture.rs:922-977) beside `dg` -- DepthBuf of the sample being traced and of the pixel so far
    // (the minimum t_distance, accum.rs:266-297), and the layers: bits 0-1 the sample's, bits 2-3 the pixel's (0 none, SPLIT_WORLD, SPLIT_UI)
    constexpr uint32_t SPLIT_WORLD = 1u, SPLIT_UI = 2u;
    double sp_smp = __longlong_as_double(0x7ff0000000000000LL), sp_px = sp_smp;
    uint32_t sp_lay = 0u;
    // a hit of `layer_code`'s layer reached the accumulator: Split::add's layer rule (ColorBuf::opacity_category is Invisible iff the transmittance is 1)
    auto split_layer_after_add = [&](uint32_t layer_code) {
        if (!(sp_lay & 3u) && acc.t != 1.0f) sp_lay |= layer_code;
    };

    uint32_t ev = EV_NEWRAY | EV_TAKE;  // every lane starts by taking a pixel
#ifdef AIC_PROFILE
    // the counters live in the little LDS the kernel leaves free: as registers they would spill the stepping loop
    __shared__ uint32_t s_prof[WGT / 64u][40];
    __shared__ uint32_t s_ray_t0[NCOL];  // per ray: the clock when it started
    uint32_t ray_dur_max = 0u, ray_dur_steps = 0u; // per lane: the longest ray's duration and its step count
    uint32_t tail_trips = 0u, tail_events = 0u, tail_lanes = 0u;  // -DAIC_TAIL_PROF: after the wave saw the queue dry: trips, event phases, lanes stepping at trip start
    uint32_t *const prof = s_prof[tid >> 6];
    if (lane < 40u) prof[lane] = 0u;
    uint32_t prof_tm = (uint32_t)__builtin_readcyclecounter();
    const uint32_t prof_t0 = prof_tm;
#define AIC_PROF(i, v) { const uint32_t v_ = (uint32_t)(v); if (lane == 0u) prof[i] += v_; }
#ifdef AIC_TAIL_PROF
// phase clocks after the wave saw the queue dry go to slots 24.. instead (12 step, 13+18 shade, 14 enter, 15-17 ray, 19 scheduler)
#define AIC_TICK(i) { const uint32_t now_ = (uint32_t)__builtin_readcyclecounter(); const int j_ = (i) == 12 ? 24 : (i) == 13 || (i) == 18 ? 25 : (i) == 14 ? 26 : (i) == 19 ? 28 : 27; \
                      if (lane == 0u) prof[__builtin_amdgcn_readfirstlane((int)dry) ? j_ : (i)] += now_ - prof_tm; prof_tm = now_; }
#else
#define AIC_TICK(i) { const uint32_t now_ = (uint32_t)__builtin_readcyclecounter(); if (lane == 0u) prof[i] += now_ - prof_tm; prof_tm = now_; }
#endif
#else
#define AIC_PROF(i, v)
#define AIC_TICK(i)
#endif
// -DAIC_SECTION_MARKS: comments in the listing that tools/listing_lines.py --sections splits the instruction stream by (static counts per section; the
// markers are volatile asm statements and pin a little of the schedule, so this is a reading aid, not the production build)
#ifdef AIC_SECTION_MARKS
#define AIC_SECTION(name) asm volatile("; AIC_SECTION " #name ::: "memory")
#else
#define AIC_SECTION(name)
#endif
    uint32_t next_idx = F.tile * F.tile;  // wave-uniform: next unassigned pixel of tile_cur (tile_px = tile exhausted)
    if (XCHG && lane == 0u) { s_tile_state[tid >> 6][0] = 0u; s_tile_state[tid >> 6][1] = 0u; s_tile_state[tid >> 6][2] = next_idx; }

    // FACE_TABLE (raycast.rs:618-623) applied late: the Face of the cube the level is in
    auto face_now = [&]() -> uint32_t {
        if (lax & 8u) return lax & 7u;
        // the sign of the ray along a stepped axis is its octant bit (a stepped axis has a non-zero direction)
        const uint32_t positive = (st >> (26u - lax)) & 1u;
        return (positive ? 1u : 4u) + lax;
    };
    // per-ray constants of the Raycaster, rebuilt from the stored direction when an event needs them
    auto make_rd = [&](double dx, double dy, double dz) {
        RayDir r;
        r.dx = dx; r.dy = dy; r.dz = dz;
        r.tdx = tdx; r.tdy = tdy; r.tdz = tdz;
        r.sx = signum_101(dx); r.sy = signum_101(dy); r.sz = signum_101(dz);
        r.fast = (st & ST_DIR_FAST) != 0u;
        return r;
    };
    // coordinate (relative to the level's lower corner) from the steps left along an axis
    // (the counters hold steps left MINUS ONE, so that running out is the borrow of the decrement: see dda_step)
    auto coord = [](uint32_t positive, int size, uint32_t r) -> int { return positive ? size - 1 - (int)r : (int)r; };

    // -- State::step (raycast.rs:577-626) along the axis of the smallest t_max (strict <, ties to the
    //    later axis: raycast.rs:584-596): X iff tx<ty && tx<tz, Y iff !(tx<ty) && ty<tz, else Z.
    //    One exec-masked run per axis: last_t = t; t += t_delta; steps_left -= 1; offset += stride. --
    auto dda_step = [&](const unsigned long long m_who) -> unsigned long long {
        unsigned long long sv, mx, bz, by, bx;
        // last_t = the smallest t_max, whichever axis holds it: Z iff tz is that minimum (ties go to the later axis),
        // Y iff ty is and tz is not, X otherwise -- two v_min and two compares instead of three compares and three copies.
        // The steps-left counters are biased by one, so "ran out" is the borrow of the decrement (the carry-out of an
        // exec-masked v_sub_co is zero for the lanes it does not run on). Keeping the stepped axis in wave masks instead
        // of `lax` (3 vector instructions less, 6 scalar more) was measured and is slower: profiles/r03_experiments.txt I.
        asm volatile(
            "s_and_saveexec_b64 %[sv], %[m]\n\t"
            "v_min_f64 %[lt], %[tx], %[ty]\n\t"
            "v_min_f64 %[lt], %[lt], %[tz]\n\t"
            "v_cmp_eq_f64 %[mx], %[tz], %[lt]\n\t"        // Z
            "v_cmp_eq_f64 vcc, %[ty], %[lt]\n\t"
            "s_andn2_b64 vcc, vcc, %[mx]\n\t"             // Y
            "s_mov_b64 exec, %[mx]\n\t"
            "v_add_f64 %[tz], %[tz], %[tdz]\n\t"
            "v_sub_co_u32 %[rz], %[bz], %[rz], 1\n\t"
            "v_add_u32 %[bo], %[bo], %[ssz]\n\t"
            "v_mov_b32 %[lax], 2\n\t"
            "s_or_b64 %[mx], %[mx], vcc\n\t"
            "s_mov_b64 exec, vcc\n\t"
            "v_add_f64 %[ty], %[ty], %[tdy]\n\t"
            "v_sub_co_u32 %[ry], %[by], %[ry], 1\n\t"
            "v_add_u32 %[bo], %[bo], %[ssy]\n\t"
            "v_mov_b32 %[lax], 1\n\t"
            "s_andn2_b64 exec, %[m], %[mx]\n\t"           // X = stepping lanes that took neither
            "v_add_f64 %[tx], %[tx], %[tdx]\n\t"
            "v_sub_co_u32 %[rx], %[bx], %[rx], 1\n\t"
            "v_add_u32 %[bo], %[bo], %[ssx]\n\t"
            "v_mov_b32 %[lax], 0\n\t"
            "s_mov_b64 exec, %[sv]\n\t"
            "s_or_b64 %[bz], %[bz], %[by]\n\t"
            "s_or_b64 %[bz], %[bz], %[bx]\n\t"
            : [tx] "+v"(tx), [ty] "+v"(ty), [tz] "+v"(tz), [lt] "+v"(last_t), [rx] "+v"(rx), [ry] "+v"(ry), [rz] "+v"(rz),
              [bo] "+v"(boff), [lax] "+v"(lax), [sv] "=&s"(sv), [mx] "=&s"(mx),
              [bz] "=&s"(bz), [by] "=&s"(by), [bx] "=&s"(bx)
            : [tdx] "v"(tdx), [tdy] "v"(tdy), [tdz] "v"(tdz), [ssx] "v"(ssx), [ssy] "v"(ssy), [ssz] "v"(ssz), [m] "s"(m_who)
            : "vcc", "scc");  // (the scalar mask operations write SCC)
        return bz;  // lanes whose level ran out of steps: it left its bounds
    };
    // (XCHG) counts a round that could do nothing; true once the wave has had 2^22 of them (a bug's hang would cost the GPU box). The count is cumulative over the
    // wave's life, not reset by progress (a reset would be a masked LDS store in every round): an idle round sleeps >= 256 cycles, so the bound is >= 10^9 cycles --
    // half a second -- of ONE wave's life spent waiting for rays in transit, against frames of milliseconds with a few such rounds per wave
    // (profiles/r05_phase_cycles.txt: 649 / 4415 in a whole C2 / C3 frame). A wave that does give up says so: DevCounters::bailed makes the frame fail on the host.
    auto spun_out = [&]() -> bool {
        const uint32_t n_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_idle_spins[threadIdx.x >> 6]) + 1u;
        if (lane == 0u) s_idle_spins[threadIdx.x >> 6] = n_;
        if (n_ > (1u << 22)) {
            // (the argument through the opaque kernel-argument pointer, like the event phase's: a plain use of `F` here would hold the pointer in registers for the life of the wave)
            typedef const __attribute__((address_space(4))) DevFrame KFrameB;
            KFrameB *Fb = (KFrameB *)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(Fb));
            if (lane == 0u) atomicAdd(&Fb->sub[Fb->n_sub > 1u ? (blockIdx.x & (Fb->n_sub - 1u)) : 0u].counters->bailed, 1ull);
            return true;
        }
        return false;
    };
    for (;;) {
        AIC_SECTION(scheduler);
        // ---- wave scheduler: step, or run ONE kind of parked work for all lanes waiting on it ----
        // Kinds: SHADE (light + composite a surface), ENTER (a block), RAY (finish / start a ray). A
        // kind is run when enough lanes wait on it to fill the wave reasonably (AIC_T_BATCH), or when
        // so few lanes can still step (AIC_N_FEW) that waiting longer only idles the wave.
        unsigned long long m_st = __ballot(ev < 4u);
        unsigned long long b_shade = __ballot((ev & EV_SHADE) != 0u);
        unsigned long long b_enter = __ballot((ev & EV_ENTER) != 0u);
        unsigned long long b_ray = __ballot((ev & (EV_FINISH | EV_NEWRAY)) != 0u);
        int n_step = (int)wave_popc(m_st);
        int c_shade = (int)wave_popc(b_shade), c_enter = (int)wave_popc(b_enter), c_ray = (int)wave_popc(b_ray);
        uint32_t run = 0u;  // kind to run this trip (an EV_* bit), 0 = step
        if constexpr (XCHG) {
            // ---- regime-sorted waves: run the kind that fills the wave best, own lanes plus what the workgroup's pool can add ----
            // what this round's exchange (if any) decided: the lanes whose claim succeeded, those of them that took a spare column, the slot's address and
            // index, the tag the slot is released under, the kind taken (the swap itself sits on the round's common path, below)
            unsigned long long x_got = 0ull, x_fresh = 0ull;
            // (left undefined in a round without an exchange -- nothing reads them under an empty mask -- rather than zeroed: four vector moves in every round)
            // (two vector registers and a scalar carried to the swap: each one zeroed in a round without an exchange is an instruction in every round)
            uint32_t x_paddr = 0u, x_slot_tag = 0u;  // the slot's address; its index | the released tag << 8
            uint32_t x_want = 0u;                    // (wave-uniform)
            // a wave that is full of one kind as it stands (AIC_XCHG_FULL lanes: at most one kind can be) runs it without looking at the pool
            static_assert(AIC_XCHG_FULL > 32, "two kinds could both be full");
            static_assert(EV_SHADE == (2u << 1) && EV_ENTER == (2u << 2) && EV_FINISH == (2u << 3), "the kinds' event bits");
            bool settled = true;  // the kind's own lanes are known to be there (no look at the counts after the exchange)
            {
                // (the partial maxima through opaque_s: fused, the three become a v_max3 with two copies in front and a v_readfirstlane behind)
                const int m01 = opaque_s(n_step > c_shade ? n_step : c_shade), m23 = opaque_s(c_enter > c_ray ? c_enter : c_ray);
                if ((m01 > m23 ? m01 : m23) >= AIC_XCHG_FULL) run = c_ray >= AIC_XCHG_FULL ? EV_FINISH : (c_enter >= AIC_XCHG_FULL ? EV_ENTER : (c_shade >= AIC_XCHG_FULL ? EV_SHADE : 0u));
                else run = 0xffffffffu;
            }
            if (run == 0xffffffffu) {
            // parked rays by kind, read at the top of the round. A count is never BEHIND the tags (a parked ray is counted before its slot is released, and taken
            // off after it is claimed), so it is never negative and "every count zero" means that no claimable ray is parked; it can run AHEAD of them (a ray
            // claimed by another wave and not yet taken off): then the kind chosen for it may find nothing, which the end of the round handles.
            // (A plain LDS load behind a compiler barrier, so that it is made again in every round: through a `volatile` pointer it was compiled as a FLAT load --
            //  address-space inference leaves volatile accesses alone -- followed by s_waitcnt vmcnt(0), i.e. every scheduler round waited for every store the
            //  wave still had in flight. Made here, not at the top of the round: a wave that is full of one kind does not wait for counts it does not read.)
            asm volatile("" ::: "memory");
            const u32x4 cs = s_census;
            const int pk_step = __builtin_amdgcn_readfirstlane((int)cs.x), pk_shade = __builtin_amdgcn_readfirstlane((int)cs.y),
                      pk_enter = __builtin_amdgcn_readfirstlane((int)cs.z), pk_ray = __builtin_amdgcn_readfirstlane((int)cs.w);
            // the kind with the most lanes -- its own + the parked rays that fit into the wave's other lanes; ties go to the events, the later kind first (a
            // parked event lane blocks its ray, a stepping lane can wait): the four totals as keys  total << 9 | kind << 7 | own lanes  and one maximum
            // (kind: 0 stepping, 1 SHADE, 2 ENTER, 3 RAY; EV_SHADE / EV_ENTER / EV_FINISH = 2 << kind)
            auto key_of = [](int own, int pk, int kind) -> int {
                const int all = own + pk;
                return ((all < 64 ? all : 64) << 9) | (kind << 7) | own;
            };
            const int key0 = key_of(n_step, pk_step, 0), key1 = key_of(c_shade, pk_shade, 1), key2 = key_of(c_enter, pk_enter, 2), key3 = key_of(c_ray, pk_ray, 3);
            const int ka = opaque_s(key0 > key1 ? key0 : key1), kb = opaque_s(key2 > key3 ? key2 : key3), kmax = ka > kb ? ka : kb;
            if (kmax < 512) break;  // nothing of its own and nothing parked: whoever parks a ray later is running and serves it
            const int best = kmax >> 9, kind = (kmax >> 7) & 3, mine = kmax & 127;
            run = kind == 0 ? 0u : (2u << kind);
            settled = mine != 0;
            AIC_TICK(19);
            const int dry_i = __builtin_amdgcn_readfirstlane((int)dry);
            const int alive = n_step + c_shade + c_enter + c_ray, parked = pk_step + pk_shade + pk_enter + pk_ray;
            const int n_others = alive - mine;  // lanes holding a ray that will not run now (and may be parked)
            // An exchange costs a few hundred instructions: it is made for a top-up of at least AIC_XCHG_MIN_GAIN lanes, for a kind the wave has none of, or -- while
            // the image has pixels left and the pool a free slot -- to park at least AIC_XCHG_PARK_MIN lanes:
            //     best - mine >= MIN_GAIN  ||  mine == 0  ||  (!dry && parked < NPOOL && n_others >= PARK_MIN)
            // as one comparison of integers that are >= 0 where their term holds (a dozen scalar instructions; as booleans every term is a compare, a 64-bit
            // select and a 64-bit and / or)
            static_assert(AIC_XCHG_PARK_MIN > 0, "parking wants lanes to park");
            const int park_room = (int)NPOOL - 1 - parked, not_dry = -dry_i;
            const int park_ok_i = park_room < not_dry ? park_room : not_dry;                             // >= 0: parking is possible
            const int t_park = n_others - AIC_XCHG_PARK_MIN, t_gain = best - mine - AIC_XCHG_MIN_GAIN, t_none = -opaque_s(mine);  // (opaque: else the negation is made on the vector unit, for the carry that says mine != 0)
            const int t_p = park_ok_i < t_park ? park_ok_i : t_park;
            const int t_a = opaque_s(t_gain > t_none ? t_gain : t_none);  // (kept apart: fused, the two maxima become a v_max3 with copies in front and a vector compare behind)
            if ((t_a > t_p ? t_a : t_p) >= 0) {
                AIC_SECTION(exchange);
                const bool may_park = park_ok_i >= 0 && n_others > 0;
                // ---- the exchange: lanes that would idle ("givers": empty lanes first, then rays of other kinds) are paired with parked rays of the wanted
                // kind, and -- while the image has pixels left -- what remains of them with free slots. A pairing is a claim (compare-and-swap of the slot's
                // tag), a plain swap of the 40 hot dwords and the column index, and the release of the slot under the tag of what it now holds. ----
                // (the lane number through an empty asm: what is derived from it -- LDS addresses of the tags and lists, comparisons with the pool size -- is
                //  otherwise computed before the persistent loop and kept in registers the event code needs)
                uint32_t ln = lane;
                asm volatile("" : "+v"(ln));
                // (written as straight-line selects and exec-masked stores: per-lane `if`s and short-circuit conditions cost a saved / restored exec mask each, and
                //  assigning the hot variables inside a branch makes the compiler copy all of them on the path that does not take it -- in every round)
                const uint32_t want = run == 0u ? TAG_STEP : (run == EV_SHADE ? TAG_SHADE : (run == EV_ENTER ? TAG_ENTER : TAG_RAY));
                const bool e_done = ev == EV_DONE, e_take = ev == (EV_NEWRAY | EV_TAKE);
                const bool empty = e_done | e_take;
                uint32_t my_tag = (ev & (EV_FINISH | EV_NEWRAY)) != 0u ? TAG_RAY : TAG_STEP;
                my_tag = (ev & EV_ENTER) != 0u ? TAG_ENTER : my_tag;
                my_tag = (ev & EV_SHADE) != 0u ? TAG_SHADE : my_tag;
                my_tag = empty ? TAG_FREE : my_tag;
                const bool giver = (my_tag != want) & (!e_take | (want != TAG_RAY));  // (an empty lane about to take a pixel IS the RAY kind)
                const unsigned long long m_giv = __builtin_amdgcn_ballot_w64(giver);
                auto below = [](unsigned long long m) -> uint32_t { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); };
                const uint32_t n_giv = wave_popc(m_giv);
                const uint32_t rank = below(m_giv);  // (givers in lane order)
                // the slots' tags, three per lane (the array is padded to 192 with BUSY); the first 64 slots of the wanted kind and the first 64 free ones go
                // into the wave's pairing lists
                const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)((tid - ln) >> 6));
                const uint32_t t0 = __hip_atomic_load(&s_tag[ln], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const uint32_t t1 = NPOOL > 64u ? __hip_atomic_load(&s_tag[ln + 64u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : TAG_BUSY;
                const uint32_t t2 = NPOOL > 128u ? __hip_atomic_load(&s_tag[ln + 128u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : TAG_BUSY;
                const unsigned long long w0 = __builtin_amdgcn_ballot_w64(t0 == want), w1 = __builtin_amdgcn_ballot_w64(t1 == want), w2 = __builtin_amdgcn_ballot_w64(t2 == want);
                // (every wave would otherwise list the same lowest slots first, and two waves exchanging at the same moment would fight over them: odd waves
                //  list from the top down)
                const uint32_t nw0 = wave_popc(w0), nw1 = wave_popc(w1), nw2 = wave_popc(w2), n_w = nw0 + nw1 + nw2;
                const bool down = (wv & 1u) != 0u;
                uint8_t *const pick_w = s_pick[wv][0], *const pick_f = s_pick[wv][1];
                { const uint32_t u_ = below(w0), i_ = down ? n_w - 1u - u_ : u_; if ((t0 == want) & (i_ < 64u)) pick_w[i_] = (uint8_t)ln; }
                if (NPOOL > 64u) { const uint32_t u_ = nw0 + below(w1), i_ = down ? n_w - 1u - u_ : u_; if ((t1 == want) & (i_ < 64u)) pick_w[i_] = (uint8_t)(ln + 64u); }
                if (NPOOL > 128u) { const uint32_t u_ = nw0 + nw1 + below(w2), i_ = down ? n_w - 1u - u_ : u_; if ((t2 == want) & (i_ < 64u)) pick_w[i_] = (uint8_t)(ln + 128u); }
                uint32_t n_f = 0u;
                if (may_park) {  // (uniform) the free slots, for the lanes that park
                    const unsigned long long f0 = __builtin_amdgcn_ballot_w64(t0 == TAG_FREE), f1 = __builtin_amdgcn_ballot_w64(t1 == TAG_FREE), f2 = __builtin_amdgcn_ballot_w64(t2 == TAG_FREE);
                    const uint32_t nf0 = wave_popc(f0), nf1 = wave_popc(f1);
                    n_f = nf0 + nf1 + wave_popc(f2);
                    { const uint32_t u_ = below(f0), i_ = down ? n_f - 1u - u_ : u_; if ((t0 == TAG_FREE) & (i_ < 64u)) pick_f[i_] = (uint8_t)ln; }
                    if (NPOOL > 64u) { const uint32_t u_ = nf0 + below(f1), i_ = down ? n_f - 1u - u_ : u_; if ((t1 == TAG_FREE) & (i_ < 64u)) pick_f[i_] = (uint8_t)(ln + 64u); }
                    if (NPOOL > 128u) { const uint32_t u_ = nf0 + nf1 + below(f2), i_ = down ? n_f - 1u - u_ : u_; if ((t2 == TAG_FREE) & (i_ < 64u)) pick_f[i_] = (uint8_t)(ln + 128u); }
                }
                __builtin_amdgcn_wave_barrier();  // (the lists are written by some lanes and read by others of this wave: LDS operations of a wave are performed in order; this keeps the compiler from reordering them)
                const uint32_t n_take = n_w < n_giv ? n_w : n_giv;  // (at most 64)
                const uint32_t n_free = n_f < 64u ? n_f : 64u;
                // a giver of rank < n_take takes a parked ray; the rays of the ranks after that are parked while slots are free
                const bool takes = giver & (rank < n_take);
                const uint32_t j_ = rank - n_take;
                const bool parks = giver & !empty & (rank >= n_take) & (j_ < n_free);  // (n_free is 0 unless may_park)
                const uint32_t expect = takes ? want : TAG_FREE;
                const uint32_t slot = (takes | parks) ? (uint32_t)(takes ? pick_w : pick_f)[takes ? rank : (j_ & 63u)] : 0u;
                bool got = false;
                if (takes | parks) {
                    uint32_t seen = expect;
                    got = __hip_atomic_compare_exchange_strong(&s_tag[slot], &seen, TAG_BUSY, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                // (nothing of a ray lives in global memory except the antialiasing sums, and whoever stores those waits for the store at once: cold_sums_store)
                x_got = __builtin_amdgcn_ballot_w64(got);
                x_fresh = x_got & ~__builtin_amdgcn_ballot_w64(takes);
                x_paddr = (uint32_t)(uintptr_t)&s_pool[0][0] + slot * 160u;
                x_slot_tag = slot | (my_tag << 8); x_want = want;
                AIC_PROF(37, wave_popc(__builtin_amdgcn_ballot_w64(takes | parks)) - wave_popc(x_got));  // claims lost to another wave
                if (x_got == 0ull) { AIC_PROF(38, 1); }  // an exchange that moved nothing
            // (the two masks through v_readfirstlane: they are wave-uniform by construction, but a build in which the compiler's divergence analysis loses that --
            //  the -DAIC_PROFILE one did -- would hand vector registers to the scalar operands below, and to every mask of the stepping phase after them)
            {
                auto uniform64 = [](unsigned long long m) -> unsigned long long {
                    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
                };
                x_got = uniform64(x_got);
                x_fresh = uniform64(x_fresh);
            }
            // ---- The swap proper, under exec = the lanes whose claim succeeded: one LDS exchange (`ds_wrxchg_rtn`: write the register, return what was there)
            // per hot variable, IN PLACE -- like the stepping code's asm blocks. (Assigned from loaded values in C++, the compiler renames the hot variables
            // and copies all 38 registers around each block. Earlier builds kept these blocks on the round's common path, skipped by an empty mask, because
            // inside the exchange's branch the same copies appeared at the branch; with the in-place asm they do not, and a round without an exchange -- four
            // in five -- no longer passes through them; profiles/r05_experiments.txt L has the listings' instruction counts.) ----
            if (x_got != 0ull) {
                unsigned long long sv;
                asm volatile(
                    "s_and_saveexec_b64 %[sv], %[m]\n\t"
                    "s_cbranch_execz .Lxa%=\n\t"
                    "ds_wrxchg_rtn_b64 %[x0], %[p], %[x0]\n\t"
                    "ds_wrxchg_rtn_b64 %[x1], %[p], %[x1] offset:8\n\t"
                    "ds_wrxchg_rtn_b64 %[x2], %[p], %[x2] offset:16\n\t"
                    "ds_wrxchg_rtn_b64 %[x3], %[p], %[x3] offset:24\n\t"
                    "ds_wrxchg_rtn_b64 %[x4], %[p], %[x4] offset:32\n\t"
                    "ds_wrxchg_rtn_b64 %[x5], %[p], %[x5] offset:40\n\t"
                    "ds_wrxchg_rtn_b64 %[x6], %[p], %[x6] offset:48\n\t"
                    "s_waitcnt lgkmcnt(0)\n"
                    ".Lxa%=:\n\t"
                    "s_mov_b64 exec, %[sv]\n\t"
                    : [x0] "+v"(tx), [x1] "+v"(ty), [x2] "+v"(tz), [x3] "+v"(last_t), [x4] "+v"(tdx), [x5] "+v"(tdy), [x6] "+v"(tdz), [sv] "=&s"(sv)
                    : [p] "v"(x_paddr), [m] "s"(x_got)
                    : "memory", "scc");
                asm volatile(
                    "s_and_saveexec_b64 %[sv], %[m]\n\t"
                    "s_cbranch_execz .Lxb%=\n\t"
                    "ds_wrxchg_rtn_b32 %[w0], %[p], %[w0] offset:56\n\t"
                    "ds_wrxchg_rtn_b32 %[w1], %[p], %[w1] offset:60\n\t"
                    "ds_wrxchg_rtn_b32 %[w2], %[p], %[w2] offset:64\n\t"
                    "ds_wrxchg_rtn_b32 %[w3], %[p], %[w3] offset:68\n\t"
                    "ds_wrxchg_rtn_b32 %[w4], %[p], %[w4] offset:72\n\t"
                    "ds_wrxchg_rtn_b32 %[w5], %[p], %[w5] offset:76\n\t"
                    "ds_wrxchg_rtn_b32 %[w6], %[p], %[w6] offset:80\n\t"
                    "ds_wrxchg_rtn_b32 %[w7], %[p], %[w7] offset:84\n\t"
                    "ds_wrxchg_rtn_b32 %[w8], %[p], %[w8] offset:88\n\t"
                    "ds_wrxchg_rtn_b32 %[w9], %[p], %[w9] offset:92\n\t"
                    "ds_wrxchg_rtn_b32 %[wa], %[p], %[wa] offset:96\n\t"
                    "ds_wrxchg_rtn_b32 %[wb], %[p], %[wb] offset:100\n\t"
                    "s_waitcnt lgkmcnt(0)\n"
                    ".Lxb%=:\n\t"
                    "s_mov_b64 exec, %[sv]\n\t"
                    : [w0] "+v"(rx), [w1] "+v"(ry), [w2] "+v"(rz), [w3] "+v"(boff), [w4] "+v"(ssx), [w5] "+v"(ssy), [w6] "+v"(ssz), [w7] "+v"(thr), [w8] "+v"(raw),
                      [w9] "+v"(lax), [wa] "+v"(st), [wb] "+v"(count), [sv] "=&s"(sv)
                    : [p] "v"(x_paddr), [m] "s"(x_got)
                    : "memory", "scc");
                asm volatile(
                    "s_and_saveexec_b64 %[sv], %[m]\n\t"
                    "s_cbranch_execz .Lxc%=\n\t"
                    "ds_wrxchg_rtn_b32 %[w0], %[p], %[w0] offset:104\n\t"
                    "ds_wrxchg_rtn_b32 %[w1], %[p], %[w1] offset:108\n\t"
                    "ds_wrxchg_rtn_b32 %[w2], %[p], %[w2] offset:112\n\t"
                    "ds_wrxchg_rtn_b32 %[w3], %[p], %[w3] offset:116\n\t"
                    "ds_wrxchg_rtn_b32 %[w4], %[p], %[w4] offset:120\n\t"
                    "ds_wrxchg_rtn_b32 %[w5], %[p], %[w5] offset:124\n\t"
                    "ds_wrxchg_rtn_b32 %[w6], %[p], %[w6] offset:128\n\t"
                    "ds_wrxchg_rtn_b32 %[w7], %[p], %[w7] offset:132\n\t"
                    "ds_wrxchg_rtn_b32 %[w8], %[p], %[w8] offset:136\n\t"
                    "ds_wrxchg_rtn_b32 %[w9], %[p], %[w9] offset:140\n\t"
                    "ds_wrxchg_rtn_b32 %[wa], %[p], %[wa] offset:144\n\t"
                    "ds_wrxchg_rtn_b32 %[wb], %[p], %[wb] offset:148\n\t"
                    "ds_wrxchg_rtn_b32 %[wc], %[p], %[wc] offset:152\n\t"
                    "s_waitcnt lgkmcnt(0)\n\t"
                    "s_mov_b64 exec, %[f]\n\t"            // the lanes that took a spare column: an empty lane about to take a pixel
                    "v_mov_b32 %[w0], 0xa0\n"             // ev = EV_NEWRAY | EV_TAKE
                    ".Lxc%=:\n\t"
                    "s_mov_b64 exec, %[sv]\n\t"
                    : [w0] "+v"(ev), [w1] "+v"(blk_pal_off), [w2] "+v"(blk_geo), [w3] "+v"(blk_vsz), [w4] "+v"(acc.l0), [w5] "+v"(acc.l1), [w6] "+v"(acc.l2), [w7] "+v"(acc.t),
                      [w8] "+v"(pend0), [w9] "+v"(pend1), [wa] "+v"(pend2), [wb] "+v"(pend_tr), [wc] "+v"(col), [sv] "=&s"(sv)
                    : [p] "v"(x_paddr), [m] "s"(x_got), [f] "s"(x_fresh)
                    : "memory", "scc");
                static_assert((EV_NEWRAY | EV_TAKE) == 0xa0u, "the literal in the asm above");
                const bool got = __builtin_amdgcn_inverse_ballot_w64(x_got), fresh = __builtin_amdgcn_inverse_ballot_w64(x_fresh);
                // the counts: every lane that parked a ray adds it to its kind (LDS atomics on one word each: a few cycles per lane, two instructions) BEFORE
                // its slot is released under the tag of what it now holds -- LDS operations of a wave are performed in order, so no wave can claim the ray, and
                // take it off the count, before it is on it: a count is never negative; one lane takes off what was taken
                const uint32_t n_picked = wave_popc(x_got & ~x_fresh);
                const uint32_t x_slot = x_slot_tag & 255u, x_tag = x_slot_tag >> 8;
                if (got && x_tag != TAG_FREE) atomicAdd(reinterpret_cast<uint32_t *>(&s_census) + (x_tag - 1u), 1u);
                if (got) __hip_atomic_store(&s_tag[x_slot], x_tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (lane == 0u && n_picked != 0u) atomicSub(reinterpret_cast<uint32_t *>(&s_census) + (x_want - 1u), n_picked);
                (void)fresh;
                AIC_PROF(31, 1);
                AIC_PROF(32, wave_popc(x_got));
                AIC_PROF(34, n_picked);
                AIC_PROF(35, wave_popc(__builtin_amdgcn_ballot_w64(got && x_tag != TAG_FREE)));
                m_st = __ballot(ev < 4u);
                b_shade = __ballot((ev & EV_SHADE) != 0u);
                b_enter = __ballot((ev & EV_ENTER) != 0u);
                b_ray = __ballot((ev & (EV_FINISH | EV_NEWRAY)) != 0u);
                n_step = (int)wave_popc(m_st);
                c_shade = (int)wave_popc(b_shade); c_enter = (int)wave_popc(b_enter); c_ray = (int)wave_popc(b_ray);
                AIC_TICK(33);
            }
            }
            }
            else { AIC_TICK(19); }
            AIC_SECTION(scheduler_tail);
            if (!settled && (run == 0u ? n_step : (run == EV_SHADE ? c_shade : (run == EV_ENTER ? c_enter : c_ray))) == 0) {
                // (the kind was chosen for what the pool holds, and every claim was lost to another wave -- or only rays in transit were found)
                AIC_PROF(36, 1);
                if (spun_out()) break;
                __builtin_amdgcn_s_sleep(4);
                continue;
            }
        } else {
        if ((m_st | b_shade | b_enter | b_ray) == 0ull) break;
        {
            int best = c_shade;
            uint32_t kind = EV_SHADE;
            if (c_enter > best) { best = c_enter; kind = EV_ENTER; }
            if (c_ray > best) { best = c_ray; kind = EV_FINISH; }
            // thresholds scale with the lanes still alive, so that a wave that is running out of rays
            // (the frame's tail) keeps batching instead of running every event for a lane or two
            const int alive = n_step + c_shade + c_enter + c_ray;
            const int part_t = (alive * AIC_FRAC_T) >> 3, part_n = (alive * AIC_FRAC_N) >> 3;
            const int t_lo = opaque_s(part_t > 0 ? part_t : 1);  // (kept apart from the min: fused, the pair becomes a v_med3 and a v_readfirstlane)
            const int t_batch = t_lo < AIC_T_BATCH ? t_lo : AIC_T_BATCH;
            const int n_few = part_n < AIC_N_FEW ? part_n : AIC_N_FEW;
            if (best > 0 && (best >= t_batch || n_step <= n_few)) run = kind;
        }
        AIC_TICK(19);
        }
        if (run != 0u) {
            AIC_SECTION(event_prologue);
            // ============================ event phase ======================================
            // the kernel arguments, through an opaque pointer (see the top of the kernel): `F`, `L`, `opt` below shadow the
            // by-value parameter for the whole phase
            typedef const __attribute__((address_space(4))) DevFrame KFrame;
            KFrame *Fq = (KFrame *)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(Fq));
            KFrame &F = *Fq;
            const auto &L = F.layer;
            const auto &opt = L.opt;
            // the frame this workgroup belongs to (DevSub: a launch may trace several; everything per frame is a scalar load at a uniform offset)
            typedef const __attribute__((address_space(4))) DevSub KSub;
            KSub *Sq = reinterpret_cast<KSub *>(reinterpret_cast<const __attribute__((address_space(4))) char *>(Fq) + offsetof(DevFrame, sub)) +
                       (F.n_sub > 1u ? (blockIdx.x & (F.n_sub - 1u)) : 0u);
            asm volatile("" : "+s"(Sq));
            KSub &S = *Sq;
            const bool ui_pass = F.pass == 1;
            const bool include_sky = F.pass == 0;  // (pass 2: a ray batch traced with include_sky = false, sr.rs:145-161 -- a final pass in every other respect)
            const bool fog_on = (opt.fog != 0) && include_sky;
            const size_t npix = (size_t)F.width * F.local_rows;
            const int n_samples = F.antialias ? 4 : 1;
            const int olx = L.lo[0], oly = L.lo[1], olz = L.lo[2];
            const int osx_i = L.size[0], osy_i = L.size[1], osz_i = L.size[2];
            const uint32_t tile_px = F.tile * F.tile;  // pixels per tile: 256 or 64
            const uint32_t macro_shift = (uint32_t)__ffs((int)F.macro) - 1u;
            const uint32_t macro_px_shift = macro_shift + (uint32_t)__ffs((int)F.tile) - 1u;  // log2 of a macro tile's edge in pixels
            const uint32_t n_virtual = (F.macros_x * F.macros_y) << (macro_shift * 2u);  // work items incl. the macro tiles' overhang
            // sky colour seen along this ray (Sky::sample, sky.rs:32-41); the octant was fixed at ray start. An octant sky is
            // read per lane from the kernel-argument segment as ordinary memory: indexing the array per lane in registers
            // would make the compiler keep a copy of it in scratch.
            auto sky_now = [&](float out[3]) {
                if (L.sky_kind != 0) {
                    const float *p = (const float *)((const char *)(const void *)Fq + offsetof(DevFrame, layer) + offsetof(DevLayer, sky)) + 3u * ((st >> 24) & 7u);
                    out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
                } else {
                    out[0] = L.sky[0][0]; out[1] = L.sky[0][1]; out[2] = L.sky[0][2];
                }
            };
            AIC_PROF(0, 1);
            AIC_PROF(1, c_shade + c_enter + c_ray);
#ifdef AIC_TAIL_PROF
            if (__builtin_amdgcn_readfirstlane((int)dry)) { tail_events++; AIC_PROF(30, 1); }
#endif
            AIC_PROF(4, run == EV_SHADE ? 1 : 0); AIC_PROF(5, run == EV_SHADE ? c_shade : 0);
            AIC_PROF(6, run == EV_ENTER ? 1 : 0); AIC_PROF(7, run == EV_ENTER ? c_enter : 0);
            AIC_PROF(8, run == EV_FINISH ? 1 : 0); AIC_PROF(9, run == EV_FINISH ? c_ray : 0);
            // -- The ray of a pixel: RtScene::trace_patch's sample point (renderer.rs:424-451) through Camera::project_ndc_into_world
            //    (camera_struct.rs:238-257), or MultiOrthoCamera::project_pixel_into_world for orthographic views. `o` = the ray's origin and, if asked
            //    for, `dir` = its direction as given (not yet sanitised). NEWRAY runs this when the ray starts; the exchanging variants run it AGAIN
            //    (origin only) wherever a later event needs the origin, instead of keeping 24 bytes per ray for the whole of its life: same code, same
            //    inputs (the pixel in K_PXY, the sample in st, the kernel arguments), hence the same bits. Returns false when there is no ray. --
            auto ray_of_pixel = [&](const uint32_t x, const uint32_t lrow, const int sample, const bool want_dir, double o[3], double dir[3]) -> bool {
                // The common cameras first, behind ONE scalar fetch (DevFrame::ray_mode, made by the launcher): a pixel grid with the host-made edge tables and a layer
                // that holds a space. (The general form below asks five kernel arguments one after the other -- strips? pixel centres? patches? tables? orthographic? --
                // each a scalar load and a wait in front of its branch: ~600 cycles of NEWRAY's and ENTER's few thousand.) Same operations on the same values as below.
                const uint32_t mode = F.ray_mode;
                if (mode <= 1u) {
                    const double *const ex = F.edge_x, *const ey = F.edge_y;
                    uint32_t y = lrow;
                    if (mode == 1u) {
                        const uint32_t srows = opaque_s(F.strip_rows);
                        const uint32_t strip = lrow / srows;
                        y = (F.part + strip * F.n_parts) * srows + (lrow - strip * srows);
                    }
                    const double x0 = ex[x], x1 = ex[x + 1u], y0 = ey[y], y1 = ey[y + 1u];
                    double px, py;
                    if (n_samples == 4) {
                        const double ux = (sample == 0) ? 1. / 8. : (sample == 1) ? 3. / 8. : (sample == 2) ? 5. / 8. : 7. / 8.;
                        const double uy = (sample == 0) ? 5. / 8. : (sample == 1) ? 1. / 8. : (sample == 2) ? 7. / 8. : 3. / 8.;
                        px = x0 + (x1 - x0) * ux;
                        py = y0 + (y1 - y0) * uy;
                    } else {
                        px = (x0 + x1) / 2.0;
                        py = (y0 + y1) / 2.0;
                    }
                    unproject(S.inv, px, py, 0.0, o);
                    if (want_dir) {
                        double f[3];
                        unproject(S.inv, px, py, 1.0, f);
                        dir[0] = f[0] - o[0]; dir[1] = f[1] - o[1]; dir[2] = f[2] - o[2];
                    }
                    return true;
                }
                const size_t pix = (size_t)lrow * F.width + x;
                if (F.rays) {
                    // aic_trace_rays: the ray as the host gave it, SpaceRaytracer::trace_ray's argument (sr.rs:113-120) -- [pix][6] doubles, origin then direction, 48
                    // bytes at a 16-byte boundary (the host checks): three 16-byte vector loads under one wait (the base is uniform, the address per lane), or, for the
                    // exchanging variants' re-derived origin, the first 24 bytes. The layer holds a space (checked by the host as well).
                    const double2 *const r = reinterpret_cast<const double2 *>(F.rays + 6u * pix);
                    const double2 r0 = r[0], r1 = r[1];
                    o[0] = r0.x; o[1] = r0.y; o[2] = r1.x;
                    if (want_dir) {
                        const double2 r2 = r[2];
                        dir[0] = r1.y; dir[1] = r2.x; dir[2] = r2.y;
                    }
                    return true;
                }
                // global row of this local row under the strip partition
                uint32_t y = lrow;
                if (F.n_parts > 1u) {
                    const uint32_t srows = opaque_s(F.strip_rows);
                    const uint32_t strip = lrow / srows;
                    y = (F.part + strip * F.n_parts) * srows + (lrow - strip * srows);
                }
                // aic_trace_pixels (the recording variants): the batch position names a pixel of the target frame, and from here on the image path runs on that
                // pixel and that frame's shape -- its edge tables, its width and height for pixel centres (the tile decode has checked the entry's range)
                const bool listed = DIAG && F.pixels;
                uint32_t gx = x;
                if (listed) {
                    const uint32_t p_ = F.pixels[pix], pw_ = opaque_s(F.px_width);
                    y = p_ / pw_;
                    gx = p_ - y * pw_;
                }
                double px, py;  // renderer.rs:428-433 sample points, else the patch centre
                if (F.pixel_centers) {  // Viewport::normalize_fb_x / _y (viewport.rs:89-99): the text renderer's rays
                    const uint32_t fw = opaque_s(listed ? F.px_width : F.width), fh = opaque_s(listed ? F.px_height : F.height);
                    px = ((double)gx + 0.5) / (double)fw * 2.0 - 1.0;
                    py = -(((double)y + 0.5) / (double)fh * 2.0 - 1.0);
                } else {
                    double x0, x1, y0, y1;  // the pixel's NdcRect {min: (x0, y0), max: (x1, y1)} (renderer.rs:537-550)
                    if (F.patches) {
                        const double *r = F.patches + 4u * pix;
                        x0 = r[0]; y0 = r[1]; x1 = r[2]; y1 = r[3];
                    } else if (F.edge_x) {
                        // fb_x_edge / fb_y_edge of the pixel's two edges each, from the frame's tables (DevFrame::edge_x: made by the same operations)
                        x0 = F.edge_x[gx]; x1 = F.edge_x[gx + 1u]; y0 = F.edge_y[y]; y1 = F.edge_y[y + 1u];
                    } else {
                        const uint32_t fw = opaque_s(F.width), fh = opaque_s(F.height);
                        x0 = fb_x_edge(fw, gx); x1 = fb_x_edge(fw, gx + 1);
                        y0 = fb_y_edge(fh, y); y1 = fb_y_edge(fh, y + 1);
                    }
                    if (n_samples == 4) {
                        const double ux = (sample == 0) ? 1. / 8. : (sample == 1) ? 3. / 8. : (sample == 2) ? 5. / 8. : 7. / 8.;
                        const double uy = (sample == 0) ? 5. / 8. : (sample == 1) ? 1. / 8. : (sample == 2) ? 7. / 8. : 3. / 8.;
                        px = x0 + (x1 - x0) * ux;
                        py = y0 + (y1 - y0) * uy;
                    } else {
                        px = (x0 + x1) / 2.0;
                        py = (y0 + y1) / 2.0;
                    }
                }
                bool have_ray = L.present != 0;
                o[0] = o[1] = o[2] = 0.0;
                if (want_dir) dir[0] = dir[1] = dir[2] = 0.0;
                if (have_ray && F.ortho_n) {
                    // MultiOrthoCamera::project_pixel_into_world (ortho.rs:186-199, 284-294): the view whose rectangle holds
                    // the pixel, its transform applied to the pixel, then TryFrom<Ray> for AaRay / From<AaRay> for Ray
                    // (ray.rs:305-358: the origin becomes cube + f32 offset, the direction the unit axis vector).
                    // trace_axis_aligned_ray produces what trace_ray produces on that Ray (axis_aligned.rs:8-9).
                    int vsel = -1;
                    for (int v = 0; v < F.ortho_n; v++) {
                        const uint32_t vx = F.ortho[v].x0, vy = F.ortho[v].y0, vw = F.ortho[v].w, vh = F.ortho[v].h;
                        if (vsel < 0 && gx >= vx && y >= vy && gx - vx < vw && y - vy < vh) vsel = v;
                    }
                    have_ray = false;
                    if (vsel >= 0) {
                        const DevOrthoView *V = &F.ortho[vsel];
                        double p[3];
                        unproject(V->m, (double)(gx - V->x0), (double)(y - V->y0), 0.0, p);
                        int cube[3];
                        if (cube_containing(p, cube)) {
                            have_ray = true;
                            for (int a = 0; a < 3; a++) {
                                o[a] = (double)cube[a] + (double)(float)(p[a] - (double)cube[a]);
                                if (want_dir) dir[a] = V->dir[a];
                            }
                        }
                    }
                } else if (have_ray) {
                    unproject(S.inv, px, py, 0.0, o);
                    if (want_dir) {
                        double f[3];
                        unproject(S.inv, px, py, 1.0, f);
                        dir[0] = f[0] - o[0]; dir[1] = f[1] - o[1]; dir[2] = f[2] - o[2];
                    }
                }
                return have_ray;
            };
            // The exchanging variants' global part of the cold state: the four antialiasing sums, 16 bytes per column of this workgroup, in frames traced with
            // antialiasing only. Loads are workgroup-scope atomics (`sc0`: past the CU's vector L1, which a store made by another wave of the workgroup does
            // not update -- the sums may last have been written by a lane of another wave -- and served by the L2; agent scope, `sc1`, goes past the XCD's L2
            // as well). A store is waited for at once: the ray may be parked and claimed by another wave in the very next round.
            // Layout: per workgroup four arrays of NCOL floats: a wave's lanes read neighbouring words (columns stay mostly in lane order).
            char *const cold_wg = XCHG ? reinterpret_cast<char *>(F.ray_cold) + (size_t)blockIdx.x * (size_t)(NCOL * 16u) : nullptr;
            auto off32 = [&](uint32_t k) -> uint32_t { return (k * NCOL + col) * 4u; };
            auto cold_origin = [&](double &ox, double &oy, double &oz) {
                if constexpr (XCHG) {
                    const uint32_t pxy_ = c32[K_PXY][col];
                    double o_[3];
                    (void)ray_of_pixel(pxy_ & 0xffffu, pxy_ >> 16, (int)((st >> 14) & 3u), false, o_, nullptr);
                    ox = o_[0]; oy = o_[1]; oz = o_[2];
                } else {
                    ox = c64[XCHG ? 0 : (int)C_OX][col]; oy = c64[XCHG ? 0 : (int)C_OY][col]; oz = c64[XCHG ? 0 : (int)C_OZ][col];
                }
            };
            auto cold_direction = [&](double &dx, double &dy, double &dz) { dx = c64[C_DX][col]; dy = c64[C_DY][col]; dz = c64[C_DZ][col]; };
            auto cold_sums_load = [&](float v[4]) {
                if constexpr (XCHG) {
                    for (uint32_t k = 0; k < 4u; k++) v[k] = __uint_as_float(__hip_atomic_load(reinterpret_cast<uint32_t *>(cold_wg + off32(k)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                } else {
                    v[0] = __uint_as_float(c32[XCHG ? 0 : (int)K_S0][col]); v[1] = __uint_as_float(c32[XCHG ? 0 : (int)K_S1][col]);
                    v[2] = __uint_as_float(c32[XCHG ? 0 : (int)K_S2][col]); v[3] = __uint_as_float(c32[XCHG ? 0 : (int)K_ST][col]);
                }
            };
            auto cold_sums_store = [&](float v0, float v1, float v2, float v3) {
                if constexpr (XCHG) {
                    *reinterpret_cast<float *>(cold_wg + off32(0u)) = v0; *reinterpret_cast<float *>(cold_wg + off32(1u)) = v1;
                    *reinterpret_cast<float *>(cold_wg + off32(2u)) = v2; *reinterpret_cast<float *>(cold_wg + off32(3u)) = v3;
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (in L2 before another wave can be handed the ray)
                } else {
                    c32[XCHG ? 0 : (int)K_S0][col] = __float_as_uint(v0); c32[XCHG ? 0 : (int)K_S1][col] = __float_as_uint(v1);
                    c32[XCHG ? 0 : (int)K_S2][col] = __float_as_uint(v2); c32[XCHG ? 0 : (int)K_ST][col] = __float_as_uint(v3);
                }
            };
            const uint32_t posx = (st >> 26) & 1u, posy = (st >> 25) & 1u, posz = (st >> 24) & 1u;
            // -- shading a discovered surface: compute_illumination + trace_through_span +
            //    Surface::to_light (surface.rs:73-206; sr.rs:697-740). For Volumetric transparency the
            //    span's exit distance is the t of the ray's NEXT TraceStep, which is already fixed when
            //    the surface is discovered: it is the t_max of the step the level takes next. The
            //    contribution is therefore computed here in full and merely *applied* by the stepping code
            //    when that next step is counted (so the order count -> stop-check -> accumulate is kept). --
            // (one kind runs per phase: each kind's section sits behind a UNIFORM branch on `run`, the per-lane test inside it -- written as one combined condition
            //  the copies that carry a section's conditionally updated variables to the merge behind it are made in every phase, whichever kind runs)
            if (run == EV_SHADE) {
            AIC_SECTION(shade_geometry);
            if (ev & EV_SHADE) {
                const bool inb = (st & ST_IN_BLOCK) != 0;
                const uint32_t blk_res = 1u << (blk_geo >> 24), blk_vlo = blk_geo & 0xffffffu;
                const double as = inb ? __hiloint2double((int)((1023u - (blk_geo >> 24)) << 20), 0) : 1.0;  // 1 / resolution
                const double t_enter = last_t * as;  // surface.rs:385-386
                const uint32_t s_rx = c32[K_SRX][col], s_ry = c32[K_SRY][col], s_rz = c32[K_SRZ][col];
                // the Space cube, and the current level's cube in absolute coordinates
                const int ocx = coord(posx, osx_i, inb ? s_rx : rx) + olx, ocy = coord(posy, osy_i, inb ? s_ry : ry) + oly,
                          ocz = coord(posz, osz_i, inb ? s_rz : rz) + olz;
                Lvl ca;
                ca.tx = tx; ca.ty = ty; ca.tz = tz; ca.last_t = last_t; ca.st = face_now() << 2;
                if (inb) {
                    ca.cx = coord(posx, (int)(blk_vsz & 255u), rx) + (int)(blk_vlo & 255u);
                    ca.cy = coord(posy, (int)((blk_vsz >> 8) & 255u), ry) + (int)((blk_vlo >> 8) & 255u);
                    ca.cz = coord(posz, (int)((blk_vsz >> 16) & 255u), rz) + (int)((blk_vlo >> 16) & 255u);
                } else {
                    ca.cx = ocx; ca.cy = ocy; ca.cz = ocz;
                }
                // colour record of the surface: the block's single voxel, or the voxel's palette entry
                const uint32_t shade_ref = inb ? (blk_pal_off + raw) : (0x80000000u | (raw & idx_mask));
                // ... fetched HERE, ahead of the light: both records begin with rgba and emission (DevBlock, DevPaletteEntry: 32 bytes), so it is one address and
                // two loads without a branch, and they are in flight beside the light's texel loads. (Written where the record is used, the compiler issued them
                // there -- behind the wait for the texels: two memory round trips in a row in every SHADE phase; round 6.)
                static_assert(offsetof(DevBlock, color) == 0 && offsetof(DevBlock, emission) == 16 && offsetof(DevPaletteEntry, color) == 0 && offsetof(DevPaletteEntry, emission) == 16, "one record layout");
                const char *const rec_p = (shade_ref & 0x80000000u) ? reinterpret_cast<const char *>(&L.blocks[shade_ref & 0xffffu]) : reinterpret_cast<const char *>(&L.palette[shade_ref]);
                const float4 rec_col = *reinterpret_cast<const float4 *>(rec_p);
                const float4 rec_em = *reinterpret_cast<const float4 *>(rec_p + 16);  // (.w: DevBlock::kind / the palette entry's pad -- unused)
                // illumination (surface.rs:113-206)
                float i0 = 1.0f, i1 = 1.0f, i2 = 1.0f;
                uint32_t nl = 0;
                double ip[3] = {0.0, 0.0, 0.0};  // the surface point in space coordinates (LMODE 2: light interpolation; 3: the bounce rays' origin)
                AIC_SECTION(shade_light);
                if (LMODE != 0) {
                    const int face = lvl_face(ca);
                    if (LMODE == 1 || LMODE == 3) {  // Flat; Bounce falls back to it for surfaces that are not fully opaque (surface.rs:171-176)
                        int nx = 0, ny = 0, nz = 0;
                        if (face == 1) nx = -1; else if (face == 2) ny = -1; else if (face == 3) nz = -1;
                        else if (face == 4) nx = 1; else if (face == 5) ny = 1; else if (face == 6) nz = 1;
                        const uint32_t txl = get_packed_light<DIAG>(L, ocx + nx, ocy + ny, ocz + nz, nl);
                        i0 = lut[txl & 255u]; i1 = lut[(txl >> 8) & 255u]; i2 = lut[(txl >> 16) & 255u];
                    }
                    if (LMODE >= 2) {
                        // (the origin enters intersection_point only for a lane whose step is Face7::Within or whose ray does not move along some axis --
                        //  raycast.rs:409-439 -- : it is fetched for those lanes, i.e. hardly ever; half of the SHADE event's cold-state traffic)
                        double ox = 0.0, oy = 0.0, oz = 0.0, dx, dy, dz;  // (the origin as the lane's LEVEL sees it: the block's own coordinates inside a block)
                        cold_direction(dx, dy, dz);
                        const bool need_o = (face == FACE_WITHIN) | (dx == 0.0) | (dy == 0.0) | (dz == 0.0);
                        if (__ballot(need_o) != 0ull) {
                            if (need_o) {
                                cold_origin(ox, oy, oz);
                                if (inb) {
                                    const double kd = (double)blk_res;
                                    ox = (ox - (double)ocx) * kd; oy = (oy - (double)ocy) * kd; oz = (oz - (double)ocz) * kd;
                                }
                            }
                        }
                        // one copy of intersection_point for both levels (round 6: it was written per level, and a wave shading cube faces and voxel faces
                        // together ran both); a voxel's point goes back to space coordinates (surface.rs:406-407)
                        double vp[3];
                        intersection_point(ca, ox, oy, oz, dx, dy, dz, vp);
                        ip[0] = inb ? vp[0] * as + (double)ocx : vp[0];
                        ip[1] = inb ? vp[1] * as + (double)ocy : vp[1];
                        ip[2] = inb ? vp[2] * as + (double)ocz : vp[2];
                    }
                    if (LMODE == 2) {
                        // get_interpolated_light (sr.rs:248-359; aic_lightmath.h), then rgb / max(weight, 0.1)
                        float fin[4];
                        lm_interpolated_light(light_view(L), lut, ocx, ocy, ocz, ip[0], ip[1], ip[2], face, opt.lighting, fin, DIAG ? &nl : nullptr);
                        const float w = fmaxf(fin[3], 0.1f);
                        if (__ballot(w != 1.0f) == 0ull) {  // x / 1.0f == x: fully lit neighbourhoods (the usual case) need no division
                            i0 = fin[0]; i1 = fin[1]; i2 = fin[2];
                        } else {
                            // Three quotients by the same w in [0.1, 1]: the compiler's own correctly rounded f32 division (v_rcp_f32, one Newton step on the
                            // reciprocal, q = x r, two residual corrections, a last fused one) with the reciprocal and its refinement made ONCE and without the
                            // operand scaling and the special-case fix-up, which do nothing here: w is a normal number near one, x is a light value -- zero, or
                            // between 2^-15 times an interpolation weight and 2^12 --, so v_div_scale_f32 leaves both alone and no operand is infinite or NaN
                            // (18 instructions instead of 33, one quarter-rate reciprocal instead of three; round 6).
                            const float r0 = __builtin_amdgcn_rcpf(w);
                            const float rr = __builtin_fmaf(__builtin_fmaf(-w, r0, 1.0f), r0, r0);
                            auto quot = [&](const float x) -> float {
                                float q = x * rr;
                                q = __builtin_fmaf(__builtin_fmaf(-w, q, x), rr, q);
                                return __builtin_fmaf(__builtin_fmaf(-w, q, x), rr, q);
                            };
                            i0 = quot(fin[0]); i1 = quot(fin[1]); i2 = quot(fin[2]);
                        }
                    }
                }
                AIC_TICK(18);
                AIC_SECTION(shade_colour_span);
                // colour record
                float r = rec_col.x, g = rec_col.y, b = rec_col.z, a = rec_col.w, e0 = rec_em.x, e1 = rec_em.y, e2 = rec_em.z;
                bool will_flush = true;
                if (VOL) {
                    // exit distance = t of the next TraceStep: the next step of this level, or -- if this
                    // level cannot step any more -- of the enclosing cube grid; none => the span is never emitted
                    double t_exit = 0.0;
                    if (!(ev & EV_DEAD)) {
                        const int pk = pick_axis(tx, ty, tz);
                        t_exit = (pk == 0 ? tx : (pk == 1 ? ty : tz)) * as;
                    } else if (inb && (st & ST_OUTER_ALIVE)) {
                        const double s_tx = c64[C_STX][col], s_ty = c64[C_STY][col], s_tz = c64[C_STZ][col];
                        const int pk = pick_axis(s_tx, s_ty, s_tz);  // the suspended outer level's next step
                        t_exit = pk == 0 ? s_tx : (pk == 1 ? s_ty : s_tz);
                    } else {
                        will_flush = false;
                    }
                    // trace_through_span (sr.rs:720-740) + apply_transmittance (raytracer_components.rs:215-258)
                    float thickness = (float)((t_exit - t_enter) * c64[C_TABS][col]);
                    thickness = fmaxf(thickness, 0.0f);
                    float coeff;
                    if (thickness == 0.0f) {
                        if (a == 1.0f) coeff = 1.0f;
                        else { r = g = b = a = 0.f; coeff = 0.0f; }
                    } else {
                        const float unit_t = 1.0f - a;
                        // powf(0, y>0) == 0 and powf(1, y) == 1 exactly: skip the general evaluation
                        float depth_t;
                        if (unit_t == 0.0f) depth_t = 0.0f;
                        else if (unit_t == 1.0f) depth_t = 1.0f;
                        else if (!(thickness < __uint_as_float(0x7f800000u))) depth_t = 0.0f;  // powf(0 < x < 1, +inf) == 0
                        else depth_t = powf_table(unit_t, thickness, s_pow);  // 0 < unit_t < 1 normal (aic_upload_* reject alpha outside [0, 1]), thickness > 0 finite
                        a = zo_clamped(1.0f - depth_t);
                        const float ec = (unit_t == 1.0f) ? thickness : (depth_t - 1.f) / (unit_t - 1.f);
                        coeff = fmaxf(ec, 0.0f);
                    }
                    const float c = ps_clamped(coeff);
                    e0 = ps_mul(e0, c); e1 = ps_mul(e1, c); e2 = ps_mul(e2, c);
                }
                AIC_SECTION(shade_to_light_fog);
                // Surface::to_light (surface.rs:73-106)
                if (opt.transparency == 2) {  // limit_alpha (graphics_options.rs:496-507)
                    if (a > opt.threshold) a = 1.0f;
                    else { r = g = b = a = 0.f; }
                }
                // (Volumetric: only for a span that WILL be emitted -- the reference lights a surface when its span comes out of
                //  DepthIter and passes the stop check, i.e. at the ray's next counted step: sr.rs:183-199)
                if (LMODE == 3 && a == 1.0f && (!VOL || (will_flush && count <= 999u))) {
                    // compute_illumination with the RNG and a fully opaque diffuse colour (surface.rs:85-88, 119-166): `samples` secondary
                    // rays from just above the surface, directions normal + UnitSphere sample; their mean replaces the Flat light
                    const int face = lvl_face(ca);
                    double nvx = 0.0, nvy = 0.0, nvz = 0.0;
                    if (face == 1) nvx = -1.0; else if (face == 2) nvy = -1.0; else if (face == 3) nvz = -1.0;
                    else if (face == 4) nvx = 1.0; else if (face == 5) nvy = 1.0; else if (face == 6) nvz = 1.0;
                    const float *sky_mem = (const float *)((const char *)(const void *)Fq + offsetof(DevFrame, layer) + offsetof(DevLayer, sky));
                    const uint32_t n_samples_b = (uint32_t)opt.bounce_samples & 255u;  // `samples: u8`
                    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
                    for (uint32_t k = 0; k < n_samples_b; k++) {
                        double u[3];
                        bounce_unit_sphere(brng, u);
                        float c3[3];
                        sec_steps += bounce_secondary_ray<DIAG>(L, sky_mem, lut, s_pow, BIG, ip[0] + nvx * 0.0001, ip[1] + nvy * 0.0001, ip[2] + nvz * 0.0001,
                                                                nvx + u[0], nvy + u[1], nvz + u[2], c3);
                        m0 += c3[0]; m1 += c3[1]; m2 += c3[2];
                    }
                    const float kk = ps_clamped(1.0f / (float)n_samples_b);  // Rgb * f32::from(samples).recip() (color.rs:912-925)
                    i0 = ps_mul(m0, kk); i1 = ps_mul(m1, kk); i2 = ps_mul(m2, kk);
                    nl = 0;  // (the Flat texel read above is not a get_packed_light call of the reference's for this surface)
                }
                float o0 = 0.f, o1 = 0.f, o2 = 0.f, tr = 1.0f;
                const bool visible = !(a == 0.f && e0 == 0.f && e1 == 0.f && e2 == 0.f);
                if (visible) {
                    o0 = ps_mul(ps_mul(r, i0), a) + e0;
                    o1 = ps_mul(ps_mul(g, i1), a) + e1;
                    o2 = ps_mul(ps_mul(b, i2), a) + e2;
                    tr = 1.0f - a;
                    if (fog_on) {  // distance_fog (sr.rs:745-768)
                        float sky[3];
                        sky_now(sky);
                        const float fog_blend = opt.fog == 1 ? 1.0f : (opt.fog == 2 ? 0.5f : 0.0f);
                        float rel = (float)t_enter * __uint_as_float(c32[K_TVIEW][col]);
                        rel = rel < 0.0f ? 0.0f : (rel > 1.0f ? 1.0f : rel);
                        const float sq = rel * rel;
                        float amount;
                        if (opt.fog == 1) {
                            // Abrupt: blend == 1, so the exponential term is (finite, >= 0) * 0.0 == +0.0 and
                            // +0.0 + rel^4 * 1.0 == rel^4 exactly -- no exp needed
                            amount = zo_clamped((sq * sq) * 1.0f);
                        } else {
                            const float fog_exp = 1.0f - expf_table(-1.6f * rel, s_pow);
                            const float fudged = fog_exp / 0.79810348f;
                            amount = zo_clamped(fudged * (1.0f - fog_blend) + (sq * sq) * fog_blend);
                        }
                        const float comp = 1.0f - amount;
                        o0 = ps_mul(o0, comp) + ps_mul(sky[0], amount);
                        o1 = ps_mul(o1, comp) + ps_mul(sky[1], amount);
                        o2 = ps_mul(o2, comp) + ps_mul(sky[2], amount);
                        tr *= comp;
                    }
                }
                AIC_SECTION(shade_apply);
                SurfDiag sd;
                if (DIAG) {
                    sd.nlight = nl;
                    sd.cube[0] = ocx; sd.cube[1] = ocy; sd.cube[2] = ocz;
                    if (inb) {
                        sd.voxel[0] = ca.cx; sd.voxel[1] = ca.cy; sd.voxel[2] = ca.cz;
                        sd.res = (int)blk_res; sd.block = (int)c32[XCHG ? 0 : (int)K_BLK][col];
                    } else {
                        sd.voxel[0] = sd.voxel[1] = sd.voxel[2] = 0;
                        sd.res = 1; sd.block = (int)(shade_ref & 0xffffu);
                    }
                    sd.face = lvl_face(ca);
                }
                if (VOL) {
                    // DepthIter.last_surface: applied when the next TraceStep is counted
                    if (will_flush) {
                        // The span is applied when the ray's next TraceStep is counted and passes the stop check (sr.rs:625-656).
                        // For a lane whose level can step and that is below the step cap that is CERTAIN: its next step (a lookup or the
                        // exit step) is produced, counted (count + 1 <= 1000) and not stopped (the ray is not opaque, or it would not be
                        // shading). Nothing reads the accumulator in between, so the same additions can be made now -- unless they make
                        // the ray opaque: the stop check of that next step still has to see it transparent, so then the span waits as
                        // before. A lane without a pending span takes the bookkeeping-free fast steps at once.
                        bool early = !DIAG && !(ev & EV_DEAD) && count <= 999u;
                        const float n0 = acc.l0 + o0 * acc.t, n1 = acc.l1 + o1 * acc.t, n2 = acc.l2 + o2 * acc.t, nt = acc.t * tr;
                        early = early && !(nt < 1.0f / 256.0f);
                        // A span that makes the ray opaque decides the rest of the ray, whatever lies behind it: the ray's next step is
                        // counted and applies the span (the accumulator is opaque from there), the step after that -- if the iterators
                        // still yield one -- is counted and stops the ray (sr.rs:183-189, 625-656). What those two steps find is
                        // irrelevant (a surface would never be lit, an EnterBlock's second item is that stopping step), only whether they
                        // exist: a level that is not over always yields a next step (a cell or its exit step), and a second one unless that
                        // next step is the exit step of the cube grid, or of a block whose enclosing grid level has ended. So the lane
                        // finishes here: two lookups, two full stepping passes and a scheduler round trip less for every ray that ends
                        // on a solid. (Not the aux-recording variant: its per-level lookup counters follow the reference's iterators.)
                        const bool finish_now = !DIAG && !(ev & EV_DEAD) && count <= 998u && (nt < 1.0f / 256.0f);
                        if (finish_now) {
                            const int pk = pick_axis(tx, ty, tz);
                            const uint32_t r_next = pk == 0 ? rx : (pk == 1 ? ry : rz);  // steps left on that axis minus one: 0 = the exit step is next
                            const bool second = (r_next != 0u) || (inb && (st & ST_OUTER_ALIVE));
                            acc.l0 = n0; acc.l1 = n1; acc.l2 = n2; acc.t = nt;
                            count += second ? 2u : 1u;
                            st |= ST_OPAQUE;
                            ev = (ev & EV_SHADE) | EV_FINISH;  // (EV_SHADE is cleared below)
                        } else if (early) {
                            acc.l0 = n0; acc.l1 = n1; acc.l2 = n2; acc.t = nt;
                        } else {
                            pend0 = o0; pend1 = o1; pend2 = o2; pend_tr = tr;
                            st |= ST_HAS_LAST;
                        }
                        if (DIAG) { pend_d = sd; pend_t = t_enter; pend_visible = visible; }
                    }
                } else if (visible) {
                    cb_add(acc, o0, o1, o2, tr);  // trace_through_surface (sr.rs:697-717)
                    if (cb_opaque(acc)) {
                        st |= ST_OPAQUE;
                        // (as above, Surface transparency: the ray's next step is counted and stops it; a level that is not over yields one)
                        if (!DIAG && !(ev & EV_DEAD) && count <= 999u) {
                            count += 1u;
                            ev = (ev & EV_SHADE) | EV_FINISH;
                        }
                    }
                    if (DIAG) {
                        dg.n_hits++;
                        dg.n_light += sd.nlight;
                        sp_smp = fmin(sp_smp, t_enter);
                        split_layer_after_add(F.hit_layer ? SPLIT_UI : SPLIT_WORLD);
                        if (!dg.hit) {
                            dg.hit = 1;
                            dg.layer = F.hit_layer;
                            for (int a2 = 0; a2 < 3; a2++) { dg.cube[a2] = sd.cube[a2]; dg.voxel[a2] = sd.voxel[a2]; }
                            dg.res = sd.res; dg.face = sd.face; dg.block = sd.block; dg.t = t_enter;
                        }
                    }
                }
                ev &= ~EV_SHADE;
            }
            AIC_SECTION(shade_end);
            } else if (run == EV_ENTER) {
            AIC_SECTION(enter);
            // -- entering a recursive block: RaycastStep::recursive_raycast (raycast.rs:458-476),
            //    advanced to its first in-bounds voxel (or to its end) --
            if (ev & EV_ENTER) {
                const uint32_t blk_index = raw & idx_mask;
                if (DIAG) c32[XCHG ? 0 : (int)K_BLK][col] = blk_index;
                const DevBlock *tb = &L.blocks[blk_index];
                const uint32_t blk_res = tb->kind & 255u;
                const uint32_t blk_vlo = tb->vlo_packed;
                blk_geo = ((31u - (uint32_t)__clz((int)blk_res)) << 24) | blk_vlo;
                blk_vsz = tb->vsize_packed;
                blk_pal_off = tb->pal_off;
                double ox, oy, oz, edx, edy, edz;
                cold_origin(ox, oy, oz);
                cold_direction(edx, edy, edz);
                const uint32_t n_invisible = tb->n_invisible;
                const uint32_t vox_off = tb->vox_off;
                const double kd = (double)blk_res;
                const int acx = coord(posx, osx_i, rx) + olx, acy = coord(posy, osy_i, ry) + oly, acz = coord(posz, osz_i, rz) + olz;
                const double sx_ = (ox - (double)acx) * kd, sy_ = (oy - (double)acy) * kd, sz_ = (oz - (double)acz) * kd;
                // suspend the outer level; its Face goes to st[16..18]
                c64[C_STX][col] = tx; c64[C_STY][col] = ty; c64[C_STZ][col] = tz;
                c32[K_SRX][col] = rx; c32[K_SRY][col] = ry; c32[K_SRZ][col] = rz; c32[K_SBOFF][col] = boff;
                st = (st & ~((7u << 16) | ST_OUTER_ALIVE)) | (face_now() << 16) | ((ev & EV_DEAD) ? 0u : ST_OUTER_ALIVE);
                const int ilx = (int)(blk_vlo & 255u), ily = (int)((blk_vlo >> 8) & 255u), ilz = (int)((blk_vlo >> 16) & 255u);
                const int isx = (int)(blk_vsz & 255u), isy = (int)((blk_vsz >> 8) & 255u), isz = (int)((blk_vsz >> 16) & 255u);
                const RayDir rd = make_rd(edx, edy, edz);
                const LvlLim ll = lvl_init(sx_, sy_, sz_, rd, true, ilx, ily, ilz, ilx + isx, ily + isy, ilz + isz, true, 0.5 / c64[C_TABS][col]);  // (0.5 / direction.length(), raycast.rs:669: the quotient NEWRAY's fast-forward used)
                const FirstCube f = lvl_first_masks(ll.s, rd, ilx, ily, ilz, ilx + isx, ily + isy, ilz + isz);
                const int vcx = f.cx - ilx, vcy = f.cy - ily, vcz = f.cz - ilz;
                boff = 2u * (vox_off + (uint32_t)(((uint32_t)vcx * (uint32_t)isy + (uint32_t)vcy) * (uint32_t)isz + (uint32_t)vcz));
                // The first voxel's lookup, taken here where the stepping trip would count it and do nothing else: the level goes on, no span is pending
                // (DepthIter), the ray is not opaque and the step stays under the 1000-step cap (count_step_should_stop, sr.rs:625-656).
                constexpr bool first_lookup = !DIAG && !BIG;
                const bool first_elig = first_lookup && f.got && f.inbounds && !(st & (ST_HAS_LAST | ST_OPAQUE)) && count <= 999u;
                uint32_t first_raw = 0u;  // (a register of its own: `raw` keeps the live range it has without this lookup)
                if constexpr (first_lookup) { AIC_ISSUE_FIRST_LOOKUP(first_elig, first_raw); }
                tx = f.tx; ty = f.ty; tz = f.tz; last_t = f.last_t;
                rx = posx ? (uint32_t)(isx - 1 - vcx) : (uint32_t)vcx;
                ry = posy ? (uint32_t)(isy - 1 - vcy) : (uint32_t)vcy;
                rz = posz ? (uint32_t)(isz - 1 - vcz) : (uint32_t)vcz;
                ssx = posx ? 2 * isy * isz : -2 * isy * isz; ssy = posy ? 2 * isz : -2 * isz; ssz = posz ? 2 : -2;
                thr = n_invisible;
                lax = f.lax;
                st |= ST_IN_BLOCK;
                // a produced first voxel still needs its lookup (FRESH) unless the lookup made here found an invisible one: that is an Invisible TraceStep,
                // counted, and the lane leaves stepping; a level that produced nothing, or ended with it, is DEAD
                bool first_invisible = false;
                if constexpr (first_lookup) {
                    AIC_WAIT_LOOKUP(first_raw);
                    first_invisible = first_elig && first_raw < thr;
                    count += first_invisible ? 1u : 0u;
                }
                ev = ((f.got && !first_invisible) ? EV_FRESH : 0u) | (f.inbounds ? 0u : EV_DEAD);
            }
            AIC_SECTION(enter_end);
            } else {
            AIC_SECTION(finish);
            // -- finishing a ray: TracingState::finish + layer tail + (last sample) encode & store --
            uint32_t pxy = 0;
            int sample = 0;
            bool want = false;
            if (run == EV_FINISH) {
                pxy = c32[K_PXY][col];
                sample = (ev & EV_TAKE) ? 0 : (int)((st >> 14) & 3u);  // (a lane about to take a pixel starts at sample 0 whatever its state word holds: a lane
                                                                         //  that parked its ray keeps the word of the slot's previous content)
            }
            if (run == EV_FINISH && (ev & EV_FINISH)) {
                if (st & ST_TRACED) {
                    // finish (sr.rs:658-693): the sky hit, then the optional cost visualisation
                    if (include_sky) {
                        float sky[3];
                        sky_now(sky);
                        cb_add(acc, sky[0] * 1.0f, sky[1] * 1.0f, sky[2] * 1.0f, 0.0f);
                    } else {
                        cb_add(acc, 0.f, 0.f, 0.f, 1.0f);
                    }
                    if (opt.debug_pixel_cost) {  // accum.rs:228-234
                        const float n = ps_clamped((float)count);
                        const float red = ps_clamped(ps_mul(0.02f, n) * 1.0f);
                        const float green = ps_clamped(ps_mul(0.002f, n) * 1.0f);
                        float cur_rgba[4];
                        cb_to_rgba(acc, cur_rgba);
                        const float blue = ps_clamped(luminance(cur_rgba[0], cur_rgba[1], cur_rgba[2]) * 0.2f);
                        acc.l0 = red; acc.l1 = green; acc.l2 = blue; acc.t = 0.0f;
                    }
                    { uint32_t t_ = threadIdx.x; asm volatile("" : "+v"(t_)); s_steps[t_] += count + (LMODE == 3 ? sec_steps : 0u); }  // (the address made here, not held across the loop)  // RaytraceInfo + secondary_info (sr.rs:690-692)
#ifdef AIC_PROFILE
                    { const uint32_t dur_ = (uint32_t)__builtin_readcyclecounter() - s_ray_t0[col];
                      if (dur_ > ray_dur_max) { ray_dur_max = dur_; ray_dur_steps = count; } }
#endif
                    if (DIAG) {
                        px_steps += count + (LMODE == 3 ? sec_steps : 0u);
                        // the Sky hit (t_distance +inf: no smaller depth) and the DebugOverrideRg hit are made with the options of the layer traced
                        split_layer_after_add(F.hit_layer ? SPLIT_UI : SPLIT_WORLD);
                    }
                }
                const uint32_t x = pxy & 0xffffu, lrow = pxy >> 16;
                float aa_sum[4] = {0.f, 0.f, 0.f, 0.f};
                if (S.tile_cost && count > 48u) {
                    // longest ray of the macro tile so far. Only rays long enough to matter for the frame's
                    // tail are recorded (the rest leave their tile at cost 0: handed out last, in index
                    // order), and the plain read filters out almost every atomic.
                    uint32_t *tc = &S.tile_cost[(lrow >> macro_px_shift) * F.macros_x + (x >> macro_px_shift)];  // tile edge and macro are powers of two
                    if (count > *tc) atomicMax(tc, count);
                }
                const size_t pix = (size_t)lrow * F.width + x;
                if (ui_pass) {
                    S.acc_buf[(size_t)sample * npix + pix] = make_float4(acc.l0, acc.l1, acc.l2, acc.t);
                    if (DIAG) {  // (the sample's layer needs no carrying: after a UI trace it is the UI's iff the ColorBuf is visible)
                        double *const sd_ = F.split_depth[F.n_sub > 1u ? (blockIdx.x & (F.n_sub - 1u)) : 0u];
                        if (sd_) sd_[(size_t)sample * npix + pix] = sp_smp;
                    }
                } else {
                    if (!F.bare_trace && !cb_opaque(acc)) {  // renderer.rs:474-477: P::paint(NO_WORLD_TO_SHOW) replaces the accumulator
                        // (render_orthographic has no such layer tail: ortho.rs:103-131; nor has SpaceRaytracer::trace_ray, aic_trace_rays)
                        acc.l0 = 0.f + (NO_WORLD_TO_SHOW * 1.0f) * 1.0f;
                        acc.l1 = acc.l0;
                        acc.l2 = acc.l0;
                        acc.t = 1.0f * (1.0f - 1.0f);
                        if (DIAG) {  // P::paint: a default Split and one Paint hit, made with the world's options and no t_distance
                            sp_smp = __longlong_as_double(0x7ff0000000000000LL);
                            sp_lay = (sp_lay & ~3u) | SPLIT_WORLD;
                        }
                    }
                    if (DIAG) {  // Split::mean: the smallest depth, the first sample's layer that has one
                        sp_px = fmin(sp_px, sp_smp);
                        if (!(sp_lay & 12u)) sp_lay |= (sp_lay & 3u) << 2;
                    }
                    if (n_samples == 4) {
                        cold_sums_load(aa_sum);
                        aa_sum[0] += acc.l0; aa_sum[1] += acc.l1; aa_sum[2] += acc.l2; aa_sum[3] += acc.t;
                        if (sample < 3) cold_sums_store(aa_sum[0], aa_sum[1], aa_sum[2], aa_sum[3]);  // (the last sample's sums are used below and dropped)
                    }
                }
                sample++;
                if (sample < n_samples) {
                    ev = EV_NEWRAY;  // next antialiasing sample of the same pixel
                } else {
                    if (!ui_pass) {
                        ColorBuf pixel;
                        if (n_samples == 4) {  // ColorBuf::mean (raytracer_components.rs:97-102)
                            pixel.l0 = aa_sum[0] / 4.0f; pixel.l1 = aa_sum[1] / 4.0f; pixel.l2 = aa_sum[2] / 4.0f; pixel.t = aa_sum[3] / 4.0f;
                        } else {
                            pixel = acc;
                        }
                        // encoder: Camera::post_process_color(Rgba::from(buf)).to_srgb8()
                        float c[4];
                        cb_to_rgba(pixel, c);
                        // where the pixel's result goes: its place in the image, or -- a pixel list (the recording variants) -- entry pixels[i] of the target
                        // frame in place, else i, with the Split's depth plane behind the target frame's or the list's colour texels. The entry is loaded again
                        // here, not carried from NEWRAY in a register.
                        size_t opix = pix, depth_plane = npix * 8u;
                        if (DIAG && F.pixels) {
                            if (F.px_in_place) { opix = F.pixels[pix]; depth_plane = (size_t)F.px_width * F.px_height * 8u; }
                            else depth_plane = (size_t)F.n_patches * 8u;
                        }
                        if (DIAG && F.out_mode == 3) {
                            // Split: the two texels raytrace_to_texture stores (raytrace_to_texture.rs:646-674) -- one 8-byte and one 4-byte store
                            const uint32_t sub_ = F.n_sub > 1u ? (blockIdx.x & (F.n_sub - 1u)) : 0u;
                            const uint32_t pl = (sp_lay >> 2) & 3u;
                            const float e = pl == SPLIT_UI ? F.split_ui_exposure[sub_] : (pl == SPLIT_WORLD ? S.exposure : 1.0f);
                            float a = 1.0f - pixel.t;  // into_premultiplied_rgba: (1 - t).clamp(0, 1)
                            a = a < 0.0f ? 0.0f : a;
                            a = a > 1.0f ? 1.0f : a;
                            auto f16_bits = [](float v) -> uint32_t { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v); };  // half::f16::from_f32: to nearest even, overflow to infinity
                            reinterpret_cast<uint2 *>(S.out)[opix] =
                                make_uint2(f16_bits(pixel.l0 * e) | (f16_bits(pixel.l1 * e) << 16), f16_bits(pixel.l2 * e) | (f16_bits(a) << 16));
                            double d = sp_px;  // depth_buf.depth().clamp(0.0, 1.0)
                            d = d < 0.0 ? 0.0 : d;
                            d = d > 1.0 ? 1.0 : d;
                            // depth_transform.transform_point3d_homogeneous(point3(0., 0., d)), euclid's operation order
                            const double z_ = ((0.0 * 0.0 + 0.0 * 0.0) + d * F.depth_zw[0]) + F.depth_zw[1];
                            const double w_ = ((0.0 * 0.0 + 0.0 * 0.0) + d * F.depth_zw[2]) + F.depth_zw[3];
                            const float layer_factor = pl == SPLIT_WORLD ? 1.0f : -1.0f;  // layer.unwrap_or(InLayer::Ui) as i8
                            reinterpret_cast<float *>(reinterpret_cast<char *>(S.out) + depth_plane)[opix] = (float)(z_ / w_) * layer_factor;
                        } else if (F.out_mode != 0) {  // float outputs: the linear Rgba, or the ColorBuf as it is
                            reinterpret_cast<float4 *>(S.out)[opix] =
                                F.out_mode == 1 ? make_float4(c[0], c[1], c[2], c[3]) : make_float4(pixel.l0, pixel.l1, pixel.l2, pixel.t);
                        } else {
                        const float ex = S.exposure;
                        float r = ps_mul(c[0], ex), g = ps_mul(c[1], ex), bl = ps_mul(c[2], ex);
                        const float m = F.maximum_intensity;
                        if (isfinite(m)) {  // ToneMappingOperator::apply (graphics_options.rs:352-368)
                            if (F.tone_mapping == 0) {
                                r = r < 0.f ? 0.f : (r > m ? m : r);
                                g = g < 0.f ? 0.f : (g > m ? m : g);
                                bl = bl < 0.f ? 0.f : (bl > m ? m : bl);
                            } else {
                                const float scale = ps_clamped(1.0f / (1.0f + luminance(r, g, bl) / m));
                                r = ps_mul(r, scale); g = ps_mul(g, scale); bl = ps_mul(bl, scale);
                            }
                        }
                        uint32_t R, G, B;
                        srgb8_rgb_bucket(r, g, bl, F.srgb_buckets, R, G, B);  // (the sRGB8 bucket table stays in global memory: 6.5 KB every workgroup reads)
                        const uint32_t A = round_sat_u8(c[3] * 255.0f);
                        S.out[opix] = R | (G << 8) | (B << 16) | (A << 24);
                        }
                    }
                    if (DIAG) {
                        if (F.aux) {
                            DevAux &a = F.aux[pix];
                            a.hit = dg.hit & 1;
                            for (int k = 0; k < 3; k++) { a.cube[k] = dg.cube[k]; a.voxel[k] = dg.voxel[k]; }
                            a.resolution = dg.res; a.face = dg.face; a.block_index = dg.block;
                            a.cubes_traced = px_steps_prev + px_steps; a.layer = dg.layer; a.t_distance = dg.t;
                        }
                        tot_outer += dg.n_outer; tot_inner += dg.n_inner; tot_hits += dg.n_hits; tot_light += dg.n_light;
                    }
                    sample = 0;
                    ev = EV_NEWRAY | EV_TAKE;
                }
            }
            AIC_SECTION(refill);
            if (run == EV_FINISH) { AIC_TICK(16) }
            // -- starting a ray: lane refill + Camera::project_ndc_into_world + Raycaster::within --
            if (run == EV_FINISH) {
                // wave-level refill (uniform control flow): hand the next unassigned pixels to the
                // lanes that finished a pixel -- ballot + prefix popcount -- pulling a fresh tile
                // from the global counter whenever the current one is used up.
                want = (ev & (EV_NEWRAY | EV_TAKE)) == (EV_NEWRAY | EV_TAKE);
                uint32_t wv_ = 0u;  // (XCHG) the wave's number, made here: derived before the loop, the address of its LDS words would be one more register held across it
                if constexpr (XCHG) {
                    wv_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
                    asm volatile("" : "+s"(wv_));
                    tile_x0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_tile_state[wv_][0]);
                    tile_y0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_tile_state[wv_][1]);
                    next_idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_tile_state[wv_][2]);
                }
                for (;;) {
                    const unsigned long long need = __ballot(want);
                    if (need == 0ull) break;
                    if (next_idx >= tile_px) {
                        // next work item: tiles are numbered macro tile by macro tile (macro x macro tiles
                        // each, row-major inside), and the macro tiles are taken in `tile_order` -- the
                        // previous frame's costliest first -- so that long rays start early while
                        // neighbouring tiles still run together and share their cache lines
                        uint32_t t = n_virtual;
                        if (!dry) {
                            const int leader = __ffsll((long long)need) - 1;
                            if (F.n_queues > 1u) {
                                // the XCD's own queue; when it is empty, the next XCD's (for good: `my_queue` moves on), until all have been seen empty
                                const uint32_t nq = F.n_queues;
                                uint32_t xcc;
                                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                                uint32_t queues_tried = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_queues_tried[threadIdx.x >> 6]);
                                uint32_t my_queue = ((xcc & 15u) + queues_tried) % nq;
                                const uint32_t tried_before = queues_tried;
                                while (queues_tried < nq) {
                                    uint32_t u = 0u;
                                    if ((int)lane == leader) u = atomicAdd(&S.counters->tile_next_q[my_queue][0], 1u);
                                    u = (uint32_t)__builtin_amdgcn_readlane((int)u, leader);
                                    const uint32_t q0 = S.queue_start[my_queue], q1 = S.queue_start[my_queue + 1u];
                                    const uint32_t j = u >> (macro_shift * 2u);
                                    if (j < q1 - q0) {
                                        t = ((q0 + j) << (macro_shift * 2u)) | (u & ((1u << (macro_shift * 2u)) - 1u));
                                        break;
                                    }
                                    my_queue = my_queue + 1u == nq ? 0u : my_queue + 1u;
                                    queues_tried++;
                                }
                                if (queues_tried != tried_before && lane == 0u) s_queues_tried[threadIdx.x >> 6] = queues_tried;
                            } else {
                                if ((int)lane == leader) t = atomicAdd(&S.counters->tile_next, 1u);
                                t = (uint32_t)__builtin_amdgcn_readlane((int)t, leader);  // (a scalar: what depends on it -- `dry` -- stays wave-uniform for the compiler)
                            }
                        }
                        if (t >= n_virtual) {  // image exhausted
#ifdef AIC_PROFILE
                            if (lane == 0u && prof[2] == 0u) prof[2] = (uint32_t)__builtin_readcyclecounter() - prof_t0;  // wave saw the queue run dry
#endif
                            dry = 1u;
                            next_idx = tile_px;
                            if (want) ev = EV_DONE;  // these lanes are done
                            break;
                        }
                        const uint32_t m_shift = macro_shift * 2u;
                        uint32_t mt = t >> m_shift;
                        const uint32_t inner = t & ((1u << m_shift) - 1u);
                        if (S.tile_order) mt = S.tile_order[mt];
                        // (divisors taken through opaque_s: a division by a loop-invariant value is otherwise expanded into a
                        //  reciprocal that is computed before the persistent loop and then lives in -- or is spilled from -- a VGPR)
                        const uint32_t mx_ = opaque_s(F.macros_x);
                        const uint32_t mrow = mt / mx_;
                        const uint32_t tx_ = ((mt - mrow * mx_) << macro_shift) + (inner & ((1u << macro_shift) - 1u));
                        const uint32_t ty_ = (mrow << macro_shift) + (inner >> macro_shift);
                        tile_x0 = tx_ * F.tile;
                        tile_y0 = ty_ * F.tile;
                        if (tile_x0 >= F.width || tile_y0 >= F.local_rows) continue;  // a macro tile's overhang past the image edge
                        next_idx = 0;
                    }
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));  // lanes of `need` below this one (v_mbcnt: no mask of the lanes below to keep in registers)
                    const uint32_t avail = tile_px - next_idx;
                    if (want && rank < avail) {
                        const uint32_t pidx = next_idx + rank;
                        // pixel order inside a tile: four 8x8 quadrants, row-major inside each
                        const uint32_t x = tile_x0 + (pidx & 7u) + (((pidx >> 6) & 1u) << 3);
                        const uint32_t lrow = tile_y0 + ((pidx >> 3) & 7u) + (((pidx >> 7) & 1u) << 3);
                        if (x < F.width && lrow < F.local_rows && (!F.n_patches || lrow * F.width + x < F.n_patches)) {  // pixels of partial tiles outside the image are skipped
                            // (a pixel list's entry outside its target frame -- a device list, which the host cannot check -- is skipped like them: no ray, no store)
                            if (!(DIAG && F.pixels) || F.pixels[lrow * F.width + x] < F.px_width * F.px_height) {
                                pxy = x | (lrow << 16);
                                want = false;
                            }
                        }
                    }
                    const uint32_t n_need = wave_popc(need);
                    next_idx += n_need < avail ? n_need : avail;
                }
                if constexpr (XCHG) {
                    if (lane == 0u) { s_tile_state[wv_][0] = tile_x0; s_tile_state[wv_][1] = tile_y0; s_tile_state[wv_][2] = next_idx; }
                }
            }
            AIC_SECTION(newray);
            if (run == EV_FINISH) { AIC_TICK(17) }
            if (run == EV_FINISH && (ev & EV_NEWRAY) && ev != EV_DONE && !want) {
                const uint32_t x = pxy & 0xffffu, lrow = pxy >> 16;
                const size_t pix = (size_t)lrow * F.width + x;
                if (ev & EV_TAKE) {
                    if (n_samples == 4) { const float z_ = KF(0.f); cold_sums_store(z_, z_, z_, z_); }
                    if (DIAG) {
                        dg.n_outer = dg.n_inner = dg.n_hits = dg.n_light = 0; dg.layer = 0; dg.hit = 0; dg.res = dg.face = dg.block = 0; dg.t = 0.0;
                        for (int a = 0; a < 3; a++) dg.cube[a] = dg.voxel[a] = 0;
                        px_steps = 0; px_steps_prev = 0;
                        if (F.use_init && F.aux) {  // continue the UI pre-pass's per-pixel record
                            const DevAux &a = F.aux[pix];
                            dg.hit = a.hit;
                            for (int k = 0; k < 3; k++) { dg.cube[k] = a.cube[k]; dg.voxel[k] = a.voxel[k]; }
                            dg.res = a.resolution; dg.face = a.face; dg.block = a.block_index; dg.t = a.t_distance;
                            dg.layer = a.layer;
                            px_steps_prev = a.cubes_traced;
                        }
                        sp_px = __longlong_as_double(0x7ff0000000000000LL);
                        sp_lay = 0u;
                    }
                }
                if (DIAG) {
                    sp_smp = __longlong_as_double(0x7ff0000000000000LL);
                    sp_lay &= ~3u;
                }
                if (F.use_init) {
                    const float4 v = S.acc_buf[(size_t)sample * npix + pix];
                    acc.l0 = v.x; acc.l1 = v.y; acc.l2 = v.z; acc.t = v.w;
                    if (DIAG) {  // the sample's Split as the UI trace left it
                        const double *const sd_ = F.split_depth[F.n_sub > 1u ? (blockIdx.x & (F.n_sub - 1u)) : 0u];
                        if (sd_) sp_smp = sd_[(size_t)sample * npix + pix];
                        split_layer_after_add(SPLIT_UI);
                    }
                } else {
                    acc.l0 = acc.l1 = acc.l2 = 0.f;
                    acc.t = KF(1.0f);  // made here: as a literal it is hoisted into a register that lives across the whole loop
                }
                if (DIAG && sample > 0) dg.hit = dg.hit | 2;  // only the first sample's position is reported
                if (!ui_pass && S.has_backdrop) {  // Exception::Backdrop hit: ColorBuf::from(Rgba)
                    const float a = opaque_s(S.backdrop[3]);
                    cb_add(acc, S.backdrop[0] * a, S.backdrop[1] * a, S.backdrop[2] * a, 1.0f - a);
                    if (DIAG) split_layer_after_add(SPLIT_UI);  // (made with the UI's options, renderer.rs:242-250; no t_distance)
                }
                count = 0;
                st = (uint32_t)sample << 14;
                double o[3], dir[3];
                const bool have_ray = ray_of_pixel(x, lrow, sample, true, o, dir);
                if (have_ray) {
                    const double ox = o[0], oy = o[1], oz = o[2];
                    const double dirx = dir[0], diry = dir[1], dirz = dir[2];
                    if (LMODE == 3) {  // SmallRng::seed_from_u64(bits(dx) + bits(dy) + bits(dz)) of the ray as given (sr.rs:165-178)
                        brng = bounce_rng_seed((unsigned long long)__double_as_longlong(dirx) + (unsigned long long)__double_as_longlong(diry) +
                                               (unsigned long long)__double_as_longlong(dirz));
                        sec_steps = 0;
                    }
                    const double t_abs = sqrt(dirx * dirx + diry * diry + dirz * dirz);  // sr.rs:146
                    c64[C_TABS][col] = t_abs;
                    c32[K_TVIEW][col] = __float_as_uint((float)(t_abs / opt.view_distance));  // sr.rs:149-151
                    const RayDir rd = raydir_init(dirx, diry, dirz);
                    c64[C_DX][col] = rd.dx; c64[C_DY][col] = rd.dy; c64[C_DZ][col] = rd.dz;
                    if constexpr (!XCHG) { c64[XCHG ? 0 : (int)C_OX][col] = ox; c64[XCHG ? 0 : (int)C_OY][col] = oy; c64[XCHG ? 0 : (int)C_OZ][col] = oz; }
                    tdx = rd.tdx; tdy = rd.tdy; tdz = rd.tdz;
                    const uint32_t qx = dirx >= 0.0 ? 1u : 0u, qy = diry >= 0.0 ? 1u : 0u, qz = dirz >= 0.0 ? 1u : 0u;
                    const uint32_t octant = (qx << 2) + (qy << 1) + qz;
                    const int ohx = olx + osx_i, ohy = oly + osy_i, ohz = olz + osz_i;
                    // the sanitised direction equals the original unless it was zeroed, in which case no fast-forward happens
                    const double half_over_len = 0.5 / t_abs;
                    const LvlLim ll = lvl_init(ox, oy, oz, rd, true, olx, oly, olz, ohx, ohy, ohz, true, half_over_len);
                    const FirstCube fs = lvl_first_masks(ll.s, rd, olx, oly, olz, ohx, ohy, ohz);
                    const int ccx = fs.cx - olx, ccy = fs.cy - oly, ccz = fs.cz - olz;
                    boff = 2u * (uint32_t)(((uint32_t)ccx * (uint32_t)osy_i + (uint32_t)ccy) * (uint32_t)osz_i + (uint32_t)ccz);
                    // the first cube's lookup, as in ENTER: a new ray has no span pending and its count is zero; one that starts opaque (the backdrop, the UI
                    // pass's pixel) stays FRESH and ends in the stepping trip with its one step
                    constexpr bool first_lookup = !DIAG && !BIG;
                    const bool first_elig = first_lookup && fs.got && fs.inbounds && !cb_opaque(acc);
                    uint32_t first_raw = 0u;  // (a register of its own: `raw` keeps the live range it has without this lookup)
                    if constexpr (first_lookup) { AIC_ISSUE_FIRST_LOOKUP(first_elig, first_raw); }
                    tx = fs.tx; ty = fs.ty; tz = fs.tz; last_t = fs.last_t;
                    rx = qx ? (uint32_t)(osx_i - 1 - ccx) : (uint32_t)ccx;
                    ry = qy ? (uint32_t)(osy_i - 1 - ccy) : (uint32_t)ccy;
                    rz = qz ? (uint32_t)(osz_i - 1 - ccz) : (uint32_t)ccz;
                    ssx = qx ? ostx : -ostx; ssy = qy ? osty : -osty; ssz = qz ? 2 : -2;
                    thr = outer_thr;
                    lax = fs.lax;
                    st = ST_TRACED | (octant << 24) | ((uint32_t)sample << 14) | (rd.fast ? ST_DIR_FAST : 0u);
#ifdef AIC_PROFILE
                    s_ray_t0[col] = (uint32_t)__builtin_readcyclecounter();
#endif
                    if (cb_opaque(acc)) st |= ST_OPAQUE;
                    bool first_invisible = false;
                    if constexpr (first_lookup) {
                        AIC_WAIT_LOOKUP(first_raw);
                        first_invisible = first_elig && first_raw < thr;
                        count += first_invisible ? 1u : 0u;
                    }
                    ev = ((fs.got && !first_invisible) ? EV_FRESH : 0u) | (fs.inbounds ? 0u : EV_DEAD);
                } else {
                    ev = EV_FINISH;
                }
            }
            if (run == EV_FINISH && !want) c32[K_PXY][col] = pxy;
            AIC_SECTION(newray_end);
            }
            if (run == EV_SHADE) { AIC_TICK(13) } else if (run == EV_ENTER) { AIC_TICK(14) } else { AIC_TICK(15) }
            continue;
        }

        AIC_SECTION(stepping);
        // ============================ stepping phase ======================================
        // One Amanatides-Woo step of the lane's current level -- the cube grid or a block's voxel
        // volume: same registers, same code, one 2-byte lookup in the shared pool
        // (SurfaceIter::next + Raycaster::next + State::step).
        //
        // The chip issues about one instruction per 4 cycles per SIMD, vector or scalar (tools/ubench/issue_rate; 2.2 for the simplest),
        // so the trip is written for instruction count: every decision is a 64-bit wave mask in SGPRs (a lane flag
        // costs nothing to test), per-lane state is updated IN PLACE by short exec-masked runs in inline assembly
        // (left to the compiler, the divergent branches of this loop become chains of Flow blocks with ~150 register
        // copies per trip), and the rare paths -- leaving a block, applying a pending span -- sit behind uniform
        // branches.
        {
        typedef unsigned long long mask_t;
        mask_t m_act = m_st;                                                           // lanes stepping
        mask_t m_fresh = __builtin_amdgcn_ballot_w64((ev & EV_FRESH) != 0u);           // (only ever set on stepping lanes)
        mask_t m_dead = __builtin_amdgcn_ballot_w64((ev & EV_DEAD) != 0u) & m_act;
        mask_t m_inb = __builtin_amdgcn_ballot_w64((st & ST_IN_BLOCK) != 0u);
        mask_t m_opq = __builtin_amdgcn_ballot_w64((st & ST_OPAQUE) != 0u);
        mask_t m_hl = VOL ? __builtin_amdgcn_ballot_w64((st & ST_HAS_LAST) != 0u) : 0ull;
        // a trip adds at most AIC_STEP_REPS * (2 * AIC_FAST_STEPS + 2) to a lane's step count (a fast step may bring a bonus step with it): lanes this
        // far below the 1000-step cap (count_step_should_stop, sr.rs:639-651) cannot reach it during the trip
        static_assert(AIC_STEP_REPS * (2 * AIC_FAST_STEPS + 2) < 1000, "the fast steps of a trip stay below the step cap");
        const mask_t m_far_from_cap = __builtin_amdgcn_ballot_w64(count < 1000u - (uint32_t)(AIC_STEP_REPS * (2 * AIC_FAST_STEPS + 2)));
        // what the trip decides for each lane is collected in masks and written to the event words once, after the loop
        mask_t t_shade = 0ull, t_enter = 0ull, t_fin = 0ull, t_deadpark = 0ull;
        // Fast steps need AIC_FAST_MIN takers while the frame is in full swing (other waves want the issue slots); once this wave has
        // seen the pixel queue dry it is draining its last rays and what counts is how soon the longest of them ends: a lone ray
        // then takes its fast steps too (38 instructions a step instead of a full pass's ~180).
        const uint32_t fast_min = (uint32_t)AIC_FAST_MIN - (uint32_t)__builtin_amdgcn_readfirstlane((int)dry) * (uint32_t)(AIC_FAST_MIN - 1);  // (`dry` is wave-uniform; the compiler cannot tell)
        AIC_PROF(22, 1);
        AIC_PROF(23, __popcll(m_act));
#ifdef AIC_TAIL_PROF
        if (__builtin_amdgcn_readfirstlane((int)dry)) { tail_trips++; tail_lanes += (uint32_t)__popcll(m_act); AIC_PROF(29, 1); }
#endif
#define AIC_LANE(m) __builtin_amdgcn_inverse_ballot_w64(m)
#pragma unroll 1
        for (int rep = 0; rep < AIC_STEP_REPS && m_act != 0ull; rep++) {
            AIC_PROF(10, 1);
            AIC_PROF(11, __popcll(m_act));
            mask_t m_step = m_act & ~(m_fresh | m_dead);  // the level takes its next step
            // (the step itself: dda_step, defined above the persistent loop -- the SHADE event's fused step uses it too)
            // -- Steps that cannot mean anything, taken ahead of the bookkeeping below. Four steps in five find an invisible cube
            //    or voxel inside the bounds while the ray has no span pending (DepthIter), is not opaque yet and is far from the
            //    1000-step cap: such a TraceStep is counted and has no other effect (sr.rs:625-656, surface.rs:453-491). A lane
            //    in that state takes up to AIC_FAST_STEPS of them here -- step, look up, count: a third of the instructions of a
            //    full pass -- and goes on into the full pass below with a further step; a lane whose fast step found something
            //    or left the bounds has taken its step of this pass and joins the bookkeeping with that lookup. --
#ifndef AIC_TAIL_PROF
            AIC_PROF(24, __popcll(m_step & m_hl));
            AIC_PROF(25, __popcll(m_step & ~(m_hl | m_opq) & m_far_from_cap));
#endif
            mask_t m_pre_exit = 0ull, m_pre_look = 0ull;  // lanes whose step of this pass was taken here: left the bounds / looked something up
            if (!BIG) {
                mask_t m_f = m_step & ~(m_hl | m_opq) & m_far_from_cap;
#pragma unroll
                for (int f = 0; f < AIC_FAST_STEPS; f++) {
                    // a fast step costs the same however few lanes take it: too few, and their steps are cheaper taken by
                    // the full passes that run anyway
                    if (wave_popc(m_f) < fast_min) break;
                    mask_t m_fx, m_fe, m_fb;
                    if (DIAG) {
                        m_fx = dda_step(m_f);
                        const mask_t m_fl = m_f & ~m_fx;
                        mask_t sv;
                        asm volatile(
                            "s_mov_b64 %[sv], exec\n\t"
                            "s_mov_b64 exec, %[m]\n\t"
                            "global_load_ushort %[raw], %[bo], %[pool]\n\t"
                            "s_mov_b64 exec, %[sv]\n\t"
                            : [raw] "+v"(raw), [sv] "=&s"(sv)
                            : [bo] "v"(boff), [pool] "s"(pool_bits), [m] "s"(m_fl)
                            : "memory");
                        dg.n_inner += AIC_LANE(m_fl & m_inb) ? 1u : 0u; dg.n_outer += AIC_LANE(m_fl & ~m_inb) ? 1u : 0u;
                        AIC_WAIT_RAW();
                        // a code >= thr is a visible voxel, or a cube whose block is visible or recursive (class bits): the full pass decides
                        m_fe = __builtin_amdgcn_ballot_w64(raw >= thr) & m_fl;
                        m_fb = m_fl & ~m_fe;  // an Invisible TraceStep: counted, nothing else
                        asm volatile("v_addc_co_u32 %0, vcc, 0, %0, %1" : "+v"(count) : "s"(m_fb) : "vcc");
                    } else {
                        // The whole fast step as one block: the DDA step of dda_step above, then -- exec narrowing as it goes instead of
                        // being restored and set again -- the lookup under the lanes still inside their bounds, the comparison with the
                        // level's threshold under the same mask, and the count under the lanes that found nothing. (Left to the compiler,
                        // the pieces come with hazard nops between them, a vector compare for the loop's 64-bit population count,
                        // and six more mask operations.)
                        // Then the BONUS step. A cube-grid entry that came back OPEN (aic_device.h) says that all six face neighbours are in bounds and
                        // invisible: whichever way the lane steps next it produces an Invisible TraceStep, so it takes that step here -- the same DDA
                        // arithmetic, addition by addition, and the count -- with no bounds test (the steps-left counters still decrement), no lookup
                        // and no wait. Taken when at least AIC_BONUS_MIN lanes can (the block is issued for the whole wave). The lane goes on as after
                        // any fast step: last_t and lax are the bonus step's, and `raw` is not read again before the lane's next lookup.
                        mask_t sv, mx, by, bx;
#if AIC_BONUS_MIN > 1
                        uint32_t bn;
#define AIC_BONUS_GATE "s_bcnt1_i32_b64 %[bn], %[bx]\n\t" "s_cmp_lt_u32 %[bn], %[bmin]\n\t" "s_cbranch_scc1 1f\n\t"
#define AIC_BONUS_GATE_OUT , [bn] "=&s"(bn)
#else
#define AIC_BONUS_GATE "s_cbranch_scc0 1f\n\t"  // (SCC of the s_andn2: some lane is left)
#define AIC_BONUS_GATE_OUT
#endif
                        asm volatile(
                            "s_and_saveexec_b64 %[sv], %[m]\n\t"
                            "v_min_f64 %[lt], %[tx], %[ty]\n\t"
                            "v_min_f64 %[lt], %[lt], %[tz]\n\t"
                            "v_cmp_eq_f64 %[mx], %[tz], %[lt]\n\t"        // Z
                            "v_cmp_eq_f64 vcc, %[ty], %[lt]\n\t"
                            "s_andn2_b64 vcc, vcc, %[mx]\n\t"             // Y
                            "s_mov_b64 exec, %[mx]\n\t"
                            "v_add_f64 %[tz], %[tz], %[tdz]\n\t"
                            "v_sub_co_u32 %[rz], %[fx], %[rz], 1\n\t"
                            "v_add_u32 %[bo], %[bo], %[ssz]\n\t"
                            "v_mov_b32 %[lax], 2\n\t"
                            "s_or_b64 %[mx], %[mx], vcc\n\t"
                            "s_mov_b64 exec, vcc\n\t"
                            "v_add_f64 %[ty], %[ty], %[tdy]\n\t"
                            "v_sub_co_u32 %[ry], %[by], %[ry], 1\n\t"
                            "v_add_u32 %[bo], %[bo], %[ssy]\n\t"
                            "v_mov_b32 %[lax], 1\n\t"
                            "s_andn2_b64 exec, %[m], %[mx]\n\t"           // X = stepping lanes that took neither
                            "v_add_f64 %[tx], %[tx], %[tdx]\n\t"
                            "v_sub_co_u32 %[rx], %[bx], %[rx], 1\n\t"
                            "v_add_u32 %[bo], %[bo], %[ssx]\n\t"
                            "v_mov_b32 %[lax], 0\n\t"
                            "s_or_b64 %[fx], %[fx], %[by]\n\t"
                            "s_or_b64 %[fx], %[fx], %[bx]\n\t"            // left the bounds
                            "s_andn2_b64 exec, %[m], %[fx]\n\t"           // still inside: look up
                            "global_load_ushort %[raw], %[bo], %[pool]\n\t"
                            "s_waitcnt vmcnt(0)\n\t"
                            "v_cmp_ge_u32 vcc, %[raw], %[thr]\n\t"        // found something (a visible voxel, a visible or recursive block)
                            "s_mov_b64 %[fe], vcc\n\t"
                            "s_andn2_b64 exec, exec, vcc\n\t"             // an Invisible TraceStep: counted, nothing else
                            "s_mov_b64 %[fb], exec\n\t"
                            "v_add_u32 %[cnt], 1, %[cnt]\n\t"
                            "v_cmp_gt_u32 vcc, %[inv], %[raw]\n\t"        // tag OPEN ...
                            "s_andn2_b64 %[bx], vcc, %[inb]\n\t"          // ... of a cube, not a voxel code: the bonus lanes
                            AIC_BONUS_GATE
                            "s_mov_b64 exec, %[bx]\n\t"
                            "v_min_f64 %[lt], %[tx], %[ty]\n\t"
                            "v_min_f64 %[lt], %[lt], %[tz]\n\t"
                            "v_cmp_eq_f64 %[mx], %[tz], %[lt]\n\t"        // Z
                            "v_cmp_eq_f64 vcc, %[ty], %[lt]\n\t"
                            "s_andn2_b64 vcc, vcc, %[mx]\n\t"             // Y
                            "s_mov_b64 exec, %[mx]\n\t"
                            "v_add_f64 %[tz], %[tz], %[tdz]\n\t"
                            "v_add_u32 %[rz], -1, %[rz]\n\t"
                            "v_add_u32 %[bo], %[bo], %[ssz]\n\t"
                            "v_mov_b32 %[lax], 2\n\t"
                            "s_or_b64 %[mx], %[mx], vcc\n\t"
                            "s_mov_b64 exec, vcc\n\t"
                            "v_add_f64 %[ty], %[ty], %[tdy]\n\t"
                            "v_add_u32 %[ry], -1, %[ry]\n\t"
                            "v_add_u32 %[bo], %[bo], %[ssy]\n\t"
                            "v_mov_b32 %[lax], 1\n\t"
                            "s_andn2_b64 exec, %[bx], %[mx]\n\t"          // X
                            "v_add_f64 %[tx], %[tx], %[tdx]\n\t"
                            "v_add_u32 %[rx], -1, %[rx]\n\t"
                            "v_add_u32 %[bo], %[bo], %[ssx]\n\t"
                            "v_mov_b32 %[lax], 0\n\t"
                            "s_mov_b64 exec, %[bx]\n\t"
                            "v_add_u32 %[cnt], 1, %[cnt]\n\t"
                            "1:\n\t"
                            "s_mov_b64 exec, %[sv]\n\t"
                            : [tx] "+v"(tx), [ty] "+v"(ty), [tz] "+v"(tz), [lt] "+v"(last_t), [rx] "+v"(rx), [ry] "+v"(ry), [rz] "+v"(rz),
                              [bo] "+v"(boff), [lax] "+v"(lax), [raw] "+v"(raw), [cnt] "+v"(count), [sv] "=&s"(sv), [mx] "=&s"(mx),
                              [fx] "=&s"(m_fx), [by] "=&s"(by), [bx] "=&s"(bx), [fe] "=&s"(m_fe), [fb] "=&s"(m_fb) AIC_BONUS_GATE_OUT
                            : [tdx] "v"(tdx), [tdy] "v"(tdy), [tdz] "v"(tdz), [ssx] "v"(ssx), [ssy] "v"(ssy), [ssz] "v"(ssz), [m] "s"(m_f),
                              [pool] "s"(pool_bits), [thr] "v"(thr), [inb] "s"(m_inb), [inv] "n"(kCubeTagInvisible << kCubeClassShift), [bmin] "n"(AIC_BONUS_MIN)
                            : "memory", "vcc", "scc");
#undef AIC_BONUS_GATE
#undef AIC_BONUS_GATE_OUT
                    }
                    AIC_PROF(20, 1);
                    AIC_PROF(21, __popcll(m_f));
                    m_pre_exit |= m_fx;
                    m_pre_look |= m_fe;
                    m_f = m_fb;
                }
                m_step &= ~(m_pre_exit | m_pre_look);
            }
            // -- left the bounds? (raycast.rs:265-274) only the axis just stepped can have run out of steps --
            const mask_t m_exit = dda_step(m_step) | m_pre_exit;
            // -- can the level step again? valid_for_stepping (raycast.rs:563-570): "the smallest t_max is finite" held when
            //    the level was set up (lvl_first marks a level that cannot step as dead), and a step only adds the finite
            //    t_delta of an axis whose t_max was finite, so it holds for every level this loop sees: no per-step check --
            // a cube is produced by a fresh level, or by a step that stays in bounds
            const mask_t m_load = m_fresh | (m_step & ~m_exit);  // lookups still to be made; the fast steps' hold theirs in `raw` already
            const mask_t m_lookup = m_load | m_pre_look;
            // the level is over: it left its bounds, cannot step again, or had ended before
            const mask_t m_over = m_exit | m_dead;
            // -- the lookup: one u16 from the pool, for whichever level this is (scalar base + 32-bit byte offset) --
            {
                mask_t sv;
                asm volatile(
                    "s_mov_b64 %[sv], exec\n\t"
                    "s_mov_b64 exec, %[m]\n\t"
                    "global_load_ushort %[raw], %[bo], %[pool]\n\t"
                    "s_mov_b64 exec, %[sv]\n\t"
                    : [raw] "+v"(raw), [sv] "=&s"(sv)
                    : [bo] "v"(boff), [pool] "s"(pool_bits), [m] "s"(m_load)
                    : "memory");
            }
            if (DIAG) { dg.n_inner += AIC_LANE(m_load & m_inb) ? 1u : 0u; dg.n_outer += AIC_LANE(m_load & ~m_inb) ? 1u : 0u; }
            const mask_t m_produced = m_lookup | m_exit;  // the include_exit step is an Invisible TraceStep
            // ---- TracingState::count_step_should_stop (sr.rs:625-656) ----
            asm volatile("v_addc_co_u32 %0, vcc, 0, %0, %1" : "+v"(count) : "s"(m_produced) : "vcc");
            const mask_t m_stop = m_produced & (__builtin_amdgcn_ballot_w64(count > 1000u) | m_opq);
            const mask_t m_go = m_produced & ~m_stop;
            AIC_WAIT_RAW();
            // TraceStep of a looked-up code: voxel -- visible iff its (re-ordered) palette code is past the invisible
            // ones; cube -- the class of its block rides in the top two bits of the grid entry (aic_device.h)
            mask_t m_blk, m_surf;
            if (BIG) {
                // block tables past 16384 entries: plain 16-bit indices, classes from the table in global memory
                uint32_t cls = 0u;
                if (AIC_LANE(m_lookup & ~m_inb)) cls = (F.layer.cls[raw >> 4] >> ((raw & 15u) << 1)) & 3u;
                m_blk = __builtin_amdgcn_ballot_w64(cls == 2u);
                m_surf = (__builtin_amdgcn_ballot_w64(raw >= thr) & m_lookup & m_inb) | __builtin_amdgcn_ballot_w64(cls == 1u);
            } else {
                m_blk = __builtin_amdgcn_ballot_w64(raw >= (kCubeTagRecursive << kCubeClassShift)) & m_lookup & ~m_inb;
                m_surf = __builtin_amdgcn_ballot_w64(raw >= thr) & m_lookup & ~m_blk;
            }
            const mask_t m_some = m_blk | m_surf;
#ifndef AIC_TAIL_PROF
            AIC_PROF(30, __popcll(m_some | m_exit | m_dead));  // lanes of this pass that needed its bookkeeping
#endif
            // -- the level is finished: resume the cube grid, or the ray is complete --
            // (degenerate rays only) a surface / block produced by a level that is over still needs this level's
            // state for its event: the level stays, marked dead, and is left on a later trip
            const mask_t m_defer = m_over & m_some;
            const mask_t m_leave = m_over & ~m_some & m_inb;
            const mask_t m_rayover = m_over & ~m_some & ~m_inb;
            mask_t m_newdead = 0ull;
            if (m_leave != 0ull) {
#ifndef AIC_TAIL_PROF
                AIC_PROF(26, 1);
                AIC_PROF(27, __popcll(m_leave));
#endif
                // Everything under exec = the leaving lanes, in one block: the suspended level comes back from its LDS columns; the
                // cube grid's strides are +-stride by the octant bits of st (bit set = the ray goes up that axis:
                // m - (stride ^ m) with m = the bit sign-extended is +stride for m = -1, -stride for m = 0); the outer level's Face
                // from st[16..18]; it goes on stepping if it was alive when the block was entered.
                mask_t sv;
                uint32_t t_;
                // LDS byte addresses of the lane's columns (the low half of a generic LDS pointer is the LDS offset)
                const uint32_t lds64 = (uint32_t)(uintptr_t)&c64[0][col], lds32 = (uint32_t)(uintptr_t)&c32[0][col];
                asm volatile(
                    "s_mov_b64 %[sv], exec\n\t"
                    "s_mov_b64 exec, %[m]\n\t"
                    "ds_read_b64 %[tx], %[a64] offset:%[o0]\n\t"
                    "ds_read_b64 %[ty], %[a64] offset:%[o1]\n\t"
                    "ds_read_b64 %[tz], %[a64] offset:%[o2]\n\t"
                    "ds_read_b32 %[rx], %[a32] offset:%[p0]\n\t"
                    "ds_read_b32 %[ry], %[a32] offset:%[p1]\n\t"
                    "ds_read_b32 %[rz], %[a32] offset:%[p2]\n\t"
                    "ds_read_b32 %[bo], %[a32] offset:%[p3]\n\t"
                    "v_bfe_i32 %[t], %[st], 26, 1\n\t"
                    "v_xor_b32 %[ssx], %[osx], %[t]\n\t"
                    "v_sub_u32 %[ssx], %[t], %[ssx]\n\t"
                    "v_bfe_i32 %[t], %[st], 25, 1\n\t"
                    "v_xor_b32 %[ssy], %[osy], %[t]\n\t"
                    "v_sub_u32 %[ssy], %[t], %[ssy]\n\t"
                    "v_bfe_i32 %[t], %[st], 24, 1\n\t"
                    "v_xor_b32 %[ssz], 2, %[t]\n\t"
                    "v_sub_u32 %[ssz], %[t], %[ssz]\n\t"
                    "v_mov_b32 %[thr], %[othr]\n\t"
                    "v_bfe_u32 %[t], %[st], 16, 3\n\t"
                    "v_or_b32 %[lax], 8, %[t]\n\t"
                    "v_and_b32 %[t], %[alive], %[st]\n\t"
                    "v_cmp_eq_u32 %[nd], 0, %[t]\n\t"               // the outer level had ended already (inactive lanes: 0)
                    "v_and_b32 %[st], %[notinb], %[st]\n\t"
                    "s_waitcnt lgkmcnt(0)\n\t"
                    "s_mov_b64 exec, %[sv]\n\t"
                    : [tx] "+v"(tx), [ty] "+v"(ty), [tz] "+v"(tz), [rx] "+v"(rx), [ry] "+v"(ry), [rz] "+v"(rz),
                      [bo] "+v"(boff), [ssx] "+v"(ssx), [ssy] "+v"(ssy), [ssz] "+v"(ssz), [thr] "+v"(thr), [lax] "+v"(lax), [st] "+v"(st),
                      [t] "=&v"(t_), [sv] "=&s"(sv), [nd] "=&s"(m_newdead)
                    : [a64] "v"(lds64), [a32] "v"(lds32), [m] "s"(m_leave), [osx] "s"(ostx), [osy] "s"(osty), [othr] "n"(BIG ? 0x10000u : (kCubeTagVisible << kCubeClassShift)),
                      [alive] "n"(ST_OUTER_ALIVE), [notinb] "n"(~ST_IN_BLOCK),
                      [o0] "n"(C_STX * NCOL * 8), [o1] "n"(C_STY * NCOL * 8), [o2] "n"(C_STZ * NCOL * 8),
                      [p0] "n"(K_SRX * NCOL * 4), [p1] "n"(K_SRY * NCOL * 4),
                      [p2] "n"(K_SRZ * NCOL * 4), [p3] "n"(K_SBOFF * NCOL * 4)
                    : "memory");
                m_inb &= ~m_leave;
            }
            // ---- DepthIter::next (surface.rs:453-491): a pending surface's span ends at this step;
            // its contribution was computed when it was shaded, apply it now ----
            if (VOL) {
                const mask_t m_apply = m_go & m_hl;
                if (m_apply != 0ull) {
#ifndef AIC_TAIL_PROF
                    AIC_PROF(28, 1);
                    AIC_PROF(29, __popcll(m_apply));
#endif
                    const bool apply = AIC_LANE(m_apply);
                    acc.l0 = apply ? acc.l0 + pend0 * acc.t : acc.l0;
                    acc.l1 = apply ? acc.l1 + pend1 * acc.t : acc.l1;
                    acc.l2 = apply ? acc.l2 + pend2 * acc.t : acc.l2;
                    acc.t = apply ? acc.t * pend_tr : acc.t;
                    const mask_t m_now_opq = __builtin_amdgcn_ballot_w64(acc.t < 1.0f / 256.0f) & m_apply;  // cb_opaque
                    st = apply ? ((st & ~ST_HAS_LAST) | (AIC_LANE(m_now_opq) ? ST_OPAQUE : 0u)) : st;
                    m_hl &= ~m_apply;
                    m_opq |= m_now_opq;
                    if (DIAG && apply && pend_visible) {
                        dg.n_hits++;
                        dg.n_light += pend_d.nlight;
                        sp_smp = fmin(sp_smp, pend_t);
                        split_layer_after_add(hit_layer_s ? SPLIT_UI : SPLIT_WORLD);
                        if (!dg.hit) {
                            dg.hit = 1;
                            dg.layer = hit_layer_s;
                            for (int a2 = 0; a2 < 3; a2++) { dg.cube[a2] = pend_d.cube[a2]; dg.voxel[a2] = pend_d.voxel[a2]; }
                            dg.res = pend_d.res; dg.face = pend_d.face; dg.block = pend_d.block; dg.t = pend_t;
                        }
                    }
                }
            }
            // DepthIter emits a second, buffered item for EnterBlock (surface.rs:478-488): count it too
            mask_t m_stop2 = 0ull;
            if (VOL) {
                const mask_t m_second = m_go & m_blk;
                asm volatile("v_addc_co_u32 %0, vcc, 0, %0, %1" : "+v"(count) : "s"(m_second) : "vcc");
                m_stop2 = m_second & (__builtin_amdgcn_ballot_w64(count > 1000u) | m_opq);
            }
            // A surface discovered by the very step whose pending span made the ray opaque is never lit: DepthIter has emitted the
            // span and keeps the new surface as last_surface, but the ray's next step fails count_step_should_stop and that
            // surface's span is never produced (surface.rs:453-491, sr.rs:183-189). Until round 4 such a lane was sent to SHADE all
            // the same -- exact, its result was never applied, and wasted: every ray that ends on a solid with something behind it
            // paid one whole SHADE event for nothing (and, with Bounce lighting, traced secondary rays the reference never traces).
            const mask_t m_shade = m_go & m_surf & ~m_opq;
            const mask_t m_enter = m_go & m_blk & ~m_stop2;
            const mask_t m_fin = m_stop | m_stop2 | m_rayover;
            // a lane that parks leaves the trip with its event; one whose level ended while it still owes an event keeps DEAD
            t_shade |= m_shade;
            t_enter |= m_enter;
            t_fin |= m_fin;
            t_deadpark |= (m_defer & ~m_fin) | (m_newdead & m_fin);
            m_act &= ~(m_shade | m_enter | m_fin);
            m_dead = m_newdead & m_act;
            m_fresh = 0ull;
        }
        // new event words: the lanes that took part drop FRESH / DEAD, then take what the trip decided; a lane still
        // stepping whose level ended on the last step carries DEAD into the next trip
        ev = AIC_LANE(m_st) ? 0u : ev;
        ev = AIC_LANE(t_shade) ? EV_SHADE : ev;
        ev = AIC_LANE(t_enter) ? EV_ENTER : ev;
        ev = AIC_LANE(t_fin) ? EV_FINISH : ev;
        if ((t_deadpark | m_dead) != 0ull) ev = AIC_LANE(t_deadpark | m_dead) ? (ev | EV_DEAD) : ev;
#undef AIC_LANE
        }
        AIC_TICK(12);
    }

    AIC_SECTION(epilogue);
    // the frame this workgroup belongs to (as in the event phase: through the opaque kernel-argument pointer)
    typedef const __attribute__((address_space(4))) DevFrame KFrameE;
    typedef const __attribute__((address_space(4))) DevSub KSubE;
    KFrameE *Fe = (KFrameE *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(Fe));
    const uint32_t n_sub_e = Fe->n_sub > 1u ? Fe->n_sub : 1u;
    KSubE &SE = Fe->sub[blockIdx.x & (n_sub_e - 1u)];
    DevCounters *const counters_e = SE.counters;
#ifdef AIC_PROFILE
    if (lane == 0) {
        prof[3] = (uint32_t)__builtin_readcyclecounter() - prof_t0;  // wave lifetime
        const uint32_t wid = blockIdx.x * (WGT / 64u) + (threadIdx.x >> 6);
        if (wid < 2048u) {
            counters_e->wave_prof[wid][0] = prof_t0;
            counters_e->wave_prof[wid][1] = prof_t0 + prof[2];
            counters_e->wave_prof[wid][2] = prof_t0 + prof[3];
            counters_e->wave_prof[wid][3] = prof[9];
        }
        atomicMax(&counters_e->prof[0], (unsigned long long)prof[3]);
        atomicMax(&counters_e->prof[1], (unsigned long long)prof[2]);
    }
#ifdef AIC_TAIL_PROF
    {   // trips (12 bits), event phases (10 bits) and mean lanes stepping per trip (x16, 10 bits) after the wave saw the queue dry
        const uint32_t wid = blockIdx.x * (WGT / 64u) + (threadIdx.x >> 6);
        const uint32_t ml = tail_trips ? (tail_lanes * 16u) / tail_trips : 0u;
        if (lane == 0 && wid < 2048u) counters_e->wave_prof[wid][3] = (tail_trips > 4095u ? 4095u : tail_trips) | ((tail_events > 1023u ? 1023u : tail_events) << 12) | ((ml > 1023u ? 1023u : ml) << 22);
    }
#endif
#ifdef AIC_RAY_PROF
    {   // the wave's longest ray: duration in the upper bits, its step count in the lower 10
        uint32_t best_ = (ray_dur_max & ~1023u) | (ray_dur_steps > 1023u ? 1023u : ray_dur_steps);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const uint32_t o_ = (uint32_t)__shfl_down((int)best_, off, 64); best_ = o_ > best_ ? o_ : best_; }
        const uint32_t wid = blockIdx.x * (WGT / 64u) + (threadIdx.x >> 6);
        if (lane == 0 && wid < 2048u) counters_e->wave_prof[wid][3] = best_;
    }
#endif
    if (lane == 0) for (int i = 2; i < 40; i++) atomicAdd(&counters_e->prof[i], (unsigned long long)prof[i]);
#endif
    // ---- RaytraceInfo sum (renderer.rs:555): wave reduction then one atomic per wave ----
    uint32_t t_end = threadIdx.x;
    asm volatile("" : "+v"(t_end));  // (as above: the word's address is not a value to keep for the life of the wave)
    unsigned long long s = s_steps[t_end];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0 && s) atomicAdd(&counters_e->cubes_traced, s);
    if (DIAG) {
        unsigned long long v[4] = {tot_outer, tot_inner, tot_hits, tot_light};
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
        }
        if (lane == 0) {
            if (v[0]) atomicAdd(&counters_e->n_outer, v[0]);
            if (v[1]) atomicAdd(&counters_e->n_inner, v[1]);
            if (v[2]) atomicAdd(&counters_e->n_hits, v[2]);
            if (v[3]) atomicAdd(&counters_e->n_light, v[3]);
        }
    }
    // the last wave out hands the frame's sums to the host (pinned memory; the end of the kernel makes the stores visible)
    // (No fences: an agent-scope release fence writes the XCD's whole L2 back -- the frame's pixels -- and 4096 waves doing that cost 10 % of a C2
    //  frame. The sums are agent-scope atomics, performed at the memory side; the wave waits for its own to be acknowledged before it is counted, and
    //  the last wave reads them with agent-scope loads.)
    unsigned long long *const host_counters_e = SE.host_counters;
    if (lane == 0 && host_counters_e) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // (the waves of THIS frame: the grid is a multiple of n_sub workgroups, dealt to the frames round-robin)
        if (atomicAdd(&counters_e->waves_done, 1u) == (gridDim.x / n_sub_e) * (blockDim.x >> 6) - 1u) {
            unsigned long long *const src = &counters_e->cubes_traced;  // five consecutive sums and `bailed` (DevCounters)
#pragma unroll
            for (int i = 0; i < 6; i++) host_counters_e[i] = __hip_atomic_load(&src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---------------------------------------------------------------------------------------
// the image kernel's launchers (declared in aic_launch.h)

template <bool VOL, int LMODE, bool DIAG, bool BIG, bool XC>
static void launch_trace_x(const DevFrame &F, hipStream_t stream) {
    // persistent waves: enough workgroups to fill the chip at the kernel's occupancy, never more
    // waves than tiles (each wave pulls 8x8-pixel tiles from counters->tile_next)
    const uint32_t n_tiles = F.tiles_x * F.tiles_y;
    constexpr bool XCHG = XC && !DIAG && LMODE != 3;
    constexpr uint32_t WGT = XCHG ? (uint32_t)AIC_XWG_THREADS : (uint32_t)AIC_WG_THREADS;
    const uint32_t wg_waves = WGT / 64u;
    const uint32_t n_sub = F.n_sub > 1u ? F.n_sub : 1u;  // frames of this launch (DevSub): each gets an equal share of the resident grid
    const uint32_t resident_groups = F.n_cus * 4u * (uint32_t)((DIAG || LMODE == 3) ? 2 : AIC_MIN_WAVES) / wg_waves / n_sub;  // 4 SIMDs per CU, that many waves on each
    // A frame smaller than the chip that is STREAMED (aic_render_submit: a rank's strips of a multi-GPU frame, several in
    // flight) gets a grid in proportion to its tiles -- four tiles per wave, so that lanes are refilled instead of waves ending
    // after one tile, and the kernels of the frames in flight are resident side by side (an eighth of a 1080p frame, 8 in
    // flight: 0.105 ms per frame against 0.138 with one tile per wave). A synchronous frame (aic_render) is a matter of
    // latency: one tile per wave, as many waves as there are tiles.
    const uint32_t tiles_per_wave = F.tiles_per_wave ? F.tiles_per_wave : 1u;  // (the host's choice; AIC_TILES_PER_WAVE, read when the context is made, overrides it)
    const uint32_t by_tiles = (n_tiles + wg_waves - 1u) / wg_waves;
    uint32_t grid = (n_tiles + wg_waves * tiles_per_wave - 1u) / (wg_waves * tiles_per_wave);
    const uint32_t floor_groups = by_tiles < 128u ? by_tiles : 128u;
    if (grid < floor_groups) grid = floor_groups;
    if (grid > resident_groups) grid = resident_groups;
    if (XCHG && F.antialias && grid > F.ray_cold_groups / n_sub) grid = F.ray_cold_groups / n_sub;  // (the host sizes the antialiasing sums' buffer for the resident grid: trace_ray_cold_bytes)
    grid *= n_sub;
    if (grid == 0) return;
    DevFrame G = F;
    G.ray_mode = (F.layer.present && !F.pixel_centers && !F.patches && !F.rays && !F.pixels && !F.ortho_n && F.edge_x && F.edge_y) ? (F.n_parts > 1u ? 1u : 0u) : 2u;  // (DevFrame::ray_mode)
    hipLaunchKernelGGL((trace_image_kernel<VOL, LMODE, DIAG, BIG, XC>), dim3(grid), dim3(WGT), 0, stream, G);
}

// The production variants (no per-pixel records, not Bounce) exist twice: with the lane exchange (a frame of many tiles per persistent wave) and without
// (DevFrame::exchange == 0: a frame of a tile or two per wave -- a rank's share of a multi-GPU frame, the test images -- which the pool only costs).
template <bool VOL, int LMODE, bool DIAG, bool BIG>
static void launch_trace(const DevFrame &F, hipStream_t stream) {
    if constexpr (!DIAG && LMODE != 3) {
        if (F.exchange && (F.ray_cold || !F.antialias)) { launch_trace_x<VOL, LMODE, DIAG, BIG, true>(F, stream); return; }
    }
    launch_trace_x<VOL, LMODE, DIAG, BIG, false>(F, stream);
}

template <bool DIAG, bool BIG>
static void launch_trace_diag(const DevFrame &F, bool vol, int lmode, hipStream_t stream) {
    if (vol) {
        if (lmode == 0) launch_trace<true, 0, DIAG, BIG>(F, stream);
        else if (lmode == 1) launch_trace<true, 1, DIAG, BIG>(F, stream);
        else if (lmode == 3) launch_trace<true, 3, DIAG, BIG>(F, stream);
        else launch_trace<true, 2, DIAG, BIG>(F, stream);
    } else {
        if (lmode == 0) launch_trace<false, 0, DIAG, BIG>(F, stream);
        else if (lmode == 1) launch_trace<false, 1, DIAG, BIG>(F, stream);
        else if (lmode == 3) launch_trace<false, 3, DIAG, BIG>(F, stream);
        else launch_trace<false, 2, DIAG, BIG>(F, stream);
    }
}

// DevFrame::ray_cold of the exchanging variants (antialiased frames): 16 bytes per LDS column (a lane's or a pool slot's) of every workgroup of the resident grid
size_t trace_ray_cold_bytes(uint32_t n_cus, uint32_t *groups) {
    const uint32_t g = n_cus * 4u * (uint32_t)AIC_MIN_WAVES / ((uint32_t)AIC_XWG_THREADS / 64u);
    *groups = g;
    return (size_t)g * ((size_t)AIC_XWG_THREADS + (size_t)AIC_POOL) * 16u;
}

void launch_trace_image(const DevFrame &F, bool diag, hipStream_t stream) {
    const bool vol = F.layer_transparency == 1;
    const int l = F.layer_lighting;
    const int lmode = l == 0 ? 0 : (l == 1 ? 1 : (l == 5 ? 3 : 2));  // None, Flat, Bounce, the interpolated three
    const bool big = F.layer.cls_in_code == 0u;  // block table past 16384 entries: untagged cube grid
    if (diag) {
        if (big) launch_trace_diag<true, true>(F, vol, lmode, stream);
        else launch_trace_diag<true, false>(F, vol, lmode, stream);
    } else {
        if (big) launch_trace_diag<false, true>(F, vol, lmode, stream);
        else launch_trace_diag<false, false>(F, vol, lmode, stream);
    }
}

}  // namespace aic
