// aic_raycast.h -- the reference's Raycaster restated for the device (part of the aic_trace.hip translation unit):
//   Raycaster, its State / FirstLast and RaycastStep::intersection_point (all-is-cubes-base/src/raycast.rs:63-832)
//   Cube::containing (all-is-cubes-base/src/math/cube.rs:97-119)
// One DDA level -- the cube grid or a block's voxels -- is a Lvl: lvl_init is Raycaster::new(..).within(..), lvl_next is Raycaster::next, and
// lvl_first_masks is `next` from FirstLast::Beginning written on wave masks for the image kernel's ENTER / NEWRAY events. f64 in the reference's
// exact operation order (built with -ffp-contract=off): hit cubes, faces and t are bit-exact. probe_raycast_kernel (aic_probe_kernels.h) pins all
// of it against the reference's step tables.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef AIC_DEV
#define AIC_DEV __device__ __forceinline__
#endif

namespace aic {

constexpr int FACE_WITHIN = 0;
constexpr int I32_MIN_ = (-2147483647 - 1);
constexpr int I32_MAX_ = 2147483647;

// first_last states (raycast.rs:153-165)
constexpr uint32_t FL_BEGINNING = 0, FL_INBOUNDS = 1, FL_ENDED = 2;

// ---------------------------------------------------------------------------------------
// f64 helpers with the reference's semantics

AIC_DEV int signum_101(double x) {  // raycast.rs:782-788
    if (x == 0.0) return 0;
    if (x != x) return 0;
    return (__double2hiint(x) < 0) ? -1 : 1;
}

// f64::rem_euclid(1.0): fmod(x,1) == x - trunc(x) exactly (sign of x kept, like fmod)
AIC_DEV double rem_euclid1(double x) {
    double r = x - trunc(x);
    r = copysign(r, x);
    return r < 0.0 ? r + 1.0 : r;
}

// ---- f64 divisions that cost less than the generic sequence, with the generic sequence's bits ----
// The compiler's a / b is v_div_scale x2, v_rcp_f64 (quarter rate), four fused multiply-adds that refine the reciprocal, a multiply, two more
// multiply-adds, v_div_fmas, v_div_fixup: 11 instructions, IEEE-correct for every input. Two cheaper forms, each used only where its precondition holds
// for the lane (checked on the operands' exponent fields) and replaced by the generic quotient, under the lanes' exec mask, where it does not:
//  * div_known_recip: the divisor's correctly rounded reciprocal y = RN(1 / b) is at hand (a ray's t_delta = 1 / |direction|, raycast.rs:766). Then
//    q0 = a * y is within 1.5 ulp of a / b, q1 = q0 + (a - b q0) y is a faithful quotient, and one more residual step q2 = q1 + (a - b q1) y is a / b
//    correctly rounded (Markstein's theorem: a faithful q, the exact residual r = a - b q, and y within half an ulp of 1 / b give RN(q + r y) = RN(a / b),
//    absent overflow / underflow) -- five multiply-adds, no reciprocal instruction (lvl_init). tests: the probe's step tables and 400 random rays (t bit-exact).
//  * three quotients by one divisor (the unprojection's x / w, y / w, z / w) share the reciprocal's refinement: with operands whose exponents are far from
//    the ends of the range v_div_scale scales nothing, v_div_fmas is a plain fused multiply-add and v_div_fixup passes the quotient through, so
//    the shared form performs the generic sequence's own operations on the same values.
// A block behind a wave-uniform branch that must STAY a branch: arithmetic without side effects is otherwise speculated -- the compiler computes the rare
// path for every wave and selects (seen with the generic division below: 11 instructions per quotient, executed always). An empty volatile asm
// statement cannot be speculated.
#ifndef AIC_RARE_PATH
#define AIC_RARE_PATH() asm volatile("" ::: "memory")
#endif
// Exponent window of an operand, on the high dword: biased exponent in [768, 1280), i.e. 2^-255 <= |v| < 2^257; and the wider [512, 1536).
AIC_DEV bool f64_exp_in_768_1280(double v) { return (((uint32_t)__double2hiint(v) << 1) - (768u << 21)) < (512u << 21); }
AIC_DEV bool f64_exp_in_512_1536(double v) { return (((uint32_t)__double2hiint(v) << 1) - (512u << 21)) < (1024u << 21); }
AIC_DEV double div_known_recip(double a, double b, double y) {  // a / b for normal b > 0, y = RN(1 / b); a, b and a / b far from overflow and underflow; a is not -0
    const double q0 = a * y;
    const double r0 = fma(-b, q0, a);
    const double q1 = fma(r0, y, q0);
    const double r1 = fma(-b, q1, a);
    return fma(r1, y, q1);
}
// raycast.rs:797-819, split around its division: the dividend 1 - s.rem_euclid(1) (s and ds negated together for ds < 0: |ds| is the divisor either way) ...
AIC_DEV double scale_step_dividend(double s, double ds) { return 1.0 - rem_euclid1(ds < 0.0 ? -s : s); }
// ... and what becomes of the quotient q = dividend / |ds|
AIC_DEV double scale_step_result(double q, double s, double ds) {
    return (ds == 0.0 && !(s != s)) ? __longlong_as_double(0x7ff0000000000000LL) : q;
}

// cube.rs:97-119
AIC_DEV bool cube_containing(const double p[3], int out[3]) {
    const double MIN_INCLUSIVE = -2147483648.0;
    const double MAX_EXCLUSIVE = 2147483648.0;
    bool ok = (MIN_INCLUSIVE <= p[0]) & (MIN_INCLUSIVE <= p[1]) & (MIN_INCLUSIVE <= p[2]) & (p[0] < MAX_EXCLUSIVE) &
              (p[1] < MAX_EXCLUSIVE) & (p[2] < MAX_EXCLUSIVE);
    if (ok) {
        out[0] = (int)floor(p[0]);
        out[1] = (int)floor(p[1]);
        out[2] = (int)floor(p[2]);
    }
    return ok;
}

// Per-ray constants: Parameters::new (raycast.rs:749-771) minus the origin. Kept as scalars
// (never indexed dynamically) so they live in VGPRs.
struct RayDir {
    double dx, dy, dz;     // direction (zeroed if any |component| is not < 1e100)
    double tdx, tdy, tdz;  // t_delta = 1/|d|
    int sx, sy, sz;        // step = signum_101(d)
    bool fast;             // every component is zero or has its exponent in [768, 1280): divisions by it may use t_delta (div_by_dir)
};
AIC_DEV bool raydir_fast(double dx, double dy, double dz) {
    const int fx = f64_exp_in_768_1280(dx) | (dx == 0.0), fy = f64_exp_in_768_1280(dy) | (dy == 0.0), fz = f64_exp_in_768_1280(dz) | (dz == 0.0);
    return (fx & fy & fz) != 0;
}

AIC_DEV RayDir raydir_init(double dx, double dy, double dz) {
    RayDir r;
    const bool all_small = (fabs(dx) < 1e100) && (fabs(dy) < 1e100) && (fabs(dz) < 1e100);
    r.dx = all_small ? dx : 0.0;
    r.dy = all_small ? dy : 0.0;
    r.dz = all_small ? dz : 0.0;
    r.sx = signum_101(r.dx); r.sy = signum_101(r.dy); r.sz = signum_101(r.dz);
    r.tdx = 1.0 / fabs(r.dx); r.tdy = 1.0 / fabs(r.dy); r.tdz = 1.0 / fabs(r.dz);
    r.fast = raydir_fast(r.dx, r.dy, r.dz);
    return r;
}

// State of one DDA level (raycast.rs:99-121 State + FirstLast), with the step deferred: the
// reference emits `current()` and then advances; here the advance is performed at the start
// of the following `next`, which is observationally identical and lets `c*` double as the
// emitted cube.
struct Lvl {
    double tx, ty, tz;  // t_max
    double last_t;
    int cx, cy, cz;
    uint32_t st;        // bits 0-1 first_last | 2-4 last_face | 5-6 pick | 7 need_step | 8 include_exit
};
// While INBOUNDS: the coordinate value that means "left the bounds", per axis.
struct Lim {
    int x, y, z;
};
AIC_DEV uint32_t lvl_fl(const Lvl &s) { return s.st & 3u; }
AIC_DEV int lvl_face(const Lvl &s) { return (int)((s.st >> 2) & 7u); }

AIC_DEV int pick_axis(double tx, double ty, double tz) {  // raycast.rs:584-596
    if (tx < ty) return (tx < tz) ? 0 : 2;
    return (ty < tz) ? 1 : 2;
}

// Raycaster::new(origin, dir) [.within(lo,hi, include_exit)]  (raycast.rs:196-230, 513-545, 632-704)
struct LvlLim {
    Lvl s;
    Lim lim;
};
// Written without early exits (round 6): every lane computes everything and `valid` decides at the end -- a level that is State::EMPTY comes back as
// FL_ENDED with unspecified t_max / cube (nothing reads them: Raycaster::next returns None at once). With the exits, each one cost a saved exec mask, a
// branch and a dozen moves of default values on the path of every lane that did not take it.
AIC_DEV bool cube_containing_flat(double x, double y, double z, int out[3]) {  // cube.rs:97-119; `out` is unspecified when there is no cube
    const double MIN_INCLUSIVE = -2147483648.0;
    const double MAX_EXCLUSIVE = 2147483648.0;
    const int ok = (int)(MIN_INCLUSIVE <= x) & (int)(MIN_INCLUSIVE <= y) & (int)(MIN_INCLUSIVE <= z) & (int)(x < MAX_EXCLUSIVE) & (int)(y < MAX_EXCLUSIVE) & (int)(z < MAX_EXCLUSIVE);
    // (v_cvt_i32_f64 itself, which saturates: the C++ conversion of a value that does not fit is undefined, and the optimiser may act on that)
    const double fx = floor(x), fy = floor(y), fz = floor(z);
    asm("v_cvt_i32_f64 %0, %1" : "=v"(out[0]) : "v"(fx));
    asm("v_cvt_i32_f64 %0, %1" : "=v"(out[1]) : "v"(fy));
    asm("v_cvt_i32_f64 %0, %1" : "=v"(out[2]) : "v"(fz));
    return ok != 0;
}
AIC_DEV LvlLim lvl_init(double ox, double oy, double oz, const RayDir rd, bool bounded, int lox, int loy,
                        int loz, int hix, int hiy, int hiz, bool include_exit, double half_over_len) {
    LvlLim out;
    Lvl &s = out.s;
    Lim &lim = out.lim;
    int cube_o[3];
    int valid = cube_containing_flat(ox, oy, oz, cube_o);
    // MAXIMUM_BOUNDS.contains_cube (raycast.rs:485-499, 521-523); else State::EMPTY: produces nothing
    // (c in [MIN + 1, MAX - 2]  <=>  (unsigned)(c - (MIN + 1)) < 2^32 - 3)
    valid &= (int)((uint32_t)cube_o[0] - 0x80000001u < 0xfffffffdu) & (int)((uint32_t)cube_o[1] - 0x80000001u < 0xfffffffdu) & (int)((uint32_t)cube_o[2] - 0x80000001u < 0xfffffffdu);
    // bounds = MAXIMUM_BOUNDS ∩ given (empty => ORIGIN_EMPTY, which contains no cube)
    if (bounded) {
        lox = max(lox, I32_MIN_ + 1); loy = max(loy, I32_MIN_ + 1); loz = max(loz, I32_MIN_ + 1);
        hix = min(hix, I32_MAX_ - 1); hiy = min(hiy, I32_MAX_ - 1); hiz = min(hiz, I32_MAX_ - 1);
    } else {
        lox = loy = loz = I32_MIN_ + 1;
        hix = hiy = hiz = I32_MAX_ - 1;
    }
    valid &= (int)(hix > lox) & (int)(hiy > loy) & (int)(hiz > loz);
    // fast_forward (raycast.rs:632-704): plane_origin takes the upper bound on axes the ray descends, else the lower bound; one ray-plane
    // intersection per moving axis. If the largest t is positive the ray starts again half a cube short of it (`t_start`), else where it is
    // (t_start = +0: `ff` is the origin itself, and adding +0 to a t_max -- a quotient that is positive, +0 or infinite -- changes nothing).
    // One copy of the t_max arithmetic serves both (round 6; it was written twice, each copy behind its own per-lane branch).
    double t_start = 0.0;
    double ffx = ox, ffy = oy, ffz = oz;
    int cube[3] = {cube_o[0], cube_o[1], cube_o[2]};
    if (bounded) {
        const double pox = (double)((rd.sx < 0) ? hix : lox);
        const double poy = (double)((rd.sy < 0) ? hiy : loy);
        const double poz = (double)((rd.sz < 0) ? hiz : loz);
        const double relx = pox - ox, rely = poy - oy, relz = poz - oz;
        // ray_plane_intersection (raycast.rs:821-832) with an axis-aligned unit normal n = +-1:
        // (rel.n)/(dir.n) == rel_a / dir_a exactly (the +-1 factors and the +-0 terms cancel for the
        // finite values that reach this point). rel_a / dir_a = +-(rel_a / |dir_a|), the quotient by the reciprocal at hand (div_known_recip) for lanes
        // whose rel_a is neither zero nor tiny (the origin is inside i32, so it is not huge); computed for every lane, used for the moving axes.
        const int okx = f64_exp_in_512_1536(relx) | (rd.sx == 0), oky = f64_exp_in_512_1536(rely) | (rd.sy == 0), okz = f64_exp_in_512_1536(relz) | (rd.sz == 0);
        const bool ff_fast = ((int)rd.fast & okx & oky & okz) != 0;
        double qx = div_known_recip(relx, fabs(rd.dx), rd.tdx), qy = div_known_recip(rely, fabs(rd.dy), rd.tdy), qz = div_known_recip(relz, fabs(rd.dz), rd.tdz);
        if (__builtin_amdgcn_ballot_w64(!ff_fast) != 0ull) {  // (never, in an ordinary frame)
            AIC_RARE_PATH();
            if (!ff_fast) { qx = relx / fabs(rd.dx); qy = rely / fabs(rd.dy); qz = relz / fabs(rd.dz); }
        }
        double max_t = 0.0;
        max_t = rd.sx != 0 ? fmax(max_t, rd.sx < 0 ? -qx : qx) : max_t;
        max_t = rd.sy != 0 ? fmax(max_t, rd.sy < 0 ? -qy : qy) : max_t;
        max_t = rd.sz != 0 ? fmax(max_t, rd.sz < 0 ? -qz : qz) : max_t;
        const bool go = max_t > 0.0;  // last_t_distance == 0 at this point
        // 0.5 / direction.length() (raycast.rs:669) is a per-ray constant, computed once by the caller
        double ts = max_t - half_over_len;
        ts = isfinite(ts) ? ts : max_t;
        t_start = go ? ts : 0.0;
        ffx = go ? ox + rd.dx * ts : ox; ffy = go ? oy + rd.dy * ts : oy; ffz = go ? oz + rd.dz * ts : oz;
    }
    // the cube of the fast-forwarded origin; a fast-forwarded origin without one makes the level State::EMPTY (without a fast-forward it is the
    // origin's own cube, which `valid` has already judged)
    if (bounded) valid &= (int)cube_containing_flat(ffx, ffy, ffz, cube);
    {
        // scale_to_integer_step on each axis (raycast.rs:797-819). The dividends are in [2^-53, 1] or +0: with a direction in the window (RayDir::fast)
        // div_known_recip's precondition holds
        const double ax = scale_step_dividend(ffx, rd.dx), ay = scale_step_dividend(ffy, rd.dy), az = scale_step_dividend(ffz, rd.dz);
        double qx = div_known_recip(ax, fabs(rd.dx), rd.tdx), qy = div_known_recip(ay, fabs(rd.dy), rd.tdy), qz = div_known_recip(az, fabs(rd.dz), rd.tdz);
        if (__builtin_amdgcn_ballot_w64(!rd.fast) != 0ull) {
            AIC_RARE_PATH();
            if (!rd.fast) { qx = ax / fabs(rd.dx); qy = ay / fabs(rd.dy); qz = az / fabs(rd.dz); }
        }
        s.tx = scale_step_result(qx, ffx, rd.dx) + t_start;
        s.ty = scale_step_result(qy, ffy, rd.dy) + t_start;
        s.tz = scale_step_result(qz, ffz, rd.dz) + t_start;
    }
    s.last_t = t_start;
    s.cx = cube[0]; s.cy = cube[1]; s.cz = cube[2];
    // exit coordinate once in bounds: moving up leaves at hi, moving down leaves at lo-1
    lim.x = rd.sx > 0 ? hix : lox - 1;
    lim.y = rd.sy > 0 ? hiy : loy - 1;
    lim.z = rd.sz > 0 ? hiz : loz - 1;
    s.st = valid ? (FL_BEGINNING | ((uint32_t)FACE_WITHIN << 2) | (include_exit ? 256u : 0u)) : FL_ENDED;
    return out;
}

// RaycastStep::recursive_raycast (raycast.rs:458-476) for a step whose cube_ahead is (cx, cy, cz): the sub-ray starts at
// (origin - cube.lower_bounds) * resolution, keeps the direction (so `rd` and `half_over_len` are the outer ray's) and is cast within the block's voxel
// bounds WITH the exit step. The arithmetic of the Bounce rays' EnterBlock (aic_light_bounce.h, which keeps its own three lines: calling this from there
// moved 256 bytes of the trace kernels' code object, which stays as it is) as a function, for the cursor raycast (aic_cursor_raycast.hip).
AIC_DEV LvlLim lvl_init_recursive(double ox, double oy, double oz, int cx, int cy, int cz, double kd /* the resolution */, const RayDir rd, int lox, int loy, int loz,
                                  int hix, int hiy, int hiz, double half_over_len) {
    return lvl_init((ox - (double)cx) * kd, (oy - (double)cy) * kd, (oz - (double)cz) * kd, rd, true, lox, loy, loz, hix, hiy, hiz, true, half_over_len);
}

// The deferred State::step (raycast.rs:577-626) along the axis recorded in `pick`.
AIC_DEV Lvl lvl_do_step(Lvl s, const RayDir rd) {
    const uint32_t axis = (s.st >> 5) & 3u;
    uint32_t face;
    if (axis == 0) {
        s.last_t = s.tx; s.tx += rd.tdx; s.cx += rd.sx; face = rd.sx > 0 ? 1u : 4u;
    } else if (axis == 1) {
        s.last_t = s.ty; s.ty += rd.tdy; s.cy += rd.sy; face = rd.sy > 0 ? 2u : 5u;
    } else {
        s.last_t = s.tz; s.tz += rd.tdz; s.cz += rd.sz; face = rd.sz > 0 ? 3u : 6u;
    }
    s.st = (s.st & ~(7u << 2) & ~128u) | (face << 2);  // FACE_TABLE; clears need_step
    return s;
}

// Raycaster::next (raycast.rs:239-284). lo*/hi* are only consulted before the ray has entered
// the bounds. Returns true if a step was produced: {c*, lvl_face, last_t, t*}; *is_exit tells
// whether it is the include_exit step (the only produced step whose cube is out of bounds).
struct NextResult {
    Lvl s;
    bool got, is_exit;
};
AIC_DEV NextResult lvl_next(Lvl s, const Lim lim, const RayDir rd, int lox, int loy, int loz, int hix, int hiy, int hiz) {
    NextResult R;
    R.got = false;
    R.is_exit = false;
    for (;;) {
        const uint32_t fl = lvl_fl(s);
        if (fl == FL_ENDED) { R.s = s; return R; }
        const bool stepped = (s.st & 128u) != 0;
        const uint32_t stepped_axis = (s.st >> 5) & 3u;
        if (stepped) s = lvl_do_step(s, rd);
        bool oob_enter = false, oob_exit = false;
        if (fl == FL_INBOUNDS) {
            // only the axis just stepped can have left; it can never be "not yet entered"
            const int c = stepped_axis == 0 ? s.cx : (stepped_axis == 1 ? s.cy : s.cz);
            const int l = stepped_axis == 0 ? lim.x : (stepped_axis == 1 ? lim.y : lim.z);
            oob_exit = stepped && (c == l);
        } else {
            // is_out_of_bounds_ahead (raycast.rs:711-728)
            {
                const bool low = s.cx < lox, high = s.cx >= hix;
                oob_enter |= rd.sx == 0 ? (low | high) : (rd.sx < 0 ? high : low);
                oob_exit |= rd.sx == 0 ? (low | high) : (rd.sx < 0 ? low : high);
            }
            {
                const bool low = s.cy < loy, high = s.cy >= hiy;
                oob_enter |= rd.sy == 0 ? (low | high) : (rd.sy < 0 ? high : low);
                oob_exit |= rd.sy == 0 ? (low | high) : (rd.sy < 0 ? low : high);
            }
            {
                const bool low = s.cz < loz, high = s.cz >= hiz;
                oob_enter |= rd.sz == 0 ? (low | high) : (rd.sz < 0 ? high : low);
                oob_exit |= rd.sz == 0 ? (low | high) : (rd.sz < 0 ? low : high);
            }
        }
        if (!oob_enter && !oob_exit) {
            const int pick = pick_axis(s.tx, s.ty, s.tz);
            const double tp = pick == 0 ? s.tx : (pick == 1 ? s.ty : s.tz);
            // valid_for_stepping (raycast.rs:563-570): with NaN-free t_max (guaranteed for a
            // non-EMPTY state) it is exactly "the smallest t_max is finite".
            if (!isfinite(tp)) {
                s.st = (s.st & ~3u) | FL_ENDED;
                R.got = lvl_face(s) == FACE_WITHIN;
                R.s = s;
                return R;
            }
            s.st = (s.st & ~3u & ~(3u << 5)) | FL_INBOUNDS | ((uint32_t)pick << 5) | 128u;
            R.got = true;
            R.s = s;
            return R;
        } else if (fl == FL_BEGINNING && oob_enter && !oob_exit) {
            const int pick = pick_axis(s.tx, s.ty, s.tz);
            const double tp = pick == 0 ? s.tx : (pick == 1 ? s.ty : s.tz);
            if (!isfinite(tp)) {
                s.st = (s.st & ~3u) | FL_ENDED;
                R.s = s;
                return R;
            }
            const int c = pick == 0 ? s.cx : (pick == 1 ? s.cy : s.cz);
            const int st = pick == 0 ? rd.sx : (pick == 1 ? rd.sy : rd.sz);
            if ((st > 0 && c == I32_MAX_) || (st < 0 && c == I32_MIN_)) {  // checked_add failed
                s.st = (s.st & ~3u) | FL_ENDED;
                R.s = s;
                return R;
            }
            s.st = (s.st & ~(3u << 5)) | ((uint32_t)pick << 5) | 128u;
            continue;
        } else if (fl == FL_INBOUNDS && !oob_enter && oob_exit) {
            s.st = (s.st & ~3u) | FL_ENDED;
            if (s.st & 256u) {
                R.is_exit = true;
                R.got = true;
            }
            R.s = s;
            return R;
        } else {
            s.st = (s.st & ~3u) | FL_ENDED;
            R.s = s;
            return R;
        }
    }
}

// RaycastStep::intersection_point (raycast.rs:409-439) for the step currently held in `s`.
//
// Same arithmetic as the reference, written without per-axis control flow. For an axis the ray moves along
// and that is not the face just crossed, the reference adds  1 - clamp((t_max - t) * d)  going up and
// clamp(-((t_max - t) * d))  going down; -(x * d) == x * (-d) exactly, so both clamp the one product
// (t_max - t) * |d|. That product is never NaN (t is finite, d finite and non-zero on this path), hence
// f64::clamp(0, 1) == min(max(c, 0), 1); its only other freedom, the sign of a zero, cannot reach the result
// (1 - +-0 == 1, and cube + +-0 == cube because an integer-valued cube coordinate is never -0).
AIC_DEV double ip_axis(bool is_face_axis, bool within, int cube, double o, double d, double t_max, double last_t) {
    const double cc = (double)cube;
    const bool neg = d < 0.0;                        // signum_101(d) < 0
    double c = (t_max - last_t) * fabs(d);
    c = fmin(fmax(c, 0.0), 1.0);
    const double moved = cc + (neg ? c : 1.0 - c);   // normal cube face hit
    const double plane = cc + (neg ? 1.0 : 0.0);     // the plane just crossed
    double v = is_face_axis ? plane : ((d == 0.0) ? o : moved);   // signum_101(d) == 0: the ray does not move from the origin
    return within ? o : v;
}
AIC_DEV void intersection_point(const Lvl s, double ox, double oy, double oz, double dx, double dy, double dz, double out[3]) {
    const int face = lvl_face(s);
    const bool within = face == FACE_WITHIN;
    const int face_axis = face > 3 ? face - 4 : face - 1;  // Face::axis(): NX NY NZ PX PY PZ = 1..6
    out[0] = ip_axis(face_axis == 0, within, s.cx, ox, dx, s.tx, s.last_t);
    out[1] = ip_axis(face_axis == 1, within, s.cy, oy, dy, s.ty, s.last_t);
    out[2] = ip_axis(face_axis == 2, within, s.cz, oz, dz, s.tz, s.last_t);
}


// The first cube of a freshly initialised level, for the ENTER / RAY events: Raycaster::next run until it yields its first step or ends, so that the
// stepping loop only ever sees levels that are already inside their bounds. Written like the stepping trip (round 6): wave masks for every decision, the per-lane state updated in place by
// one exec-masked block -- lvl_next above, inlined into ENTER and NEWRAY, was compiled into ~600 instructions of nested exec-mask scaffolding with some
// thirty register copies per turn of its loop. Raycaster::next from FirstLast::Beginning (raycast.rs:239-284) is: while the cube is outside the bounds on
// the side the ray comes from and not past them (is_out_of_bounds_ahead, raycast.rs:711-728: "not yet entered"), step (State::step, raycast.rs:577-626:
// along the axis of the smallest t_max, ties to the later axis; a level whose smallest t_max is not finite cannot step and ends); a cube inside the
// bounds is emitted -- also by a level that cannot step, if it has not stepped yet (Face7::Within); anything else ends the level with nothing emitted.
// (`checked_add` of the stepped coordinate cannot fail: a coordinate at i32::MAX with the ray going up, or at MIN going down, is past the bounds.)
// Returns the emitted cube in the kernel's conventions: `lax` = the axis stepped along last, or 8 | Face7::Within for a cube emitted without a step.
struct FirstCube {
    double tx, ty, tz, last_t;
    int cx, cy, cz;
    uint32_t lax;
    bool got, inbounds;  // emitted a cube; the level can go on (FirstLast::InBounds)
};
AIC_DEV FirstCube lvl_first_masks(const Lvl s0, const RayDir rd, int lox, int loy, int loz, int hix, int hiy, int hiz) {
    typedef unsigned long long mask_t;
    FirstCube f;
    f.tx = s0.tx; f.ty = s0.ty; f.tz = s0.tz; f.last_t = s0.last_t;
    f.cx = s0.cx; f.cy = s0.cy; f.cz = s0.cz;
    f.lax = 8u | (uint32_t)FACE_WITHIN;
    const mask_t negx = __builtin_amdgcn_ballot_w64(rd.sx < 0), posx = __builtin_amdgcn_ballot_w64(rd.sx > 0);
    const mask_t negy = __builtin_amdgcn_ballot_w64(rd.sy < 0), posy = __builtin_amdgcn_ballot_w64(rd.sy > 0);
    const mask_t negz = __builtin_amdgcn_ballot_w64(rd.sz < 0), posz = __builtin_amdgcn_ballot_w64(rd.sz > 0);
    mask_t active = __builtin_amdgcn_ballot_w64(lvl_fl(s0) != FL_ENDED);
    mask_t m_got = 0ull, m_inb = 0ull, m_stepped = 0ull;
    const uint32_t finite_classes = 0x1f8u;  // v_cmp_class: -normal, -denormal, -0, +0, +denormal, +normal
    while (active != 0ull) {
        // is_out_of_bounds_ahead: per axis "not yet entered" is below the bounds going up, above going down, either for an axis the ray does not move
        // along; "left" the other way round
        const mask_t lowx = __builtin_amdgcn_ballot_w64(f.cx < lox), highx = __builtin_amdgcn_ballot_w64(f.cx >= hix);
        const mask_t lowy = __builtin_amdgcn_ballot_w64(f.cy < loy), highy = __builtin_amdgcn_ballot_w64(f.cy >= hiy);
        const mask_t lowz = __builtin_amdgcn_ballot_w64(f.cz < loz), highz = __builtin_amdgcn_ballot_w64(f.cz >= hiz);
        const mask_t enter = (lowx & ~negx) | (highx & ~posx) | (lowy & ~negy) | (highy & ~posy) | (lowz & ~negz) | (highz & ~posz);
        const mask_t exit_ = (lowx & ~posx) | (highx & ~negx) | (lowy & ~posy) | (highy & ~negy) | (lowz & ~posz) | (highz & ~negz);
        const mask_t m_in = active & ~(enter | exit_), m_go = active & enter & ~exit_;
        const mask_t m_any = m_in | m_go;
        mask_t m_fin, sv, mx, m_stp;
        double mn;
        asm volatile(
            "s_and_saveexec_b64 %[sv], %[any]\n\t"
            "v_min_f64 %[mn], %[tx], %[ty]\n\t"
            "v_min_f64 %[mn], %[mn], %[tz]\n\t"
            "v_cmp_class_f64 %[fin], %[mn], %[cls]\n\t"   // valid_for_stepping (raycast.rs:563-570): the smallest t_max is finite
            "s_and_b64 %[stp], %[fin], %[go]\n\t"          // the lanes that step
            "s_mov_b64 exec, %[stp]\n\t"
            "v_mov_b64 %[lt], %[mn]\n\t"
            "v_cmp_eq_f64 %[mx], %[tz], %[mn]\n\t"         // Z
            "v_cmp_eq_f64 vcc, %[ty], %[mn]\n\t"
            "s_andn2_b64 vcc, vcc, %[mx]\n\t"              // Y
            "s_mov_b64 exec, %[mx]\n\t"
            "v_add_f64 %[tz], %[tz], %[tdz]\n\t"
            "v_add_u32 %[cz], %[cz], %[sz]\n\t"
            "v_mov_b32 %[lax], 2\n\t"
            "s_or_b64 %[mx], %[mx], vcc\n\t"
            "s_mov_b64 exec, vcc\n\t"
            "v_add_f64 %[ty], %[ty], %[tdy]\n\t"
            "v_add_u32 %[cy], %[cy], %[sy]\n\t"
            "v_mov_b32 %[lax], 1\n\t"
            "s_andn2_b64 exec, %[stp], %[mx]\n\t"          // X = stepping lanes that took neither
            "v_add_f64 %[tx], %[tx], %[tdx]\n\t"
            "v_add_u32 %[cx], %[cx], %[sx]\n\t"
            "v_mov_b32 %[lax], 0\n\t"
            "s_mov_b64 exec, %[sv]\n\t"
            : [tx] "+v"(f.tx), [ty] "+v"(f.ty), [tz] "+v"(f.tz), [lt] "+v"(f.last_t), [cx] "+v"(f.cx), [cy] "+v"(f.cy), [cz] "+v"(f.cz), [lax] "+v"(f.lax),
              [mn] "=&v"(mn), [sv] "=&s"(sv), [mx] "=&s"(mx), [fin] "=&s"(m_fin), [stp] "=&s"(m_stp)
            : [tdx] "v"(rd.tdx), [tdy] "v"(rd.tdy), [tdz] "v"(rd.tdz), [sx] "v"(rd.sx), [sy] "v"(rd.sy), [sz] "v"(rd.sz), [any] "s"(m_any), [go] "s"(m_go),
              [cls] "s"(finite_classes)
            : "vcc", "scc");
        m_got |= m_in & (m_fin | ~m_stepped);
        m_inb |= m_in & m_fin;
        m_stepped |= m_stp;
        active = m_stp;
    }
    f.got = __builtin_amdgcn_inverse_ballot_w64(m_got);
    f.inbounds = __builtin_amdgcn_inverse_ballot_w64(m_inb);
    return f;
}

}  // namespace aic
