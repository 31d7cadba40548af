// aic_tunables.h -- the numeric build-time tunables of the trace kernels (aic_trace.hip), in one place. Each default is the measured winner; another
// value is one -D away (tools/build_variants.sh "name:-DAIC_T_BATCH=24"). Frames are bit-identical for every value: the tunables decide when work
// runs, never what a ray computes. Switches that selected whole code paths and lost are not here: they left the source as patches
// (profiles/scripts_r04/experiments_r01_r04.patch, profiles/scripts_r07/retired_switches.patch; tools/build_variants.sh puts them back with AIC_PATCH=).
// The measurement builds -- AIC_PROFILE, AIC_TAIL_PROF, AIC_RAY_PROF, AIC_SECTION_MARKS -- are plain #ifdefs inside the kernel.
#pragma once

// ---- occupancy and workgroup shape
#ifndef AIC_MIN_WAVES
#define AIC_MIN_WAVES 4  // waves per SIMD the production variants are built for (128 VGPRs; cold lane state lives in LDS)
#endif
#ifndef AIC_WG_THREADS
#define AIC_WG_THREADS 256  // threads per persistent workgroup (a multiple of 64)
#endif

// ---- the wave scheduler: when parked work runs
#ifndef AIC_T_BATCH
#define AIC_T_BATCH 32  // run a kind of parked work once this many lanes wait on it
#endif
#ifndef AIC_N_FEW
#define AIC_N_FEW 24    // ... or once at most this many lanes can still step (32 until the fast steps made stepping cheaper: r03 E)
#endif
// Both thresholds scale with the lanes still alive, so that a wave that is running out of rays (the frame's tail) keeps batching instead of running every
// event for a lane or two: at most this many eighths of the lanes alive
#ifndef AIC_FRAC_T
#define AIC_FRAC_T 4  // of AIC_T_BATCH
#endif
#ifndef AIC_FRAC_N
#define AIC_FRAC_N 3  // of AIC_N_FEW
#endif

// ---- the stepping trip
#ifndef AIC_STEP_REPS
#define AIC_STEP_REPS 2  // full stepping passes per scheduler trip (3 until round 4; swept again with AIC_FAST_STEPS once no pending span kept lanes
                         // out of the fast steps: profiles/r04_experiments.txt G)
#endif
#ifndef AIC_FAST_STEPS
#define AIC_FAST_STEPS 16  // bookkeeping-free steps a lane may take ahead of each full pass (at least 1; 8 until round 4) ...
#endif
#ifndef AIC_FAST_MIN
#define AIC_FAST_MIN 16  // ... while at least this many lanes of the wave can take one (at least 1)
#endif

#ifndef AIC_BONUS_MIN
#define AIC_BONUS_MIN 1  // a fast step that found OPEN cubes (aic_device.h) takes their lanes one step further without a lookup if at least this many lanes can (1 .. 64)
#endif

// ---- the lane exchange between the waves of a workgroup (the XC variants; aic_trace.hip "Lane exchange")
#ifndef AIC_XWG_THREADS
#define AIC_XWG_THREADS 256  // threads of a workgroup of the exchanging variants (four per CU, a pool of 72 each: measured ahead of two workgroups of 512 with a pool of 160,
                             // whose eight waves lose more claims to one another and fill the frame's tail worse -- profiles/r05_experiments.txt B)
#endif
#ifndef AIC_POOL
#define AIC_POOL (AIC_XWG_THREADS >= 512 ? 160 : 64)  // parked rays per workgroup (<= 192: up to three tags per lane are scanned); what the CU's 160 KB leave room for beside 80-byte
                                                       // columns (round 5: 72 slots beside 72-byte columns, the ray's origin and direction in global memory)
#endif
#ifndef AIC_XCHG_FULL
#define AIC_XCHG_FULL 48     // a wave with this many lanes of one kind runs it as it is
#endif
#ifndef AIC_XCHG_MIN_GAIN
#define AIC_XCHG_MIN_GAIN 8  // a wave that has lanes of the chosen kind tops up only if the pool adds at least this many
#endif
#ifndef AIC_XCHG_PARK_MIN
#define AIC_XCHG_PARK_MIN 8  // an exchange that only parks (nothing to take) is made for at least this many lanes
#endif

// ---- the reprojection post-process (aic_reproject.hip). Unlike everything above this one is part of what is computed (decision 3), and
// tests/reproject_ref.py carries the same value
#ifndef AIC_REPROJECT_RATIO_CAP
#define AIC_REPROJECT_RATIO_CAP 8.0f  // the largest sprite scale: a sample just in front of the new camera covers a disc of at most 9.2 pixels, not the screen
#endif
