// aic_split_texel.h -- what the kernels that read a resident Split frame's depth plane share on the device: the validity test of a colour texel and the
// distance along the view axis of a depth value. The bodies are the reprojection's own (aic_reproject.hip), moved here unchanged so that the export
// (aic_present.hip, export_kernel) unprojects a depth with the same instructions.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef AIC_DEV
#define AIC_DEV __device__ __forceinline__
#endif

namespace aic {

// gf_valid (resampling.wgsl:121-125): the alpha half of a texel is above -0.5; false for the marker (0, 0, 0, -1) of "nothing known" and for a NaN alpha
AIC_DEV bool texel_valid(uint2 v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v.y >> 16)) > -0.5f; }

// the view-space distance of depth t (rt-copy.wgsl:210-223); z = {ipz.z, ipw.z, ipz.w, ipw.w} of the camera's inverse projection, f32, one rounding per
// operation (-ffp-contract=off)
AIC_DEV float lin_depth(float t, const float *z) { return -(t * z[0] + z[1]) / (t * z[2] + z[3]); }

}  // namespace aic
