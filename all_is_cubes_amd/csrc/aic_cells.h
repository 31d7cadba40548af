// aic_cells.h -- the terminal's character cells (aic_cells.hip) as the host ABI code sees them: the parameter struct (aic_cells_rule.h, with the rule
// itself) and the launch.
//
// aic_image_cells / aic_render_cells restate image_patch_to_character (all-is-cubes-desktop/src/terminal/chars.rs:18-173) with ColorMode::convert
// (terminal/options.rs:78-139) on the device, one lane per cell: a patch of 1x1, 1x2 or 2x4 pixels of a float frame and its first-hit records becomes one
// aic_cell. DESIGN.md 4.22 has the arithmetic; tests/cells_ref.py is that text in NumPy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aic_cells_rule.h"

namespace aic {

hipError_t launch_cells(const CellsParams &p, hipStream_t stream);

}  // namespace aic
