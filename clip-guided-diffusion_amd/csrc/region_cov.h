// Region prompts: the share of a prompt's mask that a cutout box sees, from the mask's summed-area table (include/cgd_mi355x.h,
// cgd_spherical_loss_regions).  One device function for the two loss kernels (guidance.hip, direction.hip) and the coverage op (regions.hip).
#pragma once
#include <hip/hip_runtime.h>

// What a `_regions` launch adds to the plain one's arguments; all pointers are device memory.
struct RegionArgs {
  const int* sat;        // (R, H+1, W+1): S[y][x] = sum of the 8-bit mask over rows < y and columns < x
  const int* region_of;  // (P): the prompt's table, or -1 for "everywhere"
  const float* power;    // (P): exponent of the coverage, > 0
  const int* geo;        // this step's table, rows (oy, ox, h, w): the first cutn are the boxes
  int H, W;
};

// cov ** power of prompt p on cut `cut`: four table reads, an exact integer numerator, one division.  1 for a prompt without a region, 0
// for an empty box.  The corners are clamped to the frame, so that a table row that is no box of this frame cannot read outside the table.
__device__ __forceinline__ float region_weight(const RegionArgs& rg, int cut, int p) {
  const int r = rg.region_of[p];
  if (r < 0) return 1.f;
  const int oy = rg.geo[cut * 4 + 0], ox = rg.geo[cut * 4 + 1], h = rg.geo[cut * 4 + 2], w = rg.geo[cut * 4 + 3];
  if (h <= 0 || w <= 0) return 0.f;
  const int y0 = min(max(oy, 0), rg.H), y1 = min(max(oy + h, 0), rg.H);
  const int x0 = min(max(ox, 0), rg.W), x1 = min(max(ox + w, 0), rg.W);
  const int st = rg.W + 1;
  const int* S = rg.sat + (long)r * (rg.H + 1) * st;
  const int num = S[y1 * st + x1] - S[y0 * st + x1] - S[y1 * st + x0] + S[y0 * st + x0];
  const float cov = (float)num / (float)(255 * h * w);
  const float pw = rg.power[p];
  return pw == 1.f ? cov : powf(cov, pw);
}
