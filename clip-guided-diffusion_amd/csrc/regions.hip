// Region prompts: the host-side argument check of the `_regions` loss entries and the coverage op of the tests and the benchmark.  The losses
// themselves are the REGIONS instantiations of the kernels in guidance.hip and direction.hip; the coverage device function is region_cov.h.
#include "common.h"
#include "guidance.h"
#include "region_cov.h"

namespace {

// out[cut][p] = cov ** power as the loss kernels weigh prompt p on cut `cut`
__global__ __launch_bounds__(256) void region_coverage_kernel(float* __restrict__ out, int cutn, int P, RegionArgs rg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cutn * P) return;
  out[i] = region_weight(rg, i / P, i % P);
}

}  // namespace

int cgd_check_regions(cgd_ctx* ctx, const cgd_regions& rg, int P) {
  if (!rg.sat || !rg.region_of || !rg.region_of_host || !rg.power || !rg.geo) CGD_FAIL(ctx, "regions: null pointer");
  if (rg.R < 1) CGD_FAIL(ctx, "regions: R must be at least 1");
  if (rg.H < 1 || rg.W < 1 || 255L * rg.H * rg.W >= (1L << 31)) CGD_FAIL(ctx, "regions: 255 * H * W must be positive and below 2^31 (int32 table)");
  for (int p = 0; p < P; ++p)
    if (rg.region_of_host[p] < -1 || rg.region_of_host[p] >= rg.R) CGD_FAIL(ctx, "regions: region_of entry outside [-1, R)");
  return 0;
}

int cgd_launch_region_coverage(cgd_ctx* ctx, const cgd_regions& rg, float* out, int cutn, int P, hipStream_t s) {
  if (!out) CGD_FAIL(ctx, "regions: null pointer");
  if (cutn < 1 || P < 1 || (long)cutn * P >= (1L << 31)) CGD_FAIL(ctx, "regions: cutn and P must be positive");
  CGD_TRY(cgd_check_regions(ctx, rg, P));
  CGD_LAUNCH(region_coverage_kernel, dim3(cdiv((long)cutn * P, 256)), dim3(256), 0, s, out, cutn, P,
             RegionArgs{rg.sat, rg.region_of, rg.power, rg.geo, rg.H, rg.W});
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
