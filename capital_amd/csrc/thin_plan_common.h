// thin_plan_common.h -- what tri_thin_plan.h and sym_thin_plan.h share.  No HIP: a host compiler builds the plans too (tests/*_thin_plan).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define THIN_HD __host__ __device__
#else
#define THIN_HD
#endif
namespace thin_plan {
THIN_HD inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
THIN_HD inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
THIN_HD inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
}  // namespace thin_plan
