// Host-side helpers shared by the C-ABI entry points (error reporting, launch checks).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include "dmc.h"

namespace dmc {
void set_error(const char* fmt, ...);
inline hipStream_t as_stream(void* s) { return (hipStream_t)s; }
inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return 2;
  }
  return 0;
}
inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
}  // namespace dmc

// Launch-plan options (A/B switches for measurement and tests). Read ONCE per process from the environment
// (DMC_* variables, at the first planner call) into one table; afterwards only dmc_set_option() /
// dmc_reset_options() change it. The planners read plain fields, never the environment.
namespace dmc {
enum Opt {
  OPT_NO_NARROW, OPT_NO_GLDS, OPT_NO_SPLITK, OPT_NO_BUFLDS, OPT_NO_HALO, OPT_HALO_PRO, OPT_GN_STATS_SPLIT,
  OPT_GN_BWD_SPLIT, OPT_ATTN_STAGED, OPT_ATTN_HG, OPT_WG_BLOCKS, OPT_GN_STATS_ONE_MAX, OPT_GN_BWD_ONE_MAX,
  OPT_NO_XCD, OPT_NO_EPI_STATS, OPT_WG_MINPIX, OPT_GN_BWD_SLICES, OPT_NO_SKGN, OPT_WG_HALO_TARGET, OPT_SK_TARGET,
  OPT_NO_NHALO, OPT_GN_BWD_FUSED, OPT_GEMM1X1_WK, OPT_GN_BWD_NT,
  OPT_REG_EPI, OPT_GEMM1X1, OPT_WG_PIPE, OPT_IMG_MASK, OPT_IMG_GN, OPT_WG_IMG4, OPT_RESAMPLE_FOLD, OPT_COUNT
};
long opt(Opt o);
}  // namespace dmc

// Scan orders of the DiM Mamba mixer over the h x w token grid. order: bit 0 reverse, bit 1
// column-major, bit 2 snake (every other line walked backwards). A logical position p in [0, h*w) is q = reverse ?
// h*w-1-p : p, line a = q / inner, place b = q % inner (inner = column ? h : w); dmc_order_token_ab is the token
// (row-major index i*w + j) at (a, b), so a kernel that walks p by +-1 carries (a, b) and maps each position it reaches without a division.
namespace dmc {
// mul / shift: q / inner for 0 <= q < 2^31 as (q * mul) >> shift, exact (shift = 31 + ceil(log2 inner), mul =
// ceil(2^shift / inner) <= 2^32 + 1: the error term q * (mul * inner - 2^shift) / (inner * 2^shift) is below 1 / inner),
// so the kernels never run an integer division. make_scan_ord fills them on the host.
struct ScanOrd { int h, w, order, shift; unsigned long long mul; };
__host__ __device__ inline int order_inner(ScanOrd o) { return (o.order & 2) ? o.h : o.w; }
inline ScanOrd make_scan_ord(int h, int w, int order) {
  ScanOrd o{h, w, order, 31, 0};
  const unsigned long long d = (unsigned long long)order_inner(o);
  while ((1ull << (o.shift - 31)) < d) ++o.shift;
  o.mul = ((1ull << o.shift) + d - 1) / d;
  return o;
}
__host__ __device__ inline int order_token_ab(ScanOrd o, int a, int b) {
  if ((o.order & 4) && (a & 1)) b = order_inner(o) - 1 - b;
  return (o.order & 2) ? b * o.w + a : a * o.w + b;
}
// 0 <= q < h*w -> a = q / inner, b = q % inner
__host__ __device__ inline void order_line(ScanOrd o, int q, int& a, int& b) {
  a = (int)(((unsigned long long)(unsigned)q * o.mul) >> o.shift);
  b = q - a * order_inner(o);
}
__host__ __device__ inline int order_token(ScanOrd o, int p) {   // 0 <= p < h*w
  int a, b;
  order_line(o, (o.order & 1) ? o.h * o.w - 1 - p : p, a, b);
  return order_token_ab(o, a, b);
}
}  // namespace dmc

#define DMC_REQUIRE(cond, ...)       \
  do {                               \
    if (!(cond)) {                   \
      dmc::set_error(__VA_ARGS__);   \
      return 1;                      \
    }                                \
  } while (0)
