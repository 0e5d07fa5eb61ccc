// nearmedian_wide.hip — gfx950 kernel of stage 2 of the "wise_bulyan" defense
// for 129 to 1024 selected clients with fp32 rows, exported through
// include/fedagg.h (fedagg_nearmedian_mean_wide_f32; the operation is
// specified at fedagg_nearmedian_mean_f32) and linked into libfedagg.so.  The
// kernel is nearmedian_mean_lanes_kernel (nearmedian.h) with E = MedF32.  Its
// own translation unit: the lane-group sorts compile beside trimmed_wide.hip's.

#include "nearmedian.h"

extern "C" {

int fedagg_nearmedian_mean_wide_f32(const float* const* d_src, int32_t K, int64_t N, int32_t keep, float* d_out,
                                    uint32_t flags, fedagg_stream_t stream) {
  (void)flags;  // one kernel form for every alignment
  constexpr const char* what = "fedagg_nearmedian_mean_wide_f32";
  if (int rc = nearmedian_args(what, d_src, K, N, keep, d_out, FEDAGG_NEARMEDIAN_WIDE_MAX_CLIENTS)) return rc;
  if (N == 0) return FEDAGG_OK;  // launch_lanes bounds the grid ("N too large")
  return nearmedian_wide_dispatch<MedF32>(what, d_src, K, N, keep, d_out, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
