// nearmedian.hip — gfx950 kernel of stage 2 of the "wise_bulyan" defense for
// fp32 rows: per coordinate the mean of the `keep` client values nearest the
// coordinate's median, exported through include/fedagg.h
// (fedagg_nearmedian_mean_f32, where the operation is specified) and linked
// into libfedagg.so.  The kernel is nearmedian_mean_kernel (nearmedian.h) with
// E = MedF32.  Its own translation unit: trimmed.hip is untouched, and the two
// sets of unpruned networks compile side by side.

#include "nearmedian.h"

extern "C" {

int fedagg_nearmedian_mean_f32(const float* const* d_src, int32_t K, int64_t N, int32_t keep, float* d_out,
                               uint32_t flags, fedagg_stream_t stream) {
  (void)flags;  // one kernel form for every alignment
  constexpr const char* what = "fedagg_nearmedian_mean_f32";
  if (int rc = nearmedian_args(what, d_src, K, N, keep, d_out, FEDAGG_NEARMEDIAN_MAX_CLIENTS)) return rc;
  if (N == 0) return FEDAGG_OK;
  return nearmedian_dispatch<MedF32>(what, d_src, K, N, keep, d_out, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
