// nearmedian_wide16.hip — gfx950 kernel of stage 2 of the "wise_bulyan"
// defense for bf16 and f16 rows, 129 to 1024 selected clients:
// nearmedian_mean_lanes_kernel (nearmedian.h) on 2-byte elements widened
// exactly as they arrive; the sort, the LDS ring of partners (fp32 words) and
// the chain are the fp32 kernel's, the mean rounded once to the rows' type.
// Exported through include/fedagg.h (fedagg_nearmedian_mean_wide_16) and
// linked into libfedagg.so.  Its own translation unit, compiled beside
// nearmedian16.hip and without packed fp32 operations (build.py UNIT_FLAGS).

#include "nearmedian.h"

extern "C" {

int fedagg_nearmedian_mean_wide_16(int32_t dtype, const void* const* d_src, int32_t K, int64_t N, int32_t keep,
                                   void* d_out, uint32_t flags, fedagg_stream_t stream) {
  (void)flags;  // one kernel form for every alignment: rows are aligned to their element only
  constexpr const char* what = "fedagg_nearmedian_mean_wide_16";
  if (int rc = nearmedian_args(what, d_src, K, N, keep, d_out, FEDAGG_NEARMEDIAN_WIDE_MAX_CLIENTS)) return rc;
  if (dtype != FEDAGG_DT_BF16 && dtype != FEDAGG_DT_F16)
    return set_error(FEDAGG_EINVAL, std::string(what) + ": dtype must be FEDAGG_DT_BF16 or FEDAGG_DT_F16");
  if (N == 0) return FEDAGG_OK;  // launch_lanes bounds the grid ("N too large")
  auto st = reinterpret_cast<hipStream_t>(stream);
  auto src = reinterpret_cast<const uint16_t* const*>(d_src);
  auto out = static_cast<uint16_t*>(d_out);
  if (dtype == FEDAGG_DT_BF16) return nearmedian_wide_dispatch<MedBF16>(what, src, K, N, keep, out, st);
  return nearmedian_wide_dispatch<NearF16>(what, src, K, N, keep, out, st);
}

}  // extern "C"
