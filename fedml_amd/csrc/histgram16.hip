// histgram16.hip — the fused history update and uncentred Gram of the
// "foolsgold_cos" defense for bf16 / f16 client rows (gfx950), exported through
// include/fedagg.h and linked into libfedagg.so beside histgram.hip, which
// holds the fp32 entry and describes the engine.
//
//   fedagg_histgram_16   a_i = fl32(fl32(w(x_i) - w(ref)) + h_i), h_i = a_i in
//                        place, d_out = A A^T (K x K, fp64, both triangles),
//                        K <= 128; w: the exact widening of a bf16 / f16 value
//
// A 16-bit model's clients stay 16-bit on the card; their histories are fp32
// (an accumulated sum).  Once a history has been added, a is a general fp32
// value, so every stage splits it into all three bf16 planes and runs the six
// products of the fp32 kernel: the engine (8 waves, one block per CU,
// 64-column stages, double-buffered planes, fp32 over kSplitFold stages and
// fp64 across, the row-pair tile schedule, the partial layout, the finish) is
// csrc/histgram.h's template, unchanged.  What 16-bit rows change is the front
// of a stage:
//
// * Loads.  Column ownership is the fp32 kernel's: 16 lanes by 4 columns per
//   row, 4 rows per wave-load.  A lane's four columns of a client row are 8
//   bytes (one global_load_dwordx2, non-temporal), its four columns of the
//   history still 16 (dwordx4, non-temporal), its piece of ref 8 (a plain
//   load: every wave of the block reads the same 128 bytes).  The lane that
//   loads a column of x loads that column of h, forms a, stores it and splits
//   it: a column belongs to one chunk, so to one block, and within the block
//   to that one lane, and the update in place is race-free with no cross-lane
//   step.
// * Alignment.  The 8-byte loads need the piece on an 8-byte boundary: an
//   8-byte aligned row pointer and a stage whose first column is a multiple of
//   4.  Bucket rows are aligned; a chunk may start anywhere.  The kernel
//   decides per wave (a ballot over its rows' pointers, once) and per stage
//   (the first column, a scalar), separately for ref: both are wave-uniform
//   branches.  Every other stage, and a partial one, loads 2-byte elements
//   under fetch's masks into the same packed registers; after the load the two
//   forms are the same instructions, so the results are the same bits at every
//   alignment.  The history pieces take the fp32 kernel's 16-byte loads and
//   stores in every full stage whatever the 16-bit rows' alignment.
// * Widening.  The two-stage prefetch holds x and ref as raw packed words and
//   widens them when the stage is split: bf16 by v_lshlrev_b32 16 / v_and
//   0xffff0000, f16 by v_cvt_f32_f16 (denormals kept).
//
// Registers.  A stage in flight is, per lane, LPW = 4 client pieces of 2 VGPRs,
// 4 history pieces of 4 and the ref piece of 2: 26 VGPRs where the fp32 kernel
// holds 36, 52 against 72 for the two stages of the pipeline.  The block runs
// 8 waves on 4 SIMDs, two per SIMD (launch_bounds(kSplit8BS, 1)): a budget of
// 256 VGPRs.  Compiled for gfx950 (-Rpass-analysis=kernel-resource-usage),
// K = 113 .. 128 (NB = 8) with a history: 216 VGPRs for bf16 and for f16 (the
// fp32 kernel: 234), 167 without one, no AGPRs, 122,880 bytes of LDS (the
// planes, as the fp32 kernel), no scratch and no spill at any NB, with or
// without a history.
//
// Traffic per element and client falls from 12 bytes (x 4, h 4 + 4) to 10, and
// no fp32 copy of the K client rows is made; what that is worth is measured by
// tools/foolsgold16_probe.py (NOTES.md §5c and §7d, defense.HISTGRAM16_AUTO).
//
// This unit is compiled without packed fp32 VALU instructions (build.py,
// UNIT_FLAGS, which gives the reason); its VALU work is shifts, converts,
// single subtracts and adds.

#include "histgram.h"

extern "C" {

int fedagg_histgram_16(int32_t dtype, const void* const* d_src, int32_t K, const void* d_ref, float* const* d_hist,
                       const int64_t* d_chunks, int64_t n_chunks, double* d_out, double* d_work, int64_t work_len,
                       fedagg_stream_t stream) {
  if (dtype == FEDAGG_DT_BF16)
    return histgram_call<bf16_t>("fedagg_histgram_16", reinterpret_cast<const bf16_t* const*>(d_src), K,
                                 static_cast<const bf16_t*>(d_ref), d_hist, d_chunks, n_chunks, d_out, d_work,
                                 work_len, stream);
  if (dtype == FEDAGG_DT_F16)
    return histgram_call<f16_t>("fedagg_histgram_16", reinterpret_cast<const f16_t* const*>(d_src), K,
                                static_cast<const f16_t*>(d_ref), d_hist, d_chunks, n_chunks, d_out, d_work, work_len,
                                stream);
  return set_error(FEDAGG_EINVAL, "fedagg_histgram_16: dtype must be FEDAGG_DT_BF16 or FEDAGG_DT_F16");
}

}  // extern "C"
