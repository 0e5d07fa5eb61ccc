// histgram.hip — the fused history update and uncentred Gram of the
// "foolsgold_cos" defense (gfx950), exported through include/fedagg.h and
// linked into libfedagg.so beside robust.hip.
//
//   fedagg_histgram_f32   a_i = fl(fl(x_i - ref) + h_i), h_i = a_i in place,
//                         d_out = A A^T (K x K, fp64, both triangles), K <= 128
//
// FoolsGold judges the cosine of every pair of clients' ACCUMULATED updates, so
// a round has to add this round's update x_i - ref to each client's history
// row and then needs the inner products of all the histories.  Composed from
// the other kernels that is a torch add over K rows (read x, ref, h; write h),
// a Gram pass and a norm pass over h: five row sets of traffic.  Here one pass
// reads x and h, writes h and multiplies the fresh a while it is in registers:
// three row sets.
//
// The engine is robust.hip's pairgram_split8_kernel: 8 waves, one block per
// CU, 64-column stages, each value split exactly into three bf16 planes
// a = h + m + l (rows of kSplitRB bytes, double-buffered), six
// v_mfma_f32_16x16x32_bf16 per tile and 32 columns, the raw rows prefetched two
// stages ahead, one barrier per stage, fp32 over kSplitFold stages and fp64
// across, its row-pair tile schedule at every group count (as robust16.hip;
// the 2 x 2 group blocks the fp32 Gram runs at 8 groups save LDS fragment
// reads, and this kernel waits for HBM three times as long per stage) and the
// same partial layout.  What differs is the front of a stage:
//
// * No centre.  Distances are translation invariant and the Gram kernel
//   subtracts the stage's column mean to condition them; cosines are about the
//   origin, and an uncentred Gram entry's error, ~1e-7 |a_i||a_j|, is already
//   an absolute ~1e-7 in the cosine.  So there are no column sums, no sSum
//   exchange and no LDS phase before the split: a lane splits what it loaded.
// * Each lane prefetches, beside its LPW client pieces, the matching 16-byte
//   pieces of its LPW history rows (non-temporal: read once) and its piece of
//   ref (a plain load: all of the block's waves read the same 256 bytes).
//   That is a second register set per stage in flight; the block runs two
//   waves per SIMD, so it fits the 256-VGPR budget without spilling.
// * When a stage is split, the lane forms a, stores its piece into the history
//   row (non-temporal; a column belongs to one chunk and so to one block, and
//   within the block to the one lane that loaded it: the update in place is
//   race-free) and splits the same registers into the planes.  A partial
//   stage loads and stores by element under fetch's masks; rows past K are
//   zero in the planes and are never stored.
//
// The kernel, its finish and the call are csrc/histgram.h's, a template on the
// client rows' element type that histgram16.hip instantiates for bf16 / f16
// rows; this unit instantiates it for fp32 rows.
//
// This unit is compiled without packed fp32 VALU instructions (build.py,
// UNIT_FLAGS, which gives the reason); its VALU work is single subtracts, adds
// and converts.

#include "histgram.h"

extern "C" {

// fedagg_robust_work_len(FEDAGG_WORK_HISTGRAM, K, n_chunks), for robust.hip
__attribute__((visibility("hidden"))) int64_t fedagg_histgram_work_len_internal(int32_t K, int64_t n_chunks) {
  if (K > kGramMax) return -1;
  return int64_t(histgram_groups(n_chunks, 0, 0)) * gram_tiles(K) * 256;
}

int fedagg_histgram_f32(const float* const* d_src, int32_t K, const float* d_ref, float* const* d_hist,
                        const int64_t* d_chunks, int64_t n_chunks, double* d_out, double* d_work, int64_t work_len,
                        fedagg_stream_t stream) {
  return histgram_call<float>("fedagg_histgram_f32", d_src, K, d_ref, d_hist, d_chunks, n_chunks, d_out, d_work,
                              work_len, stream);
}

}  // extern "C"
