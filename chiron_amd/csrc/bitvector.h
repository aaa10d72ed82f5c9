// The column step of the bit-parallel edit-distance automaton (Myers 1999, "advance_block", in Hyyro's form), shared by the edit
// distance of ctc_loss.hip (blocks of 64 truth positions chained through hin / hout) and the pattern search of demux.hip (one
// block a pattern, the first row free: hin = 0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chiron {

// One column of the DP for one 64-row block: Pv / Mv are the block's vertical +1 / -1 differences, Eq the rows whose base matches
// the column's, hin the horizontal delta entering the block at its first row, `high` the bit of its last row; returns the
// horizontal delta leaving that row.  A block of exactly 64 rows relies on the wrap of the 64-bit add.
__device__ __forceinline__ int advance_block(uint64_t& Pv, uint64_t& Mv, uint64_t Eq, int hin, uint64_t high) {
  const uint64_t Xv = Eq | Mv;
  if (hin < 0) Eq |= 1ull;
  const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  uint64_t Ph = Mv | ~(Xh | Pv);
  uint64_t Mh = Pv & Xh;
  int hout = 0;
  if (Ph & high) hout += 1;
  if (Mh & high) hout -= 1;
  Ph <<= 1;
  Mh <<= 1;
  if (hin < 0) Mh |= 1ull;
  else if (hin > 0) Ph |= 1ull;
  Pv = Mh | ~(Xv | Ph);
  Mv = Ph & Xv;
  return hout;
}

}  // namespace chiron
