// The index arithmetic of a planner slice of a recording (fsdp_submit_sequence, include/fsdp.h): one place for the host
// library, the staging kernels of sequence_kernel.h and a stand-alone test program (tests/test_sequence_tickets_cpu.py).
//
// A recording holds `total` planners x n_steps steps, step-major: recording frame r = step * total + planner.  A call plans the
// planners [lo, lo + n): its frame f = step * n + p is recording frame step * total + lo + p.  The frames of one step are
// adjacent in the recording, so a slice is n_steps segments, each contiguous in the offsets, the cone rows, the poses and the
// records; the segments themselves are `total` frames apart.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) && !defined(FSDP_EMU)
#define FSDP_SLICE_HD __host__ __device__ __forceinline__
#else
#define FSDP_SLICE_HD inline
#endif

namespace fsdp {

struct SeqSlice {
  int n, n_steps, lo, total;  // planners of the call, steps, first planner, planners of the recording
  FSDP_SLICE_HD bool whole() const { return lo == 0 && total == n; }
  FSDP_SLICE_HD long long frames() const { return (long long)n * n_steps; }
};

// where a slice may lie: 1 <= n, 0 <= lo, lo + n <= total (no overflow: compared in 64 bits)
FSDP_SLICE_HD bool seq_slice_valid(const SeqSlice& s) {
  return s.n >= 1 && s.n_steps >= 1 && s.lo >= 0 && (long long)s.lo + s.n <= (long long)s.total;
}

// call frame (step, p) -> recording frame
FSDP_SLICE_HD long long seq_rec_frame(const SeqSlice& s, long long step, long long p) { return step * s.total + s.lo + p; }
// call frame f -> recording frame
FSDP_SLICE_HD long long seq_rec_of_call(const SeqSlice& s, long long f) {
  const long long step = f / s.n;
  return seq_rec_frame(s, step, f - step * s.n);
}
// recording frame r -> the call's frame, or -1 where r belongs to a planner outside the slice (or lies beyond the recording)
FSDP_SLICE_HD long long seq_call_of_rec(const SeqSlice& s, long long r) {
  if (r < 0) return -1;
  const long long step = r / s.total, p = r - step * s.total - s.lo;
  if (step >= s.n_steps || p < 0 || p >= s.n) return -1;
  return step * s.n + p;
}

// One segment per step: src = its first cone row in the recording (the offset of the slice's first frame of the step), dst = its
// first row in the call's dense device copy (the rows of the earlier segments).
struct SeqSeg {
  int32_t src, dst;
};

// The segments of slice s from the recording's offsets (n_steps * total + 1 entries, any base): seg[0 .. n_steps) and, in
// seg[n_steps].dst, the slice's cone rows (seg[n_steps].src = 0).  *max_cones: most cones in a frame of the slice.
// Returns 0, or 1 = an offset below 0, 2 = offsets that decrease inside a segment, 3 = more than 2^31 - 1 rows.
inline int seq_slice_segments(const SeqSlice& s, const int32_t* off, SeqSeg* seg, int* max_cones) {
  long long rows = 0;
  int most = 0;
  for (int t = 0; t < s.n_steps; t++) {
    const int32_t* o = off + seq_rec_frame(s, t, 0);
    if (o[0] < 0) return 1;
    seg[t].src = o[0];
    seg[t].dst = (int32_t)rows;
    for (int p = 0; p < s.n; p++) {
      const long long d = (long long)o[p + 1] - o[p];  // (in 64 bits: a corrupt offset must not overflow before it is refused)
      if (d < 0) return 2;
      if (d > most) most = (int)d;  // (o[p] >= o[0] >= 0: fits)
    }
    rows += (long long)o[s.n] - o[0];
    if (rows > 0x7fffffff) return 3;
  }
  seg[s.n_steps].src = 0;
  seg[s.n_steps].dst = (int32_t)rows;
  if (max_cones) *max_cones = most;
  return 0;
}

// offset of call frame (step, p) in the dense copy, given its segment and the recording's offsets
FSDP_SLICE_HD long long seq_dense_offset(const SeqSeg& g, int32_t rec_offset) { return (long long)g.dst + ((long long)rec_offset - g.src); }

}  // namespace fsdp
