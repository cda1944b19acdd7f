// The seam between the host library (fsdp_lib.hip) and the chain kernels of a sequence pass (sequence_kernel.h), which are
// compiled as a translation unit of their own (sequence_lib.hip).
#pragma once

#include <stdint.h>

#ifndef FSDP_EMU
#include <hip/hip_runtime.h>
#endif

#include "sequence_slice.h"  // SeqSlice, SeqSeg
#include "sort_cache.h"  // SortCacheView, SeqSpecRec

namespace fsdp {
struct MatchOut;
struct PathOut;
struct SortOut;
// the list block of a sequence pass: [0] heads appended, [1] frames planned again (a 16-byte header, zeroed by one memset per
// pass), then (frame, predecessor) per head: SEQ_LIST + 2 * frames ints
constexpr int SEQ_HEADS = 0, SEQ_REPLANNED = 1, SEQ_LIST = 4;
}  // namespace fsdp

#ifndef FSDP_EMU  // (the host emulator launches the kernels itself: tests/emu/emu_sequence.cpp)
struct fsdp_seq_launch_args {
  int n_planners, n_steps;
  const double* poses;
  const fsdp::MatchOut* matched;
  const double* initial_prev;  // (n_planners, PATH_POINTS, 4) or NULL
  const double* gpath;
  int n_gpath;
  double* arena;
  fsdp::PathOut* out;
  int* seq;                // the list block
  double* final_prev;      // (n_planners, PATH_POINTS, 4)
  int32_t* replanned_out;  // device view of the pass trailer's spare word
  const fsdp::Params* prm;
};
// header memset -> seq_mark_kernel -> seq_chain_kernel -> seq_final_kernel on `stream`.  Weak: a library built from fsdp_lib.hip
// alone (the variant builds of tools/) has no sequence kernels, and fsdp_plan_sequence says so.
extern "C" __attribute__((weak)) void fsdp_seq_launch(hipStream_t stream, const fsdp_seq_launch_args* a);
// Its first step (header memset -> seq_mark_kernel) and its last (seq_final_kernel) alone: a sequence pass with per-frame global
// paths puts seq_chain_table_kernel between them (sequence_table_launch.h); gpath / n_gpath are not read.
extern "C" __attribute__((weak)) void fsdp_seq_launch_mark(hipStream_t stream, const fsdp_seq_launch_args* a);
extern "C" __attribute__((weak)) void fsdp_seq_launch_final(hipStream_t stream, const fsdp_seq_launch_args* a);

// A planner slice of a recording (fsdp_submit_sequence with page-locked arrays): seq_slice_in_kernel in front of the pass,
// seq_slice_out_kernel behind its assembly.  Every src of the first and every dst of the second is the device view of a
// page-locked host array, already advanced to the slice's first frame (planner lo of step 0) or first row.
struct fsdp_seq_slice_in_args {
  fsdp::SeqSlice s;
  const fsdp::SeqSeg* seg;   // n_steps + 1 segments (the ticket's page-locked block)
  const int32_t* src_off;    // cone_offsets + lo
  const double* src_cones;   // cones_xyt + 3 * cone_base: the lowest row any segment reads
  const double* src_poses;   // poses + 4 * lo
  const double* src_init;    // initial_prev + lo rows, or NULL
  int32_t cone_base;
  long long src_rows;        // rows behind src_cones that the segments span
  long long rows;            // cone rows of the slice = seg[n_steps].dst
  int32_t* dst_off;          // the slot's dense device copies: offsets from 0 without gaps, call order (step-major)
  double* dst_cones;
  double* dst_poses;
  double* dst_init;
};
struct fsdp_seq_slice_out_args {
  fsdp::SeqSlice s;
  int rec_bytes;             // sizeof(fsdp_frame_result) or sizeof(fsdp_compact_result): multiples of 8
  const void* src_records;   // the slot's result block, dense
  void* dst_records;         // results + lo records
  const double* src_final;   // the slot's final_prev rows
  double* dst_final;         // final_prev + lo rows, or NULL
};
extern "C" __attribute__((weak)) void fsdp_seq_launch_slice_in(hipStream_t stream, const fsdp_seq_slice_in_args* a);
extern "C" __attribute__((weak)) void fsdp_seq_launch_slice_out(hipStream_t stream, const fsdp_seq_slice_out_args* a);

// fsdp_plan_sequence_cached (sequence_cache_kernel.h, compiled as sequence_cache_lib.hip): the speculative sorting kernels in the
// place of the plain ones, and the cache chain between the sorting results and the matching.
struct fsdp_seqc_launch_args {
  int n_planners, n_steps;
  const int32_t* off;  // the batch as the sorting stage plans it (filtered when use_unknown_cones = 0)
  const double* cones;
  const double* poses;
  fsdp::SortOut* sorted;
  int* big;             // the big route's list
  void* big_state;      // SortSharedBig blocks, `big_blocks` of them
  int big_blocks;
  bool small;           // no frame holds more than 128 cones
  const fsdp::Params* prm;
  fsdp::SeqSpecRec* rec;  // (frames)
  fsdp::SortCacheView cache;  // the call reads `prev`, writes `next` and, for the last step, `hits`; base 0: frame f is planner f % n_planners
  int8_t* hits;        // (frames, 2)
  int32_t* resorted;   // (planners)
};
extern "C" __attribute__((weak)) void fsdp_seqc_launch_sort(hipStream_t stream, const fsdp_seqc_launch_args* a);
extern "C" __attribute__((weak)) void fsdp_seqc_launch_sort_big(hipStream_t stream, const fsdp_seqc_launch_args* a);
// seq_cache_mark_kernel -> seq_cache_resolve_kernel
extern "C" __attribute__((weak)) void fsdp_seqc_launch_chain(hipStream_t stream, const fsdp_seqc_launch_args* a);
#endif
