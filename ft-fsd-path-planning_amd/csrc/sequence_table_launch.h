// The seam between the host library (fsdp_lib.hip) and the TABLE twin of seq_chain_kernel (sequence_table_kernel.h), which is compiled
// as a translation unit of its own (sequence_table_lib.hip), like the path wrappers' twins behind gpath_table_launch.h: every earlier
// kernel compiles to what it was.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "sequence_launch.h"  // fsdp_seq_launch_args: the pass as the chain kernels take it

// seq_chain_table_kernel on `stream`, between fsdp_seq_launch_mark and fsdp_seq_launch_final (sequence_launch.h): the arguments of
// the plain chain but for its pair (a->gpath, a->n_gpath are not read), plus the context's table (device memory) and the pass's
// ids, dense in the call's frame order: device memory, or the device view of page-locked host memory.
// Weak: a library built without sequence_table_lib.hip has no such kernel, and fsdp_plan_sequence_paths says so.
extern "C" __attribute__((weak)) void fsdp_seqt_launch_chain(hipStream_t stream, const fsdp_seq_launch_args* a, const double* table_xy,
                                                             const int32_t* table_off, int n_paths, const int32_t* ids);
