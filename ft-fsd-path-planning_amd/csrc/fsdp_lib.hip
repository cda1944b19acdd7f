// libfsdp_hip.so — host side of the C ABI declared in include/fsdp.h.
//
// A context owns one GPU: up to FSDP_MAX_OVERLAP *pass slots*, each with its own HIP stream, its own copy of a batch's
// inputs, its own intermediates and its own result block — so several DIFFERENT batches are in flight at once
// (fsdp_submit / fsdp_collect: H2D, the kernels of a pass and the D2H of one batch run on the slot's stream and overlap
// with the other slots') — plus one resident batch that fsdp_run / fsdp_time_runs replay (the benchmark's form).
// Launch geometry: one 64-lane workgroup (= one wavefront) per frame or per 2 / 4 / 8 / 16 frames, so a 4096-frame batch
// is thousands of workgroups over 256 CUs / 8 XCDs (consecutive frames land on consecutive XCDs; frames are independent,
// no inter-workgroup traffic).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/fsdp.h"
#include "sort_kernel.h"
#include "match_kernel.h"
#include "path_kernel.h"
#include "skidpad_kernel.h"
#include "assemble_kernel.h"
#include "filter_kernel.h"
#include "fsdp_comm.h"
#include "sort_rank_kernels.h"  // (behind the pass kernels: the kernels in front of it keep their order in the code object)
#include "sequence_launch.h"    // (the chain kernels of fsdp_plan_sequence are a translation unit of their own: sequence_lib.hip)
#include "host_buffers.h"       // (no kernels: DeviceBuf / PinnedBuf and the stores a slot and a context own)
#include "device_io_launch.h"   // (the kernels of a device ticket are a translation unit of their own: device_io_lib.hip)
#include "skid_device_launch.h"  // (the kernels of a skidpad device ticket live in that unit too)
#include "sort_history_launch.h"  // (the history instantiations of the sorting kernels likewise: sort_history_lib.hip)
#include "gpath_table_launch.h"   // (the path wrappers of a pass with per-frame global paths likewise: gpath_table_lib.hip)
#include "sequence_table_launch.h"  // (the chain kernel of a sequence pass with per-frame global paths likewise: sequence_table_lib.hip)

using namespace fsdp;

static_assert(FSDP_MAX_LEN == MAX_LEN && FSDP_MAX_MATCH == MAX_MATCH && FSDP_PATH_POINTS == PATH_POINTS &&
                  FSDP_MAX_NEIGHBORS == KNN && FSDP_MAX_CONES == BIG_CONES,
              "header/device constant mismatch");

static thread_local std::string g_create_error;

constexpr int SORT_BIG_BLOCKS = 32;

// A stream or an event that is destroyed with its owner (move-only, handed to the runtime as the handle it holds)
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
  Handle& operator=(Handle&& o) noexcept {
    std::swap(h, o.h);
    return *this;
  }
  ~Handle() {
    if (h) (void)Destroy(h);
  }
  operator H() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;

// one batch of frames as the caller hands it over (host memory, checked by check_batch).  cone_offsets[0] = off[0] >= 0: the
// batch's cones are the rows [off[0], off[n]) of `cones` — a slice of a larger batch is handed over by pointing at its offsets
// (include/fsdp.h)
struct Batch {
  int n = 0;
  const int32_t* off = nullptr;
  const double* cones = nullptr;
  const double* poses = nullptr;
  const double* prev = nullptr;  // optional previous paths (n,40,4)
  size_t total = 0;              // cone rows: off[n] - off[0]
  int max_cones = 0;             // most cones in a frame
  // frames [lo, hi) (max_cones stays the whole batch's: every part runs the kernels the whole would)
  Batch slice(int lo, int hi) const {
    return Batch{hi - lo, off + lo, cones, poses + 4 * (size_t)lo, prev ? prev + (size_t)PATH_POINTS * 4 * (size_t)lo : nullptr,
                 (size_t)(off[hi] - off[lo]), max_cones};
  }
};

// Tickets queue up behind each other on a slot's stream (stream order protects the slot's buffers), so a slot always has
// its next batch waiting when the current one ends — the host's collect / submit round trip is off the GPU's critical path.
constexpr int SLOT_QUEUE = 2;   // tickets per slot
constexpr int N_TRAILERS = SLOT_QUEUE + 1;  // pass trailers per slot: one per ticket entry (a ticket may stay uncollected while the
                                            // slot's other entry turns over many times) + one for resident / blocking passes

// one pass slot: a stream, the inputs of the batch submitted to it, the intermediates of a pass and its results
struct Work {
  int index = 0;
  Stream stream;  // (first: whatever the slot owns is freed before its stream goes; fsdp_destroy / release_slot synchronise it before)
  InputStore<> in;
  PassStore<> buf;   // the intermediates of a pass and its result block
  bool skid_attempted = true;             // ... which ran for that step (not once every planner is relocalized)
  DeviceBuf<SortSharedBig> d_sort_big;    // frame states of sort_big_kernel, allocated when the route is first needed
  FilterStore<> filt;                     // use_unknown_cones = False
  SeqStore<> seq_buf;                     // fsdp_plan_sequence
  SeqCacheStore<> seqc_buf;               // fsdp_plan_sequence_cached
  PinnedBuf<PassTrailer> h_trailer;  // N_TRAILERS of them: pinned, host-coherent, written by assemble_kernel: a ticket's entry
                                     // index, or SLOT_QUEUE (resident / blocking passes)
  int seq = 0;                       // passes launched on this slot
  // the most recent pass launched on the slot (verify_pass re-runs it with the route kernels when they were needed)
  const InputStore<>* pass_in = nullptr;
  bool ran_big = false, ran_retry = false, unverified = false, pass_skid = false;
  int gang_members = 0, gang_first = 0, gang_n = 0;  // ... was a ganged pass of so many members; its last member's first frame and frames
  // A sequence pass (fsdp_plan_sequence*, fsdp_submit_sequence*) as its ticket describes it: the ticket's pass — and the rerun
  // fsdp_collect issues when the pass lacked a route — resolves the planners' previous-path chains between the path stage and the
  // assembly.  enqueue_ticket hands it to the launches inside the pass's description (Pass::sq): nothing about the pass in progress
  // is kept on the context.  The pointers are the caller's, valid and untouched until fsdp_collect like the batch's.
  struct SeqPass {
    bool on = false;
    SeqSlice s = {};           // planners [lo, lo + n) of a recording of `total`, n_steps steps (whole call: lo = 0, total = n)
    bool cached = false;       // fsdp_plan_sequence_cached: the speculative sorting kernels and the cache chain (never with Ticket::cache_lo)
    const char* who = "";      // the entry point, for error texts
    const int32_t* off = nullptr;  // the whole recording's arrays (a slice's frames are not contiguous in them: t.batch holds counts only)
    const double* cones = nullptr;
    const double* poses = nullptr;
    const double* init = nullptr;   // the slice's first initial_prev row, or NULL
    double* final_prev = nullptr;   // the slice's first final_prev row, or NULL
    long long* n_replanned = nullptr;
    const int32_t* path_ids = nullptr;  // fsdp_*_sequence_paths: the whole recording's path ids (n_steps * total, step-major), or NULL
    // set by enqueue_ticket
    double* final_dev = nullptr;    // where seq_final_kernel writes: page-locked host memory (the caller's rows or the ticket's h_fin), or the slot's d_seq_final
    bool fin_staged = false;        // final_prev goes through h_fin (fsdp_collect copies it out)
  };
  // A device ticket's pass (fsdp_submit_device): the caller's arrays in the memory of the context's GPU.  The pass runs with both
  // route kernels and is never repeated, so what it wrote is final when the ticket's event fires.
  struct DevPass {
    bool on = false;
    int cap = 0;                       // cone_capacity: rows per frame of `cones`
    const int32_t* counts = nullptr;
    const double* cones = nullptr;
    const double* poses = nullptr;
    const double* prev = nullptr;      // or NULL
    double* paths = nullptr;
    int32_t* status = nullptr;
    double* next_prev = nullptr;       // or NULL; may be `prev`
    fsdp_compact_result* records = nullptr;  // or NULL
    // a skidpad device ticket (fsdp_skidpad_submit_device): its step's records, or NULL
    fsdp_skidpad_info* skid_info = nullptr;
    fsdp_path_result* skid_records = nullptr;
    const int32_t* path_ids = nullptr;  // fsdp_submit_device_paths: the frames' path ids (n), or NULL
  };
  // tickets of fsdp_submit / fsdp_skidpad_submit / fsdp_submit_sequence queued on this slot's stream (id -1: free entry).  A ticket
  // holds the whole description of its pass: enqueue_ticket launches the first pass and fsdp_collect's rerun from it alone.
  struct Ticket {
    long long id = -1;
    bool skid = false;
    bool pending = false;  // skidpad step whose path kernel waits for the rest of its group (flush_skid)
    int seq = 0;                       // the slot's pass counter of this ticket's pass (checked against its trailer)
    bool ran_big = false, ran_retry = false;
    long long in_flight = 0;           // frames on the GPU the pass was planned for (launch_path; a repeated pass keeps them)
    // the caller's buffers: valid and untouched until fsdp_collect (a pass that has to be repeated reads them again)
    Batch batch;
    fsdp_frame_result* user_results = nullptr;
    fsdp_skidpad_info* user_info = nullptr;
    bool via_stage = false;                // results go through h_stage (the caller's buffer is pageable)
    bool compact = false;                  // user_results holds compact records: fsdp_path_result (skidpad step) or
                                           // fsdp_compact_result (fsdp_submit_compact)
    size_t rec_bytes() const { return !compact ? sizeof(fsdp_frame_result) : (skid ? sizeof(PathOut) : sizeof(fsdp_compact_result)); }
    PinnedBuf<fsdp_frame_result> h_stage;  // pinned + mapped: the assembly kernel writes a pageable caller's results here
    PinnedBuf<char> h_in;                  // pinned + mapped: a small pageable batch is packed here and read by the sorting kernel itself
    PinnedBuf<SkidInfo> h_info;            // pinned
    PinnedBuf<SeqSeg> h_seg;               // pinned + mapped: the per-step segments of a planner slice (seq_slice_in_kernel reads them)
    PinnedBuf<double> h_fin;               // pinned + mapped: seq_final_kernel writes a pageable caller's final_prev rows here
    SeqPass sq;                            // a sequence ticket's pass
    int cache_lo = -1;                     // >= 0: a chunk of a lock-step call that advances the sorting cache (the _cached sorting
                                           // kernels); its frame 0 is this planner
    DevPass dev;                           // a device ticket's pass
    const int32_t* path_ids = nullptr;     // fsdp_submit_paths: the caller's path ids (n), checked against the table by the submit; a
                                           // repeated pass reads them again like the batch itself
    PinnedBuf<int32_t> h_ids;              // pinned + mapped: pageable path ids are staged here and read by the path kernels themselves
    PinnedBuf<int32_t> h_bad;              // pinned + mapped: the lowest frame of a device ticket whose count was out of range, or -1;
                                           // [1], a skidpad device ticket: 1 when a planner was not relocalized after the step;
                                           // [2], fsdp_submit_device_paths: the lowest frame whose path id was out of range, or -1
    unsigned reloc_epoch = 0;              // a skidpad step: fsdp_ctx::skid_reloc_epoch when it was submitted
    Event after;                           // a device ticket: recorded on the producer's stream, waited for by the slot's
    Event done;                            // recorded behind the ticket's last command
    // the entry is free again: what the caller owned, and what described his pass, is forgotten
    void release() {
      id = -1;
      user_results = nullptr;
      user_info = nullptr;
      compact = false;
      sq = SeqPass();
      dev = DevPass();
      cache_lo = -1;
      path_ids = nullptr;
    }
  } tk[SLOT_QUEUE];
};

struct fsdp_ctx {
  int device = 0;
  int mission = 0;
  hipStream_t stream = nullptr;  // = slot[0].stream
  Event ev[8];
  std::string err;
  Work slot[FSDP_MAX_OVERLAP];
  InputStore<> res;       // the resident batch of fsdp_upload (every slot's fsdp_run pass reads it)
  size_t res_rows = 0;    // ... and its cone rows
  bool resident = false;  // res describes a batch fsdp_run may plan
  bool res_checked = false;  // a verified pass over the resident batch has set expect_big / expect_retry exactly
  // The most recent pass (launch_pass, a skidpad step), what fsdp_download, fsdp_resident_frames and fsdp_debug_* read: they
  // return data of exactly this pass or fail.  slot < 0: none, or its buffers were released / reused since.
  struct LastPass {
    int slot = -1;
    int n = 0;               // its frames
    bool in_result = false;  // its results are in the slot's result block (an fsdp_run / fsdp_time_runs pass)
    bool whole = false;      // it covered the whole call (not a chunk of a blocking call)
    int offset = 0;          // a ganged pass: the last member's first frame in the slot's blocks (n = that member's frames)
  } last;
  DeviceBuf<double> d_default_path;  // (40,4)
  Params params;                     // configuration constants (fsdp_params) ...
  DeviceBuf<Params> d_params;        // ... and their device copy, read by every kernel
  DeviceBuf<double> d_chord;         // (40,2) almost-straight chord (trivial path of the skidpad mission)
  DeviceBuf<double> d_gpath;         // PathPlanner.global_path (n_gpath,2), or NULL
  int n_gpath = 0;
  // fsdp_set_global_path_table: n_gpt polylines one behind the other, path k the points [off[k], off[k + 1]); read only by a pass
  // that carries path ids (fsdp_submit_paths, fsdp_submit_device_paths)
  DeviceBuf<double> d_gpt_xy;        // (off[n_gpt], 2); at least one point's room, so that an empty entry still has an address
  DeviceBuf<int32_t> d_gpt_off;      // (n_gpt + 1)
  int n_gpt = 0;
  // fsdp_set_option (include/fsdp.h): what a test or a measurement may pin; 0 = the library's own choice
  int force_path_mode = 0;    // "path_mode": 0 = by batch size; 1 = one kernel (64 lanes per frame); 2 = three kernels
  int fit_g = 4;              // "fit_g": lanes per frame of fit_kernel when frames are packed: 4 = exactly the Givens quad, sixteen
                              // frames per wavefront (+1.6 % frames/s over 8 since the basis records are 32 bytes)
  int force_pack = 0;         // "pack": 0 = by frames in flight; 1 = 4 frames per wavefront; 2 = packed
  std::string stage_names;    // kernels of the most recent pass, comma-separated
  bool profile_sort = false;  // profiling build: which kernel fsdp_profile_path runs
  int overlap = 1;
  int hw_queues = 4;          // "hw_queues": hardware queues the runtime grants this process (HIP's default; the library reads no environment)
  int gang = 0;               // "gang": members per ganged pass of fsdp_time_runs: 0 = by overlap and hw_queues; 1 = never; k > 1 = k
  size_t gang_grown_from = 0;  // frames slot 0 held before it first grew for ganged passes: fsdp_set_overlap sizes new slots by this
                               // or by the resident batch, whichever is more, instead of by the grown slot 0
  unsigned turn = 0;
  long long next_ticket = 0;
  int last_ticket_slot = -1;  // slot of the most recent ticket
  int outstanding = 0;  // tickets submitted and not yet collected
  // The route kernels (sort_big_kernel, path_retry_kernel) are launched only when a pass is expected to need them: a pass
  // that turns out to need a kernel it did not get is re-run with it before anybody sees its results (verify_pass), and
  // from then on the kernel is part of every pass until ROUTE_DECAY (4096) passes in a row came back with an empty list.
  bool expect_big = false, expect_retry = false;
  int retry_hint = 0;  // the longest retry list a recent pass reported (decays by an eighth per pass): sizes path_retry_kernel's grid
  int clean_big = 0, clean_retry = 0;
  bool poison = false;        // "poison": every pass first fills its intermediates and scratch with 0xFF bytes (tests: no result depends on what a buffer held before)
  int plan_chunks = 0;        // "plan_chunks": most chunks a blocking fsdp_plan_batch call is pipelined in (0: up to 4; 1: never cut)
  bool always_route = false;  // "always_route": both route kernels with every pass (tests: results never depend on the prediction)
  long long reruns = 0;  // passes re-run by verify_pass (diagnostics: fsdp_route_stats)
  bool no_sort128 = false;  // "no_sort128": always the 255-cone state of the sorting kernel (tests)
  std::vector<Event> tev;  // per-launch timing events of fsdp_time_runs
  int timed_iters = 0, timed_stages = 0;  // the most recent fsdp_time_runs (fsdp_time_results reads its events)
  bool time_main_only = false;            // fsdp_time_detail: events only around the path stage's main kernel
  bool time_kernel_clock = false;         // fsdp_time_detail bit 1: the refit kernel's launches note their own start / end clock
  std::vector<unsigned> tev_recorded;     // per pass of the most recent fsdp_time_runs: which of its events were recorded
  std::vector<int> tev_members;           // ... and how many passes its launches cover: a gang's members at its first pass, 0 at the others
  DeviceBuf<unsigned long long> d_kclock;  // [2 * iters]: first-wavefront-start | last-wavefront-end of the refit kernel, per timed pass
  int gang_primed[FSDP_MAX_OVERLAP] = {};  // slot i has executed a ganged pass of so many members since `primed` was last cleared
  bool primed[FSDP_MAX_OVERLAP] = {};     // slot i has executed a pass of the current packing (its stream / hardware queue is set up)
  // skidpad mission
  DeviceBuf<double> d_table, d_noise;
  SkidTables tables = {};
  fsdp_comm::Comm comm;  // RCCL communicator of this rank (fsdp_comm_init), or none
  double skid_consts[5] = {};  // reference centres (right xy, left xy) + table spacing, computed on the device
  bool have_tables = false;
  DeviceBuf<SkidState> d_skid, d_skid_backup;
  DeviceBuf<uint32_t> d_skid_sync;   // [0] ticket counter of skid_path_kernel, [1 + i] steps instance i has published
  uint32_t skid_ticket_base = 0;
  int skid_step_no = 0;              // steps submitted since fsdp_skidpad_reset
  bool skid_all_reloc = false;       // a collected step reported every planner relocalized: cones have no reader any more
  unsigned skid_reloc_epoch = 0;     // counts the resets (of all planners, or through a device step's mask): a step submitted before
                                     // one says nothing about the planners after it, whenever it is collected
  int skid_group_env = 0;            // "skid_group": steps per launch when the caller submits ahead (0: chosen from the instance count)
  // fsdp_skidpad_time_groups: HIP events around the packed kernels of every group of steps (select | prep | fit | finish | commit)
  bool skid_time_groups = false;
  std::vector<Event> skid_group_ev;       // six per group
  std::vector<int> skid_group_frames;     // (instance, step) pairs per group
  std::string skid_group_names;
  int skid_pack_min = 2048;          // (instance, step) pairs from which a group goes through the packed kernels (one step of
                                     // 2048 planners: 1.49 M frames/s packed, 1.40 M a wavefront each; 1024: 0.98 / 1.08 M)
  SkidGroupStore<> group;            // workspace of a group that goes through the packed kernels
  int skid_pending[SKID_GROUP_MAX] = {};  // slots whose step waits for its group's launch, oldest first
  int n_skid_pending = 0;
  int n_instances = 0;
  // pinned host staging of the stage-level entry points
  PinnedBuf<SortOut> h_sort;
  PinnedBuf<MatchOut> h_match;
  PinnedBuf<PathOut> h_path;
  // the sorting cache (fsdp_sort_cache_reset, sort_cache.h): one entry per planner in each of two buffers; the kernels of a
  // call read buffer cache_cur and write the other, and the call swaps them once it has succeeded
  int n_cache = 0;
  int cache_cur = 0;
  SortCacheStore<> cache;                     // the two buffers, their layout and the planners' regions
  std::vector<int8_t> cache_hits;             // codes of the most recent call
  // (no field says what the call in progress is: a pass is described by the Pass its caller builds — for a ticket, from the ticket)
};
// (an empty route launch costs a stream ~1 % of a pass; a pass repeated because the kernel was missing costs a whole pass and
// stalls the caller's collect: once needed, a route stays for a long time)
constexpr int ROUTE_DECAY = 4096;

#define HIP_TRY(ctx, call)                                                                       \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
      return 2;                                                                                  \
    }                                                                                            \
  } while (0)

// Synchronous copies go through the context's own stream: the library never touches the null stream (every stream the
// process uses takes one of the runtime's GPU_MAX_HW_QUEUES hardware queues, and overlapped passes need theirs).
static hipError_t copy_sync(fsdp_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(c->stream);
}

// stream, trailer and intermediates of slot w for passes of up to n frames
static int ensure_work(fsdp_ctx* c, Work& w, int n) {
  if (!w.stream) HIP_TRY(c, hipStreamCreateWithFlags(&w.stream.h, hipStreamNonBlocking));
  if (!w.h_trailer) {
    HIP_TRY(c, w.h_trailer.reserve(N_TRAILERS, 0, Pin::MappedCoherent));
    memset(w.h_trailer, 0, sizeof(PassTrailer) * N_TRAILERS);
  }
  if ((size_t)n <= w.buf.frames()) return 0;
  HIP_TRY(c, hipStreamSynchronize(w.stream));
  if (c->last.slot == w.index) c->last = fsdp_ctx::LastPass();  // (its results and scratch are about to go)
  HIP_TRY(c, w.buf.reserve((size_t)n, c->mission == 2));
  // the list counters are zero between passes: assemble_kernel resets them at the end of every pass
  HIP_TRY(c, hipMemsetAsync(w.buf.d_big, 0, sizeof(int), w.stream));
  HIP_TRY(c, hipMemsetAsync(w.buf.d_retry, 0, sizeof(int), w.stream));
  return 0;
}
// the slot gives back its buffers and its stream (nothing of it is in flight)
static void release_slot(Work& w) {
  if (w.stream) (void)hipStreamSynchronize(w.stream);
  const int idx = w.index;
  w = Work();
  w.index = idx;
}

// p as the GPU addresses it if p is page-locked host memory (fsdp_host_alloc, fsdp_host_register: mapped into the device's
// address space, reachable by kernels and by asynchronous copies), else NULL
static void* device_view(const void* p) {
  if (!p) return nullptr;
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // (an unregistered pointer is an error in older runtimes: not ours to keep)
    return nullptr;
  }
  return a.type == hipMemoryTypeHost ? a.devicePointer : nullptr;
}
// the whole extent [p, p + bytes) is page-locked and one mapping: a view that starts inside a registered range and runs past
// its end would let a kernel read / write unmapped host memory (a device fault instead of an error code) — such a buffer
// takes the pageable path (round-3 advisor)
static bool is_pinned(const void* p, size_t bytes) {
  const char* dv = (const char*)device_view(p);
  if (!dv) return false;
  if (bytes <= 1) return true;
  const char* de = (const char*)device_view((const char*)p + bytes - 1);
  return de != nullptr && de - dv == (ptrdiff_t)(bytes - 1);
}
// Where a ticket's pass writes for the caller: `user` itself if its `bytes` are page-locked over their whole extent (the kernels
// write it over PCIe), else the ticket's own mapped block of `count` T's, grown with room for `want` (what it held is gone: nothing
// queued may use it any more; *staged: fsdp_collect copies it out).  *dev: the device view of whichever it is.
template <class T>
static int host_target(fsdp_ctx* c, T* user, size_t bytes, PinnedBuf<T>& block, size_t count, size_t want, const char* what, T** dev, bool* staged) {
  *staged = !is_pinned(user, bytes);
  if (*staged) HIP_TRY(c, block.reserve(count, want, Pin::Mapped));
  *dev = (T*)device_view(*staged ? block.get() : user);
  if (*dev) return 0;
  c->err = std::string("internal: ") + what + " is not mapped into the device's address space";
  return 2;
}
// every row of the batch the staging kernels read (stage_in_kernel, sort_kernel's StageIn) is page-locked: the offsets, the cone
// rows from cones + 3 * off[0], the poses and the previous paths
static bool inputs_pinned(const Batch& b) {
  const size_t n = (size_t)b.n;
  return b.n > 0 && is_pinned(b.off, sizeof(int32_t) * (n + 1)) && is_pinned(b.poses, sizeof(double) * 4 * n) &&
         (b.total == 0 || is_pinned(b.cones + 3 * (size_t)b.off[0], sizeof(double) * 3 * b.total)) &&
         (!b.prev || is_pinned(b.prev, sizeof(double) * PATH_POINTS * 4 * n));
}

// ---- device memory: the counterpart of is_pinned for the arrays of a device ticket --------------------------------------------
// [p, p + bytes) lies in ONE allocation of plain device memory on the context's GPU (not managed, not another GPU's, not host
// memory of any kind, and known to the runtime this library links)
static bool device_owns(const fsdp_ctx* c, const void* p, size_t bytes) {
  if (!p) return false;
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (a.type != hipMemoryTypeDevice || a.isManaged || a.device != c->device) return false;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  const char* lo = (const char*)base;
  return (const char*)p >= lo && bytes <= size && (size_t)((const char*)p - lo) <= size - bytes;
}
// p is device memory (any GPU's): what a host entry point must not dereference
static bool is_device_memory(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice && !a.isManaged;
}
struct NamedPtr {
  const char* name;
  const void* p;
};
// the host entry points' mirror of fsdp_submit_device's pointer rule: an error code instead of a host crash in check_batch
static int refuse_device_pointers(fsdp_ctx* c, const char* who, std::initializer_list<NamedPtr> ptrs) {
  for (const NamedPtr& x : ptrs)
    if (is_device_memory(x.p)) {
      c->err = std::string(who) + ": " + x.name + " is device memory; this entry point takes host pointers (device arrays go through fsdp_submit_device)";
      return 1;
    }
  return 0;
}

// ---- the kernels of one pass ----------------------------------------------------------------------------------------------
// sort_kernel -> [sort_big_kernel] -> match_kernel -> path stage -> [path_retry_kernel] -> assemble_kernel, all on the
// slot's stream.  The bracketed ones are the *routes* for what the fast kernels hand on (device lists): frames beyond the
// sorting kernel's LDS capacities, frames for the exact one-frame-per-wavefront path kernel.  On the bench workload both
// lists are empty in every pass, and a launch that finds its list empty still costs its place in the stream (round 2: two
// route kernels + two counter memsets = 7 % of the overlapped kernel time): they are launched only when expected
// (fsdp_ctx::expect_*), assemble_kernel reports the list lengths, and verify_pass re-runs a pass that needed a route it
// did not get.  Results never depend on the route or on the prediction.
constexpr int MAX_STAGES = FSDP_MAX_STAGES;
struct StageEvents {  // optional timing: ev[k] is recorded before stage k, ev[n_stages] after the last
  Event* ev = nullptr;
  int n = 0;
  bool main_only = false;   // record only the events around the path stage's main kernel (and the last one of the pass)
  unsigned recorded = 0;    // bit k: ev[k] was recorded
  unsigned long long* clock_first = nullptr;  // device words for the refit kernel's own clock readings (fit_kernel)
  unsigned long long* clock_last = nullptr;
};
enum MarkKind { MARK_PLAIN = 0, MARK_MAIN = 1, MARK_LAST = 2 };
static void mark(const Work& q, StageEvents* t, MarkKind kind = MARK_PLAIN) {
  if (!t || !t->ev) return;
  if (!t->main_only || kind != MARK_PLAIN) {
    (void)hipEventRecord(t->ev[t->n], q.stream);
    t->recorded |= 1u << t->n;
  }
  t->n++;
}

static bool sort128(const fsdp_ctx* c, const Inputs& in) { return in.max_cones <= SortShared128::MAX_N && !c->no_sort128; }

// the sorting cache as a launch sees it whose frame 0 is planner `base`
static SortCacheView cache_view(const fsdp_ctx* c, int base) {
  const int p = c->cache_cur, x = 1 - p;
  SortCacheView v;
  v.prev = c->cache.d_hdr[p];
  v.next = c->cache.d_hdr[x];
  v.prev_xyt = c->cache.d_xyt[p];
  v.prev_off = c->cache.d_off[p];
  v.next_xyt = c->cache.d_xyt[x];
  v.next_off = c->cache.d_off[x];
  v.hits = c->cache.d_hits;
  v.base = base;
  return v;
}

// fsdp_plan_sequence_cached: what sequence_cache_lib.hip's launches need, once per pass (launch_pass)
static fsdp_seqc_launch_args seqc_args(const fsdp_ctx* c, Work& q, const Inputs& in, const SeqSlice& s) {
  fsdp_seqc_launch_args a;
  a.n_planners = s.n;
  a.n_steps = s.n_steps;
  a.off = in.d_off;
  a.cones = in.d_cones;
  a.poses = in.d_poses;
  a.sorted = q.buf.d_sort;
  a.big = q.buf.d_big;
  a.big_state = nullptr;  // (launch_sort_big allocates the blocks on first use)
  a.big_blocks = SORT_BIG_BLOCKS;
  a.small = sort128(c, in);
  a.prm = c->d_params;
  a.rec = q.seqc_buf.d_seqc_rec;
  a.cache = cache_view(c, 0);  // (frame f is planner f % n_planners: seq_cache_mark_kernel takes the view as it is)
  a.hits = q.seqc_buf.d_seqc_hits;
  a.resorted = q.seqc_buf.d_seqc_resorted;
  return a;
}

// Which instantiation of the three sorting kernels (sort_kernel_128 | sort_kernel, sort_big_kernel) a launch takes, and what that
// instantiation needs.  Whoever describes the launch chooses it, once: the cached one for a lock-step call that advances the sorting
// cache, the speculative one for a pass of fsdp_plan_sequence_cached, the ranked one for fsdp_sort_batch_ranked, the history
// one for fsdp_sort_batch_history, else the plain one.
struct SortVariant {
  enum Kind { PLAIN, CACHED, SPEC, RANKED, HISTORY } kind = PLAIN;
  SortCacheView cache;                    // CACHED: the cache buffers and the planner of the launch's frame 0
  fsdp_seqc_launch_args* seqc = nullptr;  // SPEC: the pass's launch arguments (launch_pass: seqc_args)
  const SortRankView* rank = nullptr;     // RANKED: where the rows go ...
  SortRankScratchBig* scratch = nullptr;  // ... and sort_big_kernel_ranked's block for the cost terms (SORT_BIG_BLOCKS of them)
  fsdp_sort_hist_launch_args* hist = nullptr;  // HISTORY: the call's launch arguments (sort_history_lib.hip)
  const char* suffix() const {
    static const char* const names[] = {"", "_cached", "_spec", "_ranked", "_history"};
    return names[kind];
  }
};

// Both launches append the name of the kernel they took to `names` (fsdp_stage_names).
// st: the batch's stage-in (src_off != NULL: the kernel brings it onto the device itself; the ranked kernels have none)
// gang (plain variant only): the pass is a ganged one, its twin kernels stage the members' frames (sort_kernel.h StageGang)
static void launch_sort(fsdp_ctx* c, Work& q, const Inputs& in, const StageIn& st, std::string& names, const SortVariant& var,
                        const StageGang* gang = nullptr) {
  const bool small = sort128(c, in);
  const dim3 grid(in.n_frames), block(WAVE);
  if (gang) {
    hipLaunchKernelGGL((small ? sort_kernel_128_gang : sort_kernel_gang), grid, block, 0, q.stream, *gang, q.buf.d_sort, q.buf.d_big, c->d_params);
    names += small ? "sort_kernel_128_gang" : "sort_kernel_gang";
    return;
  }
  if (var.kind == SortVariant::RANKED)
    hipLaunchKernelGGL((small ? sort_kernel_128_ranked : sort_kernel_ranked), grid, block, 0, q.stream, in.n_frames, in.d_off, in.d_cones,
                       in.d_poses, q.buf.d_sort, q.buf.d_big, c->d_params, *var.rank);
  else if (var.kind == SortVariant::CACHED)
    hipLaunchKernelGGL((small ? sort_kernel_128_cached : sort_kernel_cached), grid, block, 0, q.stream, in.n_frames, in.d_off, in.d_cones,
                       in.d_poses, q.buf.d_sort, q.buf.d_big, c->d_params, st, var.cache);
  else if (var.kind == SortVariant::SPEC)
    fsdp_seqc_launch_sort(q.stream, var.seqc);
  else if (var.kind == SortVariant::HISTORY) {
    var.hist->small = small;
    fsdp_sort_hist_launch(q.stream, var.hist);
  } else
    hipLaunchKernelGGL((small ? sort_kernel_128 : sort_kernel), grid, block, 0, q.stream, in.n_frames, in.d_off, in.d_cones, in.d_poses,
                       q.buf.d_sort, q.buf.d_big, c->d_params, st);
  names += std::string(small ? "sort_kernel_128" : "sort_kernel") + var.suffix();
}
static int launch_sort_big(fsdp_ctx* c, Work& q, const Inputs& in, std::string& names, const SortVariant& var) {
  HIP_TRY(c, q.d_sort_big.reserve(SORT_BIG_BLOCKS));
  const dim3 grid(SORT_BIG_BLOCKS), block(WAVE);
  if (var.kind == SortVariant::RANKED)
    hipLaunchKernelGGL(sort_big_kernel_ranked, grid, block, 0, q.stream, in.d_off, in.d_cones, in.d_poses, q.buf.d_sort, q.buf.d_big, q.d_sort_big,
                       c->d_params, *var.rank, var.scratch);
  else if (var.kind == SortVariant::CACHED)
    hipLaunchKernelGGL(sort_big_kernel_cached, grid, block, 0, q.stream, in.d_off, in.d_cones, in.d_poses, q.buf.d_sort, q.buf.d_big, q.d_sort_big,
                       c->d_params, var.cache);
  else if (var.kind == SortVariant::SPEC) {
    var.seqc->big_state = q.d_sort_big;
    fsdp_seqc_launch_sort_big(q.stream, var.seqc);
  } else if (var.kind == SortVariant::HISTORY) {
    var.hist->big_state = q.d_sort_big;
    fsdp_sort_hist_launch_big(q.stream, var.hist);
  } else
    hipLaunchKernelGGL(sort_big_kernel, grid, block, 0, q.stream, in.d_off, in.d_cones, in.d_poses, q.buf.d_sort, q.buf.d_big, q.d_sort_big,
                       c->d_params);
  names += std::string("sort_big_kernel") + var.suffix();
  return 0;
}
static void launch_match(fsdp_ctx* c, Work& q, const Inputs& in) {
  hipLaunchKernelGGL(match_kernel<MATCH_G>, dim3((in.n_frames + WAVE / MATCH_G - 1) / (WAVE / MATCH_G)), dim3(WAVE), 0, q.stream,
                     in.n_frames, in.d_off, in.d_cones, in.d_poses, q.buf.d_sort, q.buf.d_match, c->d_params);
}
// ---- the path stage of one pass ------------------------------------------------------------------------------------------
// Small batches (<= PATH_SMALL_BATCH frames: single-frame calls, latency): one kernel, one frame per wavefront.
// Large batches: three kernels (path_kernel.h: path_prep_kernel -> fit_kernel -> path_finish_kernel).  Either way the
// frames the fast kernels hand on (retry list on the device) are planned by the exact kernel in the same stream.
template <int GF, int NKC = FIT_KNOTS>
static void launch_fit(fsdp_ctx* c, Work& q, int n, const StageEvents* t = nullptr) {
  hipLaunchKernelGGL((fit_kernel<GF, NKC>), dim3((n + WAVE / GF - 1) / (WAVE / GF)), dim3(WAVE), 0, q.stream, n,
                     q.buf.d_arena, q.buf.d_mid, q.buf.d_retry, c->d_params, t ? t->clock_first : nullptr, t ? t->clock_last : nullptr);
}
template <int G, int NKC = FIT_KNOTS>
static void launch_prep(fsdp_ctx* c, Work& q, const Inputs& in, const double* prev) {
  const int n = in.n_frames;
  hipLaunchKernelGGL((path_prep_kernel<G, NKC>), dim3((n + WAVE / G - 1) / (WAVE / G)), dim3(WAVE), 0, q.stream, n, in.d_poses, q.buf.d_match,
                     c->d_default_path, prev, c->d_gpath, c->n_gpath, q.buf.d_arena, q.buf.d_path, q.buf.d_mid, q.buf.d_retry, c->d_params);
}
template <int G, int NKC = FIT_KNOTS>
static void launch_finish(fsdp_ctx* c, Work& q, int n) {
  hipLaunchKernelGGL((path_finish_kernel<G, NKC>), dim3((n + WAVE / G - 1) / (WAVE / G)), dim3(WAVE), 0, q.stream, n, q.buf.d_arena, q.buf.d_mid, q.buf.d_path,
                     q.buf.d_retry, c->d_params);
}

// the same steps through the packed kernels (csrc/skidpad_kernel.h "steps in flight, many frames per wavefront")
static void skid_group_mark(fsdp_ctx* c) {  // (timing of the groups' kernels on request: fsdp_skidpad_time_groups)
  if (!c->skid_time_groups) return;
  Event e;
  if (hipEventCreate(&e.h) != hipSuccess) return;
  (void)hipEventRecord(e, c->stream);
  c->skid_group_ev.push_back(std::move(e));
}
template <int G, int GF>
static void launch_skid_packed_kernels(fsdp_ctx* c, int frames) {
  hipStream_t xs = c->stream;
  if (c->skid_time_groups && c->skid_group_names.empty())  // (the first group's instantiations: a replay's last, shorter group may take the 16-lane ones)
    c->skid_group_names = "skid_select_kernel,skid_prep_kernel<" + std::to_string(G) + ">,fit_kernel<" + std::to_string(GF) + ">,path_finish_kernel<" +
                          std::to_string(G) + ">,skid_commit_kernel";
  skid_group_mark(c);
  hipLaunchKernelGGL(skid_prep_kernel<G>, dim3((frames + WAVE / G - 1) / (WAVE / G)), dim3(WAVE), 0, xs, frames, c->group.d_g_sel, c->tables, c->d_chord,
                     c->d_default_path, c->group.d_g_arena, c->group.d_g_mid);
  skid_group_mark(c);
  hipLaunchKernelGGL((fit_kernel<GF, FIT_KNOTS>), dim3((frames + WAVE / GF - 1) / (WAVE / GF)), dim3(WAVE), 0, xs, frames, c->group.d_g_arena, c->group.d_g_mid,
                     c->group.d_g_retry, c->d_params, (unsigned long long*)nullptr, (unsigned long long*)nullptr);
  skid_group_mark(c);
  hipLaunchKernelGGL(path_finish_kernel<G>, dim3((frames + WAVE / G - 1) / (WAVE / G)), dim3(WAVE), 0, xs, frames, c->group.d_g_arena, c->group.d_g_mid, c->group.d_g_out,
                     c->group.d_g_retry, c->d_params);
  skid_group_mark(c);
}

// Lanes per frame: a serial instruction costs its issue cycles whatever the number of active lanes, so the more frames
// share a wavefront the cheaper a frame gets — as long as there are enough wavefronts for every SIMD.  With at least
// PACK_FRAMES frames in flight (batch size x passes overlapped) the fit kernel packs 16 frames into a wavefront (4 lanes
// each: exactly the Givens quad) and the kernels around it 8; below that, 4 frames per wavefront everywhere.
constexpr int PACK_FRAMES = 12288;

// How many frames are in flight on the GPU decides the packing.  A resident batch replayed through `overlap` slots keeps
// overlap x n frames in flight; a ticket of fsdp_submit counts what is really queued (the frames of the uncollected tickets
// plus its own): a lone batch submitted to a context of depth 10 is a lone batch, and gets the lanes of one.
static long long frames_in_flight(const fsdp_ctx* c, int n, bool ticket) {
  if (!ticket) return (long long)n * c->overlap;
  long long sum = n;
  for (int i = 0; i < FSDP_MAX_OVERLAP; i++)
    for (const Work::Ticket& t : c->slot[i].tk)
      if (t.id >= 0 && !t.skid) sum += t.batch.n;
  return sum;
}

// one launch of a pass with per-frame global paths (gpath_table_launch.h); ids: the pass's path ids as the GPU addresses them
static void launch_gpt(fsdp_ctx* c, Work& q, const Inputs& in, const int32_t* ids, int form, unsigned blocks = 0) {
  fsdp_gpt_launch_args a;
  a.form = form;
  a.n_frames = in.n_frames;
  a.blocks = blocks;
  a.poses = in.d_poses;
  a.matched = q.buf.d_match;
  a.default_path = c->d_default_path;
  a.prev_paths = in.use_prev ? in.d_prev : nullptr;
  a.table_xy = c->d_gpt_xy;
  a.table_off = c->d_gpt_off;
  a.n_paths = c->n_gpt;
  a.ids = ids;
  a.arena = q.buf.d_arena;
  a.out = q.buf.d_path;
  a.mid = q.buf.d_mid;
  a.retry = q.buf.d_retry;
  a.prm = c->d_params;
  fsdp_gpt_launch(q.stream, &a);
}

// the path stage's fast kernels (no route, no assembly); returns whether it was the three-kernel form
// ids: not NULL for a pass with per-frame global paths — the TABLE twins of the wrappers that read a global path, and of the three-kernel
// forms the one a context-wide path takes (32 knots per fit, 8 lanes per frame), for all of its frames: those with id -1 ride along
static bool launch_path(fsdp_ctx* c, Work& q, const Inputs& in, StageEvents* t, std::string& names, long long in_flight, const int32_t* ids = nullptr) {
  const double* prev = in.use_prev ? in.d_prev : nullptr;
  const int n = in.n_frames;
  // (the packed kernels hold degree-3 fits only: a context with max_deg < 3 plans every batch with the one-kernel stage)
  // (by the frames in flight, like the packing: a 1024-frame chunk of a 4096-frame call is not a small batch)
  const bool split = c->params.max_deg != 3 ? false : (c->force_path_mode ? c->force_path_mode == 2 : in_flight > PATH_SMALL_BATCH);
  if (!split) {
    mark(q, t, MARK_MAIN);
    // A context whose fits may be of degree 1 or 2 (max_deg < 3: utils/spline_fit.py:113) has no three-kernel form (those kernels
    // hold cubic fits only); its large batches run the one-kernel stage with FOUR frames per wavefront (16 lanes each, all
    // degrees, 32 knots per fit, the scaling-free divisions; what that form cannot hold goes to the exact kernel like any other
    // frame the packed kernels hand on) instead of one frame per wavefront.
    const bool mono16 = c->force_path_mode != 1 && c->params.max_deg != 3 && in_flight > PATH_SMALL_BATCH;
    if (ids) {
      launch_gpt(c, q, in, ids, mono16 ? PATH_G_LATENCY : PATH_G_SMALL);
      names += mono16 ? "path_table_kernel<16>," : "path_table_kernel<64>,";
      return split;
    }
    if (mono16)
      hipLaunchKernelGGL(path_kernel<PATH_G_LATENCY>, dim3((n + WAVE / PATH_G_LATENCY - 1) / (WAVE / PATH_G_LATENCY)), dim3(WAVE), 0, q.stream, n, in.d_poses,
                         q.buf.d_match, c->d_default_path, prev, c->d_gpath, c->n_gpath, q.buf.d_arena, q.buf.d_path, q.buf.d_retry, c->d_params);
    else
      hipLaunchKernelGGL(path_kernel<PATH_G_SMALL>, dim3(n), dim3(WAVE), 0, q.stream, n, in.d_poses, q.buf.d_match, c->d_default_path, prev,
                         c->d_gpath, c->n_gpath, q.buf.d_arena, q.buf.d_path, q.buf.d_retry, c->d_params);
    names += mono16 ? "path_kernel<16>," : "path_kernel<64>,";
    return split;
  }
  mark(q, t);
  // A context with a global path (set_global_path; the acceleration / ebs_test missions run on their known path) fits 100+ m
  // polylines that need 17-32 knots (87 % of such frames; never more than 32 on the reference's tables): the WIDE instantiations
  // of the three kernels — 32 knots per fit in the frame's LDS workspace, eight lanes per frame — keep them on the packed kernels
  // instead of sending every frame to the exact one.
  // (a pass with ids: the same three, the first one as its TABLE twin — one sequence of launches for both, so that the kernels
  // of this translation unit keep their order in the code object)
  if (ids || c->n_gpath > 0) {
    if (ids)
      launch_gpt(c, q, in, ids, PATH_G_SPLIT);
    else
      launch_prep<8, WIDE_KNOTS>(c, q, in, prev);
    mark(q, t, MARK_MAIN);
    launch_fit<8, WIDE_KNOTS>(c, q, n, t);
    mark(q, t, MARK_MAIN);
    launch_finish<8, WIDE_KNOTS>(c, q, n);
    names += ids ? "path_table_prep_kernel<8,32>," : "path_prep_kernel<8,32>,";
    names += "fit_kernel<8,32>,path_finish_kernel<8,32>,";
    return split;
  }
  const bool packed = c->force_pack ? c->force_pack == 2 : in_flight >= PACK_FRAMES;
  const int gf = packed ? c->fit_g : 16;
  if (packed)
    launch_prep<8>(c, q, in, prev);
  else
    launch_prep<16>(c, q, in, prev);
  mark(q, t, MARK_MAIN);
  if (gf == 4)
    launch_fit<4>(c, q, n, t);
  else if (gf == 8)
    launch_fit<8>(c, q, n, t);
  else
    launch_fit<16>(c, q, n, t);
  mark(q, t, MARK_MAIN);
  if (packed)
    launch_finish<8>(c, q, n);
  else
    launch_finish<16>(c, q, n);
  const std::string g = packed ? "8" : "16";
  names += "path_prep_kernel<" + g + ">,fit_kernel<" + std::to_string(gf) + ">,path_finish_kernel<" + g + ">,";
  return split;
}
// sized: by the retry lists the context's recent passes reported (fsdp_ctx::retry_hint) instead of for the worst case.  A pass that is
// only EXPECTED to need the kernel (one batch in thousands had a frame for it) used to launch 1024 workgroups that found an empty list:
// nothing to compute, but on a chip full of other passes' wavefronts the last of them was dispatched ~1.7 ms later, and the pass's
// assembly waits for it (the stream of different batches: 355 such launches, 12 % of the summed kernel time of the trace).  The kernel
// walks its list grid-stride: any grid plans any list.
static void launch_path_retry(fsdp_ctx* c, Work& q, const Inputs& in, bool sized = false, const int32_t* ids = nullptr) {
  const double* prev = in.use_prev ? in.d_prev : nullptr;
  int rb = in.n_frames < 1024 ? in.n_frames : 1024;  // one wavefront per SIMD at most; blocks beyond the list's length return at once
  if (sized) rb = std::max(1, std::min(rb, 16 + 2 * c->retry_hint));
  if (ids) {  // (a pass with per-frame global paths: the same lookup)
    launch_gpt(c, q, in, ids, 0, (unsigned)rb);
    return;
  }
  hipLaunchKernelGGL(path_retry_kernel, dim3(rb), dim3(WAVE), 0, q.stream, in.d_poses, q.buf.d_match, c->d_default_path, prev, c->d_gpath,
                     c->n_gpath, q.buf.d_arena, q.buf.d_path, q.buf.d_retry, c->d_params);
}
// The description of one pass, beyond its slot and its inputs: what it writes where, where its sorting kernel finds the batch, which
// kernels it is made of and what it is planned for.  The default is a pass over the resident batch; a ticket's pass is built from
// the ticket (enqueue_ticket).  The launches read nothing else about the pass: the context holds no per-call state.
// one member of a ganged pass: a batch on the device or in page-locked host memory (device views), as StageMember takes it
struct GangMember {
  const int32_t* off = nullptr;
  const double* cones = nullptr;  // the array's row 0 (the member's rows start at off[0] = base)
  const double* poses = nullptr;
  const double* prev = nullptr;
  int n = 0;
  int32_t base = 0;
  size_t rows = 0;
};
struct Pass {
  std::vector<GangMember> members;    // not empty: a ganged pass over the members' frames, one behind the other; the slot's own input
                                      // store (launch_pass's `in_`: reserved and described for the sum) receives the copies
  fsdp_frame_result* host = nullptr;  // NULL: results into the slot's result block; else the device view of a page-locked host buffer
                                      // that assemble_kernel writes straight over PCIe (a ticket: no copy command at all)
  bool compact = false;               // ... as fsdp_compact_result records (fsdp_submit_compact)
  int trailer = SLOT_QUEUE;           // the pass's trailer: a ticket's entry index, or SLOT_QUEUE (resident / blocking passes)
  SkidInfo* info = nullptr;           // skidpad: device view of the page-locked block the planners' information records go to
  StageIn stage;                      // src_off != NULL: device views of the caller's page-locked batch, which the sorting kernel
                                      // brings onto the device itself (sort_kernel.h StageIn)
  StageEvents* events = nullptr;      // optional timing (fsdp_time_runs)
  bool force_routes = false;          // both route kernels whatever is expected (a pass that runs again because it lacked one)
  long long in_flight = -1;           // frames on the GPU while this pass runs, its own included (launch_path); < 0: a resident batch
                                      // replayed through every slot of the overlap depth
  SortVariant sort;                   // the sorting kernels' instantiation: PLAIN, CACHED, or SPEC (its arguments are made by launch_pass)
  const Work::SeqPass* sq = nullptr;  // a sequence pass: the chain kernels between the path stage and the assembly
  bool device = false;                // a device ticket's pass: `host` (or NULL: the slot's block) is device memory, the results are handed
                                      // out by device_out_kernel, and path_retry_kernel's grid is always sized from the retry hint
  const int32_t* path_ids = nullptr;  // a pass with per-frame global paths: the frames' ids into the context's path table, as the GPU
                                      // addresses them (device memory, or the device view of page-locked host memory)
};

// skid: a skidpad step's records (path stage only, on the context's stream)
static void launch_assemble(fsdp_ctx* c, Work& q, int n, const Pass& pass, bool skid) {
  long long blocks = ((long long)n + 3) / 4;  // one wavefront per frame, four per workgroup (grid-stride beyond the cap)
  // results that go straight to host memory leave at the link's pace: a few hundred wavefronts keep it busy, more would
  // only sit on the SIMDs' wavefront slots with their stores pending while the other slots' kernels wait for a place
  const long long cap = pass.host && !pass.device ? 128 : 16384;  // (32 / 128 / 512 workgroups towards host memory: 5.1 / 5.2 / 5.4 M frames/s streamed, inside the noise: profiles/r06_streaming_probe.txt)
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  q.seq++;
  hipStream_t s = skid ? c->stream : q.stream;
  const bool filtered = !skid && !c->params.use_unknown_cones;  // (indices back into the caller's cone lists: launch_filter's map)
  const int32_t* remap = filtered ? q.filt.f_map : nullptr;
  const int32_t* remap_off = filtered ? q.filt.f_off : nullptr;
  if (pass.compact) {  // fsdp_compact_result records (into the slot's result block or the caller's page-locked buffer)
    hipLaunchKernelGGL(assemble_compact_kernel, dim3((unsigned)blocks), dim3(256), 0, s, n, q.buf.d_sort, q.buf.d_match, q.buf.d_path,
                       (fsdp_compact_result*)(pass.host ? pass.host : q.buf.d_result), q.buf.d_big, q.buf.d_retry, q.h_trailer.device() + pass.trailer, q.seq, remap, remap_off);
    return;
  }
  hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)blocks), dim3(256), 0, s, n, skid ? (const SortOut*)nullptr : q.buf.d_sort,
                     skid ? (const MatchOut*)nullptr : q.buf.d_match, q.buf.d_path, pass.host ? pass.host : q.buf.d_result, q.buf.d_big, q.buf.d_retry, q.h_trailer.device() + pass.trailer,
                     q.seq, (const int32_t*)(pass.info ? q.buf.d_skid_info : nullptr), (int32_t*)pass.info, pass.info ? (int)(sizeof(SkidInfo) / 4) * n : 0,
                     remap, remap_off);
}

// The chain kernels of a sequence pass (sequence_kernel.h, launched by sequence_lib.hip), behind the path stage and its retry route:
// every frame was planned with the constant initial path; the runs of frames that read it are planned again in order, a wavefront
// per run.
static void launch_sequence(fsdp_ctx* c, Work& q, const Inputs& in, const Pass& pass) {
  const Work::SeqPass& sq = *pass.sq;
  fsdp_seq_launch_args a;
  a.n_planners = sq.s.n;
  a.n_steps = sq.s.n_steps;
  a.poses = in.d_poses;
  a.matched = q.buf.d_match;
  a.initial_prev = sq.init ? q.seq_buf.d_seq_init : nullptr;
  a.gpath = c->d_gpath;
  a.n_gpath = c->n_gpath;
  a.arena = q.buf.d_arena;
  a.out = q.buf.d_path;
  a.seq = q.seq_buf.d_seq;
  a.final_prev = sq.final_dev;
  a.replanned_out = &(q.h_trailer.device() + pass.trailer)->pad;
  a.prm = c->d_params;
  if (pass.path_ids) {  // (per-frame global paths: the TABLE twin of the chain kernel between the two kernels that read no global path)
    fsdp_seq_launch_mark(q.stream, &a);
    fsdp_seqt_launch_chain(q.stream, &a, c->d_gpt_xy, c->d_gpt_off, c->n_gpt, pass.path_ids);
    fsdp_seq_launch_final(q.stream, &a);
    return;
  }
  fsdp_seq_launch(q.stream, &a);
}

// use_unknown_cones = False: the batch without its UNKNOWN cones into the slot's filter buffers; returns the view the
// stage kernels plan (same poses / previous paths)
static int launch_filter(fsdp_ctx* c, Work& q, const InputStore<>& in, Inputs* view) {
  if (!q.filt.fits(in.frames(), in.cone_rows())) {  // (room for whatever the batch's own buffers can hold)
    HIP_TRY(c, hipStreamSynchronize(q.stream));
    HIP_TRY(c, q.filt.reserve(in.frames(), in.cone_rows()));
  }
  const int n = in.n_frames;
  hipLaunchKernelGGL(filter_count_kernel, dim3(n), dim3(WAVE), 0, q.stream, n, in.d_off, in.d_cones, q.filt.f_cnt);
  hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(1024), 0, q.stream, n, q.filt.f_cnt, q.filt.f_off);
  hipLaunchKernelGGL(filter_scatter_kernel, dim3(n), dim3(WAVE), 0, q.stream, n, in.d_off, in.d_cones, q.filt.f_off, q.filt.f_cones, q.filt.f_map);
  *view = in.view();
  view->d_off = q.filt.f_off;
  view->d_cones = q.filt.f_cones;
  return 0;
}

// sorting -> matching -> path stage -> result assembly of batch `in` on slot q as `pass` describes the pass (Pass() = a pass over the
// resident batch into the slot's result block); it becomes the context's most recent pass
static int launch_pass(fsdp_ctx* c, Work& q, const InputStore<>& in_, const Pass& pass) {
  StageEvents* const t = pass.events;
  if ((size_t)in_.n_frames > q.buf.frames()) {  // (a growth that failed left the slot empty: an error code, never a launch on what is not there)
    c->err = "internal: slot " + std::to_string(q.index) + " holds no room for a pass of " + std::to_string(in_.n_frames) + " frames";
    return 2;
  }
  c->primed[q.index] = true;
  const bool with_big = pass.force_routes || c->always_route || c->expect_big;
  const bool with_retry = pass.force_routes || c->always_route || c->expect_retry;
  Inputs in = in_.view();
  if (!c->params.use_unknown_cones)
    if (int rc = launch_filter(c, q, in_, &in)) return rc;
  std::string names;
  if (c->poison) {
    // (tests) whatever a previous pass, another batch or the allocator left in the slot's buffers is gone: 0xFF bytes = NaNs, -1 indices
    const size_t m = (size_t)in.n_frames;
    (void)hipMemsetAsync(q.buf.d_sort, 0xff, sizeof(SortOut) * m, q.stream);
    (void)hipMemsetAsync(q.buf.d_match, 0xff, sizeof(MatchOut) * m, q.stream);
    (void)hipMemsetAsync(q.buf.d_path, 0xff, sizeof(PathOut) * m, q.stream);
    (void)hipMemsetAsync(q.buf.d_mid, 0xff, sizeof(PathMid) * m, q.stream);
    (void)hipMemsetAsync(q.buf.d_arena, 0xff, sizeof(double) * (size_t)ARENA_DOUBLES * m, q.stream);
    (void)hipMemsetAsync(q.buf.d_result, 0xff, sizeof(fsdp_frame_result) * m, q.stream);
    (void)hipMemsetAsync(q.buf.d_big + 1, 0xff, sizeof(int) * m, q.stream);
    (void)hipMemsetAsync(q.buf.d_retry + 1, 0xff, sizeof(int) * m, q.stream);
  }
  fsdp_seqc_launch_args seqc;
  SortVariant var = pass.sort;
  if (var.kind == SortVariant::SPEC) {
    seqc = seqc_args(c, q, in, pass.sq->s);
    var.seqc = &seqc;
  }
  StageGang gang;
  int last_first = 0, last_n = in.n_frames;
  if (!pass.members.empty()) {
    if (pass.members.size() > (size_t)GANG_MAX || var.kind != SortVariant::PLAIN || !c->params.use_unknown_cones) {
      c->err = "internal: a ganged pass takes at most " + std::to_string(GANG_MAX) + " members, the plain sorting kernels and unfiltered inputs";
      return 2;
    }
    int frames = 0;
    size_t rows = 0;
    for (const GangMember& gm : pass.members) {
      StageMember& sm = gang.m[gang.n_members++];
      sm.src_off = gm.off;
      sm.src_cones = gm.cones + 3 * (size_t)gm.base;
      sm.src_poses = gm.poses;
      sm.src_prev = in.use_prev ? gm.prev : nullptr;
      sm.base = gm.base;
      sm.first_frame = last_first = frames;
      sm.first_row = (int32_t)rows;
      last_n = gm.n;
      frames += gm.n;
      rows += gm.rows;
    }
    if (frames != in.n_frames || !in_.fits((size_t)frames, rows, in.use_prev)) {
      c->err = "internal: slot " + std::to_string(q.index) + "'s input store does not hold the ganged pass's " + std::to_string(frames) + " frames";
      return 2;
    }
    gang.dst_off = in.d_off;
    gang.dst_cones = in.d_cones;
    gang.dst_poses = in.d_poses;
    gang.dst_prev = in.use_prev ? in.d_prev : nullptr;
    gang.n_frames = frames;
  }
  mark(q, t);
  launch_sort(c, q, in, pass.stage, names, var, pass.members.empty() ? nullptr : &gang);
  names += ',';
  if (with_big) {
    mark(q, t);
    if (int rc = launch_sort_big(c, q, in, names, var)) return rc;
    names += ',';
  }
  if (var.kind == SortVariant::SPEC) {  // (fsdp_plan_sequence_cached: the sorting results become those of the cache-on lock-step calls)
    fsdp_seqc_launch_chain(q.stream, &seqc);
    names += "seq_cache_mark_kernel,seq_cache_resolve_kernel,";
  }
  mark(q, t);
  launch_match(c, q, in);
  names += "match_kernel<" + std::to_string(MATCH_G) + ">,";
  const bool split = launch_path(c, q, in, t, names, pass.in_flight >= 0 ? pass.in_flight : frames_in_flight(c, in.n_frames, false), pass.path_ids);
  MarkKind after_path = split ? MARK_PLAIN : MARK_MAIN;  // (the one-kernel path stage is the main kernel: close its bracket)
  if (with_retry) {
    mark(q, t, after_path);
    after_path = MARK_PLAIN;
    launch_path_retry(c, q, in, !pass.force_routes || c->retry_hint > 0 || pass.device, pass.path_ids);
    names += pass.path_ids ? "path_table_retry_kernel," : "path_retry_kernel,";
  }
  if (pass.sq) {  // (fsdp_plan_sequence: never timed)
    launch_sequence(c, q, in, pass);
    names += pass.path_ids ? "seq_mark_kernel,seq_chain_table_kernel,seq_final_kernel," : "seq_mark_kernel,seq_chain_kernel,seq_final_kernel,";
  }
  mark(q, t, after_path);
  launch_assemble(c, q, in.n_frames, pass, false);
  names += "assemble_kernel";
  mark(q, t, MARK_LAST);
  c->stage_names = names;
  q.pass_in = &in_;
  q.ran_big = with_big;
  q.ran_retry = with_retry;
  q.unverified = pass.trailer == SLOT_QUEUE;  // (a ticket's pass is settled by fsdp_collect, through the ticket's own trailer)
  q.pass_skid = false;
  q.gang_members = (int)pass.members.size();
  q.gang_first = last_first;
  q.gang_n = last_n;
  if (q.gang_members > 0) c->gang_primed[q.index] = std::max(c->gang_primed[q.index], q.gang_members);
  c->last = fsdp_ctx::LastPass{q.index, last_n, pass.host == nullptr && !pass.device, true, last_first};
  return 0;
}

static PassTrailer read_trailer(const Work& q, int idx) {
  const PassTrailer* h = q.h_trailer + idx;
  PassTrailer tr;
  tr.seq = __atomic_load_n(&h->seq, __ATOMIC_ACQUIRE);
  tr.n_big = __atomic_load_n(&h->n_big, __ATOMIC_RELAXED);
  tr.n_retry = __atomic_load_n(&h->n_retry, __ATOMIC_RELAXED);
  tr.pad = 0;
  return tr;
}

// A pass's trailer against the routes it ran: keeps the expectations and the retry hint up to date — for a pass over the
// resident batch exactly what that batch needs from now on, else with decay — and says whether the pass lacked a route
// kernel it needed and must run again (with both).
// members: the pass was a gang of so many batches — the retry hint sizes a single pass's grid, so it takes the list length per member.
static bool settle_routes(fsdp_ctx* c, const PassTrailer& tr, bool ran_big, bool ran_retry, bool resident, int members = 1) {
  auto track = [](bool needed, bool& expect, int& clean) {
    if (needed) {
      expect = true;
      clean = 0;
    } else if (expect && ++clean >= ROUTE_DECAY) {
      expect = false;
      clean = 0;
    }
  };
  const int per_pass = members > 1 ? (tr.n_retry + members - 1) / members : tr.n_retry;
  c->retry_hint = std::max(per_pass, c->retry_hint - (c->retry_hint + 7) / 8);
  if (resident) {
    c->expect_big = tr.n_big > 0;
    c->expect_retry = tr.n_retry > 0;
    c->clean_big = c->clean_retry = 0;
    c->res_checked = true;
  } else {
    track(tr.n_big > 0, c->expect_big, c->clean_big);
    track(tr.n_retry > 0, c->expect_retry, c->clean_retry);
  }
  const bool rerun = (tr.n_big > 0 && !ran_big) || (tr.n_retry > 0 && !ran_retry);
  if (rerun) c->reruns++;
  return rerun;
}

// The slot's stream is idle: did its most recent pass get the route kernels it needed?  If not, the pass runs again with
// both (same inputs, same slot; the caller copies results afterwards).
static int verify_pass(fsdp_ctx* c, Work& q) {
  if (!q.unverified || q.pass_skid) {
    q.unverified = false;
    return 0;
  }
  q.unverified = false;
  const PassTrailer tr = read_trailer(q, SLOT_QUEUE);
  if (tr.seq != q.seq) {
    c->err = "internal: pass trailer out of date (slot " + std::to_string(q.index) + ")";
    return 2;
  }
  if (settle_routes(c, tr, q.ran_big, q.ran_retry, q.pass_in == &c->res, q.gang_members)) {
    // (a ganged pass left its members' copies in the slot's own input store: it runs again as the plain pass over that store which
    // every kernel behind the sorting kernel has seen anyway; what the readers hand out stays the last member's block, whichever
    // slot the context's most recent pass was on)
    const int members = q.gang_members, first = q.gang_first, n = q.gang_n;
    Pass again;
    again.force_routes = true;
    if (int rc = launch_pass(c, q, *q.pass_in, again)) return rc;
    if (members > 0) {
      q.gang_members = members, q.gang_first = first, q.gang_n = n;
      c->last.n = n;
      c->last.offset = first;
    }
    HIP_TRY(c, hipStreamSynchronize(q.stream));
    HIP_TRY(c, hipGetLastError());
    q.unverified = false;
  }
  return 0;
}

// wait for every pass in flight (all slots) and settle their routes
static int flush_skid(fsdp_ctx* c);
static int sync_all(fsdp_ctx* c) {
  if (int rc = flush_skid(c)) return rc;
  for (int i = 0; i < FSDP_MAX_OVERLAP; i++) {
    Work& w = c->slot[i];
    if (!w.stream) continue;
    HIP_TRY(c, hipStreamSynchronize(w.stream));
    if (int rc = verify_pass(c, w)) return rc;  // (a ticket's pass is settled by its fsdp_collect: it never sets `unverified`)
  }
  return 0;
}

static int ensure_slots(fsdp_ctx* c, int n_frames) {
  for (int i = 0; i < c->overlap; i++)
    if (int rc = ensure_work(c, c->slot[i], n_frames)) return rc;
  return 0;
}

static int busy_error(fsdp_ctx* c, const char* who) {
  c->err = std::string(who) + ": " + std::to_string(c->outstanding) + " ticket(s) of fsdp_submit not collected yet (fsdp_collect them first)";
  return 1;
}

static void assemble(const SortOut* s, const MatchOut* m, const PathOut* p, fsdp_frame_result* r) {
  // stage-level entry points: r may already hold fields from earlier stages when only part of the pipeline ran
  if (s) {
    r->status = s->status;
    r->n_left = s->n_left;
    r->n_right = s->n_right;
    memcpy(r->left_idx, s->left_idx, sizeof(r->left_idx));
    memcpy(r->right_idx, s->right_idx, sizeof(r->right_idx));
    r->n_configs_left = s->n_configs_left;
    r->n_configs_right = s->n_configs_right;
    memcpy(r->first_k_left, s->first_k_left, sizeof(r->first_k_left));
    memcpy(r->first_k_right, s->first_k_right, sizeof(r->first_k_right));
    r->best_cost_left = s->best_cost_left;
    r->best_cost_right = s->best_cost_right;
  }
  if (m) {
    if (m->status != 0) r->status = m->status;
    r->n_left_v = m->n_left_v;
    r->n_right_v = m->n_right_v;
    memcpy(r->left_v, m->left_v, sizeof(r->left_v));
    memcpy(r->right_v, m->right_v, sizeof(r->right_v));
    memcpy(r->l2r, m->l2r, sizeof(r->l2r));
    memcpy(r->r2l, m->r2l, sizeof(r->r2l));
  }
  if (p) {
    if (p->status != 0) r->status = p->status;
    memcpy(r->path, p->path, sizeof(r->path));
    r->path_fallback = p->fallback;
    r->n_dense = p->n_dense;
  }
}

// validate a batch description into *b (prev: optional previous paths)
static int check_batch(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses, const double* prev, Batch* b) {
  if (n_frames < 0 || (n_frames > 0 && (!off || !poses))) {
    c->err = "batch: NULL offsets / poses";
    return 1;
  }
  // cone_offsets[0] = b >= 0: the batch's cones are the rows [b, cone_offsets[n_frames]) of cones_xyt — a slice of a larger
  // batch is handed over by pointing at its offsets, without rebasing or copying anything (include/fsdp.h)
  if (n_frames > 0 && off[0] < 0) {
    c->err = "cone_offsets[0] must be >= 0";
    return 1;
  }
  *b = Batch{n_frames, off, cones, poses, prev, n_frames > 0 ? (size_t)(off[n_frames] - off[0]) : 0, 0};
  if (n_frames > 0 && off[n_frames] < off[0]) {
    c->err = "cone_offsets must be non-decreasing";
    return 1;
  }
  for (int i = 0; i < n_frames; i++) {
    const int d = off[i + 1] - off[i];
    if (d < 0) {
      c->err = "cone_offsets must be non-decreasing";
      return 1;
    }
    b->max_cones = std::max(b->max_cones, d);
  }
  if (b->total > 0 && !cones) {
    c->err = "cones_xyt is NULL";
    return 1;
  }
  return 0;
}

// room for batch b in `in`, which then describes it (the caller fills the buffers)
static int take_batch(fsdp_ctx* c, InputStore<>& in, const Batch& b) {
  HIP_TRY(c, in.reserve(b.n > 0 ? (size_t)b.n : 1, b.total, b.prev != nullptr));
  in.n_frames = b.n;
  in.max_cones = b.max_cones;
  in.use_prev = b.prev != nullptr;
  return 0;
}

// host -> device of a batch on `stream` (asynchronous for page-locked sources)
static int upload_inputs(fsdp_ctx* c, InputStore<>& in, hipStream_t stream, const Batch& b) {
  if (int rc = take_batch(c, in, b)) return rc;
  if (b.n == 0) return 0;
  const int32_t* off = b.off;
  const double* cones = b.cones;
  if (off[0] != 0) {
    // a slice of a larger batch: the offsets rebased to 0 (the slot's own pageable copy) and the cones from the slice's first row
    in.off_rebased.resize((size_t)b.n + 1);
    for (int i = 0; i <= b.n; i++) in.off_rebased[(size_t)i] = off[i] - off[0];
    if (cones) cones += 3 * (size_t)off[0];
    off = in.off_rebased.data();
  }
  HIP_TRY(c, hipMemcpyAsync(in.d_off, off, sizeof(int32_t) * ((size_t)b.n + 1), hipMemcpyHostToDevice, stream));
  if (b.total) HIP_TRY(c, hipMemcpyAsync(in.d_cones, cones, sizeof(double) * 3 * b.total, hipMemcpyHostToDevice, stream));
  HIP_TRY(c, hipMemcpyAsync(in.d_poses, b.poses, sizeof(double) * 4 * (size_t)b.n, hipMemcpyHostToDevice, stream));
  if (b.prev) HIP_TRY(c, hipMemcpyAsync(in.d_prev, b.prev, sizeof(double) * PATH_POINTS * 4 * (size_t)b.n, hipMemcpyHostToDevice, stream));
  return 0;
}

// the same through stage_in_kernel: every source is page-locked host memory (inputs_pinned)
static int stage_inputs(fsdp_ctx* c, InputStore<>& in, hipStream_t stream, const Batch& b) {
  if (int rc = take_batch(c, in, b)) return rc;
  if (b.n == 0) return 0;
  CopySegs S;
  S.n = 0;
  // a slice of a larger batch (cone_offsets[0] = b > 0): the kernel subtracts b from the offsets on their way in and the cones
  // are read from row b — nothing is rebased or copied on the host, nothing pageable is handed to the runtime (round-5 advisor:
  // a pageable copy made the host wait for the stream's earlier work)
  S.rebase = b.off[0];
  S.seg[S.n++] = CopySeg{device_view(b.off), in.d_off.get(), sizeof(int32_t) * ((unsigned long long)b.n + 1)};
  if (b.total) S.seg[S.n++] = CopySeg{device_view(b.cones + 3 * (size_t)b.off[0]), in.d_cones.get(), sizeof(double) * 3ull * b.total};
  S.seg[S.n++] = CopySeg{device_view(b.poses), in.d_poses.get(), sizeof(double) * 4ull * (unsigned long long)b.n};
  if (b.prev) S.seg[S.n++] = CopySeg{device_view(b.prev), in.d_prev.get(), sizeof(double) * PATH_POINTS * 4ull * (unsigned long long)b.n};
  hipLaunchKernelGGL(stage_in_kernel, dim3(256), dim3(256), 0, stream, S);
  return 0;
}

// ---- the sorting cache ----------------------------------------------------------------------------------------------------
static void cache_free(fsdp_ctx* c) {
  c->cache = SortCacheStore<>();
  c->cache_hits.clear();
  c->n_cache = 0;
  c->cache_cur = 0;
}

// A call that advances the cached planners: frame i is planner i.  The buffer the call writes gets room for every planner's
// entry — a region as large as the most cones the planner was ever given (its previous entry, which a frame the reference
// raises on keeps, fits too).  Nothing is in flight (the blocking calls have synchronised).
static int cache_prepare(fsdp_ctx* c, int n_frames, const int32_t* off, const char* who) {
  if (n_frames != c->n_cache) {
    c->err = std::string(who) + ": the sorting cache is on for " + std::to_string(c->n_cache) + " planners, the batch holds " +
             std::to_string(n_frames) + " frames (frame i is planner i)";
    return 1;
  }
  const int x = 1 - c->cache_cur;
  std::vector<int32_t> lay((size_t)n_frames + 1);
  size_t rows = 0;
  for (int i = 0; i < n_frames; i++) {
    c->cache.region[(size_t)i] = std::max(c->cache.region[(size_t)i], off[i + 1] - off[i]);
    lay[(size_t)i] = (int32_t)rows;
    rows += (size_t)c->cache.region[(size_t)i];
    if (rows > 0x7fffffff) {
      c->err = std::string(who) + ": the sorting cache's cone store exceeds 2^31 rows";
      return 1;
    }
  }
  lay[(size_t)n_frames] = (int32_t)rows;
  HIP_TRY(c, c->cache.reserve_rows(x, rows));
  if (lay != c->cache.layout[x]) {
    HIP_TRY(c, copy_sync(c, c->cache.d_off[x], lay.data(), sizeof(int32_t) * lay.size(), hipMemcpyHostToDevice));
    c->cache.layout[x].swap(lay);
  }
  return 0;
}

// after a successful call: its hit codes to the host, and its entries become the previous ones
static int cache_finish(fsdp_ctx* c) {
  HIP_TRY(c, copy_sync(c, c->cache_hits.data(), c->cache.d_hits, c->cache_hits.size(), hipMemcpyDeviceToHost));
  c->cache_cur = 1 - c->cache_cur;
  return 0;
}

extern "C" {

const char* fsdp_version(void) { return "fsdp-hip 0.3 (gfx950)"; }
int fsdp_result_size(void) { return (int)sizeof(fsdp_frame_result); }
void fsdp_shapes(int32_t* out4) {
  out4[0] = FSDP_MAX_LEN;
  out4[1] = FSDP_MAX_NEIGHBORS;
  out4[2] = FSDP_MAX_MATCH;
  out4[3] = FSDP_PATH_POINTS;
}

int fsdp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* fsdp_last_error(const fsdp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

void fsdp_default_params(fsdp_params* p) {
  if (!p) return;
  // fsd_path_planning/config.py:33-41 (sorting), :48 (fitting), :55-59 (path), :124-129 + full_pipeline.py:65 (matching)
  p->max_n_neighbors = 5;
  p->max_dist = 6.5;
  p->max_dist_to_first = 6.0;
  p->max_length = 12;
  p->threshold_directional_angle = 40 * FSDP_DEG;  // np.deg2rad(40)
  p->threshold_absolute_angle = 65 * FSDP_DEG;
  p->use_unknown_cones = 1;
  p->smoothing = 0.2;
  p->predict_every = 0.1;
  p->max_deg = 3;
  p->maximal_distance_for_valid_path = 5;
  p->mpc_path_length = 20;
  p->mpc_prediction_horizon = 40;
  p->min_track_width = 3;
  p->max_search_range = 5;
  p->max_search_angle = 50 * FSDP_DEG;
  p->matches_should_be_monotonic = 0;
}

// what the kernels can take: structural parameters within the compiled capacities, the fixed ones at their values
static const char* check_params(const fsdp_params& p) {
#define FSDP_STR2(x) #x
#define FSDP_STR(x) FSDP_STR2(x)
  if (p.max_n_neighbors < 1 || p.max_n_neighbors > KNN)
    return "max_n_neighbors must be in 1.." FSDP_STR(FSDP_MAX_NEIGHBORS) " (this build's shapes; the wide build takes 8: include/fsdp.h)";
  if (p.max_length < 3 || p.max_length > MAX_LEN)
    return "max_length must be in 3.." FSDP_STR(FSDP_MAX_LEN) " (this build's shapes; the wide build takes 16: include/fsdp.h)";
  if (!(p.max_dist > 0) || !(p.max_dist_to_first > 0)) return "max_dist / max_dist_to_first must be positive";
  if (!(p.smoothing > 0) || !(p.predict_every > 0)) return "smoothing / predict_every must be positive";
  if (!(p.mpc_path_length > 0) || !(p.maximal_distance_for_valid_path >= 0)) return "mpc_path_length must be positive";
  if (!(p.min_track_width > 0) || !(p.max_search_range > 0)) return "min_track_width / max_search_range must be positive";
  if (p.max_deg < 1 || p.max_deg > 3) return "max_deg must be in 1..3";
  if (p.mpc_prediction_horizon < 1 || p.mpc_prediction_horizon > FSDP_PATH_POINTS)
    return "mpc_prediction_horizon must be in 1.." FSDP_STR(FSDP_PATH_POINTS) " (rows of a result path in this build; the wide build holds 64: include/fsdp.h)";
  // the dense path update (fit #1 evaluated every predict_every over <= ~80 m) must fit the working polyline
  if (p.predict_every < 0.05) return "predict_every below 0.05 exceeds the working polyline capacity";
  // the refit is evaluated every predict_every up to 1.5 * mpc_path_length (core_calculate_path.py:248-251) into the same
  // polyline; the extension may add 50 points more (:301-331)
  if (std::ceil(p.mpc_path_length * 1.5 / p.predict_every) + 51 > PATH_CAP)
    return "mpc_path_length * 1.5 / predict_every exceeds the working polyline capacity (1408 points)";
  return nullptr;
}

int fsdp_create(int device, int mission, const fsdp_params* params, fsdp_ctx** out) {
  *out = nullptr;
  fsdp_params pp;
  fsdp_default_params(&pp);
  if (params) pp = *params;
  if (const char* why = check_params(pp)) {
    g_create_error = std::string("fsdp_create: ") + why;
    return 1;
  }
  int n = fsdp_device_count();
  if (n <= 0) {
    g_create_error = "no HIP device visible (libfsdp_hip.so has no CPU fallback)";
    return 1;
  }
  if (device < 0 || device >= n) {
    g_create_error = "device index out of range";
    return 1;
  }
  // utils/mission_types.py:11-25: acceleration = 1, skidpad = 2, ebs_test = 5 use a relocalizer (full_pipeline.py:46-50).
  // Skidpad state lives on the device (fsdp_skidpad_*).  The acceleration relocalizer is a one-off line fit per planner
  // that the host does (acceleration.py, explicit seed); the device side of those two missions is the ordinary path
  // stage with fsdp_set_global_path and empty cone lists.
  fsdp_ctx* c = new fsdp_ctx();
  c->device = device;
  c->mission = mission;
  for (int i = 0; i < FSDP_MAX_OVERLAP; i++) c->slot[i].index = i;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->slot[0].stream.h, hipStreamNonBlocking);
  c->stream = c->slot[0].stream;
  for (int i = 0; i < 8 && e == hipSuccess; i++) e = hipEventCreate(&c->ev[i].h);
  c->params.max_n_neighbors = pp.max_n_neighbors;
  c->params.max_length = pp.max_length;
  c->params.max_dist = pp.max_dist;
  c->params.max_dist_to_first = pp.max_dist_to_first;
  c->params.threshold_directional_angle = pp.threshold_directional_angle;
  c->params.threshold_absolute_angle = pp.threshold_absolute_angle;
  c->params.min_track_width = pp.min_track_width;
  c->params.max_search_range = pp.max_search_range;
  c->params.max_search_angle = pp.max_search_angle;
  c->params.smoothing = pp.smoothing;
  c->params.predict_every = pp.predict_every;
  c->params.maximal_distance_for_valid_path = pp.maximal_distance_for_valid_path;
  c->params.mpc_path_length = pp.mpc_path_length;
  c->params.max_deg = pp.max_deg;
  c->params.horizon = pp.mpc_prediction_horizon;
  c->params.matches_should_be_monotonic = pp.matches_should_be_monotonic ? 1 : 0;
  c->params.use_unknown_cones = pp.use_unknown_cones ? 1 : 0;
  c->params.retry_pack_min = 512;
  c->params.centers_cap = 0;
  c->params.centers = nullptr;
  c->params.n_centers = nullptr;
  if (e == hipSuccess) e = c->d_params.reserve(1);
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_params, &c->params, sizeof(Params), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = c->d_default_path.reserve((size_t)PATH_POINTS * 4);
  if (e != hipSuccess) {
    g_create_error = std::string("fsdp_create: ") + hipGetErrorString(e);
    delete c;
    return 2;
  }
  // constant initial previous path: almost-straight chord (path_calculator_helpers.py:26-68) fitted and
  // parameterized on the device (core_calculate_path.py:103-121)
  {
    double chord[CHORD_POINTS][2];
    default_chord_points(chord);
    DeviceBuf<double> d_arena0;
    e = c->d_chord.reserve(sizeof(chord) / sizeof(double));
    if (e == hipSuccess) e = d_arena0.reserve(ARENA_DOUBLES);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_chord, chord, sizeof(chord), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(default_path_kernel, dim3(1), dim3(WAVE), 0, c->stream, c->d_chord, d_arena0, c->d_default_path, c->d_params);
      e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) {
      g_create_error = std::string("fsdp_create(default path): ") + hipGetErrorString(e);
      delete c;
      return 2;
    }
  }
  *out = c;
  return 0;
}

void fsdp_destroy(fsdp_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (int i = 0; i < FSDP_MAX_OVERLAP; i++)
    if (c->slot[i].stream) (void)hipStreamSynchronize(c->slot[i].stream);
  (void)fsdp_comm_destroy(c);
  delete c;  // (every buffer, stream and event goes with its owner)
}

// ---- page-locked host memory for the asynchronous entry points ----------------------------------------------------------
void* fsdp_host_alloc(size_t bytes) {
  void* p = nullptr;
  // portable + mapped: a buffer allocated while one GPU is current is read and written by the kernels of any context's GPU
  // (multi.py drives every GPU of a node from one process and stages all shards in buffers of this kind)
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
void fsdp_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}
int fsdp_host_register(void* p, size_t bytes) {
  if (!p || !bytes) return 1;
  if (hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped) != hipSuccess) {
    (void)hipGetLastError();
    return 2;
  }
  return 0;
}
int fsdp_host_unregister(void* p) {
  if (!p) return 1;
  if (hipHostUnregister(p) != hipSuccess) {
    (void)hipGetLastError();
    return 2;
  }
  return 0;
}

int fsdp_host_is_pinned(const void* p, size_t bytes) { return (p && is_pinned(p, bytes)) ? 1 : 0; }

// ---- the resident batch ------------------------------------------------------------------------------------------------
int fsdp_upload(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses) {
  if (!c) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_upload");
  HIP_TRY(c, hipSetDevice(c->device));
  Batch b;
  if (int rc = check_batch(c, n_frames, off, cones, poses, nullptr, &b)) return rc;
  if (int rc = sync_all(c)) return rc;  // passes in flight still read the old inputs
  c->resident = false;  // (until the new batch stands: a failed upload leaves no batch to plan)
  if (int rc = ensure_slots(c, n_frames > 0 ? n_frames : 1)) return rc;
  if (int rc = upload_inputs(c, c->res, c->stream, b)) return rc;
  c->res_rows = b.total;
  c->resident = true;
  c->res_checked = false;
  c->last = fsdp_ctx::LastPass();  // (no pass has planned this batch yet)
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the other slots' streams read these inputs too; the caller's buffers are free again
  return 0;
}

int fsdp_set_overlap(fsdp_ctx* c, int depth) {
  if (!c || depth < 1 || depth > FSDP_MAX_OVERLAP) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_set_overlap");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sync_all(c)) return rc;
  // a smaller depth gives the slots beyond it back — their buffers AND their streams: every stream holds one of the GPU's hardware
  // queues, which all contexts and processes on the device share (a MultiPlanner next to a context that once ran twenty passes in
  // flight planned 3.9 instead of 5.1 M frames/s until those queues were released)
  for (int i = depth; i < FSDP_MAX_OVERLAP; i++) {
    Work& w = c->slot[i];
    if (!w.stream && !w.buf.d_sort && !w.h_trailer) continue;
    release_slot(w);
  }
  c->overlap = depth;
  c->turn = 0;
  if (c->last.slot >= depth) c->last = fsdp_ctx::LastPass();  // (released above)
  c->last_ticket_slot = -1;
  for (bool& p : c->primed) p = false;  // the kernels of a pass depend on the frames in flight (launch_path)
  for (int& p : c->gang_primed) p = 0;
  // (slot 0 may have grown for ganged passes: the other slots keep the size of a plain pass)
  const size_t plain = c->gang_grown_from ? std::max(c->gang_grown_from, c->resident ? (size_t)c->res.n_frames : (size_t)0) : c->slot[0].buf.frames();
  return ensure_slots(c, std::max(1, (int)plain));
}

int fsdp_run(fsdp_ctx* c) {
  if (!c) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_run");
  if (!c->resident) {
    c->err = "fsdp_run: no resident batch (fsdp_upload first)";
    return 1;
  }
  if (c->res.n_frames == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  const int si = (c->overlap > 1) ? (int)(c->turn++ % (unsigned)c->overlap) : 0;
  Work& q = c->slot[si];
  // the slot's previous pass may still need its routes: settle it before its buffers are reused (passes over a checked
  // resident batch carry exactly the routes they need: nothing to settle, no host wait)
  if (q.unverified && !(c->res_checked && q.pass_in == &c->res)) {
    HIP_TRY(c, hipStreamSynchronize(q.stream));
    if (int rc = verify_pass(c, q)) return rc;
  }
  if (int rc = launch_pass(c, q, c->res, Pass())) return rc;
  HIP_TRY(c, hipGetLastError());
  return 0;
}

int fsdp_resident_frames(const fsdp_ctx* c) { return c ? c->last.n : 0; }

int fsdp_sync(fsdp_ctx* c) {
  if (!c) return 1;
  HIP_TRY(c, hipSetDevice(c->device));
  return sync_all(c);
}

int fsdp_download(fsdp_ctx* c, fsdp_frame_result* results) {
  if (!c) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_download");
  if (c->last.slot < 0 || !c->last.in_result) {
    c->err = "fsdp_download: the most recent pass left no results on the device (it was a ticket, a blocking call or a skidpad step, or no "
             "fsdp_run has followed fsdp_upload / fsdp_set_overlap)";
    return 1;
  }
  const int n = c->last.n;
  if (!results) return 1;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sync_all(c)) return rc;
  Work& q = c->slot[c->last.slot];  // the most recent pass
  HIP_TRY(c, hipMemcpyAsync(results, q.buf.d_result + c->last.offset, sizeof(fsdp_frame_result) * (size_t)n, hipMemcpyDeviceToHost, q.stream));
  HIP_TRY(c, hipStreamSynchronize(q.stream));
  return 0;
}

int fsdp_set_previous_paths(fsdp_ctx* c, const double* prev_paths) {
  if (!c) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_set_previous_paths");
  HIP_TRY(c, hipSetDevice(c->device));
  if (!prev_paths) {
    c->res.use_prev = false;
    return 0;
  }
  if (!c->resident || c->res.n_frames <= 0) {
    c->err = "fsdp_set_previous_paths: upload a batch first";
    return 1;
  }
  if (int rc = sync_all(c)) return rc;
  HIP_TRY(c, c->res.reserve((size_t)c->res.n_frames, c->res.cone_rows(), true));
  HIP_TRY(c, copy_sync(c, c->res.d_prev, prev_paths, sizeof(double) * PATH_POINTS * 4 * (size_t)c->res.n_frames, hipMemcpyHostToDevice));
  c->res.use_prev = true;
  c->res_checked = false;
  return 0;
}

int fsdp_set_global_path(fsdp_ctx* c, const double* xy, int n) {
  if (!c || n < 0 || (n > 0 && !xy)) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_set_global_path");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sync_all(c)) return rc;
  c->d_gpath.reset();
  c->n_gpath = 0;
  c->res_checked = false;
  if (n == 0) return 0;
  HIP_TRY(c, c->d_gpath.reserve(2 * (size_t)n));
  HIP_TRY(c, copy_sync(c, c->d_gpath, xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice));
  c->n_gpath = n;
  return 0;
}

int fsdp_set_global_path_table(fsdp_ctx* c, const double* xy, const int32_t* path_offsets, int n_paths) {
  if (!c) return 1;
  const std::string who = "fsdp_set_global_path_table";
  if (c->outstanding) return busy_error(c, who.c_str());
  if (c->mission == 2) {
    c->err = who + ": a skidpad context plans along its own path table (fsdp_skidpad_set_tables)";
    return 1;
  }
  if (n_paths < 0 || (n_paths > 0 && !path_offsets)) {
    c->err = who + ": n_paths must be >= 0, and path_offsets given with n_paths > 0";
    return 1;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = refuse_device_pointers(c, who.c_str(), {{"xy", xy}, {"path_offsets", path_offsets}})) return rc;
  if (n_paths > 0 && path_offsets[0] != 0) {
    c->err = who + ": path_offsets[0] must be 0";
    return 1;
  }
  for (int k = 0; k < n_paths; k++)
    if (path_offsets[k + 1] < path_offsets[k]) {
      c->err = who + ": path_offsets must be non-decreasing (path_offsets[" + std::to_string(k + 1) + "] = " + std::to_string(path_offsets[k + 1]) + " < " +
               std::to_string(path_offsets[k]) + ")";
      return 1;
    }
  const size_t points = n_paths > 0 ? (size_t)path_offsets[n_paths] : 0;
  if (points > 0 && !xy) {
    c->err = who + ": xy is NULL";
    return 1;
  }
  if (int rc = sync_all(c)) return rc;
  c->d_gpt_xy.reset();
  c->d_gpt_off.reset();
  c->n_gpt = 0;
  if (n_paths == 0) return 0;
  HIP_TRY(c, c->d_gpt_xy.reserve(std::max<size_t>(2 * points, 2)));
  HIP_TRY(c, c->d_gpt_off.reserve((size_t)n_paths + 1));
  if (points > 0) HIP_TRY(c, copy_sync(c, c->d_gpt_xy, xy, sizeof(double) * 2 * points, hipMemcpyHostToDevice));
  HIP_TRY(c, copy_sync(c, c->d_gpt_off, path_offsets, sizeof(int32_t) * ((size_t)n_paths + 1), hipMemcpyHostToDevice));
  c->n_gpt = n_paths;
  return 0;
}

// ---- streams of batches: submit / collect ------------------------------------------------------------------------------
// One batch per ticket.  Ticket t goes to slot t % depth and is queued on that slot's stream behind the slot's previous
// ticket (up to SLOT_QUEUE per slot): host -> device of the batch, the kernels of its pass and device -> host of its results
// are enqueued by fsdp_submit, which returns at once.  Page-locked buffers (fsdp_host_alloc / fsdp_host_register) are read
// and written by kernels of the stream itself (stage_in_kernel, assemble_kernel); pageable ones work, but their copies are
// staged by the runtime and block the caller.
static Work::Ticket* find_ticket(fsdp_ctx* c, long long ticket, Work** slot) {
  if (ticket < 0) return nullptr;
  for (int i = 0; i < FSDP_MAX_OVERLAP; i++)
    for (Work::Ticket& t : c->slot[i].tk)
      if (t.id == ticket) {
        if (slot) *slot = &c->slot[i];
        return &t;
      }
  return nullptr;
}

// A pageable batch of up to SMALL_BATCH_BYTES is packed into the ticket's own page-locked block by the host (a memcpy of a few KB)
// and then treated like any page-locked batch: the sorting kernel reads it over PCIe, no copy command is issued at all — three or
// four hipMemcpyAsync calls from pageable memory cost a single-frame call ~30 us of its ~860.
constexpr size_t SMALL_BATCH_BYTES = 256 * 1024;

// ---- sequence tickets ---------------------------------------------------------------------------------------------------------
constexpr size_t SEQ_PREV_DOUBLES = (size_t)PATH_POINTS * 4;  // one planner's row of initial_prev / final_prev

// the run-head list and the planners' rows of slot q for a sequence pass of `frames` frames (the slot's stream is idle where
// something has to grow: enqueue_ticket)
static int ensure_sequence(fsdp_ctx* c, Work& q, const Work::SeqPass& sq, size_t frames) {
  const hipError_t e = q.seq_buf.reserve(frames, (size_t)sq.s.n);
  if (e == hipSuccess) return 0;
  c->err = std::string(sq.who) + ": " + hipGetErrorString(e);
  return 2;
}

// The rows of the caller's arrays a planner slice touches, first to last: n_steps segments `total` frames apart
struct SliceExtent {
  size_t span_frames;            // frames from the slice's first to behind its last: (n_steps - 1) * total + n
  int32_t cone_lo = 0, cone_hi = 0;  // cone rows [lo, hi) the segments read
};
static SliceExtent slice_extent(const SeqSlice& s, const SeqSeg* seg) {
  SliceExtent x;
  x.span_frames = (size_t)(s.n_steps - 1) * (size_t)s.total + (size_t)s.n;
  bool any = false;
  for (int t = 0; t < s.n_steps; t++) {
    const int32_t cnt = seg[t + 1].dst - seg[t].dst;
    if (cnt == 0) continue;
    x.cone_lo = any ? std::min(x.cone_lo, seg[t].src) : seg[t].src;
    x.cone_hi = any ? std::max(x.cone_hi, seg[t].src + cnt) : seg[t].src + cnt;
    any = true;
  }
  return x;
}
// every row seq_slice_in_kernel reads is page-locked
static bool slice_inputs_pinned(const Work::SeqPass& sq, const SliceExtent& x) {
  const SeqSlice& s = sq.s;
  return is_pinned(sq.off + s.lo, sizeof(int32_t) * (x.span_frames + 1)) && is_pinned(sq.poses + 4 * (size_t)s.lo, sizeof(double) * 4 * x.span_frames) &&
         (x.cone_hi == x.cone_lo || is_pinned(sq.cones + 3 * (size_t)x.cone_lo, sizeof(double) * 3 * (size_t)(x.cone_hi - x.cone_lo))) &&
         (!sq.init || is_pinned(sq.init, sizeof(double) * SEQ_PREV_DOUBLES * (size_t)s.n));
}

// A pageable planner slice, packed by the host into the ticket's page-locked block in the call's own order: from there on it
// is a contiguous page-locked batch like any other (read by the sorting kernel itself).
static int pack_slice(fsdp_ctx* c, Work::Ticket& t, Batch* b) {
  const Work::SeqPass& sq = t.sq;
  const SeqSlice& s = sq.s;
  const size_t nf = (size_t)s.frames(), rows = (size_t)t.h_seg[s.n_steps].dst;
  const size_t off_bytes = (sizeof(int32_t) * (nf + 1) + 15) & ~(size_t)15, cone_bytes = sizeof(double) * 3 * rows, pose_bytes = sizeof(double) * 4 * nf;
  HIP_TRY(c, t.h_in.reserve(off_bytes + cone_bytes + pose_bytes, 16384, Pin::Mapped));
  int32_t* so = (int32_t*)t.h_in.get();
  double* sc = (double*)(t.h_in + off_bytes);
  double* sp = (double*)(t.h_in + off_bytes + cone_bytes);
  for (int step = 0; step < s.n_steps; step++) {
    const SeqSeg g = t.h_seg[step];
    const size_t r = (size_t)seq_rec_frame(s, step, 0), f = (size_t)step * (size_t)s.n;
    for (int p = 0; p < s.n; p++) so[f + (size_t)p] = (int32_t)seq_dense_offset(g, sq.off[r + (size_t)p]);  // (within [0, rows]: the segments were checked)
    const size_t cnt = (size_t)(t.h_seg[step + 1].dst - g.dst);
    if (cnt) memcpy(sc + 3 * (size_t)g.dst, sq.cones + 3 * (size_t)g.src, sizeof(double) * 3 * cnt);
    memcpy(sp + 4 * f, sq.poses + 4 * r, sizeof(double) * 4 * (size_t)s.n);
  }
  so[nf] = (int32_t)rows;
  *b = Batch{(int)nf, so, sc, sp, nullptr, rows, b->max_cones};
  return 0;
}

// The path ids of a sequence ticket's frames (fsdp_*_sequence_paths), dense in the call's frame order, gathered from the
// recording's array into the ticket's page-locked block, where the path kernels and the chain kernel read them: 4 bytes per frame,
// in the loop that checks them against the table.  Nothing is enqueued before it; a repeated pass gathers, and checks, them again.
static int gather_sequence_ids(fsdp_ctx* c, Work::Ticket& t) {
  const Work::SeqPass& sq = t.sq;
  const SeqSlice& s = sq.s;
  HIP_TRY(c, t.h_ids.reserve((size_t)s.frames(), 1024, Pin::Mapped));
  int32_t* dst = t.h_ids.get();
  for (int step = 0; step < s.n_steps; step++) {
    const size_t r = (size_t)seq_rec_frame(s, step, 0);
    for (int p = 0; p < s.n; p++) {
      const int32_t id = sq.path_ids[r + (size_t)p];
      if (id < -1 || id >= c->n_gpt) {
        c->err = std::string(sq.who) + ": path_ids[" + std::to_string(r + (size_t)p) + "] = " + std::to_string(id) + " lies outside [-1, n_paths = " +
                 std::to_string(c->n_gpt) + ") (-1: the frame plans from its cones)";
        return 1;
      }
      *dst++ = id;
    }
  }
  return 0;
}

// enqueue ticket t's batch on slot q: inputs, the pass with its results' way back, the ticket's event.  The pass is described by
// the ticket alone (its Pass is built here from the ticket's fields, nothing is read from the call in progress): fsdp_collect's
// rerun, with force_routes, is this function of the same data.
static int enqueue_ticket(fsdp_ctx* c, Work& q, Work::Ticket& t, bool force_routes) {
  Batch b = t.batch;
  const int n = b.n;
  Work::SeqPass* sq = t.sq.on ? &t.sq : nullptr;
  const bool sliced = sq && !sq->s.whole();
  Pass pass;
  pass.sq = sq;
  pass.force_routes = force_routes;
  pass.in_flight = t.in_flight;
  pass.compact = t.compact;
  pass.trailer = (int)(&t - q.tk);  // the ticket's own trailer
  if (t.cache_lo >= 0) {
    pass.sort.kind = SortVariant::CACHED;
    pass.sort.cache = cache_view(c, t.cache_lo);  // (the chunk's frames are planners cache_lo.. of the sorting cache)
  } else if (sq && sq->cached) {
    pass.sort.kind = SortVariant::SPEC;
  }
  if (sq && sq->path_ids)
    if (int rc = gather_sequence_ids(c, t)) return rc;
  // a bigger batch than the slot has seen: its buffers are replaced — not under the feet of the passes queued on the stream
  if ((size_t)n > q.buf.frames() || !q.in.fits((size_t)n, b.total, b.prev != nullptr) || (sq && !q.seq_buf.fits((size_t)n, (size_t)sq->s.n)))
    HIP_TRY(c, hipStreamSynchronize(q.stream));
  if (int rc = ensure_work(c, q, n > 0 ? n : 1)) return rc;
  if (sq)
    if (int rc = ensure_sequence(c, q, *sq, (size_t)n)) return rc;
  const size_t init_bytes = sq ? sizeof(double) * SEQ_PREV_DOUBLES * (size_t)sq->s.n : 0;
  bool slice_in = false;  // a page-locked planner slice: seq_slice_in_kernel leaves the device copies
  SliceExtent ext;
  if (sliced) {
    // (the segments again, from the arrays the submit checked: a repeated pass reads them like the batch itself)
    HIP_TRY(c, t.h_seg.reserve((size_t)sq->s.n_steps + 1, 64, Pin::Mapped));
    if (seq_slice_segments(sq->s, sq->off, t.h_seg, nullptr) != 0 || (size_t)t.h_seg[sq->s.n_steps].dst != b.total) {
      c->err = std::string(sq->who) + ": cone_offsets changed between submit and collect";
      return 1;
    }
    ext = slice_extent(sq->s, t.h_seg);
    slice_in = slice_inputs_pinned(*sq, ext);
    if (!slice_in)
      if (int rc = pack_slice(c, t, &b)) return rc;
  }
  bool in_pinned = slice_in || sliced || inputs_pinned(b);
  const size_t off_bytes = (sizeof(int32_t) * ((size_t)n + 1) + 15) & ~(size_t)15, cone_bytes = sizeof(double) * 3 * b.total,
               pose_bytes = sizeof(double) * 4 * (size_t)n, prev_bytes = b.prev ? sizeof(double) * PATH_POINTS * 4 * (size_t)n : 0;
  const size_t in_bytes = off_bytes + cone_bytes + pose_bytes + prev_bytes;
  if (!in_pinned && n > 0 && in_bytes <= SMALL_BATCH_BYTES) {
    // (the block's previous user — this ticket entry's previous batch — was collected before the entry was handed out again)
    HIP_TRY(c, t.h_in.reserve(in_bytes, 16384, Pin::Mapped));
    int32_t* so = (int32_t*)t.h_in.get();
    double* sc = (double*)(t.h_in + off_bytes);
    double* sp = (double*)(t.h_in + off_bytes + cone_bytes);
    double* sv = (double*)(t.h_in + off_bytes + cone_bytes + pose_bytes);
    for (int i = 0; i <= n; i++) so[i] = b.off[i] - b.off[0];
    if (cone_bytes) memcpy(sc, b.cones + 3 * (size_t)b.off[0], cone_bytes);
    memcpy(sp, b.poses, pose_bytes);
    if (b.prev) memcpy(sv, b.prev, prev_bytes);
    b = Batch{n, so, sc, sp, b.prev ? sv : nullptr, b.total, b.max_cones};
    in_pinned = true;
  }
  if (slice_in) {
    if (int rc = take_batch(c, q.in, b)) return rc;
    const SeqSlice& s = sq->s;
    fsdp_seq_slice_in_args a;
    a.s = s;
    a.seg = (const SeqSeg*)device_view(t.h_seg);
    a.src_off = (const int32_t*)device_view(sq->off + s.lo);
    a.src_cones = (const double*)device_view(ext.cone_hi > ext.cone_lo ? sq->cones + 3 * (size_t)ext.cone_lo : sq->poses);  // (never read when no segment holds a cone)
    a.src_poses = (const double*)device_view(sq->poses + 4 * (size_t)s.lo);
    a.src_init = sq->init ? (const double*)device_view(sq->init) : nullptr;
    a.cone_base = ext.cone_lo;
    a.src_rows = (long long)ext.cone_hi - ext.cone_lo;
    a.rows = (long long)b.total;
    a.dst_off = q.in.d_off;
    a.dst_cones = q.in.d_cones;
    a.dst_poses = q.in.d_poses;
    a.dst_init = q.seq_buf.d_seq_init;
    if (!a.seg || !a.src_off || !a.src_cones || !a.src_poses) {
      c->err = "internal: a slice's page-locked arrays are not mapped into the device's address space";
      return 2;
    }
    fsdp_seq_launch_slice_in(q.stream, &a);
  } else if (in_pinned && c->params.use_unknown_cones && pass.sort.kind != SortVariant::SPEC) {  // (the speculative kernels read their predecessors' cones: device copies first)
    // the pass's sorting kernel reads the batch from the page-locked buffers and leaves the device copies (StageIn)
    if (int rc = take_batch(c, q.in, b)) return rc;
    StageIn& st = pass.stage;
    st.src_off = (const int32_t*)device_view(b.off);
    st.base = b.off[0];
    // (the view of the slice's first row, addressed by offsets relative to base; never read when total = 0)
    st.src_cones = (const double*)device_view(b.total ? b.cones + 3 * (size_t)b.off[0] : b.poses);
    st.src_poses = (const double*)device_view(b.poses);
    st.src_prev = b.prev ? (const double*)device_view(b.prev) : nullptr;
    st.dst_off = q.in.d_off;
    st.dst_cones = q.in.d_cones;
    st.dst_poses = q.in.d_poses;
    st.dst_prev = q.in.d_prev;
    st.n_frames = n;
  } else if (in_pinned) {
    if (int rc = stage_inputs(c, q.in, q.stream, b)) return rc;
  } else if (int rc = upload_inputs(c, q.in, q.stream, b)) {
    return rc;
  }
  if (t.path_ids && n > 0) {
    // The pass's path ids (fsdp_submit_paths), read by the path kernels themselves: the caller's array where it is page-locked, else
    // the ticket's own block (an int per frame; a repeated pass stages them again from the caller's array, like the batch)
    const int32_t* ids = t.path_ids;
    if (!is_pinned(ids, sizeof(int32_t) * (size_t)n)) {
      HIP_TRY(c, t.h_ids.reserve((size_t)n, 1024, Pin::Mapped));
      memcpy(t.h_ids.get(), ids, sizeof(int32_t) * (size_t)n);
      ids = t.h_ids;
    }
    pass.path_ids = (const int32_t*)device_view(ids);
    if (!pass.path_ids) {
      c->err = "internal: path_ids is not mapped into the device's address space";
      return 2;
    }
  } else if (sq && sq->path_ids && n > 0) {  // (a sequence ticket's ids: gathered into the ticket's block above)
    pass.path_ids = (const int32_t*)device_view(t.h_ids.get());
    if (!pass.path_ids) {
      c->err = "internal: path_ids is not mapped into the device's address space";
      return 2;
    }
  }
  // (the initial_prev rows of a sequence pass: adjacent also for a slice; seq_slice_in_kernel brought a page-locked slice's along)
  if (sq && sq->init && !slice_in) HIP_TRY(c, hipMemcpyAsync(q.seq_buf.d_seq_init, sq->init, init_bytes, hipMemcpyHostToDevice, q.stream));
  t.via_stage = false;
  if (n > 0) {
    // Results always leave the GPU inside the pass's last kernel, written over PCIe into page-locked memory: the caller's own buffer,
    // or — for a pageable one — the ticket's block, which fsdp_collect copies out (no copy command on the stream either way).
    // A planner slice's records are n_steps segments of the caller's array: seq_slice_out_kernel moves them there from the slot's
    // result block when the array (and final_prev) is page-locked; else they go through the ticket's block, dense, like any
    // pageable caller's, and fsdp_collect copies the segments out.
    char* slice_dst = sliced ? (char*)t.user_results + t.rec_bytes() * (size_t)sq->s.lo : nullptr;
    const bool slice_out = sliced && is_pinned(slice_dst, t.rec_bytes() * ext.span_frames) && (!sq->final_prev || is_pinned(sq->final_prev, init_bytes));
    if (!slice_out)  // (a slice that cannot go out in place is staged whatever its array is: NULL is never page-locked)
      if (int rc = host_target(c, sliced ? nullptr : t.user_results, t.rec_bytes() * (size_t)n, t.h_stage, (size_t)n, 64, "result block",
                               &pass.host, &t.via_stage))
        return rc;
    if (sq) {
      // final_prev leaves the GPU inside seq_final_kernel, written into page-locked memory like the records: the caller's rows, or
      // the ticket's block (the slot's d_seq_final serves the slot's next ticket before this one is collected)
      sq->fin_staged = false;
      sq->final_dev = slice_out ? q.seq_buf.d_seq_final : nullptr;
      if (sq->final_prev && !slice_out)
        if (int rc = host_target(c, sq->final_prev, init_bytes, t.h_fin, SEQ_PREV_DOUBLES * (size_t)sq->s.n, 64 * SEQ_PREV_DOUBLES,
                                 "final_prev block", &sq->final_dev, &sq->fin_staged))
          return rc;
    }
    if (int rc = launch_pass(c, q, q.in, pass)) return rc;
    t.seq = q.seq;
    t.ran_big = q.ran_big;
    t.ran_retry = q.ran_retry;
    if (slice_out) {
      fsdp_seq_slice_out_args a;
      a.s = sq->s;
      a.rec_bytes = (int)t.rec_bytes();
      a.src_records = q.buf.d_result;
      a.dst_records = device_view(slice_dst);
      a.src_final = q.seq_buf.d_seq_final;
      a.dst_final = sq->final_prev ? (double*)device_view(sq->final_prev) : nullptr;
      if (!a.dst_records || (sq->final_prev && !a.dst_final)) {
        c->err = "internal: a slice's result arrays are not mapped into the device's address space";
        return 2;
      }
      fsdp_seq_launch_slice_out(q.stream, &a);
    }
    // A planner slice, by whichever route, is never the context's "most recent pass": its frames are the call's dense order, not the
    // caller's recording, so fsdp_resident_frames / fsdp_download / fsdp_debug_* have nothing to hand out.  The whole call stays what
    // an fsdp_submit ticket is to them (launch_pass: its frame count, results not in the slot's block).
    if (sliced) c->last = fsdp_ctx::LastPass();
    HIP_TRY(c, hipGetLastError());
  }
  if (!t.done) HIP_TRY(c, hipEventCreateWithFlags(&t.done.h, hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(t.done, q.stream));
  return 0;
}

// The slot with the fewest tickets queued, starting from the one after the previous ticket's (in-order traffic: round robin),
// with its stream and a settled state, and a free ticket entry of it; 4: every entry is taken.
static int free_ticket(fsdp_ctx* c, const char* who, int n_frames, Work** slot, Work::Ticket** ticket) {
  int si = -1, best = SLOT_QUEUE;
  long long oldest = -1;
  for (int k = 0; k < c->overlap; k++) {
    const int i = (c->last_ticket_slot + 1 + k) % c->overlap;
    int cnt = 0;
    for (const Work::Ticket& e : c->slot[i].tk) {
      if (e.id < 0) continue;
      cnt++;
      if (oldest < 0 || e.id < oldest) oldest = e.id;
    }
    if (cnt < best) {
      best = cnt;
      si = i;
    }
  }
  if (si < 0) {
    c->err = std::string(who) + ": " + std::to_string(c->outstanding) + " tickets outstanding (" + std::to_string(SLOT_QUEUE) + " per slot, " +
             std::to_string(c->overlap) + " slots): collect one first, e.g. ticket " + std::to_string(oldest);
    return 4;
  }
  c->last_ticket_slot = si;
  Work& q = c->slot[si];
  Work::Ticket* t = nullptr;
  for (Work::Ticket& e : q.tk)
    if (e.id < 0 && !t) t = &e;
  if (!q.stream) {
    if (int rc = ensure_work(c, q, n_frames > 0 ? n_frames : 1)) return rc;
  }
  if (q.unverified) {  // an fsdp_run pass nobody waited for
    HIP_TRY(c, hipStreamSynchronize(q.stream));
    if (int rc = verify_pass(c, q)) return rc;
  }
  *slot = &q;
  *ticket = t;
  return 0;
}

// What the caller of issue_ticket says about the pass; the rest of the ticket is enqueue_ticket's
struct TicketSpec {
  Batch batch;
  long long in_flight = 0;               // frames on the GPU the pass is planned for
  fsdp_frame_result* results = nullptr;  // the caller's records, full or compact
  bool compact = false;
  int cache_lo = -1;                     // >= 0: a chunk of a call that advances the sorting cache, its frame 0 is this planner
  Work::SeqPass sq;                      // on: a sequence pass
  const int32_t* path_ids = nullptr;     // a pass with per-frame global paths: the caller's ids (checked by the submit)
};

// The one way a pass becomes a ticket (fsdp_submit*, the chunks of a blocking call, the sequence calls): entry t of slot q gets its
// description and is enqueued.  0: issued as t.id and counted as outstanding (a blocking call collects it and gives the number
// back: c->next_ticket).  Else no ticket went out, and an error return means the buffers are the caller's again: part of the batch
// may already be queued on the slot's stream — kernels that read his buffers or write his page-locked results — so it is waited
// for here (round-3 advisor).  (A pass that found no room left the buffers that failed to grow empty: the next one grows them again.)
static int issue_ticket(fsdp_ctx* c, Work& q, Work::Ticket& t, const TicketSpec& spec) {
  t.batch = spec.batch;
  t.skid = false;
  t.in_flight = spec.in_flight;
  t.user_results = spec.results;
  t.user_info = nullptr;
  t.compact = spec.compact;
  t.sq = spec.sq;
  t.cache_lo = spec.cache_lo;
  t.path_ids = spec.path_ids;
  if (int rc = enqueue_ticket(c, q, t, false)) {
    (void)hipStreamSynchronize(q.stream);
    (void)hipGetLastError();
    t.release();
    return rc;
  }
  t.id = c->next_ticket++;
  c->outstanding++;
  return 0;
}

// What the calls that carry path ids refuse alike (fsdp_submit_paths*, fsdp_submit_device_paths): a context where an id has no
// single meaning, or nothing to name
static int refuse_paths_call(fsdp_ctx* c, const std::string& who) {
  if (c->d_gpath) {
    c->err = who + ": the context also has a context-wide global path (fsdp_set_global_path), and a context's frames follow either that one or "
                   "the table entries their ids name — fsdp_set_global_path(ctx, NULL, 0) clears it";
    return 1;
  }
  if (c->n_cache > 0) {
    c->err = who + ": the sorting cache is on (it stays a lock-step feature of the calls without path ids: fsdp_sort_cache_reset(ctx, 0) turns it off)";
    return 1;
  }
  if (c->n_gpt == 0) {
    c->err = who + ": the context has no path table (fsdp_set_global_path_table)";
    return 1;
  }
  if (!fsdp_gpt_launch || !fsdp_gpt_launch_ids_scan) {
    c->err = who + ": this library was built without the path table kernels (csrc/gpath_table_lib.hip)";
    return 2;
  }
  return 0;
}

// with_ids: fsdp_submit_paths* (path_ids required with n_frames > 0)
static int submit_impl(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses, const double* prev_paths,
                       fsdp_frame_result* results, long long* ticket, bool compact, bool with_ids = false, const int32_t* path_ids = nullptr) {
  if (!c || !ticket) return 1;
  *ticket = -1;
  const char* who = with_ids ? "fsdp_submit_paths" : "fsdp_submit";
  if (c->mission == 2) {
    c->err = std::string(who) + ": a skidpad context plans through fsdp_skidpad_submit";
    return 1;
  }
  if (n_frames > 0 && !results) {
    c->err = std::string(who) + ": results is NULL";
    return 1;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = refuse_device_pointers(c, who, {{"cone_offsets", off}, {"cones_xyt", cones}, {"poses", poses}, {"prev_paths", prev_paths}, {"results", results}, {"path_ids", path_ids}}))
    return rc;
  if (with_ids) {
    if (int rc = refuse_paths_call(c, who)) return rc;
    if (n_frames > 0 && !path_ids) {
      c->err = std::string(who) + ": path_ids is NULL";
      return 1;
    }
    // (the host can read these ids: an id that names nothing is refused before anything is enqueued)
    for (int i = 0; i < n_frames; i++)
      if (path_ids[i] < -1 || path_ids[i] >= c->n_gpt) {
        c->err = std::string(who) + ": path_ids[" + std::to_string(i) + "] = " + std::to_string(path_ids[i]) + " lies outside [-1, n_paths = " +
                 std::to_string(c->n_gpt) + ") (-1: the frame plans from its cones)";
        return 1;
      }
  }
  Batch b;
  if (int rc = check_batch(c, n_frames, off, cones, poses, prev_paths, &b)) return rc;
  Work* qp = nullptr;
  Work::Ticket* t = nullptr;
  if (int rc = free_ticket(c, who, n_frames, &qp, &t)) return rc;
  TicketSpec spec;
  spec.batch = b;
  spec.in_flight = frames_in_flight(c, n_frames, true);
  spec.results = results;
  spec.compact = compact;
  spec.path_ids = with_ids ? path_ids : nullptr;
  if (int rc = issue_ticket(c, *qp, *t, spec)) return rc;
  *ticket = t->id;
  return 0;
}
int fsdp_submit_paths(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses, const double* prev_paths,
                      const int32_t* path_ids, fsdp_frame_result* results, long long* ticket) {
  return submit_impl(c, n_frames, off, cones, poses, prev_paths, results, ticket, false, true, path_ids);
}
int fsdp_submit_paths_compact(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses, const double* prev_paths,
                              const int32_t* path_ids, fsdp_compact_result* results, long long* ticket) {
  return submit_impl(c, n_frames, off, cones, poses, prev_paths, (fsdp_frame_result*)results, ticket, true, true, path_ids);
}
int fsdp_submit(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses, const double* prev_paths,
                fsdp_frame_result* results, long long* ticket) {
  return submit_impl(c, n_frames, off, cones, poses, prev_paths, results, ticket, false);
}
int fsdp_submit_compact(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses, const double* prev_paths,
                        fsdp_compact_result* results, long long* ticket) {
  return submit_impl(c, n_frames, off, cones, poses, prev_paths, (fsdp_frame_result*)results, ticket, true);
}

// 1: fsdp_collect will not block (unless the pass has to be repeated with a route kernel); 0: still running; < 0: unknown ticket
int fsdp_ticket_done(fsdp_ctx* c, long long ticket) {
  if (!c) return -1;
  Work::Ticket* t = find_ticket(c, ticket, nullptr);
  if (!t) return -1;
  (void)hipSetDevice(c->device);
  if (t->pending && flush_skid(c)) return -1;
  hipError_t e = hipEventQuery(t->done);
  if (e == hipSuccess) return 1;
  (void)hipGetLastError();
  return 0;
}

int fsdp_collect(fsdp_ctx* c, long long ticket) {
  if (!c) return 1;
  Work* qp = nullptr;
  Work::Ticket* tp = find_ticket(c, ticket, &qp);
  if (!tp) {
    c->err = "fsdp_collect: unknown ticket " + std::to_string(ticket);
    return 1;
  }
  Work& q = *qp;
  Work::Ticket& t = *tp;
  int rc = 0;
  hipError_t e = hipSetDevice(c->device);
  if (t.pending)
    if (int frc = flush_skid(c)) return frc;
  if (e == hipSuccess) e = hipEventSynchronize(t.done);
  if (e != hipSuccess) {
    c->err = std::string("fsdp_collect: ") + hipGetErrorString(e);
    rc = 2;
  }
  const int n = t.batch.n;
  if (rc == 0 && n > 0 && !t.skid) {
    // did the pass get the route kernels it needed?  (its own trailer: later passes of the slot write other ones)
    const PassTrailer tr = read_trailer(q, (int)(&t - q.tk));
    if (tr.seq != t.seq) {
      c->err = "internal: trailer of ticket " + std::to_string(ticket) + " overwritten";
      rc = 2;
    } else if (t.dev.on) {
      // (a device ticket ran both routes: nothing is ever rerun — a consumer on the GPU has already read its results)
      if (settle_routes(c, tr, t.ran_big, t.ran_retry, false)) {
        c->err = "internal: device ticket " + std::to_string(ticket) + " lacked a route kernel";
        rc = 2;
      } else if (const int32_t bad = __atomic_load_n(t.h_bad.get(), __ATOMIC_RELAXED); bad >= 0) {
        c->err = "fsdp_collect: counts[" + std::to_string(bad) + "] of device ticket " + std::to_string(ticket) + " lies outside [0, cone_capacity = " +
                 std::to_string(t.dev.cap) + "] (the lowest such frame; every such frame was planned as having 0 cones: the call's outputs are not to be used)";
        rc = 1;
      } else if (const int32_t bad_id = t.dev.path_ids ? __atomic_load_n(t.h_bad.get() + 2, __ATOMIC_RELAXED) : -1; bad_id >= 0) {
        c->err = "fsdp_collect: path_ids[" + std::to_string(bad_id) + "] of device ticket " + std::to_string(ticket) + " lies outside [-1, n_paths = " +
                 std::to_string(c->n_gpt) + ") (the lowest such frame; every such frame was planned from its cones, as with -1: the call's outputs are not to be used)";
        rc = 1;
      }
    } else if (settle_routes(c, tr, t.ran_big, t.ran_retry, false)) {
      // the whole ticket once more, with both route kernels and the kernels of its first pass, behind whatever the slot's
      // stream holds by now (the caller's buffers are still his to leave alone: the batch is read again from them)
      rc = enqueue_ticket(c, q, t, true);
      if (rc != 0) (void)hipStreamSynchronize(q.stream);  // (nothing of the repeated pass is left running over the caller's buffers)
      if (rc == 0 && (e = hipEventSynchronize(t.done)) != hipSuccess) {
        c->err = std::string("fsdp_collect: ") + hipGetErrorString(e);
        rc = 2;
      }
    }
  }
  if (rc == 0 && n > 0 && t.skid && t.dev.on) {
    // A skidpad device ticket.  (No skidpad step is ever run again — the block above is not for them: a step has moved its
    // planners' state on, and a consumer on the GPU has read a device ticket's results.)  The word its out kernel left: no planner
    // that was not relocalized — unless planners were reset since the step was submitted.
    if (t.reloc_epoch == c->skid_reloc_epoch && __atomic_load_n(t.h_bad.get() + 1, __ATOMIC_RELAXED) == 0) c->skid_all_reloc = true;
    if (const int32_t bad = __atomic_load_n(t.h_bad.get(), __ATOMIC_RELAXED); bad >= 0) {
      c->err = "fsdp_collect: counts[" + std::to_string(bad) + "] of device ticket " + std::to_string(ticket) + " lies outside [0, cone_capacity = " +
               std::to_string(t.dev.cap) + "] (the lowest such planner; every such planner took the step as having 0 cones: the call's outputs are not to be used, "
               "and the planners' state has advanced by the step all the same — fsdp_skidpad_reset starts them afresh)";
      rc = 1;
    }
  }
  if (rc == 0 && n > 0) {
    if (t.via_stage && t.sq.on && !t.sq.s.whole()) {  // a planner slice: the ticket's block is dense, the caller's array holds the whole recording
      const SeqSlice& s = t.sq.s;
      const size_t rec = t.rec_bytes(), seg = rec * (size_t)s.n;
      for (int step = 0; step < s.n_steps; step++)
        memcpy((char*)t.user_results + rec * (size_t)seq_rec_frame(s, step, 0), (const char*)t.h_stage.get() + seg * (size_t)step, seg);
    } else if (t.via_stage) {
      memcpy(t.user_results, t.h_stage, t.rec_bytes() * (size_t)n);
    }
    if (t.sq.on) {
      if (t.sq.fin_staged) memcpy(t.sq.final_prev, t.h_fin, sizeof(double) * SEQ_PREV_DOUBLES * (size_t)t.sq.s.n);
      // (the ticket's own trailer word: seq_final_kernel of its pass — of the repeated pass, if there was one — wrote it)
      if (t.sq.n_replanned) *t.sq.n_replanned = __atomic_load_n(&q.h_trailer[&t - q.tk].pad, __ATOMIC_RELAXED);
    }
    if (t.user_info && t.h_info) {
      if (!c->skid_all_reloc && t.reloc_epoch == c->skid_reloc_epoch) {
        bool all = true;
        for (int i = 0; i < n && all; i++) all = t.h_info[i].relocalized != 0;
        c->skid_all_reloc = all;
      }
      for (int i = 0; i < n; i++) {
        t.user_info[i].relocalized = t.h_info[i].relocalized;
        t.user_info[i].index_along_path = t.h_info[i].index_along_path;
        t.user_info[i].translation[0] = t.h_info[i].translation[0];
        t.user_info[i].translation[1] = t.h_info[i].translation[1];
        t.user_info[i].rotation = t.h_info[i].rotation;
      }
    }
  }
  t.release();
  c->outstanding--;
  return rc;
}

// ---- device tickets ---------------------------------------------------------------------------------------------------------------
void* fsdp_device_alloc(fsdp_ctx* c, size_t bytes) {
  if (!c || hipSetDevice(c->device) != hipSuccess) return nullptr;
  void* p = nullptr;
  if (alloc_result(hipMalloc(&p, bytes ? bytes : 1)) != hipSuccess) return nullptr;
  return p;
}
void fsdp_device_free(fsdp_ctx* c, void* p) {
  if (!c || !p) return;
  (void)hipSetDevice(c->device);
  (void)hipFree(p);
}
int fsdp_device_write(fsdp_ctx* c, void* dst_dev, const void* src_host, size_t bytes) {
  if (!c) return 1;
  HIP_TRY(c, hipSetDevice(c->device));
  if (bytes == 0) return 0;
  if (!src_host || !device_owns(c, dst_dev, bytes)) {
    c->err = "fsdp_device_write: dst_dev must be device memory of the context's GPU over the whole extent, src_host host memory";
    return 1;
  }
  HIP_TRY(c, copy_sync(c, dst_dev, src_host, bytes, hipMemcpyHostToDevice));
  return 0;
}
int fsdp_device_read(fsdp_ctx* c, void* dst_host, const void* src_dev, size_t bytes) {
  if (!c) return 1;
  HIP_TRY(c, hipSetDevice(c->device));
  if (bytes == 0) return 0;
  if (!dst_host || !device_owns(c, src_dev, bytes)) {
    c->err = "fsdp_device_read: src_dev must be device memory of the context's GPU over the whole extent, dst_host host memory";
    return 1;
  }
  HIP_TRY(c, copy_sync(c, dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
  return 0;
}
int fsdp_device_owns(fsdp_ctx* c, const void* p, size_t bytes) {
  if (!c || !p || hipSetDevice(c->device) != hipSuccess) return 0;
  return device_owns(c, p, bytes) ? 1 : 0;
}
void* fsdp_stream_create(fsdp_ctx* c) {
  if (!c || hipSetDevice(c->device) != hipSuccess) return nullptr;
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return s;
}
void fsdp_stream_destroy(fsdp_ctx* c, void* stream) {
  if (!c || !stream) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize((hipStream_t)stream);
  (void)hipStreamDestroy((hipStream_t)stream);
}
int fsdp_stream_wait_stream(fsdp_ctx* c, void* stream, void* after) {
  if (!c) return 1;
  if (!stream || !after) {
    c->err = "fsdp_stream_wait_stream: NULL stream";
    return 1;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  Event e;  // (destroyed at return: the runtime keeps what the enqueued wait needs)
  HIP_TRY(c, hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(e, (hipStream_t)after));
  HIP_TRY(c, hipStreamWaitEvent((hipStream_t)stream, e, 0));
  return 0;
}

// enqueue device ticket t on slot q: the producer's event, scan + gather into the slot's input copies, the pass with both routes,
// device_out_kernel, the ticket's event.  Never called twice for a ticket.
static int enqueue_device_ticket(fsdp_ctx* c, Work& q, Work::Ticket& t, hipStream_t after_stream) {
  const Work::DevPass& d = t.dev;
  const int n = t.batch.n;
  const size_t rows = t.batch.total;
  const bool with_prev = d.prev != nullptr;
  // a bigger batch than the slot has seen: its buffers are replaced — not under the feet of the passes queued on the stream
  if ((size_t)n > q.buf.frames() || !q.in.fits((size_t)n, rows, with_prev)) HIP_TRY(c, hipStreamSynchronize(q.stream));
  if (int rc = ensure_work(c, q, n)) return rc;
  // (rows and max_cones are upper bounds: n * cone_capacity, cone_capacity; batch.prev says whether the store holds previous paths)
  if (int rc = take_batch(c, q.in, t.batch)) return rc;
  HIP_TRY(c, t.h_bad.reserve(3, 16, Pin::MappedCoherent));
  t.h_bad[0] = -1;
  t.h_bad[2] = -1;
  if (after_stream) {
    if (!t.after) HIP_TRY(c, hipEventCreateWithFlags(&t.after.h, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(t.after, after_stream));
    HIP_TRY(c, hipStreamWaitEvent(q.stream, t.after, 0));
  }
  if (d.path_ids) fsdp_gpt_launch_ids_scan(q.stream, n, c->n_gpt, d.path_ids, t.h_bad.device() + 2);
  fsdp_dio_in_args a;
  a.n_frames = n;
  a.cone_capacity = d.cap;
  a.counts = d.counts;
  a.cones = d.cones;
  a.poses = d.poses;
  a.prev = d.prev;
  a.bad_frame = t.h_bad.device();
  a.dst_off = q.in.d_off;
  a.dst_cones = q.in.d_cones;
  a.dst_poses = q.in.d_poses;
  a.dst_prev = q.in.d_prev;
  fsdp_dio_launch_in(q.stream, &a);
  Pass pass;
  pass.device = true;
  pass.compact = true;
  pass.host = (fsdp_frame_result*)d.records;  // (device memory; NULL: the slot's result block)
  pass.trailer = (int)(&t - q.tk);
  pass.force_routes = true;
  pass.in_flight = t.in_flight;
  pass.path_ids = d.path_ids;
  if (int rc = launch_pass(c, q, q.in, pass)) return rc;
  t.seq = q.seq;
  t.ran_big = q.ran_big;
  t.ran_retry = q.ran_retry;
  t.via_stage = false;
  fsdp_dio_out_args o;
  o.n_frames = n;
  o.sorted = q.buf.d_sort;
  o.matched = q.buf.d_match;
  o.paths = q.buf.d_path;
  o.prev = with_prev ? q.in.d_prev.get() : nullptr;
  o.default_path = c->d_default_path;
  o.out_paths = d.paths;
  o.out_status = d.status;
  o.next_prev = d.next_prev;
  fsdp_dio_launch_out(q.stream, &o);
  HIP_TRY(c, hipGetLastError());
  if (!t.done) HIP_TRY(c, hipEventCreateWithFlags(&t.done.h, hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(t.done, q.stream));
  return 0;
}

// with_ids: fsdp_submit_device_paths (path_ids required)
static int submit_device_impl(fsdp_ctx* c, int n_frames, int cone_capacity, const int32_t* counts, const double* cones, const double* poses,
                              const double* prev_paths, const int32_t* path_ids, bool with_ids, double* paths, int32_t* status, double* next_prev,
                              fsdp_compact_result* records, void* after_stream, long long* ticket) {
  if (!c || !ticket) return 1;
  *ticket = -1;
  const std::string who = with_ids ? "fsdp_submit_device_paths" : "fsdp_submit_device";
  if (c->mission == 2) {
    c->err = who + ": a skidpad context plans through fsdp_skidpad_submit (device arrays: fsdp_skidpad_submit_device)";
    return 1;
  }
  if (c->n_cache > 0) {
    c->err = who + ": the sorting cache is on (it stays a lock-step feature of the host calls: fsdp_sort_cache_reset(ctx, 0) turns it off)";
    return 1;
  }
  if (n_frames < 1 || cone_capacity < 0) {
    c->err = who + ": n_frames must be >= 1 and cone_capacity >= 0";
    return 1;
  }
  if ((long long)n_frames * cone_capacity > 0x7fffffffll) {
    c->err = who + ": n_frames x cone_capacity = " + std::to_string((long long)n_frames * cone_capacity) + " cone rows exceed the int32 offsets of a pass";
    return 1;
  }
  if (!counts || !poses || !paths || !status || (cone_capacity > 0 && !cones)) {
    c->err = who + ": counts, poses, paths and status are required" + (cone_capacity > 0 ? ", and cones with cone_capacity > 0" : "");
    return 1;
  }
  if (!fsdp_dio_launch_in || !fsdp_dio_launch_out) {
    c->err = who + ": this library was built without the device ticket kernels (csrc/device_io_lib.hip)";
    return 2;
  }
  if (with_ids) {
    if (int rc = refuse_paths_call(c, who)) return rc;
    if (!path_ids) {
      c->err = who + ": path_ids is NULL";
      return 1;
    }
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = (size_t)n_frames, row = sizeof(double) * PATH_POINTS * 4;
  const struct {
    const char* name;
    const void* p;
    size_t bytes;
  } arrays[] = {{"counts", counts, sizeof(int32_t) * n},
                {"cones", cone_capacity > 0 ? cones : nullptr, sizeof(double) * 3 * n * (size_t)cone_capacity},
                {"poses", poses, sizeof(double) * 4 * n},
                {"prev_paths", prev_paths, row * n},
                {"path_ids", with_ids ? path_ids : nullptr, sizeof(int32_t) * n},
                {"paths", paths, row * n},
                {"status", status, sizeof(int32_t) * n},
                {"next_prev", next_prev, row * n},
                {"records", records, sizeof(fsdp_compact_result) * n}};
  for (const auto& x : arrays)
    if (x.p && !device_owns(c, x.p, x.bytes)) {
      c->err = who + ": " + x.name + " is not device memory of the context's GPU over its whole extent of " + std::to_string(x.bytes) +
               " bytes (host memory, page-locked or not, goes through fsdp_submit; managed memory, another GPU's memory and memory of "
               "another HIP runtime are not accepted)";
      return 1;
    }
  Work* qp = nullptr;
  Work::Ticket* t = nullptr;
  if (int rc = free_ticket(c, who.c_str(), n_frames, &qp, &t)) return rc;
  // (the batch as the slot's stores size it: counts only, and prev as the flag take_batch reads — the host never dereferences a device ticket's batch)
  t->batch = Batch{n_frames, nullptr, nullptr, nullptr, prev_paths, n * (size_t)cone_capacity, cone_capacity};
  t->skid = false;
  t->in_flight = frames_in_flight(c, n_frames, true);
  t->user_results = nullptr;
  t->user_info = nullptr;
  t->compact = true;
  t->sq = Work::SeqPass();
  t->cache_lo = -1;
  t->dev = Work::DevPass{true, cone_capacity, counts, cone_capacity > 0 ? cones : nullptr, poses, prev_paths, paths, status, next_prev, records};
  t->dev.path_ids = with_ids ? path_ids : nullptr;
  t->path_ids = nullptr;
  if (int rc = enqueue_device_ticket(c, *qp, *t, (hipStream_t)after_stream)) {
    (void)hipStreamSynchronize(qp->stream);
    (void)hipGetLastError();
    t->release();
    return rc;
  }
  t->id = c->next_ticket++;
  c->outstanding++;
  *ticket = t->id;
  return 0;
}
int fsdp_submit_device(fsdp_ctx* c, int n_frames, int cone_capacity, const int32_t* counts, const double* cones, const double* poses,
                       const double* prev_paths, double* paths, int32_t* status, double* next_prev, fsdp_compact_result* records,
                       void* after_stream, long long* ticket) {
  return submit_device_impl(c, n_frames, cone_capacity, counts, cones, poses, prev_paths, nullptr, false, paths, status, next_prev, records, after_stream, ticket);
}
int fsdp_submit_device_paths(fsdp_ctx* c, int n_frames, int cone_capacity, const int32_t* counts, const double* cones, const double* poses,
                             const double* prev_paths, const int32_t* path_ids, double* paths, int32_t* status, double* next_prev,
                             fsdp_compact_result* records, void* after_stream, long long* ticket) {
  return submit_device_impl(c, n_frames, cone_capacity, counts, cones, poses, prev_paths, path_ids, true, paths, status, next_prev, records, after_stream, ticket);
}

int fsdp_ticket_stream_wait(fsdp_ctx* c, long long ticket, void* stream) {
  if (!c) return 1;
  Work::Ticket* t = find_ticket(c, ticket, nullptr);
  if (!t || !t->done) {
    c->err = "fsdp_ticket_stream_wait: unknown ticket " + std::to_string(ticket) + " (a collected ticket has finished: nothing to wait for)";
    return 1;
  }
  if (!stream) {
    c->err = "fsdp_ticket_stream_wait: NULL stream";
    return 1;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if (t->pending)
    if (int rc = flush_skid(c)) return rc;
  HIP_TRY(c, hipStreamWaitEvent((hipStream_t)stream, t->done, 0));
  return 0;
}

int fsdp_ticket_capacity(const fsdp_ctx* c) { return c ? c->overlap * (c->mission == 2 ? 1 : SLOT_QUEUE) : 0; }

int fsdp_route_stats(fsdp_ctx* c, int* expect_big, int* expect_retry, long long* reruns) {
  if (!c) return 1;
  if (expect_big) *expect_big = c->expect_big ? 1 : 0;
  if (expect_retry) *expect_retry = c->expect_retry ? 1 : 0;
  if (reruns) *reruns = c->reruns;
  return 0;
}

// ---- blocking calls on host buffers -------------------------------------------------------------------------------------
// A LARGE blocking call is cut into up to PLAN_CHUNKS contiguous chunks, each a ticket on a slot of its own: one chunk's transfers
// (in place for page-locked buffers, staged by the runtime for pageable ones — then the host copies chunk k + 1 while the kernels of
// chunk k run) go under the other chunks' kernels, and the first chunk's results are on their way back while the last one is still
// being planned.  Measured (tools/plan_probe.py, profiles/r06_plan_probe.txt): at 4096 frames chunks only add launches to a pass that is
// one dependent chain anyway (2.39 -> 2.73 ms page-locked, 3.11 -> 3.32 ms pageable); from 16 384 frames they pay for pageable buffers
// (10.2 -> 8.3 ms), at 65 536 for both (36.0 -> 26.6 ms pageable, 14.8 -> 13.4 ms page-locked).  Hence: four chunks from
// PLAN_CHUNK_FROM frames on, none below.  The chunks know they share the GPU (in_flight = the whole batch) and run the kernels the
// whole batch would.  Results do not depend on the chunking.  Option "plan_chunks" = k forces up to k chunks of >= PLAN_CHUNK_MIN frames
// (tests), 1 = never.
constexpr int PLAN_CHUNKS = 4, PLAN_CHUNK_FROM = 16384, PLAN_CHUNK_MIN = 512;

static int plan_blocking(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses, const double* prev,
                         fsdp_frame_result* results, bool compact, bool sequential = false) {
  if (!c) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_plan_batch");
  if (n_frames > 0 && !results) return 1;
  if (c->mission == 2) {
    c->err = "fsdp_plan_batch: a skidpad context plans through fsdp_skidpad_step";
    return 1;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = refuse_device_pointers(c, "fsdp_plan_batch", {{"cone_offsets", off}, {"cones_xyt", cones}, {"poses", poses}, {"prev_paths", prev}, {"results", results}}))
    return rc;
  Batch b;
  if (int rc = check_batch(c, n_frames, off, cones, poses, prev, &b)) return rc;
  const bool cached = sequential && c->n_cache > 0;
  if (cached && n_frames != c->n_cache) return cache_prepare(c, n_frames, off, "fsdp_plan_batch_sequential");
  if (int rc = sync_all(c)) return rc;
  if (cached)
    if (int rc = cache_prepare(c, n_frames, off, "fsdp_plan_batch_sequential")) return rc;
  c->last = fsdp_ctx::LastPass();
  if (n_frames == 0) return 0;
  const int chunks = c->plan_chunks > 0 ? std::max(1, std::min(c->plan_chunks, n_frames / PLAN_CHUNK_MIN)) : (n_frames >= PLAN_CHUNK_FROM ? PLAN_CHUNKS : 1);
  const size_t rec = compact ? sizeof(fsdp_compact_result) : sizeof(fsdp_frame_result);
  long long ids[PLAN_CHUNKS];
  int issued = 0, rc = 0;
  for (int k = 0; k < chunks && rc == 0; k++) {
    const int lo = (int)((long long)n_frames * k / chunks), hi = (int)((long long)n_frames * (k + 1) / chunks);
    Work& q = c->slot[k];  // (slots beyond the overlap depth get their stream here: a chunk is a pass in flight)
    if ((rc = ensure_work(c, q, hi - lo))) break;
    // (an internal ticket: entry 0 of the chunk's slot, planned for the whole call's frames on the GPU)
    TicketSpec spec;
    spec.batch = b.slice(lo, hi);
    spec.in_flight = n_frames;
    spec.results = (fsdp_frame_result*)((char*)results + rec * (size_t)lo);
    spec.compact = compact;
    if (cached) spec.cache_lo = lo;  // (the chunk's frames are planners lo..hi-1 of the sorting cache)
    if ((rc = issue_ticket(c, q, q.tk[0], spec))) break;
    ids[issued++] = q.tk[0].id;
  }
  for (int k = 0; k < issued; k++) {
    const int rck = fsdp_collect(c, ids[k]);  // (every issued chunk is waited for, also after an error: the buffers are the caller's again)
    if (rc == 0) rc = rck;
  }
  if (chunks > 1) c->last.whole = false;  // (the most recent pass is one chunk)
  c->next_ticket -= issued;  // (the chunks' numbers were internal: the caller's tickets keep counting up from where they were)
  if (rc == 0 && cached) rc = cache_finish(c);  // (once, after every chunk; a failed call leaves the previous entries in place)
  return rc;
}

int fsdp_plan_batch_sequential(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses,
                               const double* prev_paths, fsdp_frame_result* results) {
  return plan_blocking(c, n_frames, off, cones, poses, prev_paths, results, false, true);
}

int fsdp_plan_batch(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses,
                    fsdp_frame_result* results) {
  return plan_blocking(c, n_frames, off, cones, poses, nullptr, results, false);
}

int fsdp_plan_batch_compact(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses, const double* prev_paths,
                            fsdp_compact_result* results) {
  return plan_blocking(c, n_frames, off, cones, poses, prev_paths, (fsdp_frame_result*)results, true);
}

// n_steps consecutive steps of n_planners planners as ONE pass (frame = step * n_planners + planner): never cut into chunks —
// a chunk border would cut every planner's chain.  The pass is a ticket whose description (Work::SeqPass) puts the chain kernels
// in front of its assembly (enqueue_ticket, launch_pass); fsdp_submit_sequence hands the ticket out, the blocking calls are
// submit + collect of the whole call on slot 0, like a chunk of plan_blocking.
// cached (fsdp_plan_sequence_cached, blocking only): the planners' sorting-cache entries are chained on the device as well (the
// speculative sorting kernels and the cache chain of sequence_cache_kernel.h); hits: (n_steps * n_planners, 2) or NULL,
// n_resorted or NULL.  The cache buffers are swapped once, after the whole call — a rerun pass reads the same entries.
struct SeqCall {
  int n_planners, n_steps, planner_lo, planners_total;
  const int32_t* off;
  const double* cones;
  const double* poses;
  const double* initial_prev;  // the recording's blocks (planners_total rows), or NULL
  fsdp_frame_result* results;
  bool compact;
  double* final_prev;
  long long* n_replanned;
  bool cached;
  bool with_ids = false;              // fsdp_*_sequence_paths: per-frame global paths
  const int32_t* path_ids = nullptr;  // ... the recording's ids (n_steps * planners_total, step-major)
};

// what every sequence entry point refuses, in one order (blocking: the call needs the context to itself)
static int seq_refusals(fsdp_ctx* c, const std::string& who, const SeqCall& k, bool blocking) {
  if (c->mission == 2) {
    c->err = who + ": a skidpad context plans through fsdp_skidpad_step";
    return 1;
  }
  if (!k.cached && c->n_cache > 0) {
    c->err = who + ": the sorting cache is on (fsdp_sort_cache_reset): it is state of lock-step calls (fsdp_plan_batch_sequential)";
    return 1;
  }
  if (!fsdp_seq_launch || !fsdp_seq_launch_slice_in || !fsdp_seq_launch_slice_out) {
    c->err = who + ": this library was built without csrc/sequence_lib.hip";
    return 1;
  }
  if (k.cached && !fsdp_seqc_launch_sort) {
    c->err = who + ": this library was built without csrc/sequence_cache_lib.hip";
    return 1;
  }
  if (k.with_ids) {
    if (int rc = refuse_paths_call(c, who)) return rc;
    if (!fsdp_seqt_launch_chain || !fsdp_seq_launch_mark || !fsdp_seq_launch_final) {
      c->err = who + ": this library was built without csrc/sequence_table_lib.hip";
      return 2;
    }
  }
  if (blocking && c->outstanding) return busy_error(c, who.c_str());
  if (k.n_planners < 1 || k.n_steps < 1) {
    c->err = who + ": n_planners and n_steps must be >= 1";
    return 1;
  }
  const SeqSlice s{k.n_planners, k.n_steps, k.planner_lo, k.planners_total};
  if (!seq_slice_valid(s)) {
    c->err = who + ": planners [" + std::to_string(k.planner_lo) + ", " + std::to_string((long long)k.planner_lo + k.n_planners) +
             ") are no slice of a recording of " + std::to_string(k.planners_total) + " planners";
    return 1;
  }
  if (k.cached && c->n_cache == 0) {
    c->err = who + ": the sorting cache is off (fsdp_sort_cache_reset(ctx, n_planners) turns it on)";
    return 1;
  }
  if (k.cached && k.n_planners != c->n_cache) {
    c->err = who + ": the sorting cache is on for " + std::to_string(c->n_cache) + " planners, the call holds " + std::to_string(k.n_planners) +
             " planners (frame f is planner f % n_planners; fsdp_sort_cache_reset)";
    return 1;
  }
  const long long frames = (long long)k.n_planners * k.n_steps;
  if (frames > (0x7fffffff - SEQ_LIST) / 2) {  // (the head list holds two ints per frame behind its header, indexed by int)
    c->err = who + ": " + std::to_string(frames) + " frames in one pass (at most 2^30 - 3)";
    return 1;
  }
  if (!k.results) {
    c->err = who + ": results is NULL";
    return 1;
  }
  if (k.with_ids && !k.path_ids) {
    c->err = who + ": path_ids is NULL";
    return 1;
  }
  // (the ids themselves are checked against the table where they are gathered, in front of everything the ticket enqueues:
  // gather_sequence_ids)
  return refuse_device_pointers(c, who.c_str(), {{"cone_offsets", k.off}, {"cones_xyt", k.cones}, {"poses", k.poses}, {"initial_prev", k.initial_prev},
                                                  {"results", k.results}, {"final_prev", k.final_prev}, {"path_ids", k.path_ids}});
}

// the call's frames as a Batch: the whole call through check_batch (its arrays are the batch); a planner slice's segments
// checked like it, the Batch holding the counts only (its frames are not contiguous: Work::SeqPass keeps the arrays)
static int seq_check_batch(fsdp_ctx* c, const SeqCall& k, Batch* b) {
  const SeqSlice s{k.n_planners, k.n_steps, k.planner_lo, k.planners_total};
  const int n = (int)s.frames();
  if (s.whole()) return check_batch(c, n, k.off, k.cones, k.poses, nullptr, b);
  if (!k.off || !k.poses) {
    c->err = "batch: NULL offsets / poses";
    return 1;
  }
  std::vector<SeqSeg> seg((size_t)s.n_steps + 1);
  int most = 0;
  const int bad = seq_slice_segments(s, k.off, seg.data(), &most);
  if (bad) {
    c->err = bad == 1 ? "cone_offsets must be >= 0" : (bad == 2 ? "cone_offsets must be non-decreasing" : "a slice's cone rows exceed 2^31 - 1");
    return 1;
  }
  *b = Batch{n, nullptr, nullptr, nullptr, nullptr, (size_t)seg[(size_t)s.n_steps].dst, most};
  if (b->total > 0 && !k.cones) {
    c->err = "cones_xyt is NULL";
    return 1;
  }
  return 0;
}

// the call as issue_ticket takes it, planned for in_flight frames on the GPU
static TicketSpec seq_spec(const Batch& b, const SeqCall& k, const char* who, long long in_flight) {
  TicketSpec spec;
  spec.batch = b;
  spec.in_flight = in_flight;
  spec.results = k.results;
  spec.compact = k.compact;
  Work::SeqPass& sq = spec.sq;
  sq.on = true;
  sq.s = SeqSlice{k.n_planners, k.n_steps, k.planner_lo, k.planners_total};
  sq.cached = k.cached;
  sq.who = who;
  sq.off = k.off;
  sq.cones = k.cones;
  sq.poses = k.poses;
  sq.init = k.initial_prev ? k.initial_prev + SEQ_PREV_DOUBLES * (size_t)k.planner_lo : nullptr;
  sq.final_prev = k.final_prev ? k.final_prev + SEQ_PREV_DOUBLES * (size_t)k.planner_lo : nullptr;
  sq.n_replanned = k.n_replanned;
  sq.path_ids = k.with_ids ? k.path_ids : nullptr;
  return spec;
}

static int plan_sequence(fsdp_ctx* c, int n_planners, int n_steps, const int32_t* off, const double* cones, const double* poses,
                         const double* initial_prev, fsdp_frame_result* results, bool compact, double* final_prev, long long* n_replanned,
                         bool cached = false, int8_t* hits = nullptr, long long* n_resorted = nullptr, bool with_ids = false,
                         const int32_t* path_ids = nullptr) {
  if (!c) return 1;
  const char* who = with_ids ? "fsdp_plan_sequence_paths" : (cached ? "fsdp_plan_sequence_cached" : "fsdp_plan_sequence");
  if (n_replanned) *n_replanned = 0;
  if (n_resorted) *n_resorted = 0;
  const SeqCall k{n_planners, n_steps, 0, n_planners, off, cones, poses, initial_prev, results, compact, final_prev, n_replanned, cached, with_ids, path_ids};
  if (int rc = seq_refusals(c, who, k, true)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const int n = n_planners * n_steps;
  Batch b;
  if (int rc = seq_check_batch(c, k, &b)) return rc;
  if (int rc = sync_all(c)) return rc;
  c->last = fsdp_ctx::LastPass();
  Work& q = c->slot[0];
  if (int rc = ensure_work(c, q, n)) return rc;
  if (cached) {
    const hipError_t e = q.seqc_buf.reserve((size_t)n, (size_t)n_planners);
    if (e != hipSuccess) {
      c->err = std::string(who) + ": " + hipGetErrorString(e);
      return 2;
    }
    // the buffer the call writes gets room for every planner's largest frame of the sequence (cache_prepare, step by step)
    for (int s = 0; s < n_steps; s++)
      if (int rc = cache_prepare(c, n_planners, off + (size_t)s * n_planners, who)) return rc;
  }
  if (int rc = issue_ticket(c, q, q.tk[0], seq_spec(b, k, who, n))) return rc;
  int rc = fsdp_collect(c, q.tk[0].id);  // (waits; runs the pass again, chain kernels included, if it lacked a route)
  c->next_ticket--;                // (the number was internal, like plan_blocking's)
  if (rc != 0) return rc;
  if (cached) {
    std::vector<int32_t> resorted((size_t)n_planners);
    HIP_TRY(c, copy_sync(c, resorted.data(), q.seqc_buf.d_seqc_resorted, sizeof(int32_t) * resorted.size(), hipMemcpyDeviceToHost));
    if (hits) HIP_TRY(c, copy_sync(c, hits, q.seqc_buf.d_seqc_hits, 2 * (size_t)n, hipMemcpyDeviceToHost));
    if (int rc = cache_finish(c)) return rc;  // (the last step's codes; the entries become the previous ones)
    long long sum = 0;
    for (int32_t v : resorted) sum += v;
    if (n_resorted) *n_resorted = sum;
  }
  return 0;
}

// The ticket form (include/fsdp.h): planners [planner_lo, planner_lo + n_planners) of a recording of planners_total, cache off.
static int submit_sequence(fsdp_ctx* c, int n_planners, int n_steps, int planner_lo, int planners_total, const int32_t* off, const double* cones,
                           const double* poses, const double* initial_prev, fsdp_frame_result* results, bool compact, double* final_prev,
                           long long* n_replanned, long long* ticket, bool with_ids = false, const int32_t* path_ids = nullptr) {
  if (!c) return 1;
  const char* who = with_ids ? "fsdp_submit_sequence_paths" : "fsdp_submit_sequence";
  if (ticket) *ticket = -1;
  if (n_replanned) *n_replanned = 0;
  const SeqCall k{n_planners, n_steps, planner_lo, planners_total, off, cones, poses, initial_prev, results, compact, final_prev, n_replanned, false, with_ids, path_ids};
  if (int rc = seq_refusals(c, who, k, false)) return rc;
  if (!ticket) {
    c->err = std::string(who) + ": ticket is NULL";
    return 1;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  Batch b;
  if (int rc = seq_check_batch(c, k, &b)) return rc;
  Work* q = nullptr;
  Work::Ticket* t = nullptr;
  if (int rc = free_ticket(c, who, 1, &q, &t)) return rc;
  if (int rc = issue_ticket(c, *q, *t, seq_spec(b, k, who, frames_in_flight(c, b.n, true)))) return rc;
  *ticket = t->id;
  return 0;
}

int fsdp_plan_sequence(fsdp_ctx* c, int n_planners, int n_steps, const int32_t* off, const double* cones, const double* poses,
                       const double* initial_prev, fsdp_frame_result* results, double* final_prev, long long* n_replanned) {
  return plan_sequence(c, n_planners, n_steps, off, cones, poses, initial_prev, results, false, final_prev, n_replanned);
}

int fsdp_plan_sequence_compact(fsdp_ctx* c, int n_planners, int n_steps, const int32_t* off, const double* cones, const double* poses,
                               const double* initial_prev, fsdp_compact_result* results, double* final_prev, long long* n_replanned) {
  return plan_sequence(c, n_planners, n_steps, off, cones, poses, initial_prev, (fsdp_frame_result*)results, true, final_prev, n_replanned);
}

int fsdp_plan_sequence_cached(fsdp_ctx* c, int n_planners, int n_steps, const int32_t* off, const double* cones, const double* poses,
                              const double* initial_prev, fsdp_frame_result* results, double* final_prev, long long* n_replanned, int8_t* hits,
                              long long* n_resorted) {
  return plan_sequence(c, n_planners, n_steps, off, cones, poses, initial_prev, results, false, final_prev, n_replanned, true, hits, n_resorted);
}

int fsdp_plan_sequence_cached_compact(fsdp_ctx* c, int n_planners, int n_steps, const int32_t* off, const double* cones, const double* poses,
                                      const double* initial_prev, fsdp_compact_result* results, double* final_prev, long long* n_replanned,
                                      int8_t* hits, long long* n_resorted) {
  return plan_sequence(c, n_planners, n_steps, off, cones, poses, initial_prev, (fsdp_frame_result*)results, true, final_prev, n_replanned, true,
                       hits, n_resorted);
}

int fsdp_submit_sequence(fsdp_ctx* c, int n_planners, int n_steps, int planner_lo, int planners_total, const int32_t* off, const double* cones,
                         const double* poses, const double* initial_prev, fsdp_frame_result* results, double* final_prev, long long* n_replanned,
                         long long* ticket) {
  return submit_sequence(c, n_planners, n_steps, planner_lo, planners_total, off, cones, poses, initial_prev, results, false, final_prev, n_replanned,
                         ticket);
}

int fsdp_submit_sequence_compact(fsdp_ctx* c, int n_planners, int n_steps, int planner_lo, int planners_total, const int32_t* off,
                                 const double* cones, const double* poses, const double* initial_prev, fsdp_compact_result* results,
                                 double* final_prev, long long* n_replanned, long long* ticket) {
  return submit_sequence(c, n_planners, n_steps, planner_lo, planners_total, off, cones, poses, initial_prev, (fsdp_frame_result*)results, true,
                         final_prev, n_replanned, ticket);
}

// The sequence calls with per-frame global paths (include/fsdp.h): path_ids covers the whole recording, step-major.
int fsdp_plan_sequence_paths(fsdp_ctx* c, int n_planners, int n_steps, const int32_t* off, const double* cones, const double* poses,
                             const double* initial_prev, const int32_t* path_ids, fsdp_frame_result* results, double* final_prev,
                             long long* n_replanned) {
  return plan_sequence(c, n_planners, n_steps, off, cones, poses, initial_prev, results, false, final_prev, n_replanned, false, nullptr, nullptr, true,
                       path_ids);
}

int fsdp_plan_sequence_paths_compact(fsdp_ctx* c, int n_planners, int n_steps, const int32_t* off, const double* cones, const double* poses,
                                     const double* initial_prev, const int32_t* path_ids, fsdp_compact_result* results, double* final_prev,
                                     long long* n_replanned) {
  return plan_sequence(c, n_planners, n_steps, off, cones, poses, initial_prev, (fsdp_frame_result*)results, true, final_prev, n_replanned, false,
                       nullptr, nullptr, true, path_ids);
}

int fsdp_submit_sequence_paths(fsdp_ctx* c, int n_planners, int n_steps, int planner_lo, int planners_total, const int32_t* off,
                               const double* cones, const double* poses, const double* initial_prev, const int32_t* path_ids,
                               fsdp_frame_result* results, double* final_prev, long long* n_replanned, long long* ticket) {
  return submit_sequence(c, n_planners, n_steps, planner_lo, planners_total, off, cones, poses, initial_prev, results, false, final_prev, n_replanned,
                         ticket, true, path_ids);
}

int fsdp_submit_sequence_paths_compact(fsdp_ctx* c, int n_planners, int n_steps, int planner_lo, int planners_total, const int32_t* off,
                                       const double* cones, const double* poses, const double* initial_prev, const int32_t* path_ids,
                                       fsdp_compact_result* results, double* final_prev, long long* n_replanned, long long* ticket) {
  return submit_sequence(c, n_planners, n_steps, planner_lo, planners_total, off, cones, poses, initial_prev, (fsdp_frame_result*)results, true,
                         final_prev, n_replanned, ticket, true, path_ids);
}

int fsdp_sort_cache_reset(fsdp_ctx* c, int n_planners) {
  if (!c) return 1;
  if (c->mission == 2) {
    c->err = "fsdp_sort_cache_reset: a skidpad context never sorts cones";
    return 1;
  }
  if (n_planners < 0) {
    c->err = "fsdp_sort_cache_reset: n_planners must be >= 0";
    return 1;
  }
  if (c->outstanding) return busy_error(c, "fsdp_sort_cache_reset");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sync_all(c)) return rc;
  cache_free(c);
  if (n_planners == 0) return 0;
  const size_t n = (size_t)n_planners;
  HIP_TRY(c, c->cache.reserve(n));
  for (int b = 0; b < 2; b++) {
    HIP_TRY(c, hipMemsetAsync(c->cache.d_hdr[b], 0, sizeof(SortCacheHdr) * n, c->stream));  // (valid = 0: no entry)
    HIP_TRY(c, hipMemsetAsync(c->cache.d_off[b], 0, sizeof(int32_t) * (n + 1), c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->cache_hits.assign(2 * n, (int8_t)-1);
  c->n_cache = n_planners;
  return 0;
}

int fsdp_sort_cache_hits(const fsdp_ctx* c, int8_t* out) {
  if (!c || !out || c->n_cache == 0) return 1;
  memcpy(out, c->cache_hits.data(), c->cache_hits.size());
  return 0;
}

// Options (include/fsdp.h fsdp_set_option): what tests and measurements pin.  Results never depend on them.
int fsdp_set_option(fsdp_ctx* c, const char* name, long long v) {
  if (!c || !name) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_set_option");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sync_all(c)) return rc;
  const std::string k(name);
  auto bad = [&]() {
    c->err = "fsdp_set_option: unknown option or value out of range: " + k + " = " + std::to_string(v);
    return 1;
  };
  if (k == "path_mode") {
    if (v < 0 || v > 2) return bad();
    c->force_path_mode = (int)v;
  } else if (k == "pack") {
    if (v < 0 || v > 2) return bad();
    c->force_pack = (int)v;
  } else if (k == "fit_g") {
    if (v != 0 && v != 4 && v != 8) return bad();
    c->fit_g = v == 8 ? 8 : 4;
  } else if (k == "always_route") {
    c->always_route = v != 0;
  } else if (k == "no_sort128") {
    c->no_sort128 = v != 0;
  } else if (k == "retry_pack_min") {
    if (v < 0 || v > 0x7fffffff) return bad();
    c->params.retry_pack_min = v == 0 ? 512 : (int)v;
    HIP_TRY(c, copy_sync(c, c->d_params, &c->params, sizeof(Params), hipMemcpyHostToDevice));
  } else if (k == "hw_queues") {
    if (v < 1 || v > 0x7fffffff) return bad();
    c->hw_queues = (int)v;
  } else if (k == "gang") {
    if (v < 0 || v > FSDP_MAX_OVERLAP) return bad();
    c->gang = (int)v;
  } else if (k == "poison") {
    c->poison = v != 0;
  } else if (k == "plan_chunks") {
    if (v < 0 || v > PLAN_CHUNKS) return bad();
    c->plan_chunks = (int)v;
  } else if (k == "skid_group") {
    if (v < 0 || v > SKID_GROUP_MAX) return bad();
    c->skid_group_env = (int)v;
  } else if (k == "skid_pack_min") {
    if (v < 0 || v > 0x7fffffff) return bad();
    c->skid_pack_min = v == 0 ? 2048 : (int)v;
  } else {
    return bad();
  }
  for (bool& p : c->primed) p = false;  // (the kernels of a pass may have changed: fsdp_time_reserve warms the slots again)
  for (int& p : c->gang_primed) p = 0;
  c->res_checked = false;
  return 0;
}

// What the link between this GPU and the host carries for page-locked buffers of `bytes` bytes: hipMemcpyAsync host -> device alone,
// device -> host alone, and both directions at once on two streams (GB/s each; measurement only — the ceiling a stream of batches
// is held against, bench.py "streaming.pcie_ceiling_GBps").
int fsdp_pcie_probe(fsdp_ctx* c, size_t bytes, int iters, double* h2d_GBps, double* d2h_GBps, double* both_each_GBps) {
  if (!c || bytes == 0 || iters <= 0) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_pcie_probe");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sync_all(c)) return rc;
  PinnedBuf<char> h_up, h_dn;
  DeviceBuf<char> d_up, d_dn;
  Stream s2;
  hipError_t e = h_up.reserve(bytes);
  if (e == hipSuccess) e = h_dn.reserve(bytes);
  if (e == hipSuccess) e = d_up.reserve(bytes);
  if (e == hipSuccess) e = d_dn.reserve(bytes);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&s2.h, hipStreamNonBlocking);
  if (e == hipSuccess) {
    memset(h_up, 1, bytes);
    e = hipMemsetAsync(d_dn, 2, bytes, c->stream);
  }
  auto run = [&](bool up, bool dn, double* each) -> hipError_t {
    hipError_t r = hipStreamSynchronize(c->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(s2);
    if (r != hipSuccess) return r;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < iters && r == hipSuccess; i++) {
      if (up) r = hipMemcpyAsync(d_up, h_up, bytes, hipMemcpyHostToDevice, c->stream);
      if (dn && r == hipSuccess) r = hipMemcpyAsync(h_dn, d_dn, bytes, hipMemcpyDeviceToHost, s2);
    }
    if (r == hipSuccess) r = hipStreamSynchronize(c->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(s2);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (each) *each = (double)bytes * iters / sec / 1e9;
    return r;
  };
  if (e == hipSuccess) e = run(true, true, nullptr);  // warm
  if (e == hipSuccess) e = run(true, false, h2d_GBps);
  if (e == hipSuccess) e = run(false, true, d2h_GBps);
  if (e == hipSuccess) e = run(true, true, both_each_GBps);
  HIP_TRY(c, e);
  return 0;
}

// ---- timing of the resident batch ---------------------------------------------------------------------------------------
// MAX_STAGES + 1 events per pass (before every kernel, after the last) + begin / end of the region
constexpr int TIMING_EPP = MAX_STAGES + 1;
static int reserve_timing(fsdp_ctx* c, int iters) {
  const size_t need = (size_t)TIMING_EPP * (size_t)iters + 2;
  while (c->tev.size() < need) {
    Event e;
    HIP_TRY(c, hipEventCreate(&e.h));
    c->tev.push_back(std::move(e));
  }
  HIP_TRY(c, c->d_kclock.reserve(2 * (size_t)iters));
  return 0;
}

// ---- ganged replay -------------------------------------------------------------------------------------------------------
// Streams that share a hardware queue run one after the other.  A replay whose overlap depth exceeds the queues the runtime grants
// (option "hw_queues") therefore keeps only hw_queues launches of n frames on the chip, however many streams it spreads its passes
// over (depth 20 on 4 queues: 4 x 256 wavefronts of fit_kernel<4> on a chip that holds 2048).  fsdp_time_runs then issues the same
// passes as gangs: g = ceil(overlap / S) passes become one pass over g x n frames (launch_pass, Pass::members) on one of S slots'
// streams, round robin, S = min(GANG_STREAMS, hw_queues) — streams beyond the queues would wait for each other again.  Frames in
// flight stay overlap x n; results are those of the single passes.
// GANG_STREAMS: measured among 1..4 at depth 20 under four queues (profiles/gang_replay.md: 5.8 / 6.3 / 6.5 / 6.4 M frames/s in a
// 20-pass region, 5.9 / 6.5 / 6.8 / 6.9 M in a 100-pass one).
constexpr int GANG_STREAMS = 4;
// members per ganged pass of fsdp_time_runs (1: the passes stay single)
static int gang_size(const fsdp_ctx* c) {
  if (!c->params.use_unknown_cones || c->gang == 1) return 1;  // (the filter kernels read a pass's inputs in front of the sorting kernel)
  if (c->gang > 1) return std::min(c->gang, c->overlap);  // (no gang is larger than the passes in flight)
  if (c->overlap <= c->hw_queues) return 1;
  const int streams = std::min(GANG_STREAMS, c->hw_queues);
  return (c->overlap + streams - 1) / streams;
}
static int gang_slots(const fsdp_ctx* c, int g) { return std::max(1, std::min(c->overlap, (c->overlap + g - 1) / g)); }
// the first `slots` slots hold room for passes of g resident batches (their stores only grow; nothing is in flight)
static int ensure_gang(fsdp_ctx* c, int g, int slots) {
  const size_t n = (size_t)c->res.n_frames * (size_t)g, rows = c->res_rows * (size_t)g;
  if (n > 0x7fffffffull || rows > 0x7fffffffull) {
    c->err = "fsdp_time_runs: a ganged pass of " + std::to_string(g) + " batches exceeds the 32-bit frame / cone offsets";
    return 1;
  }
  for (int i = 0; i < slots; i++) {
    Work& q = c->slot[i];
    if (i == 0 && c->gang_grown_from == 0 && n > q.buf.frames()) c->gang_grown_from = std::max<size_t>(1, q.buf.frames());
    if (int rc = ensure_work(c, q, (int)n)) return rc;
    if (!q.in.fits(n, rows, c->res.use_prev)) {
      HIP_TRY(c, hipStreamSynchronize(q.stream));
      HIP_TRY(c, q.in.reserve(n, rows, c->res.use_prev));
    }
  }
  return 0;
}
// a ganged pass of `members` resident batches on slot q
static int launch_gang(fsdp_ctx* c, Work& q, int members, Pass& pass) {
  GangMember gm;
  gm.off = c->res.d_off;
  gm.cones = c->res.d_cones;
  gm.poses = c->res.d_poses;
  gm.prev = c->res.use_prev ? c->res.d_prev.get() : nullptr;
  gm.n = c->res.n_frames;
  gm.base = 0;  // (fsdp_upload rebases a slice's offsets)
  gm.rows = c->res_rows;
  pass.members.assign((size_t)members, gm);
  q.in.n_frames = c->res.n_frames * members;
  q.in.max_cones = c->res.max_cones;
  q.in.use_prev = c->res.use_prev;
  pass.in_flight = frames_in_flight(c, c->res.n_frames, false);  // (overlap x n, as for the single passes: the same packing)
  return launch_pass(c, q, q.in, pass);
}

// one verified pass over the resident batch: afterwards the route expectations are exactly what this batch needs
static int check_resident(fsdp_ctx* c) {
  if (c->res_checked || !c->resident || c->res.n_frames == 0) return 0;
  if (int rc = sync_all(c)) return rc;
  Work& q = c->slot[0];
  if (int rc = launch_pass(c, q, c->res, Pass())) return rc;
  HIP_TRY(c, hipStreamSynchronize(q.stream));
  return verify_pass(c, q);  // sets res_checked and the exact expectations
}

int fsdp_time_reserve(fsdp_ctx* c, int iters) {
  if (!c || iters <= 0) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_time_reserve");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = reserve_timing(c, iters);
  if (rc) return rc;
  // The first launches on a stream pay for its hardware queue and scratch set-up: every slot of the current overlap depth
  // that has not run a pass yet runs one now (the resident batch, results overwritten by the timed passes).
  if (c->resident && c->res.n_frames > 0) {
    if ((rc = check_resident(c))) return rc;
    for (int i = 0; i < c->overlap; i++)
      if (!c->primed[i])
        if ((rc = launch_pass(c, c->slot[i], c->res, Pass()))) return rc;
    // a ganged region's slots get their room and run one gang each here, outside the region
    if (const int g = gang_size(c); g > 1) {
      const int slots = gang_slots(c, g);
      if ((rc = sync_all(c))) return rc;
      if ((rc = ensure_gang(c, g, slots))) return rc;
      for (int i = 0; i < slots; i++) {
        if (c->gang_primed[i] >= g) continue;
        Pass warm;
        if ((rc = launch_gang(c, c->slot[i], g, warm))) return rc;
      }
    }
    rc = sync_all(c);
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
  }
  return 0;
}

int fsdp_time_results(fsdp_ctx* c, float* ms_total, float* ms_stage) {
  if (!c) return 1;
  if (ms_stage)
    for (int k = 0; k < MAX_STAGES; k++) ms_stage[k] = 0;
  if (ms_total) *ms_total = 0;
  if (c->timed_iters <= 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t need = (size_t)TIMING_EPP * (size_t)c->timed_iters + 2;
  float total = 0;
  HIP_TRY(c, hipEventElapsedTime(&total, c->tev[need - 2], c->tev[need - 1]));
  if (ms_stage)
    for (int it = 0; it < c->timed_iters; it++)
      for (int st = 0; st < c->timed_stages; st++) {
        float t;
        if ((c->tev_recorded[it] >> st & 3u) != 3u) continue;  // a kernel the region did not bracket: its time stays 0
        HIP_TRY(c, hipEventElapsedTime(&t, c->tev[(size_t)TIMING_EPP * (size_t)it + st], c->tev[(size_t)TIMING_EPP * (size_t)it + st + 1]));
        ms_stage[st] += t;
      }
  if (ms_total) *ms_total = total;
  return 0;
}

int fsdp_time_runs(fsdp_ctx* c, int iters, float* ms_total, float* ms_stage) {
  if (!c || iters <= 0) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_time_runs");
  if (ms_stage)
    for (int k = 0; k < MAX_STAGES; k++) ms_stage[k] = 0;
  if (ms_total) *ms_total = 0;
  c->timed_iters = 0;
  if (!c->resident) {
    c->err = "fsdp_time_runs: no resident batch";
    return 1;
  }
  if (c->res.n_frames == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = sync_all(c);
  if (rc) return rc;
  if ((rc = check_resident(c))) return rc;  // the timed passes carry exactly the route kernels this batch needs
  // passes rotate through the slots when overlap is on and are NOT synchronised with the host in between
  constexpr int EPP = TIMING_EPP;
  const size_t need = (size_t)EPP * (size_t)iters + 2;
  rc = reserve_timing(c, iters);
  if (rc) return rc;
  hipEvent_t ev_begin = c->tev[need - 2], ev_end = c->tev[need - 1];
  // (a ganged region's slots get their room in front of the region: fsdp_time_reserve has done it for a caller who reserves)
  const int g = gang_size(c), slots = gang_slots(c, g);
  if (g > 1)
    if ((rc = ensure_gang(c, g, slots))) return rc;
  // the refit kernel's own clock readings: atomicMin over "all ones", atomicMax over zero (set before the region begins)
  const size_t kcap = c->d_kclock.capacity() / 2;  // (passes the block has room for: first readings, then last readings)
  HIP_TRY(c, hipMemsetAsync(c->d_kclock, 0xff, sizeof(unsigned long long) * kcap, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->d_kclock + kcap, 0, sizeof(unsigned long long) * kcap, c->stream));
  HIP_TRY(c, hipEventRecord(ev_begin, c->stream));
  int last_of_slot[FSDP_MAX_OVERLAP];
  bool started[FSDP_MAX_OVERLAP];
  for (int i = 0; i < FSDP_MAX_OVERLAP; i++) {
    last_of_slot[i] = -1;
    started[i] = false;
  }
  int n_stages = 0;
  c->tev_recorded.assign((size_t)iters, 0u);
  c->tev_members.assign((size_t)iters, 0);
  // Ganged (gang_size): passes it .. it + m - 1 are one launch chain on one of `slots` streams.  Its events and clock readings are
  // those of pass `it`; the gang's other passes record none (tev_recorded = 0), so fsdp_time_results sums every launch once.
  for (int it = 0; it < iters; it += g) {
    const int m = std::min(g, iters - it);
    const int si = g > 1 ? (int)(c->turn++ % (unsigned)slots) : (c->overlap > 1) ? (int)(c->turn++ % (unsigned)c->overlap) : 0;
    Work& q = c->slot[si];
    if (!started[si] && si != 0) HIP_TRY(c, hipStreamWaitEvent(q.stream, ev_begin, 0));
    started[si] = true;
    StageEvents t;
    t.ev = &c->tev[(size_t)EPP * (size_t)it];
    t.main_only = c->time_main_only;
    // (opt-in, fsdp_time_detail bit 1: the readings are two atomics per workgroup on one address — the launches of a region
    // timed without them are the production launches)
    t.clock_first = c->time_kernel_clock ? c->d_kclock + it : nullptr;
    t.clock_last = c->time_kernel_clock ? c->d_kclock + kcap + it : nullptr;
    Pass timed;
    timed.events = &t;
    if ((rc = g > 1 ? launch_gang(c, q, m, timed) : launch_pass(c, q, c->res, timed))) return rc;
    n_stages = t.n - 1;
    c->tev_recorded[it] = t.recorded;
    c->tev_members[it] = m;
    last_of_slot[si] = it;
  }
  // the end event follows the last pass of every slot
  for (int i = 1; i < FSDP_MAX_OVERLAP; i++)
    if (last_of_slot[i] >= 0) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->tev[(size_t)EPP * (size_t)last_of_slot[i] + n_stages], 0));
  HIP_TRY(c, hipEventRecord(ev_end, c->stream));
  HIP_TRY(c, hipEventSynchronize(ev_end));
  const long long reruns_before = c->reruns;
  rc = sync_all(c);
  if (rc) return rc;
  HIP_TRY(c, hipGetLastError());
  if (c->reruns != reruns_before) {
    c->err = "fsdp_time_runs: a timed pass lacked a route kernel it needed (internal: resident batch not checked)";
    return 2;
  }
  c->timed_iters = iters;
  c->timed_stages = n_stages;
  if (ms_total || ms_stage) return fsdp_time_results(c, ms_total, ms_stage);
  return 0;
}

int fsdp_time_kernel_clock(fsdp_ctx* c, double* ms_sum, int* launches) {
  if (!c || !ms_sum || !launches) return 1;
  *ms_sum = 0.0;
  *launches = 0;
  if (c->timed_iters <= 0 || !c->d_kclock) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  int khz = 0;
  HIP_TRY(c, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
  if (khz <= 0) return 0;
  const size_t kcap = c->d_kclock.capacity() / 2;
  std::vector<unsigned long long> h(2 * kcap);
  HIP_TRY(c, hipMemcpy(h.data(), c->d_kclock, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
  for (int it = 0; it < c->timed_iters && (size_t)it < kcap; it++) {
    const unsigned long long a = h[(size_t)it], b = h[kcap + (size_t)it];
    if (a == ~0ull || b == 0ull || b < a) continue;  // (a pass whose path stage was not the three-kernel form)
    *ms_sum += (double)(b - a) / (double)khz;
    *launches += c->tev_members[(size_t)it];  // (the passes the reading covers: a gang's launch is one reading for all its members)
  }
  return 0;
}

int fsdp_time_detail(fsdp_ctx* c, int every_kernel) {
  if (!c) return 1;
  c->time_main_only = (every_kernel & 1) == 0;
  c->time_kernel_clock = (every_kernel & 2) != 0;
  return 0;
}

int fsdp_stage_names(fsdp_ctx* c, char* out, int cap) {
  if (!c || !out || cap < 64) return 1;
  snprintf(out, (size_t)cap, "%s", c->stage_names.c_str());
  return 0;
}

// ---- stage-level entry points (host buffers, blocking, slot 0; the route kernels always run) ---------------------------
// their slot, whose buffers then no longer hold the most recent pass
static Work& stage_slot(fsdp_ctx* c) {
  if (c->last.slot == 0) c->last = fsdp_ctx::LastPass();
  return c->slot[0];
}

// The ranked outputs of fsdp_sort_batch_ranked on the device for the duration of one call (a diagnostic route: allocated per call)
struct RankCall {
  int top_k = 0;
  int32_t* counts = nullptr;   // caller's arrays
  int32_t* configs = nullptr;
  double* costs = nullptr;
  double* terms = nullptr;
  DeviceBuf<int32_t> d_counts, d_configs;
  DeviceBuf<double> d_costs, d_terms;
  DeviceBuf<SortRankScratchBig> d_scratch;
};

// indices of a frame planned without its UNKNOWN cones back into the caller's cone list (what assemble_kernel does for a full
// pass); map: the frame's part of launch_filter's map
static void map_back(int32_t* idx, size_t n, const int32_t* map) {
  for (size_t k = 0; k < n; k++)
    if (idx[k] >= 0) idx[k] = map[idx[k]];
}

// The history outputs of fsdp_sort_batch_history on the device for the duration of one call (a diagnostic route: allocated per call)
struct HistCall {
  int rows_cap = 0;
  int32_t* n_rows = nullptr;  // caller's arrays
  int32_t* target_length = nullptr;
  int32_t* rows = nullptr;
  uint8_t* is_end = nullptr;
  int32_t* cand = nullptr;
  uint8_t* verdict = nullptr;
  DeviceBuf<int32_t> d_n_rows, d_target, d_rows, d_cand;
  DeviceBuf<uint8_t> d_is_end, d_verdict;
};

// fsdp_sort_batch, with rk fsdp_sort_batch_ranked and with hk fsdp_sort_batch_history (the ranked / history kernels instead of the
// plain ones, never the sorting cache)
static int sort_batch_impl(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses,
                           fsdp_frame_result* results, RankCall* rk, HistCall* hk = nullptr) {
  const char* who = hk ? "fsdp_sort_batch_history" : rk ? "fsdp_sort_batch_ranked" : "fsdp_sort_batch";
  if (!c) return 1;
  if (hk) {
    if (c->mission == 2) {
      c->err = "fsdp_sort_batch_history: a skidpad context never sorts cones";
      return 1;
    }
    if (hk->rows_cap < 1) {
      c->err = "fsdp_sort_batch_history: rows_cap must be at least 1";
      return 1;
    }
    if (!hk->n_rows || !hk->target_length || !hk->rows || !hk->is_end) {
      c->err = "fsdp_sort_batch_history: NULL n_rows / target_length / rows / is_end";
      return 1;
    }
    if ((hk->cand == nullptr) != (hk->verdict == nullptr)) {
      c->err = "fsdp_sort_batch_history: cand and verdict are given together or not at all";
      return 1;
    }
    if (n_frames > 0 && (long long)n_frames * 2 * (long long)hk->rows_cap > 2147483647ll) {
      c->err = "fsdp_sort_batch_history: n_frames * 2 * rows_cap exceeds 2^31 - 1";
      return 1;
    }
    if (!fsdp_sort_hist_launch || !fsdp_sort_hist_launch_big) {
      c->err = "fsdp_sort_batch_history: this library was built without csrc/sort_history_lib.hip";
      return 1;
    }
  }
  if (rk) {
    if (c->mission == 2) {
      c->err = "fsdp_sort_batch_ranked: a skidpad context never sorts cones";
      return 1;
    }
    if (rk->top_k < 1 || rk->top_k > FSDP_RANK_MAX) {
      c->err = "fsdp_sort_batch_ranked: top_k must be in 1.." FSDP_STR(FSDP_RANK_MAX);
      return 1;
    }
    if (n_frames > 0 && (!rk->counts || !rk->configs || !rk->costs)) {
      c->err = "fsdp_sort_batch_ranked: NULL counts / configs / costs";
      return 1;
    }
  }
  if (c->outstanding) return busy_error(c, who);
  HIP_TRY(c, hipSetDevice(c->device));
  if (hk)
    if (int rc = refuse_device_pointers(c, who, {{"cone_offsets", off}, {"cones_xyt", cones}, {"poses", poses}, {"results", results},
                                                 {"n_rows", hk->n_rows}, {"target_length", hk->target_length}, {"rows", hk->rows},
                                                 {"is_end", hk->is_end}, {"cand", hk->cand}, {"verdict", hk->verdict}}))
      return rc;
  Batch b;
  if (int rc = check_batch(c, n_frames, off, cones, poses, nullptr, &b)) return rc;
  const bool cached = !rk && !hk && c->n_cache > 0;
  if (cached && n_frames != c->n_cache) return cache_prepare(c, n_frames, off, "fsdp_sort_batch");
  if (n_frames == 0) return 0;
  if (int rc = sync_all(c)) return rc;
  if (cached)
    if (int rc = cache_prepare(c, n_frames, off, "fsdp_sort_batch")) return rc;
  const size_t hrows = hk ? (size_t)n_frames * 2 * (size_t)hk->rows_cap : 0;
  if (hk) {  // (first: a call whose outputs do not fit returns with nothing planned, and its buffers go with it)
    HIP_TRY(c, hk->d_rows.reserve(hrows * MAX_LEN));
    if (hk->cand) {
      HIP_TRY(c, hk->d_cand.reserve(hrows * KNN));
      HIP_TRY(c, hk->d_verdict.reserve(hrows * KNN));
    }
    HIP_TRY(c, hk->d_is_end.reserve(hrows));
    HIP_TRY(c, hk->d_n_rows.reserve(2 * (size_t)n_frames));
    HIP_TRY(c, hk->d_target.reserve(2 * (size_t)n_frames));
  }
  Work& q = stage_slot(c);
  if (int rc = ensure_work(c, q, n_frames)) return rc;
  if (int rc = upload_inputs(c, q.in, q.stream, b)) return rc;
  Inputs in = q.in.view();
  const bool filtered = !c->params.use_unknown_cones;
  if (filtered)
    if (int rc = launch_filter(c, q, q.in, &in)) return rc;
  const size_t rows = rk ? (size_t)n_frames * 2 * (size_t)rk->top_k : 0;
  SortRankView v;
  SortVariant var;
  if (rk) {
    HIP_TRY(c, rk->d_counts.reserve(2 * (size_t)n_frames));
    HIP_TRY(c, rk->d_configs.reserve(rows * MAX_LEN));
    HIP_TRY(c, rk->d_costs.reserve(rows));
    if (rk->terms) HIP_TRY(c, rk->d_terms.reserve(rows * COST_TERMS));
    HIP_TRY(c, rk->d_scratch.reserve(SORT_BIG_BLOCKS));
    // unused rows: -1 indices, NaN costs and terms; a side without a result writes nothing
    HIP_TRY(c, hipMemsetAsync(rk->d_counts, 0, sizeof(int32_t) * 2 * (size_t)n_frames, q.stream));
    HIP_TRY(c, hipMemsetAsync(rk->d_configs, 0xff, sizeof(int32_t) * rows * MAX_LEN, q.stream));
    HIP_TRY(c, hipMemsetAsync(rk->d_costs, 0xff, sizeof(double) * rows, q.stream));
    if (rk->terms) HIP_TRY(c, hipMemsetAsync(rk->d_terms, 0xff, sizeof(double) * rows * COST_TERMS, q.stream));
    if (c->poison) {
      HIP_TRY(c, hipMemsetAsync(q.buf.d_sort, 0xff, sizeof(SortOut) * (size_t)n_frames, q.stream));
      HIP_TRY(c, hipMemsetAsync(rk->d_scratch, 0xff, sizeof(SortRankScratchBig) * SORT_BIG_BLOCKS, q.stream));
    }
    v.top_k = rk->top_k;
    v.counts = rk->d_counts;
    v.configs = rk->d_configs;
    v.costs = rk->d_costs;
    v.terms = rk->d_terms;
    var.kind = SortVariant::RANKED;
    var.rank = &v;
    var.scratch = rk->d_scratch;
  } else if (cached) {
    var.kind = SortVariant::CACHED;
    var.cache = cache_view(c, 0);  // (frame i is planner i)
  }
  fsdp_sort_hist_launch_args ha;
  if (hk) {
    // unused entries: -1 indices, 0xFF flags and codes, zero counts; a side that is not searched writes nothing
    HIP_TRY(c, hipMemsetAsync(hk->d_n_rows, 0, sizeof(int32_t) * 2 * (size_t)n_frames, q.stream));
    HIP_TRY(c, hipMemsetAsync(hk->d_target, 0, sizeof(int32_t) * 2 * (size_t)n_frames, q.stream));
    HIP_TRY(c, hipMemsetAsync(hk->d_rows, 0xff, sizeof(int32_t) * hrows * MAX_LEN, q.stream));
    HIP_TRY(c, hipMemsetAsync(hk->d_is_end, 0xff, hrows, q.stream));
    if (hk->cand) {
      HIP_TRY(c, hipMemsetAsync(hk->d_cand, 0xff, sizeof(int32_t) * hrows * KNN, q.stream));
      HIP_TRY(c, hipMemsetAsync(hk->d_verdict, 0xff, hrows * KNN, q.stream));
    }
    if (c->poison) HIP_TRY(c, hipMemsetAsync(q.buf.d_sort, 0xff, sizeof(SortOut) * (size_t)n_frames, q.stream));
    ha.n_frames = in.n_frames;
    ha.off = in.d_off;
    ha.cones = in.d_cones;
    ha.poses = in.d_poses;
    ha.sorted = q.buf.d_sort;
    ha.big = q.buf.d_big;
    ha.big_state = nullptr;  // (launch_sort_big allocates the blocks on first use)
    ha.big_blocks = SORT_BIG_BLOCKS;
    ha.small = false;        // (launch_sort decides)
    ha.prm = c->d_params;
    ha.view.rows_cap = hk->rows_cap;
    ha.view.n_rows = hk->d_n_rows;
    ha.view.target_length = hk->d_target;
    ha.view.rows = hk->d_rows;
    ha.view.is_end = hk->d_is_end;
    ha.view.cand = hk->d_cand;
    ha.view.verdict = hk->d_verdict;
    var.kind = SortVariant::HISTORY;
    var.hist = &ha;
  }
  std::string names;
  launch_sort(c, q, in, StageIn(), names, var);
  names += ',';
  if (int rc = launch_sort_big(c, q, in, names, var)) return rc;
  if (rk || hk) c->stage_names = names;  // (fsdp_sort_batch leaves the names of the most recent pass in place)
  HIP_TRY(c, hipMemsetAsync(q.buf.d_big, 0, sizeof(int), q.stream));  // (no assemble_kernel follows to reset the list)
  HIP_TRY(c, c->h_sort.reserve((size_t)n_frames, 64));
  HIP_TRY(c, hipMemcpyAsync(c->h_sort, q.buf.d_sort, sizeof(SortOut) * n_frames, hipMemcpyDeviceToHost, q.stream));
  std::vector<int32_t> map, moff;
  if (rk) {
    HIP_TRY(c, hipMemcpyAsync(rk->counts, rk->d_counts, sizeof(int32_t) * 2 * (size_t)n_frames, hipMemcpyDeviceToHost, q.stream));
    HIP_TRY(c, hipMemcpyAsync(rk->configs, rk->d_configs, sizeof(int32_t) * rows * MAX_LEN, hipMemcpyDeviceToHost, q.stream));
    HIP_TRY(c, hipMemcpyAsync(rk->costs, rk->d_costs, sizeof(double) * rows, hipMemcpyDeviceToHost, q.stream));
    if (rk->terms) HIP_TRY(c, hipMemcpyAsync(rk->terms, rk->d_terms, sizeof(double) * rows * COST_TERMS, hipMemcpyDeviceToHost, q.stream));
  }
  if (hk) {
    HIP_TRY(c, hipMemcpyAsync(hk->n_rows, hk->d_n_rows, sizeof(int32_t) * 2 * (size_t)n_frames, hipMemcpyDeviceToHost, q.stream));
    HIP_TRY(c, hipMemcpyAsync(hk->target_length, hk->d_target, sizeof(int32_t) * 2 * (size_t)n_frames, hipMemcpyDeviceToHost, q.stream));
    HIP_TRY(c, hipMemcpyAsync(hk->rows, hk->d_rows, sizeof(int32_t) * hrows * MAX_LEN, hipMemcpyDeviceToHost, q.stream));
    HIP_TRY(c, hipMemcpyAsync(hk->is_end, hk->d_is_end, hrows, hipMemcpyDeviceToHost, q.stream));
    if (hk->cand) {
      HIP_TRY(c, hipMemcpyAsync(hk->cand, hk->d_cand, sizeof(int32_t) * hrows * KNN, hipMemcpyDeviceToHost, q.stream));
      HIP_TRY(c, hipMemcpyAsync(hk->verdict, hk->d_verdict, hrows * KNN, hipMemcpyDeviceToHost, q.stream));
    }
  }
  if (filtered) {  // indices back into the caller's index space (what assemble_kernel does for a full pass)
    map.resize(b.total ? b.total : 1);
    moff.resize((size_t)n_frames + 1);
    HIP_TRY(c, hipMemcpyAsync(map.data(), q.filt.f_map, sizeof(int32_t) * b.total, hipMemcpyDeviceToHost, q.stream));
    HIP_TRY(c, hipMemcpyAsync(moff.data(), q.filt.f_off, sizeof(int32_t) * ((size_t)n_frames + 1), hipMemcpyDeviceToHost, q.stream));
  }
  HIP_TRY(c, hipStreamSynchronize(q.stream));
  if (cached)
    if (int rc = cache_finish(c)) return rc;
  for (int i = 0; i < n_frames; i++) {
    memset(&results[i], 0, sizeof(fsdp_frame_result));
    assemble(&c->h_sort[i], nullptr, nullptr, &results[i]);
    if (filtered) {
      const int32_t* fmap = map.data() + moff[i];
      map_back(results[i].left_idx, MAX_LEN, fmap);
      map_back(results[i].right_idx, MAX_LEN, fmap);
      map_back(results[i].first_k_left, 2, fmap);
      map_back(results[i].first_k_right, 2, fmap);
      if (rk) {
        const size_t per_frame = 2 * (size_t)rk->top_k * MAX_LEN;
        map_back(rk->configs + (size_t)i * per_frame, per_frame, fmap);
      }
      if (hk) {
        const size_t per_frame = 2 * (size_t)hk->rows_cap;
        map_back(hk->rows + (size_t)i * per_frame * MAX_LEN, per_frame * MAX_LEN, fmap);
        if (hk->cand) map_back(hk->cand + (size_t)i * per_frame * KNN, per_frame * KNN, fmap);
      }
    }
  }
  return 0;
}

int fsdp_sort_batch(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses,
                    fsdp_frame_result* results) {
  return sort_batch_impl(c, n_frames, off, cones, poses, results, nullptr);
}

int fsdp_sort_batch_ranked(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses,
                           fsdp_frame_result* results, int top_k, int32_t* counts, int32_t* configs, double* costs, double* terms) {
  RankCall rk;
  rk.top_k = top_k;
  rk.counts = counts;
  rk.configs = configs;
  rk.costs = costs;
  rk.terms = terms;
  return sort_batch_impl(c, n_frames, off, cones, poses, results, &rk);
}

int fsdp_sort_batch_history(fsdp_ctx* c, int n_frames, const int32_t* off, const double* cones, const double* poses,
                            fsdp_frame_result* results, int rows_cap, int32_t* n_rows, int32_t* target_length, int32_t* rows,
                            uint8_t* is_end, int32_t* cand, uint8_t* verdict) {
  HistCall hk;
  hk.rows_cap = rows_cap;
  hk.n_rows = n_rows;
  hk.target_length = target_length;
  hk.rows = rows;
  hk.is_end = is_end;
  hk.cand = cand;
  hk.verdict = verdict;
  return sort_batch_impl(c, n_frames, off, cones, poses, results, nullptr, &hk);
}

int fsdp_match_batch(fsdp_ctx* c, int n_frames, const double* sorted_left, const int32_t* n_left, const double* sorted_right,
                     const int32_t* n_right, const double* poses, fsdp_frame_result* results) {
  if (!c || n_frames < 0) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_match_batch");
  if (n_frames == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  // express the already sorted cones as a tiny frame each: cones = [left..., right...], indices 0..nl-1 / nl..nl+nr-1
  std::vector<int32_t> off(n_frames + 1, 0);
  std::vector<double> cones;
  std::vector<SortOut> so(n_frames);
  for (int f = 0; f < n_frames; f++) {
    int nl = n_left[f], nr = n_right[f];
    if (nl < 0 || nl > MAX_LEN || nr < 0 || nr > MAX_LEN) {
      c->err = "fsdp_match_batch: side length out of range";
      return 1;
    }
    memset(&so[f], 0, sizeof(SortOut));
    for (int i = 0; i < MAX_LEN; i++) so[f].left_idx[i] = so[f].right_idx[i] = -1;
    so[f].n_left = nl;
    so[f].n_right = nr;
    for (int i = 0; i < nl; i++) {
      so[f].left_idx[i] = i;
      cones.push_back(sorted_left[((size_t)f * MAX_LEN + i) * 2]);
      cones.push_back(sorted_left[((size_t)f * MAX_LEN + i) * 2 + 1]);
      cones.push_back((double)T_LEFT);
    }
    for (int i = 0; i < nr; i++) {
      so[f].right_idx[i] = nl + i;
      cones.push_back(sorted_right[((size_t)f * MAX_LEN + i) * 2]);
      cones.push_back(sorted_right[((size_t)f * MAX_LEN + i) * 2 + 1]);
      cones.push_back((double)T_RIGHT);
    }
    off[f + 1] = off[f] + nl + nr;
  }
  if (int rc = sync_all(c)) return rc;
  Work& q = stage_slot(c);
  if (int rc = ensure_work(c, q, n_frames)) return rc;
  if (int rc = upload_inputs(c, q.in, q.stream, Batch{n_frames, off.data(), cones.data(), poses, nullptr, cones.size() / 3, 2 * MAX_LEN})) return rc;
  HIP_TRY(c, hipMemcpyAsync(q.buf.d_sort, so.data(), sizeof(SortOut) * n_frames, hipMemcpyHostToDevice, q.stream));
  launch_match(c, q, q.in.view());
  HIP_TRY(c, c->h_match.reserve((size_t)n_frames, 64));
  HIP_TRY(c, hipMemcpyAsync(c->h_match, q.buf.d_match, sizeof(MatchOut) * n_frames, hipMemcpyDeviceToHost, q.stream));
  HIP_TRY(c, hipStreamSynchronize(q.stream));
  for (int i = 0; i < n_frames; i++) {
    memset(&results[i], 0, sizeof(fsdp_frame_result));
    assemble(nullptr, &c->h_match[i], nullptr, &results[i]);
  }
  return 0;
}

// centers / n_centers / centers_cap: optional side output (fsdp_path_batch_centers)
static int path_batch_impl(fsdp_ctx* c, int n_frames, const double* poses, const double* prev_paths, fsdp_frame_result* results,
                           double* centers, int32_t* n_centers, int centers_cap) {
  if (!c || n_frames < 0) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_path_batch");
  if (n_frames == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sync_all(c)) return rc;  // passes in flight still use the buffers ensure_work may replace
  // the centre points leave the kernels through a buffer the device copy of the parameters points to for this one call
  struct CentersScope {
    fsdp_ctx* c;
    DeviceBuf<double> d_xy;
    DeviceBuf<int32_t> d_n;
    ~CentersScope() {
      if (!d_xy && !d_n) return;
      c->params.centers = nullptr;
      c->params.n_centers = nullptr;
      c->params.centers_cap = 0;
      (void)hipMemcpy(c->d_params, &c->params, sizeof(Params), hipMemcpyHostToDevice);
    }
  } cs{c};
  if (centers) {
    HIP_TRY(c, cs.d_xy.reserve(2 * (size_t)centers_cap * (size_t)n_frames));
    HIP_TRY(c, cs.d_n.reserve((size_t)n_frames));
    HIP_TRY(c, hipMemset(cs.d_n, 0, sizeof(int32_t) * (size_t)n_frames));
    c->params.centers = cs.d_xy;
    c->params.n_centers = cs.d_n;
    c->params.centers_cap = centers_cap;
    HIP_TRY(c, hipMemcpy(c->d_params, &c->params, sizeof(Params), hipMemcpyHostToDevice));
  }
  Work& q = stage_slot(c);
  if (int rc = ensure_work(c, q, n_frames)) return rc;
  HIP_TRY(c, q.in.reserve((size_t)n_frames, 1, prev_paths != nullptr));
  std::vector<MatchOut> mo(n_frames);
  for (int f = 0; f < n_frames; f++) {
    memset(&mo[f], 0, sizeof(MatchOut));
    const fsdp_frame_result& r = results[f];
    if (r.n_left_v < 0 || r.n_left_v > MAX_MATCH || r.n_right_v < 0 || r.n_right_v > MAX_MATCH) {
      c->err = "fsdp_path_batch: cone count out of range";
      return 1;
    }
    mo[f].n_left_v = r.n_left_v;
    mo[f].n_right_v = r.n_right_v;
    memcpy(mo[f].left_v, r.left_v, sizeof(r.left_v));
    memcpy(mo[f].right_v, r.right_v, sizeof(r.right_v));
    memcpy(mo[f].l2r, r.l2r, sizeof(r.l2r));
    memcpy(mo[f].r2l, r.r2l, sizeof(r.r2l));
  }
  q.in.n_frames = n_frames;
  q.in.max_cones = 0;
  q.in.use_prev = prev_paths != nullptr;
  HIP_TRY(c, hipMemcpyAsync(q.buf.d_match, mo.data(), sizeof(MatchOut) * n_frames, hipMemcpyHostToDevice, q.stream));
  HIP_TRY(c, hipMemcpyAsync(q.in.d_poses, poses, sizeof(double) * 4 * (size_t)n_frames, hipMemcpyHostToDevice, q.stream));
  if (prev_paths)
    HIP_TRY(c, hipMemcpyAsync(q.in.d_prev, prev_paths, sizeof(double) * PATH_POINTS * 4 * (size_t)n_frames, hipMemcpyHostToDevice, q.stream));
  std::string names;
  launch_path(c, q, q.in.view(), nullptr, names, n_frames);
  launch_path_retry(c, q, q.in.view());
  HIP_TRY(c, hipMemsetAsync(q.buf.d_retry, 0, sizeof(int), q.stream));  // (no assemble_kernel follows to reset the list)
  c->stage_names = names + "path_retry_kernel";
  HIP_TRY(c, c->h_path.reserve((size_t)n_frames, 64));
  HIP_TRY(c, hipMemcpyAsync(c->h_path, q.buf.d_path, sizeof(PathOut) * n_frames, hipMemcpyDeviceToHost, q.stream));
  HIP_TRY(c, hipStreamSynchronize(q.stream));
  for (int i = 0; i < n_frames; i++) {
    results[i].status = 0;
    assemble(nullptr, nullptr, &c->h_path[i], &results[i]);
  }
  if (centers) {
    HIP_TRY(c, hipMemcpy(centers, cs.d_xy, sizeof(double) * 2 * (size_t)centers_cap * (size_t)n_frames, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(n_centers, cs.d_n, sizeof(int32_t) * (size_t)n_frames, hipMemcpyDeviceToHost));
  }
  return 0;
}

int fsdp_path_batch(fsdp_ctx* c, int n_frames, const double* poses, const double* prev_paths, fsdp_frame_result* results) {
  return path_batch_impl(c, n_frames, poses, prev_paths, results, nullptr, nullptr, 0);
}

int fsdp_path_batch_centers(fsdp_ctx* c, int n_frames, const double* poses, const double* prev_paths, fsdp_frame_result* results,
                            double* centers, int32_t* n_centers, int centers_cap) {
  if (!c) return 1;
  if (!centers || !n_centers || centers_cap <= 0) {
    c->err = "fsdp_path_batch_centers: centers, n_centers and a positive centers_cap are required";
    return 1;
  }
  return path_batch_impl(c, n_frames, poses, prev_paths, results, centers, n_centers, centers_cap);
}

#ifdef FSDP_PROFILE
int fsdp_profile_select(fsdp_ctx* c, int sort_kernel_instead_of_path) {
  if (!c) return 1;
  c->profile_sort = sort_kernel_instead_of_path != 0;
  return 0;
}
// profiling build only (tools/section_profile.py): per-frame per-section cycle sums of the path kernel, resident batch
int fsdp_profile_path(fsdp_ctx* c, long long* out32_per_frame) {
  if (!c || !c->resident || c->res.n_frames == 0) return 1;
  DeviceBuf<long long> buf;
  size_t bytes = sizeof(long long) * 32 * (size_t)c->res.n_frames;
  HIP_TRY(c, buf.reserve(32 * (size_t)c->res.n_frames));
  long long* d = buf;
  HIP_TRY(c, hipMemsetAsync(d, 0, bytes, c->stream));
  HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(fsdp::g_prof), &d, sizeof(d)));
  Work& q = c->slot[0];
  std::string names;
  if (c->profile_sort)
    launch_sort(c, q, c->res.view(), StageIn(), names, SortVariant());
  else
    launch_path(c, q, c->res.view(), nullptr, names, frames_in_flight(c, c->res.n_frames, false));
  HIP_TRY(c, hipMemsetAsync(q.buf.d_big, 0, sizeof(int), q.stream));
  HIP_TRY(c, hipMemsetAsync(q.buf.d_retry, 0, sizeof(int), q.stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, copy_sync(c, out32_per_frame, d, bytes, hipMemcpyDeviceToHost));
  long long* z = nullptr;
  HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(fsdp::g_prof), &z, sizeof(z)));
  return 0;
}
#endif

int fsdp_skidpad_set_tables(fsdp_ctx* c, const double* table_xy, int n_table, const double* noise, int n_noise) {
  if (!c || !table_xy || n_table < 20 || n_table > 8192 || !noise || n_noise < 6) return 1;
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = sync_all(c);
  if (rc) return rc;
  // known global path = table[::2] (skidpad_relocalizer.py:242-243)
  std::vector<double> half;
  for (int i = 0; i < n_table; i += 2) {
    half.push_back(table_xy[2 * i]);
    half.push_back(table_xy[2 * i + 1]);
  }
  c->d_table.reset();
  c->d_noise.reset();
  c->have_tables = false;
  HIP_TRY(c, c->d_table.reserve(half.size()));
  HIP_TRY(c, c->d_noise.reserve((size_t)n_noise));
  HIP_TRY(c, copy_sync(c, c->d_table, half.data(), sizeof(double) * half.size(), hipMemcpyHostToDevice));
  HIP_TRY(c, copy_sync(c, c->d_noise, noise, sizeof(double) * (size_t)n_noise, hipMemcpyHostToDevice));
  // the two reference centres and the table spacing are derived from the table on the device (skid_centers_kernel)
  DeviceBuf<double> d_full, d_scratch, d_out;
  HIP_TRY(c, d_full.reserve(2 * (size_t)n_table));
  HIP_TRY(c, d_scratch.reserve(3 * (size_t)n_table));
  HIP_TRY(c, d_out.reserve(5));
  HIP_TRY(c, hipMemcpyAsync(d_full, table_xy, sizeof(double) * 2 * (size_t)n_table, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(skid_centers_kernel, dim3(1), dim3(WAVE), 0, c->stream, d_full, n_table, d_scratch, d_out);
  HIP_TRY(c, hipMemcpyAsync(c->skid_consts, d_out, sizeof(double) * 5, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->tables.path = c->d_table;
  c->tables.n_path = (int)(half.size() / 2);
  c->tables.noise = c->d_noise;
  c->tables.n_noise = n_noise;
  c->tables.ref_right[0] = c->skid_consts[0];
  c->tables.ref_right[1] = c->skid_consts[1];
  c->tables.ref_left[0] = c->skid_consts[2];
  c->tables.ref_left[1] = c->skid_consts[3];
  c->tables.mean_distance = c->skid_consts[4];
  c->tables.prm = c->d_params;
  c->have_tables = true;
  return 0;
}

int fsdp_skidpad_constants(fsdp_ctx* c, double* out5) {
  if (!c || !out5 || !c->have_tables) return 1;
  memcpy(out5, c->skid_consts, sizeof(double) * 5);
  return 0;
}


int fsdp_skidpad_reset(fsdp_ctx* c, int n_instances) {
  if (!c || n_instances <= 0) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_skidpad_reset");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sync_all(c)) return rc;
  // (n_instances says what the planners' state holds room for: 0 until all three blocks stand)
  c->n_instances = 0;
  HIP_TRY(c, c->d_skid.reserve((size_t)n_instances));
  HIP_TRY(c, c->d_skid_backup.reserve((size_t)n_instances));
  HIP_TRY(c, c->d_skid_sync.reserve((size_t)n_instances + 1));
  c->n_instances = n_instances;
  // fresh planners: nothing latched, previous path = the constant initial path
  std::vector<SkidState> init(n_instances);
  double def[PATH_POINTS][4];
  HIP_TRY(c, copy_sync(c, def, c->d_default_path, sizeof(def), hipMemcpyDeviceToHost));
  for (auto& s : init) {
    memset(&s, 0, sizeof(s));
    memcpy(s.prev, def, sizeof(def));
  }
  HIP_TRY(c, copy_sync(c, c->d_skid, init.data(), sizeof(SkidState) * (size_t)n_instances, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemsetAsync(c->d_skid_sync, 0, sizeof(uint32_t) * ((size_t)n_instances + 1), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->skid_ticket_base = 0;
  c->skid_step_no = 0;
  c->skid_all_reloc = false;
  c->skid_reloc_epoch++;
  return 0;
}

// Steps per launch for a caller that submits ahead (half the slots at most, so that one group runs while the next one is
// being submitted).  Thousands of (instance, step) pairs go through the packed kernels of the autocross path stage: the
// group is made as large as gives them 16384 frames (the more steps share the launches the better: 1024 instances plan
// 3.0 / 3.8 / 4.1 / 4.6 M frames/s in groups of 4 / 8 / 12 / 16); below that the steps get a wavefront each (skid_path_kernel) and the
// group is what puts at least three wavefronts on every SIMD (256 CUs x 4 SIMDs; a partly filled second round costs less
// than an unfilled first one: profiles/r03_skidpad_groups.txt).
static int skid_group_size(const fsdp_ctx* c) {
  const int n = c->n_instances;
  const int half = c->overlap / 2 > 1 ? c->overlap / 2 : 1;
  auto clamp = [&](int g) { return g < 1 ? 1 : g > SKID_GROUP_MAX ? SKID_GROUP_MAX : g > half ? half : g; };
  if (c->skid_group_env > 0) return c->skid_group_env > SKID_GROUP_MAX ? SKID_GROUP_MAX : c->skid_group_env > c->overlap ? c->overlap : c->skid_group_env;
  const int packed = clamp((16384 + n - 1) / n);
  if ((long long)packed * n >= c->skid_pack_min && c->params.max_deg == 3) return packed;
  return clamp((3072 + n - 1) / n);
}

static SkidGroup skid_group_of(fsdp_ctx* c, const int* slots, int n_steps, int step0) {
  SkidGroup g;
  memset(&g, 0, sizeof(g));
  for (int k = 0; k < n_steps; k++) {
    Work& q = c->slot[slots[k]];
    g.step[k] = SkidStep{q.in.d_poses, q.skid_attempted ? q.buf.d_skid_status : nullptr, q.buf.d_arena, q.buf.d_path, q.buf.d_skid_info};
  }
  g.n_steps = n_steps;
  g.step0 = step0;
  g.ticket_base = c->skid_ticket_base;
  return g;
}

// skid_path_kernel for the steps whose inputs, relocalization status and output records sit in slots[0 .. n_steps): one
// wavefront per (instance, step), csrc/skidpad_kernel.h "steps in flight, a wavefront per (instance, step)"
static void launch_skid_path(fsdp_ctx* c, const int* slots, int n_steps, int step0) {
  const int n = c->n_instances;
  const SkidGroup g = skid_group_of(c, slots, n_steps, step0);
  c->skid_ticket_base += (uint32_t)n * (uint32_t)n_steps;
  hipLaunchKernelGGL(skid_path_kernel, dim3((unsigned)n * (unsigned)n_steps), dim3(WAVE), 0, c->stream, n, g, c->d_skid, c->tables, c->d_chord,
                     c->d_skid_sync);
}

static int launch_skid_packed(fsdp_ctx* c, const int* slots, int n_steps, int step0) {
  const int n = c->n_instances;
  const int frames = n * n_steps;
  if ((size_t)frames > c->group.frames()) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, c->group.reserve((size_t)frames, (size_t)n, (size_t)skid_group_size(c)));
  }
  const SkidGroup g = skid_group_of(c, slots, n_steps, step0);
  hipStream_t xs = c->stream;
  HIP_TRY(c, hipMemsetAsync(c->group.d_g_retry, 0, sizeof(int), xs));  // (the packed kernels' list of frames they hand on; the commit kernel goes by the frames' records)
  skid_group_mark(c);
  hipLaunchKernelGGL(skid_select_kernel, dim3((unsigned)n), dim3(WAVE), 0, xs, n, g, c->d_skid, c->tables, c->group.d_g_sel);
  if (frames >= PACK_FRAMES) {
    if (c->fit_g == 4)
      launch_skid_packed_kernels<8, 4>(c, frames);
    else
      launch_skid_packed_kernels<8, 8>(c, frames);
  } else {
    launch_skid_packed_kernels<16, 16>(c, frames);
  }
  hipLaunchKernelGGL(skid_commit_kernel, dim3((unsigned)n), dim3(WAVE), 0, xs, n, g, c->d_skid, c->tables, c->d_chord, c->group.d_g_sel, c->group.d_g_mid, c->group.d_g_out,
                     c->group.d_g_arena, c->d_skid_sync);
  skid_group_mark(c);
  if (c->skid_time_groups) c->skid_group_frames.push_back(frames);
  return 0;
}

// The path kernel, result assembly and completion event of the steps submitted so far whose launch was put off
// (fsdp_skidpad_submit): one skid_path_kernel over all of them.
static int flush_skid(fsdp_ctx* c) {
  const int n_steps = c->n_skid_pending;
  if (n_steps == 0) return 0;
  c->n_skid_pending = 0;
  HIP_TRY(c, hipSetDevice(c->device));
  const int n = c->n_instances;
  hipStream_t xs = c->stream;
  if ((long long)n * n_steps >= c->skid_pack_min && c->params.max_deg == 3) {
    if (int rc = launch_skid_packed(c, c->skid_pending, n_steps, c->skid_step_no - n_steps)) return rc;
  } else {
    launch_skid_path(c, c->skid_pending, n_steps, c->skid_step_no - n_steps);
  }
  for (int k = 0; k < n_steps; k++) {
    Work& q = c->slot[c->skid_pending[k]];
    Work::Ticket& t = q.tk[0];
    t.pending = false;
    if (t.dev.on) {
      // a device step: its records to the caller's arrays on the GPU (skid_device_out_kernel)
      fsdp_skid_dio_out_args o;
      o.n_inst = n;
      o.paths = q.buf.d_path;
      o.info = q.buf.d_skid_info;
      o.out_paths = t.dev.paths;
      o.out_status = t.dev.status;
      o.out_info = (SkidInfo*)t.dev.skid_info;
      o.out_records = (PathOut*)t.dev.skid_records;
      o.not_reloc = t.h_bad.device() + 1;
      fsdp_skid_dio_launch_out(xs, &o);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipEventRecord(t.done, xs));
      continue;
    }
    // page-locked results: assemble_kernel writes them into the caller's buffer (over PCIe); the planners' information
    // records ride along into the ticket's pinned block
    // (only a buffer that is page-locked over its WHOLE extent — decided at submit time, `via_stage` otherwise: a view
    // that merely starts inside a registered range must not be written from the device)
    fsdp_frame_result* direct = (t.user_results && !t.via_stage) ? (fsdp_frame_result*)device_view(t.user_results) : nullptr;
    if (t.compact) {
      // compact results = the path stage's own records: one plain copy (and the information records) instead of the assembly of
      // 2.4 KB results whose sorting / matching fields a skidpad step leaves empty anyway
      CopySegs segs;
      segs.n = 0;
      segs.rebase = 0;
      if (direct) segs.seg[segs.n++] = CopySeg{q.buf.d_path, direct, sizeof(PathOut) * (unsigned long long)n};
      if (t.user_info) segs.seg[segs.n++] = CopySeg{q.buf.d_skid_info, device_view(t.h_info), sizeof(SkidInfo) * (unsigned long long)n};
      if (segs.n) hipLaunchKernelGGL(stage_in_kernel, dim3(128), dim3(256), 0, xs, segs);
      HIP_TRY(c, hipGetLastError());
      if (t.via_stage) HIP_TRY(c, hipMemcpyAsync(t.h_stage, q.buf.d_path, sizeof(PathOut) * (size_t)n, hipMemcpyDeviceToHost, xs));
      HIP_TRY(c, hipEventRecord(t.done, xs));
      continue;
    }
    if (t.user_results || t.user_info) {
      Pass pass;
      pass.host = direct;
      pass.info = t.user_info ? (SkidInfo*)device_view(t.h_info) : nullptr;
      launch_assemble(c, q, t.user_results ? n : 0, pass, true);
    }
    HIP_TRY(c, hipGetLastError());
    if (t.via_stage) HIP_TRY(c, hipMemcpyAsync(t.h_stage, q.buf.d_result, sizeof(fsdp_frame_result) * (size_t)n, hipMemcpyDeviceToHost, xs));
    HIP_TRY(c, hipEventRecord(t.done, xs));
  }
  return 0;
}

// One frame for every planner instance, asynchronously.  Every command goes to the context's main stream in submit order;
// a step's transfers are kernels of that same stream when the caller's buffers are page-locked (stage_in_kernel reads the
// inputs from host memory, assemble_kernel writes results and planner information into it), so nothing ever waits for
// the host: a replay that knows its frames ahead submits ahead (up to `depth` steps, each with its own buffers on the
// device) and collects behind.  The inputs and the relocalization attempt of a step are enqueued at once; its path
// kernel is put off until `skid_group` steps have been submitted — they share one launch, with one wavefront per
// (instance, step) — or until somebody asks for the step (fsdp_collect, fsdp_ticket_done, any blocking call), so a live
// car that submits and collects one step at a time (fsdp_skidpad_step) gets one launch per step.
static int skidpad_submit_impl(fsdp_ctx* c, int n_instances, const int32_t* off, const double* cones, const double* poses,
                               fsdp_frame_result* results, fsdp_skidpad_info* info, long long* ticket, bool compact) {
  if (!c || !ticket) return 1;
  *ticket = -1;
  if (!c->have_tables || n_instances != c->n_instances || !c->d_skid) {
    c->err = "fsdp_skidpad_submit: call fsdp_skidpad_set_tables and fsdp_skidpad_reset(n_instances) first";
    return 1;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  Batch b;
  if (int rc = check_batch(c, n_instances, off, cones, poses, nullptr, &b)) return rc;
  // one step per slot (the slots only hold the steps' buffers, every command goes to the main stream): the next free one
  int si = (int)(c->next_ticket % c->overlap);
  for (int k = 0; k < c->overlap && c->slot[si].tk[0].id >= 0; k++) si = (si + 1) % c->overlap;
  Work& q = c->slot[si];
  Work::Ticket& t = q.tk[0];
  if (t.id >= 0) {
    c->err = "fsdp_skidpad_submit: all " + std::to_string(c->overlap) + " slots hold a ticket; collect one first, e.g. ticket " + std::to_string(t.id);
    return 4;
  }
  // (the slot's ticket is free, i.e. collected: nothing queued uses its buffers any more, they may be replaced)
  if (int rc = ensure_work(c, q, n_instances)) return rc;
  hipStream_t xs = c->stream;
  // Once every planner is relocalized nobody reads cones any more (Relocalizer.attempt_relocalization_calculation returns
  // at once, relocalization_base_class.py:56-57; the path comes from the known map): they stay on the host, and the
  // relocalization kernel is not launched.  (Known from the planner information of a collected step.)
  const bool attempt = !c->skid_all_reloc;
  if (!attempt) b.total = 0;
  if (inputs_pinned(b)) {
    if (int rc = stage_inputs(c, q.in, xs, b)) return rc;
  } else if (int rc = upload_inputs(c, q.in, xs, b)) {
    return rc;
  }
  q.skid_attempted = attempt;
  if (info) HIP_TRY(c, t.h_info.reserve((size_t)n_instances));
  const bool direct = results && is_pinned(results, (compact ? sizeof(PathOut) : sizeof(fsdp_frame_result)) * (size_t)n_instances);
  if (results && !direct) HIP_TRY(c, t.h_stage.reserve((size_t)n_instances));
  if (!t.done) HIP_TRY(c, hipEventCreateWithFlags(&t.done.h, hipEventDisableTiming));
  if (attempt)
    hipLaunchKernelGGL(skid_reloc_kernel, dim3((unsigned)n_instances), dim3(WAVE), 0, c->stream, n_instances, q.in.d_off, q.in.d_cones, q.in.d_poses,
                       c->d_skid, c->tables, q.buf.d_arena, q.buf.d_skid_status, c->skid_step_no);
  HIP_TRY(c, hipGetLastError());
  c->skid_step_no++;
  q.pass_in = &q.in;
  q.pass_skid = true;
  q.unverified = false;
  t.batch = b;
  t.skid = true;
  t.pending = true;
  t.user_results = results;
  t.user_info = info;
  t.via_stage = results && !direct;
  t.compact = compact;
  t.reloc_epoch = c->skid_reloc_epoch;
  c->skid_pending[c->n_skid_pending++] = si;
  c->last = fsdp_ctx::LastPass{si, n_instances, false, true};
  t.id = c->next_ticket++;
  c->outstanding++;
  *ticket = t.id;
  if (c->n_skid_pending >= skid_group_size(c)) return flush_skid(c);
  return 0;
}

int fsdp_skidpad_submit(fsdp_ctx* c, int n_instances, const int32_t* off, const double* cones, const double* poses,
                        fsdp_frame_result* results, fsdp_skidpad_info* info, long long* ticket) {
  return skidpad_submit_impl(c, n_instances, off, cones, poses, results, info, ticket, false);
}
static_assert(sizeof(fsdp_path_result) == sizeof(PathOut) && offsetof(fsdp_path_result, status) == offsetof(PathOut, status) &&
                  offsetof(fsdp_path_result, path_fallback) == offsetof(PathOut, fallback) && offsetof(fsdp_path_result, n_dense) == offsetof(PathOut, n_dense),
              "fsdp_path_result is the path stage's record");
int fsdp_skidpad_submit_compact(fsdp_ctx* c, int n_instances, const int32_t* off, const double* cones, const double* poses,
                                fsdp_path_result* results, fsdp_skidpad_info* info, long long* ticket) {
  return skidpad_submit_impl(c, n_instances, off, cones, poses, (fsdp_frame_result*)results, info, ticket, true);
}

// The same step with every array in the memory of the context's GPU (include/fsdp.h).  The way in is a device ticket's (scan +
// gather into the slot's InputStore), the relocalization attempt and the path kernels are the host route's, on the context's one
// stream; skid_device_reset_kernel goes in front of the attempt and skid_device_out_kernel behind the path kernels.  The step is
// never left pending: it joins the steps the host calls left pending, and the group is flushed.
static_assert(sizeof(fsdp_skidpad_info) == sizeof(SkidInfo) && offsetof(fsdp_skidpad_info, relocalized) == offsetof(SkidInfo, relocalized) &&
                  offsetof(fsdp_skidpad_info, index_along_path) == offsetof(SkidInfo, index_along_path) &&
                  offsetof(fsdp_skidpad_info, translation) == offsetof(SkidInfo, translation) && offsetof(fsdp_skidpad_info, rotation) == offsetof(SkidInfo, rotation),
              "fsdp_skidpad_info is the planners' information record");
int fsdp_skidpad_submit_device(fsdp_ctx* c, int n_instances, int cone_capacity, const int32_t* counts, const double* cones, const double* poses,
                               const int32_t* reset, double* paths, int32_t* status, fsdp_skidpad_info* info, fsdp_path_result* records,
                               void* after_stream, long long* ticket) {
  if (!c || !ticket) return 1;
  *ticket = -1;
  const std::string who = "fsdp_skidpad_submit_device";
  if (c->mission != 2) {
    c->err = who + ": not a skidpad context (the other missions' device tickets go through fsdp_submit_device)";
    return 1;
  }
  if (!c->have_tables || n_instances < 1 || n_instances != c->n_instances || !c->d_skid) {
    c->err = who + ": call fsdp_skidpad_set_tables and fsdp_skidpad_reset(n_instances) first";
    return 1;
  }
  if (cone_capacity < 0) {
    c->err = who + ": cone_capacity must be >= 0";
    return 1;
  }
  if ((long long)n_instances * cone_capacity > 0x7fffffffll) {
    c->err = who + ": n_instances x cone_capacity = " + std::to_string((long long)n_instances * cone_capacity) + " cone rows exceed the int32 offsets of a step";
    return 1;
  }
  if (!counts || !poses || !paths || !status || (cone_capacity > 0 && !cones)) {
    c->err = who + ": counts, poses, paths and status are required" + (cone_capacity > 0 ? ", and cones with cone_capacity > 0" : "");
    return 1;
  }
  if (!fsdp_skid_dio_launch_reset || !fsdp_skid_dio_launch_in || !fsdp_skid_dio_launch_out) {
    c->err = who + ": this library was built without the device ticket kernels (csrc/device_io_lib.hip)";
    return 2;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = (size_t)n_instances;
  const struct {
    const char* name;
    const void* p;
    size_t bytes;
  } arrays[] = {{"counts", counts, sizeof(int32_t) * n},
                {"cones", cone_capacity > 0 ? cones : nullptr, sizeof(double) * 3 * n * (size_t)cone_capacity},
                {"poses", poses, sizeof(double) * 4 * n},
                {"reset", reset, sizeof(int32_t) * n},
                {"paths", paths, sizeof(double) * PATH_POINTS * 4 * n},
                {"status", status, sizeof(int32_t) * n},
                {"info", info, sizeof(fsdp_skidpad_info) * n},
                {"records", records, sizeof(fsdp_path_result) * n}};
  for (const auto& x : arrays)
    if (x.p && !device_owns(c, x.p, x.bytes)) {
      c->err = who + ": " + x.name + " is not device memory of the context's GPU over its whole extent of " + std::to_string(x.bytes) +
               " bytes (host memory, page-locked or not, goes through fsdp_skidpad_submit; managed memory, another GPU's memory and memory of "
               "another HIP runtime are not accepted)";
      return 1;
    }
  // one step per slot, as for fsdp_skidpad_submit
  int si = (int)(c->next_ticket % c->overlap);
  for (int k = 0; k < c->overlap && c->slot[si].tk[0].id >= 0; k++) si = (si + 1) % c->overlap;
  Work& q = c->slot[si];
  Work::Ticket& t = q.tk[0];
  if (t.id >= 0) {
    c->err = who + ": all " + std::to_string(c->overlap) + " slots hold a ticket; collect one first, e.g. ticket " + std::to_string(t.id);
    return 4;
  }
  // everything the step needs room for, before anything is enqueued (the slot's ticket is collected: nothing queued uses its buffers)
  const bool attempt = reset != nullptr || !c->skid_all_reloc;
  if (int rc = ensure_work(c, q, n_instances)) return rc;
  // (rows and max_cones are upper bounds, as for a device ticket: the host never dereferences the batch)
  const Batch b{n_instances, nullptr, nullptr, nullptr, nullptr, attempt ? n * (size_t)cone_capacity : 0, cone_capacity};
  if (int rc = take_batch(c, q.in, b)) return rc;
  HIP_TRY(c, t.h_bad.reserve(2, 16, Pin::MappedCoherent));
  if (!t.done) HIP_TRY(c, hipEventCreateWithFlags(&t.done.h, hipEventDisableTiming));
  if (after_stream && !t.after) HIP_TRY(c, hipEventCreateWithFlags(&t.after.h, hipEventDisableTiming));
  hipStream_t xs = c->stream;
  if (reset) {
    // The steps the host calls left pending plan with the planners as they are: their path kernels go in front of the reset.
    if (int rc = flush_skid(c)) return rc;
    c->skid_all_reloc = false;  // (the reset planners have to relocalize again: the cones are read again)
    c->skid_reloc_epoch++;
  }
  t.h_bad[0] = -1;
  t.h_bad[1] = 0;
  if (after_stream) {
    HIP_TRY(c, hipEventRecord(t.after, (hipStream_t)after_stream));
    HIP_TRY(c, hipStreamWaitEvent(xs, t.after, 0));
  }
  if (reset) {
    fsdp_skid_dio_reset_args r;
    r.n_inst = n_instances;
    r.reset = reset;
    r.states = c->d_skid;
    r.default_path = c->d_default_path;
    fsdp_skid_dio_launch_reset(xs, &r);
  }
  fsdp_dio_in_args a;
  a.n_frames = n_instances;
  a.cone_capacity = cone_capacity;
  a.counts = counts;
  a.cones = cone_capacity > 0 ? cones : nullptr;
  a.poses = poses;
  a.prev = nullptr;
  a.bad_frame = t.h_bad.device();
  a.dst_off = q.in.d_off;
  a.dst_cones = q.in.d_cones;
  a.dst_poses = q.in.d_poses;
  a.dst_prev = nullptr;
  fsdp_skid_dio_launch_in(xs, &a, attempt ? 1 : 0);
  q.skid_attempted = attempt;
  if (attempt)
    hipLaunchKernelGGL(skid_reloc_kernel, dim3((unsigned)n_instances), dim3(WAVE), 0, xs, n_instances, q.in.d_off, q.in.d_cones, q.in.d_poses, c->d_skid,
                       c->tables, q.buf.d_arena, q.buf.d_skid_status, c->skid_step_no);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) {
    // (nothing of the step is left running over the caller's arrays, and no ticket goes out)
    (void)hipStreamSynchronize(xs);
    c->err = who + ": " + hipGetErrorString(e);
    return 2;
  }
  c->skid_step_no++;
  q.pass_in = &q.in;
  q.pass_skid = true;
  q.unverified = false;
  t.batch = b;
  t.skid = true;
  t.pending = true;
  t.user_results = nullptr;
  t.user_info = nullptr;
  t.via_stage = false;
  t.compact = true;
  t.reloc_epoch = c->skid_reloc_epoch;
  t.dev = Work::DevPass{true, cone_capacity, counts, a.cones, poses, nullptr, paths, status, nullptr, nullptr, info, records};
  c->skid_pending[c->n_skid_pending++] = si;
  c->last = fsdp_ctx::LastPass{si, n_instances, false, true};
  t.id = c->next_ticket++;
  c->outstanding++;
  *ticket = t.id;
  return flush_skid(c);
}

int fsdp_skidpad_step(fsdp_ctx* c, int n_instances, const int32_t* off, const double* cones, const double* poses,
                      fsdp_frame_result* results, fsdp_skidpad_info* info) {
  if (!c) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_skidpad_step");
  long long t;
  if (int rc = fsdp_skidpad_submit(c, n_instances, off, cones, poses, results, info, &t)) return rc;
  return fsdp_collect(c, t);
}

// Timing of the packed path-stage kernels of the groups of steps a replay forms (fsdp_skidpad_submit): enable, replay, read.
int fsdp_skidpad_time_groups(fsdp_ctx* c, int enable) {
  if (!c) return 1;
  c->skid_group_ev.clear();
  c->skid_group_frames.clear();
  c->skid_group_names.clear();
  c->skid_time_groups = enable != 0;
  return 0;
}
int fsdp_skidpad_group_times(fsdp_ctx* c, float* ms5, int* n_groups, long long* n_frames, char* names, int names_cap) {
  if (!c || !ms5 || !n_groups || !n_frames) return 1;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 5; k++) ms5[k] = 0.f;
  const size_t groups = c->skid_group_frames.size();
  if (c->skid_group_ev.size() != 6 * groups) {
    c->err = "fsdp_skidpad_group_times: incomplete event set";
    return 1;
  }
  long long frames = 0;
  for (size_t gidx = 0; gidx < groups; gidx++) {
    for (int k = 0; k < 5; k++) {
      float t = 0.f;
      HIP_TRY(c, hipEventElapsedTime(&t, c->skid_group_ev[6 * gidx + k], c->skid_group_ev[6 * gidx + k + 1]));
      ms5[k] += t;
    }
    frames += c->skid_group_frames[gidx];
  }
  *n_groups = (int)groups;
  *n_frames = frames;
  if (names && names_cap > 0) snprintf(names, (size_t)names_cap, "%s", c->skid_group_names.c_str());
  return 0;
}

int fsdp_skidpad_time_path(fsdp_ctx* c, int iters, float* ms_total) {
  if (!c || !c->d_skid || c->n_instances <= 0 || iters <= 0) return 1;
  if (c->outstanding) return busy_error(c, "fsdp_skidpad_time_path");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sync_all(c)) return rc;
  if (c->last.slot < 0 || !c->slot[c->last.slot].pass_skid || c->last.n != c->n_instances) {
    c->err = "fsdp_skidpad_time_path: run a step first";
    return 1;
  }
  size_t bytes = sizeof(SkidState) * (size_t)c->n_instances;
  HIP_TRY(c, hipMemcpyAsync(c->d_skid_backup, c->d_skid, bytes, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[4], c->stream));
  for (int i = 0; i < iters; i++) launch_skid_path(c, &c->last.slot, 1, c->skid_step_no);  // (a step number of its own: nothing to wait for)
  HIP_TRY(c, hipEventRecord(c->ev[5], c->stream));
  HIP_TRY(c, hipEventSynchronize(c->ev[5]));
  float t = 0;
  HIP_TRY(c, hipEventElapsedTime(&t, c->ev[4], c->ev[5]));
  HIP_TRY(c, hipMemcpyAsync(c->d_skid, c->d_skid_backup, bytes, hipMemcpyDeviceToDevice, c->stream));
  // the timed launches published step skid_step_no + 1 for every planner while the restored state is that of step
  // skid_step_no: put the publish counters back too, or the second step of the next group launch would not wait for the first
  HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)(c->d_skid_sync + 1), c->skid_step_no, (size_t)c->n_instances, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (ms_total) *ms_total = t;
  return 0;
}

// ---- per-stage intermediate of the path stage: the refit's spline ------------------------------------------------------
// the slot of the most recent pass, when it holds that pass of a whole call (everything in flight has finished)
static Work* debug_slot(fsdp_ctx* c, const char* who) {
  if (c->last.slot < 0 || !c->last.whole || c->last.n <= 0) {
    c->err = std::string(who) + ": no pass to read (none yet, a blocking call cut into chunks, or its slot released or reused since)";
    return nullptr;
  }
  return &c->slot[c->last.slot];
}

extern "C" int fsdp_debug_refit(fsdp_ctx* c, int32_t* n_knots, double* knots34, double* coeffs68) {
  if (!c || !n_knots || !knots34 || !coeffs68) return 1;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sync_all(c)) return rc;
  Work* qp = debug_slot(c, "fsdp_debug_refit");
  if (!qp) return 1;
  Work& q = *qp;
  const int n = c->last.n;
  std::vector<FitRec> recs((size_t)n);
  std::vector<PathMid> mids((size_t)n);
  const size_t fit_off = (size_t)ARENA_FIT * sizeof(double);  // frame_arena(): A.fit
  HIP_TRY(c, hipMemcpy2DAsync(recs.data(), sizeof(FitRec), (const char*)(q.buf.d_arena.get() + (size_t)c->last.offset * ARENA_DOUBLES) + fit_off, sizeof(double) * ARENA_DOUBLES,
                              sizeof(FitRec), (size_t)n, hipMemcpyDeviceToHost, q.stream));
  HIP_TRY(c, hipMemcpyAsync(mids.data(), q.buf.d_mid + c->last.offset, sizeof(PathMid) * (size_t)n, hipMemcpyDeviceToHost, q.stream));
  HIP_TRY(c, hipStreamSynchronize(q.stream));
  for (int i = 0; i < n; i++) {
    // only frames that went prep -> fit -> finish hold a record (the others took the exact route or ended earlier)
    const bool fast = c->stage_names.find("fit_kernel") != std::string::npos && mids[i].status == ST_OK;
    n_knots[i] = fast ? recs[i].n : -1;
    memcpy(knots34 + (size_t)i * 34, recs[i].t, sizeof(double) * 34);
    memcpy(coeffs68 + (size_t)i * 68, recs[i].c, sizeof(double) * 68);
  }
  return 0;
}

// raw doubles of a frame's scratch arena of the most recent pass (tests / debug builds)
extern "C" int fsdp_debug_arena(fsdp_ctx* c, int frame, int offset, int count, double* out) {
  if (!c || !out || frame < 0 || offset < 0 || count < 0 || offset + count > ARENA_DOUBLES) return 1;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sync_all(c)) return rc;
  Work* q = debug_slot(c, "fsdp_debug_arena");
  if (!q || frame >= c->last.n) return 1;
  HIP_TRY(c, copy_sync(c, out, q->buf.d_arena + ((size_t)c->last.offset + (size_t)frame) * ARENA_DOUBLES + offset, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
  return 0;
}

// ---- device arithmetic self-test ------------------------------------------------------------------------------------------
// One routine behind the five entry points: n elements, inputs of `per` doubles per element each, an output of out_per doubles
// per element.  Device blocks for all of them, inputs in, launch(device inputs, device output) on the context's stream, output
// back, wait.
struct SelftestIn {
  const double* host;
  int per;
};
static int run_selftest(fsdp_ctx* c, int n, std::initializer_list<SelftestIn> ins, int out_per, double* out,
                        const std::function<void(double* const*, double*)>& launch) {
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t bytes = sizeof(double) * (size_t)n;
  std::vector<DeviceBuf<double>> own(ins.size() + 1);  // the inputs in order, then the output
  std::vector<double*> d(own.size(), nullptr);
  hipError_t e = hipSuccess;
  size_t k = 0;
  for (const SelftestIn& in : ins)
    if (e == hipSuccess) e = own[k++].reserve((size_t)in.per * (size_t)n);
  if (e == hipSuccess) e = own.back().reserve((size_t)out_per * (size_t)n);
  for (k = 0; k < own.size(); k++) d[k] = own[k];
  k = 0;
  for (const SelftestIn& in : ins) {
    if (e == hipSuccess) e = hipMemcpyAsync(d[k], in.host, in.per * bytes, hipMemcpyHostToDevice, c->stream);
    k++;
  }
  if (e == hipSuccess) {
    launch(d.data(), d.back());
    e = hipMemcpyAsync(out, d.back(), out_per * bytes, hipMemcpyDeviceToHost, c->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  HIP_TRY(c, e);
  return 0;
}
// The hand-rolled sequences of spline_device.h against the compiler's IEEE operations, element-wise on the device:
// out[0][i] = sqrt_1_2(x[i]), out[1][i] = sqrt(x[i]) (x in [1, 2]); out[2][i] = div_rcp(a[i], b[i], rcp_refined(b[i])),
// out[3][i] = div_exact(a[i], b[i]) (the plain route's division: the compiler's a / b and its last-bit fix-up); out[4][i] = in_div_band(a[i]) && in_div_band(b[i]).
__global__ void math_selftest_kernel(int n, const double* __restrict__ x, const double* __restrict__ a, const double* __restrict__ b,
                                     double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = sqrt_1_2(x[i]);
  out[(size_t)n + i] = sqrt(x[i]);
  out[2 * (size_t)n + i] = div_rcp(a[i], b[i], rcp_refined(b[i]));
  out[3 * (size_t)n + i] = div_exact(a[i], b[i]);
  out[4 * (size_t)n + i] = (in_div_band(a[i]) && in_div_band(b[i])) ? 1.0 : 0.0;
}
// max_abs_nn / min_abs_nn (the one-instruction max(|a|, b) / min(|a|, b) of the Givens step) element-wise: out = [max | min]
__global__ void absminmax_selftest_kernel(int n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = max_abs_nn(a[i], b[i]);
  out[(size_t)n + i] = min_abs_nn(a[i], b[i]);
}
extern "C" int fsdp_selftest_absminmax(fsdp_ctx* c, int n, const double* a, const double* b, double* out2n) {
  if (!c || n <= 0 || !a || !b || !out2n) return 1;
  return run_selftest(c, n, {{a, 1}, {b, 1}}, 2, out2n, [&](double* const* in, double* dout) {
    hipLaunchKernelGGL(absminmax_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, in[0], in[1], dout);
  });
}

extern "C" int fsdp_selftest_math(fsdp_ctx* c, int n, const double* x, const double* a, const double* b, double* out5n) {
  if (!c || n <= 0 || !x || !a || !b || !out5n) return 1;
  return run_selftest(c, n, {{x, 1}, {a, 1}, {b, 1}}, 5, out5n, [&](double* const* in, double* dout) {
    hipLaunchKernelGGL(math_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, in[0], in[1], in[2], dout);
  });
}

// The Givens step's arithmetic (spline_device.h fpgivs_guarded<true>: max / min, the first quotient, sqrt on [1, 2], the reciprocal of dd
// seeded from the square root's own iterate, the two quotients) next to FITPACK's fpgivs with the compiler's IEEE operations:
// out = [cs | sn | dd] fast, [cs | sn | dd] IEEE, [guard: 1 = operands inside the fast sequence's band]
__global__ void givens_selftest_kernel(int n, const double* __restrict__ piv, const double* __restrict__ ww, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double w = ww[i], cs, sn;
  int bad = 0;
  fpgivs_guarded<true>(piv[i], w, cs, sn, bad);
  out[i] = cs;
  out[(size_t)n + i] = sn;
  out[2 * (size_t)n + i] = w;
  double w2 = ww[i], cs2, sn2;
  fpgivs(piv[i], w2, cs2, sn2);
  out[3 * (size_t)n + i] = cs2;
  out[4 * (size_t)n + i] = sn2;
  out[5 * (size_t)n + i] = w2;
  out[6 * (size_t)n + i] = bad ? 0.0 : 1.0;
}
extern "C" int fsdp_selftest_givens(fsdp_ctx* c, int n, const double* piv, const double* ww, double* out7n) {
  if (!c || n <= 0 || !piv || !ww || !out7n) return 1;
  return run_selftest(c, n, {{piv, 1}, {ww, 1}}, 7, out7n, [&](double* const* in, double* dout) {
    hipLaunchKernelGGL(givens_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, in[0], in[1], dout);
  });
}

// det3_lu (path_kernel.h: the sign of numpy.linalg.det of three homogeneous points) element-wise on the device
__global__ void det3_selftest_kernel(int n, const double* __restrict__ xy6, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* p = xy6 + 6 * (size_t)i;
  out[i] = det3_lu(p[0], p[1], p[2], p[3], p[4], p[5]);
}
extern "C" int fsdp_selftest_det3(fsdp_ctx* c, int n, const double* xy6, double* out) {
  if (!c || n <= 0 || !xy6 || !out) return 1;
  return run_selftest(c, n, {{xy6, 6}}, 1, out, [&](double* const* in, double* dout) {
    hipLaunchKernelGGL(det3_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, in[0], dout);
  });
}

// The device libm values the sorting stage's discrete decisions hang on (atan2 of the search predicates, start-cone bearings and
// cost terms; acos where a cosine sits within 1e-9 of a threshold) next to the correctly rounded det_atan2 (det_math.h)
__global__ void libm_selftest_kernel(int n, const double* __restrict__ y, const double* __restrict__ x, const double* __restrict__ cs,
                                     double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = atan2(y[i], x[i]);
  out[(size_t)n + i] = detm::det_atan2(y[i], x[i]);
  out[2 * (size_t)n + i] = acos(cs[i]);
}
extern "C" int fsdp_selftest_libm(fsdp_ctx* c, int n, const double* y, const double* x, const double* cs, double* out3n) {
  if (!c || n <= 0 || !y || !x || !cs || !out3n) return 1;
  return run_selftest(c, n, {{y, 1}, {x, 1}, {cs, 1}}, 3, out3n, [&](double* const* in, double* dout) {
    hipLaunchKernelGGL(libm_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, in[0], in[1], in[2], dout);
  });
}

// ---- multi-GPU: RCCL over xGMI (see fsdp_comm.h) ----------------------------------------------------------------------
#define NCCL_TRY(ctx, call)                                                                                    \
  do {                                                                                                         \
    ncclResult_t r_ = (call);                                                                                  \
    if (r_ != ncclSuccess) {                                                                                   \
      (ctx)->err = std::string(#call) + ": " + fsdp_comm::api().GetErrorString(r_);                            \
      return 3;                                                                                                \
    }                                                                                                          \
  } while (0)

int fsdp_comm_unique_id(void* out128) {
  if (!out128) return 1;
  if (!fsdp_comm::load()) {
    g_create_error = fsdp_comm::api().error;
    return 3;
  }
  static_assert(sizeof(ncclUniqueId) == FSDP_COMM_ID_BYTES, "unique id size");
  ncclUniqueId id;
  ncclResult_t r = fsdp_comm::api().GetUniqueId(&id);
  if (r != ncclSuccess) {
    g_create_error = std::string("ncclGetUniqueId: ") + fsdp_comm::api().GetErrorString(r);
    return 3;
  }
  memcpy(out128, &id, sizeof(id));
  return 0;
}

int fsdp_comm_init(fsdp_ctx* c, int rank, int world, const void* id128) {
  if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return 1;
  if (c->comm.comm) {
    c->err = "fsdp_comm_init: communicator already initialised";
    return 1;
  }
  if (!fsdp_comm::load()) {
    c->err = fsdp_comm::api().error;
    return 3;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  NCCL_TRY(c, fsdp_comm::api().CommInitRank(&c->comm.comm, world, id, rank));
  fflush(stdout);  // RCCL prints its version banner through C stdio: out now, not after the caller's own last line
  c->comm.rank = rank;
  c->comm.world = world;
  return 0;
}

int fsdp_comm_size(fsdp_ctx* c) {
  if (!c || !c->comm.comm) return 0;
  int n = 0;
  if (fsdp_comm::api().CommCount(c->comm.comm, &n) != ncclSuccess) return 0;
  return n;
}

int fsdp_comm_rank(fsdp_ctx* c) {
  if (!c || !c->comm.comm) return -1;
  int r = -1;
  if (fsdp_comm::api().CommUserRank(c->comm.comm, &r) != ncclSuccess) return -1;
  return r;
}

static int comm_staging(fsdp_ctx* c, size_t bytes) {
  HIP_TRY(c, c->comm.d_buf.reserve(bytes));
  return 0;
}

int fsdp_comm_broadcast(fsdp_ctx* c, void* host_buf, size_t bytes, int root) {
  if (!c || !c->comm.comm || (bytes > 0 && !host_buf) || root < 0 || root >= c->comm.world) return 1;
  if (bytes == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = comm_staging(c, bytes);
  if (rc) return rc;
  if (c->comm.rank == root) HIP_TRY(c, hipMemcpyAsync(c->comm.d_buf, host_buf, bytes, hipMemcpyHostToDevice, c->stream));
  NCCL_TRY(c, fsdp_comm::api().Broadcast(c->comm.d_buf.get(), c->comm.d_buf.get(), bytes, ncclUint8, root, c->comm.comm, c->stream));
  if (c->comm.rank != root) HIP_TRY(c, hipMemcpyAsync(host_buf, c->comm.d_buf, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

int fsdp_comm_allreduce(fsdp_ctx* c, double* values, int n, int op) {
  if (!c || !c->comm.comm || n < 0 || (n > 0 && !values) || op < 0 || op > 2) return 1;
  if (n == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t bytes = sizeof(double) * (size_t)n;
  int rc = comm_staging(c, bytes);
  if (rc) return rc;
  const ncclRedOp_t ops[3] = {ncclSum, ncclMax, ncclMin};
  HIP_TRY(c, hipMemcpyAsync(c->comm.d_buf, values, bytes, hipMemcpyHostToDevice, c->stream));
  NCCL_TRY(c, fsdp_comm::api().AllReduce(c->comm.d_buf.get(), c->comm.d_buf.get(), (size_t)n, ncclFloat64, ops[op], c->comm.comm, c->stream));
  HIP_TRY(c, hipMemcpyAsync(values, c->comm.d_buf, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

int fsdp_comm_barrier(fsdp_ctx* c) {
  if (!c || !c->comm.comm) return 1;
  int rc = sync_all(c);  // everything this rank has enqueued is done before it reports in
  if (rc) return rc;
  double one = 1.0;
  rc = fsdp_comm_allreduce(c, &one, 1, 0);
  if (rc) return rc;
  if ((int)one != c->comm.world) {
    c->err = "fsdp_comm_barrier: rank count mismatch";
    return 3;
  }
  return 0;
}

int fsdp_comm_destroy(fsdp_ctx* c) {
  if (!c) return 1;
  if (c->comm.comm) {
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)fsdp_comm::api().CommDestroy(c->comm.comm);
    c->comm.comm = nullptr;
  }
  c->comm.d_buf.reset();
  c->comm.rank = 0;
  c->comm.world = 1;
  return 0;
}

int fsdp_default_path(fsdp_ctx* c, double* out) {
  if (!c || !out) return 1;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, copy_sync(c, out, c->d_default_path, sizeof(double) * PATH_POINTS * 4, hipMemcpyDeviceToHost));
  return 0;
}
}
