// Host-only: the owning buffer types of the host library and the buffer stores of a context.  No kernels.
//
// Ownership rule: every device or page-locked block belongs to exactly one DeviceBuf / PinnedBuf, which knows its capacity and
// frees it.  A reserve() that fails leaves the buffer EMPTY (capacity 0), and a store whose reserve() fails is empty as a whole:
// "does it fit" is always answered by the buffers themselves, so the next call grows them again or fails again — it never
// launches on a pointer that a failed growth left behind.  A: the allocator (two static functions); the CPU test of this header
// (tests/emu/host_buffers_probe.cpp) supplies a counting one and needs no HIP runtime.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

#include "../../include/fsdp.h"
#include "sort_kernel.h"
#include "match_kernel.h"
#include "path_kernel.h"
#include "skidpad_kernel.h"
#include "sequence_launch.h"

namespace fsdp {

// page-locked memory: Default where only copy commands touch it, Mapped where a kernel does, MappedCoherent where the host polls it
enum class Pin { Default, Mapped, MappedCoherent };

#ifdef FSDP_EMU
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
struct HipDevice;
struct HipPinned;
#else
// (a failed allocation is the caller's error code, not the runtime's "last error" for some later, unrelated check to find)
inline hipError_t alloc_result(hipError_t e) {
  if (e != hipSuccess) (void)hipGetLastError();
  return e;
}
struct HipDevice {
  static hipError_t allocate(void** p, size_t bytes) { return alloc_result(hipMalloc(p, bytes)); }
  static void free(void* p) { (void)hipFree(p); }
};
struct HipPinned {  // *dev: the block as the GPU addresses it (mapped blocks)
  static hipError_t allocate(void** p, void** dev, size_t bytes, Pin pin) {
    const unsigned flags = pin == Pin::Default ? hipHostMallocDefault : pin == Pin::Mapped ? hipHostMallocMapped : hipHostMallocMapped | hipHostMallocCoherent;
    const hipError_t e = alloc_result(hipHostMalloc(p, bytes, flags));
    return e != hipSuccess || pin == Pin::Default ? e : hipHostGetDevicePointer(dev, *p, 0);
  }
  static void free(void* p) { (void)hipHostFree(p); }
};
#endif

// what the two buffer types share: a move-only owner of `capacity()` T's that frees with A::free
template <class T, class A>
class OwnedBuf {
 public:
  OwnedBuf() = default;
  OwnedBuf(OwnedBuf&& o) noexcept : p_(o.p_), dev_(o.dev_), cap_(o.cap_) { o.p_ = o.dev_ = nullptr, o.cap_ = 0; }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(p_, o.p_), std::swap(dev_, o.dev_), std::swap(cap_, o.cap_);
    }
    return *this;
  }
  ~OwnedBuf() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }  // (a buffer is handed to launches and copies as the pointer it owns)
  size_t capacity() const { return cap_; }
  void reset() {
    if (p_) A::free(p_);
    p_ = dev_ = nullptr;
    cap_ = 0;
  }

 protected:
  // count <= capacity(): nothing at all.  Else the block is freed and one of max(count, want, 1) T's allocated (what it held is
  // gone: nothing queued may use it any more; freeing first keeps the peak at one block).  Failure: empty, and the error.
  template <class Alloc>
  hipError_t grow(size_t count, size_t want, Alloc alloc) {
    if (count <= cap_) return hipSuccess;
    reset();
    want = std::max({count, want, (size_t)1});
    const hipError_t e = alloc((void**)&p_, (void**)&dev_, sizeof(T) * want);
    cap_ = e == hipSuccess ? want : 0;
    if (e != hipSuccess) p_ = dev_ = nullptr;
    return e;
  }
  T* p_ = nullptr;
  T* dev_ = nullptr;
  size_t cap_ = 0;
};

template <class T, class A = HipDevice>
struct DeviceBuf : OwnedBuf<T, A> {
  hipError_t reserve(size_t count, size_t want = 0) { return this->grow(count, want, [](void** p, void**, size_t bytes) { return A::allocate(p, bytes); }); }
};
template <class T, class A = HipPinned>
struct PinnedBuf : OwnedBuf<T, A> {
  hipError_t reserve(size_t count, size_t want = 0, Pin pin = Pin::Default) {
    return this->grow(count, want, [pin](void** p, void** dev, size_t bytes) { return A::allocate(p, dev, bytes, pin); });
  }
  T* device() const { return this->dev_; }  // the mapped address (NULL for a Pin::Default block)
};

// ---- the stores: what a pass slot and a context own.  Each reserves its buffers in turn (`e`: the first error so far), and a
// store that could not grow is empty as a whole ----------------------------------------------------------------------------
#define FSDP_STORE_TRY(e, call) \
  if ((e) == hipSuccess) (e) = (call)
template <class S>
hipError_t store_result(S& s, hipError_t e) {
  if (e != hipSuccess) s = S();
  return e;
}

// one batch of frames as the kernels see it: a view (copied by value), owned by an InputStore or a FilterStore
struct Inputs {
  int32_t* d_off = nullptr;
  double* d_cones = nullptr;
  double* d_poses = nullptr;
  double* d_prev = nullptr;  // (n_frames,40,4)
  int n_frames = 0, max_cones = 0;  // max_cones: most cones in a frame (picks the sorting kernel's state size)
  bool use_prev = false;            // d_prev holds this batch's previous paths
};

// the device copy of one batch (CSR offsets, flattened cones, poses, optional previous paths) and what it currently holds
template <class A = HipDevice>
struct InputStore {
  DeviceBuf<int32_t, A> d_off;
  DeviceBuf<double, A> d_cones, d_poses, d_prev;  // (d_prev: allocated on first use)
  int n_frames = 0, max_cones = 0;
  bool use_prev = false;
  std::vector<int32_t> off_rebased;  // offsets - cone_offsets[0] for the copy paths (kept until the slot's next batch)
  size_t frames() const { return d_poses.capacity() / 4; }
  size_t cone_rows() const { return d_cones.capacity() / 3; }
  bool fits(size_t n, size_t rows, bool with_prev) const { return n <= frames() && rows <= cone_rows() && d_cones && (!with_prev || PATH_POINTS * 4 * n <= d_prev.capacity()); }
  // (buffers only grow; the caller has made sure nothing in flight reads them.  Cones with headroom: a replay's cone count
  // creeps up from step to step, and freeing device memory synchronises the whole device)
  hipError_t reserve(size_t n, size_t rows, bool with_prev) {
    hipError_t e = d_off.reserve(n + 1);
    FSDP_STORE_TRY(e, d_poses.reserve(4 * n));
    FSDP_STORE_TRY(e, d_cones.reserve(std::max<size_t>(3 * rows, 1), 3 * (rows + rows / 2 + 64)));
    if (with_prev) FSDP_STORE_TRY(e, d_prev.reserve((size_t)PATH_POINTS * 4 * n));
    return store_result(*this, e);
  }
  Inputs view() const { return Inputs{d_off, d_cones, d_poses, d_prev, n_frames, max_cones, use_prev}; }
};

// the intermediates and the result block of a pass slot
template <class A = HipDevice>
struct PassStore {
  DeviceBuf<SortOut, A> d_sort;
  DeviceBuf<MatchOut, A> d_match;
  DeviceBuf<PathOut, A> d_path;
  DeviceBuf<double, A> d_arena;  // per-frame working polyline + basis cache (ARENA_DOUBLES doubles), HBM/L2 scratch
  DeviceBuf<int, A> d_big;       // [0] counter + frames beyond sort_kernel's LDS capacities (n + 1 ints)
  DeviceBuf<int, A> d_retry;     // [0] counter + frames for the exact re-plan kernel (n + 1 ints)
  DeviceBuf<PathMid, A> d_mid;   // hand-over records of the three-kernel path stage
  DeviceBuf<fsdp_frame_result, A> d_result;  // the pass's results in the ABI's layout (assemble_kernel)
  DeviceBuf<SkidInfo, A> d_skid_info;        // skidpad contexts
  DeviceBuf<int32_t, A> d_skid_status;       // skid_reloc_kernel's status of the step this slot holds
  size_t frames() const { return d_result.capacity(); }  // (any of them: a store is grown as a whole or empty)
  hipError_t reserve(size_t n, bool skid) {
    hipError_t e = d_sort.reserve(n);
    FSDP_STORE_TRY(e, d_match.reserve(n));
    FSDP_STORE_TRY(e, d_path.reserve(n));
    FSDP_STORE_TRY(e, d_arena.reserve((size_t)ARENA_DOUBLES * n));
    FSDP_STORE_TRY(e, d_big.reserve(n + 1));
    FSDP_STORE_TRY(e, d_retry.reserve(n + 1));
    FSDP_STORE_TRY(e, d_mid.reserve(n));
    FSDP_STORE_TRY(e, d_result.reserve(n));
    if (skid) FSDP_STORE_TRY(e, d_skid_info.reserve(n));
    if (skid) FSDP_STORE_TRY(e, d_skid_status.reserve(n));
    return store_result(*this, e);
  }
};

// use_unknown_cones = False (filter_kernel.h): the batch without its UNKNOWN cones, and the way back for the indices
template <class A = HipDevice>
struct FilterStore {
  DeviceBuf<int32_t, A> f_cnt, f_off, f_map;
  DeviceBuf<double, A> f_cones;
  bool fits(size_t n, size_t rows) const { return n + 1 <= f_off.capacity() && rows <= f_map.capacity() && f_map; }
  hipError_t reserve(size_t n, size_t rows) {
    hipError_t e = f_cnt.reserve(n);
    FSDP_STORE_TRY(e, f_off.reserve(n + 1));
    FSDP_STORE_TRY(e, f_cones.reserve(3 * rows));
    FSDP_STORE_TRY(e, f_map.reserve(rows));
    return store_result(*this, e);
  }
};

// fsdp_plan_sequence (sequence_kernel.h): the run-head list of a sequence pass, the planners' initial and final previous paths
template <class A = HipDevice>
struct SeqStore {
  DeviceBuf<int, A> d_seq;  // [0] heads, [1] frames planned again, then (frame, predecessor) per head
  DeviceBuf<double, A> d_seq_init, d_seq_final;  // (planners, 40, 4)
  static constexpr size_t PREV_DOUBLES = (size_t)PATH_POINTS * 4;  // one planner's row of initial_prev / final_prev
  bool fits(size_t n, size_t planners) const { return (size_t)SEQ_LIST + 2 * n <= d_seq.capacity() && PREV_DOUBLES * planners <= d_seq_final.capacity(); }
  hipError_t reserve(size_t n, size_t planners) {
    hipError_t e = d_seq.reserve((size_t)SEQ_LIST + 2 * n);
    FSDP_STORE_TRY(e, d_seq_init.reserve(PREV_DOUBLES * planners));
    FSDP_STORE_TRY(e, d_seq_final.reserve(PREV_DOUBLES * planners));
    return store_result(*this, e);
  }
};

// fsdp_plan_sequence_cached (sequence_cache_kernel.h): the speculative sort's per-frame records, hit codes, irregular frames per planner
template <class A = HipDevice>
struct SeqCacheStore {
  DeviceBuf<SeqSpecRec, A> d_seqc_rec;
  DeviceBuf<int8_t, A> d_seqc_hits;
  DeviceBuf<int32_t, A> d_seqc_resorted;
  hipError_t reserve(size_t n, size_t planners) {
    hipError_t e = d_seqc_rec.reserve(n);
    FSDP_STORE_TRY(e, d_seqc_hits.reserve(2 * n));
    FSDP_STORE_TRY(e, d_seqc_resorted.reserve(planners));
    return store_result(*this, e);
  }
};

// workspace of a skidpad group that goes through the packed kernels, frame = step * n_instances + instance
template <class A = HipDevice>
struct SkidGroupStore {
  DeviceBuf<double, A> d_g_arena;
  DeviceBuf<PathMid, A> d_g_mid;
  DeviceBuf<PathOut, A> d_g_out;
  DeviceBuf<int, A> d_g_retry;
  DeviceBuf<SkidSel, A> d_g_sel;
  size_t frames() const { return d_g_sel.capacity(); }
  // (room for the groups the context forms, `group` steps of n planners: 16 384 frames with 1024 planners ~ 1.4 GB, most of it fit workspace)
  hipError_t reserve(size_t n_frames, size_t n, size_t group) {
    if (n_frames <= frames()) return hipSuccess;
    const size_t m = std::max(n_frames, n * group);
    hipError_t e = d_g_arena.reserve((size_t)ARENA_DOUBLES * m);
    FSDP_STORE_TRY(e, d_g_mid.reserve(m));
    FSDP_STORE_TRY(e, d_g_out.reserve(m));
    FSDP_STORE_TRY(e, d_g_retry.reserve(m + 1));
    FSDP_STORE_TRY(e, d_g_sel.reserve(m));
    return store_result(*this, e);
  }
};

// the sorting cache (fsdp_sort_cache_reset, sort_cache.h): one entry per planner in each of two buffers, and their host-side layout
template <class A = HipDevice>
struct SortCacheStore {
  DeviceBuf<SortCacheHdr, A> d_hdr[2];
  DeviceBuf<double, A> d_xyt[2];
  DeviceBuf<int32_t, A> d_off[2];
  DeviceBuf<int8_t, A> d_hits;
  std::vector<int32_t> layout[2];  // host copies of the two buffers' region offsets
  std::vector<int32_t> region;     // rows of a planner's region: the most cones it was ever given
  size_t rows(int b) const { return d_xyt[b].capacity() / 3; }  // rows buffer b's cone store holds
  // a fresh cache for n planners: no entries, one row each
  hipError_t reserve(size_t n) {
    hipError_t e = hipSuccess;
    for (int b = 0; b < 2; b++) {
      FSDP_STORE_TRY(e, d_hdr[b].reserve(n));
      FSDP_STORE_TRY(e, d_off[b].reserve(n + 1));
      FSDP_STORE_TRY(e, d_xyt[b].reserve(3));
      layout[b].assign(n + 1, 0);
    }
    FSDP_STORE_TRY(e, d_hits.reserve(2 * n));
    region.assign(n, 0);
    return store_result(*this, e);
  }
  // room for `need` cone rows in buffer b (with headroom, like a batch's cones); failure leaves that cone store empty
  hipError_t reserve_rows(int b, size_t need) { return need <= rows(b) ? hipSuccess : d_xyt[b].reserve(3 * need, 3 * (need + need / 2 + 64)); }
};

}  // namespace fsdp
