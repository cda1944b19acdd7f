// TEST INFRASTRUCTURE — the host library's growth code (csrc/host_buffers.h: DeviceBuf, PinnedBuf and the stores) on a counting
// allocator that fails the k-th allocation.  A program of its own (tests/test_host_buffers_cpu.py builds and runs it): for every
// store a script of growing, shrinking and growing requests, once without a failure and once for every allocation the script
// makes failing.  Exit status 1 and one line on the first violated assertion.
#include "hip_emu.h"

#include "../../ft-fsd-path-planning_amd/csrc/host_buffers.h"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <set>
#include <string>
#include <vector>

using namespace fsdp;

// ---- the allocator ----------------------------------------------------------------------------------------------------------
static long g_allocs = 0;      // allocate calls so far (failed ones included)
static long g_fail_at = -1;    // the call with this number fails
static long g_frees = 0;
static std::set<void*> g_live;
static std::string g_where;

[[noreturn]] static void fail(const std::string& what) {
  printf("FAILED [%s]: %s\n", g_where.c_str(), what.c_str());
  exit(1);
}
#define CHECK(cond, what) \
  do {                    \
    if (!(cond)) fail(what); \
  } while (0)

struct Counting {
  static hipError_t get(void** p, size_t bytes) {
    if (g_allocs++ == g_fail_at) return hipErrorOutOfMemory;  // (*p untouched, as a failed hipMalloc leaves it)
    CHECK(bytes > 0, "allocation of 0 bytes");
    *p = malloc(bytes);
    g_live.insert(*p);
    return hipSuccess;
  }
  static hipError_t allocate(void** p, size_t bytes) { return get(p, bytes); }
  static hipError_t allocate(void** p, void** dev, size_t bytes, Pin pin) {
    const hipError_t e = get(p, bytes);
    if (e == hipSuccess && pin != Pin::Default) *dev = *p;
    return e;
  }
  static void free(void* p) {
    CHECK(g_live.erase(p) == 1, "a block freed twice (or never allocated)");
    g_frees++;
    ::free(p);
  }
};

// ---- what a script says about one buffer after every request --------------------------------------------------------------
struct Slot {
  const char* name;
  std::function<const void*()> ptr;
  std::function<size_t()> cap;
  size_t need = 0;  // elements the last SUCCESSFUL request asked of it (0: none yet, or dropped by a failure)
};
struct Probe {
  std::vector<Slot> slots;
  template <class B>
  void watch(const char* name, const B& b) {
    slots.push_back(Slot{name, [&b]() { return (const void*)b.get(); }, [&b]() { return b.capacity(); }, 0});
  }
  Slot& operator[](const char* name) {
    for (Slot& s : slots)
      if (std::string(s.name) == name) return s;
    fail(std::string("no buffer ") + name);
  }
  // (a) every buffer is empty with capacity 0, or holds at least what was last successfully reserved for it
  void consistent(bool after_failure) {
    for (Slot& s : slots) {
      const bool empty = s.ptr() == nullptr;
      CHECK(!empty || s.cap() == 0, std::string(s.name) + ": null with capacity " + std::to_string(s.cap()));
      CHECK(empty || s.cap() > 0, std::string(s.name) + ": a block of capacity 0");
      CHECK(empty || s.cap() >= s.need, std::string(s.name) + ": capacity " + std::to_string(s.cap()) + " below the " + std::to_string(s.need) + " reserved");
      CHECK(!empty || after_failure || s.need == 0, std::string(s.name) + ": (b) null after a successful reserve");
      if (empty) s.need = 0;
    }
  }
};

// One request: what() is the store's reserve, needs = the element counts it must leave room for (name, count; exact = the
// capacity a fresh block gets, 0 = not checked).  Asserts (a), (b), (c), (d).
struct Need {
  const char* name;
  size_t count;
  size_t exact;
};
static void request(Probe& p, const std::string& label, const std::function<hipError_t()>& what, std::vector<Need> needs) {
  g_where = label;
  std::vector<size_t> before;
  for (const Need& n : needs) before.push_back(p[n.name].cap());
  bool fits = true;
  for (size_t i = 0; i < needs.size(); i++) fits = fits && needs[i].count <= before[i] && (needs[i].count == 0 || p[needs[i].name].ptr());
  const long calls = g_allocs;
  const hipError_t e = what();
  if (fits) CHECK(g_allocs == calls && e == hipSuccess, "(c) a reserve within capacity called the allocator");
  if (e == hipSuccess) {
    for (size_t i = 0; i < needs.size(); i++) {
      Slot& s = p[needs[i].name];
      s.need = std::max(s.need, needs[i].count);
      // (d) a block that was replaced holds exactly the headroom rule's count
      if (needs[i].exact && s.cap() != before[i])
        CHECK(s.cap() == needs[i].exact, std::string("(d) ") + s.name + ": " + std::to_string(s.cap()) + " elements, the rule says " + std::to_string(needs[i].exact));
    }
  } else {
    CHECK(g_fail_at >= 0 && g_allocs > g_fail_at, "an error without a failed allocation");
  }
  p.consistent(e != hipSuccess);
}

// a script, run for every failing allocation: run(k) builds the store, plays the requests and destroys it
static void sweep(const char* name, const std::function<void()>& script) {
  g_fail_at = -1;
  g_allocs = g_frees = 0;
  g_where = name;
  script();
  const long total = g_allocs;
  CHECK(total > 0, "the script allocated nothing");
  for (long k = 0; k <= total; k++) {
    g_fail_at = k;
    g_allocs = g_frees = 0;
    g_where = std::string(name) + " k=" + std::to_string(k);
    script();
    // (e) nothing is left after destruction (a double free is caught where it happens)
    CHECK(g_live.empty(), "(e) " + std::to_string(g_live.size()) + " block(s) alive after destruction");
  }
  printf("ok %-16s %ld allocations, every one failed once\n", name, total);
}

static std::string at(const char* store, size_t a, size_t b = 0) { return std::string(store) + " " + std::to_string(a) + "/" + std::to_string(b) + (g_fail_at >= 0 ? " k=" + std::to_string(g_fail_at) : ""); }
static size_t cones_rule(size_t n) { return n + n / 2 + 64; }

int main() {
  constexpr size_t PREV = (size_t)PATH_POINTS * 4;
  // ---- the two buffer types themselves ----------------------------------------------------------------------------------
  sweep("buffers", [] {
    DeviceBuf<double, Counting> d;
    PinnedBuf<int32_t, Counting> h;
    Probe p;
    p.watch("d", d);
    p.watch("h", h);
    const size_t counts[] = {3, 40, 5, 70};
    for (size_t n : counts) {
      request(p, at("DeviceBuf", n), [&] { return d.reserve(n); }, {{"d", n, n}});
      request(p, at("PinnedBuf want 64", n), [&] { return h.reserve(n, 64, Pin::Mapped); }, {{"h", n, std::max<size_t>(n, 64)}});
      CHECK(!h.get() || h.device() == h.get(), "a mapped block without its device address");
    }
    request(p, at("PinnedBuf want 16384", 100), [&] { return h.reserve(100, 16384, Pin::Default); }, {{"h", 100, 16384}});
    // (e) a moved-from buffer is empty; the block has one owner
    const double* was = d.get();
    const size_t cap = d.capacity();
    DeviceBuf<double, Counting> e(std::move(d));
    CHECK(d.get() == nullptr && d.capacity() == 0, "(e) a moved-from buffer is not empty");
    CHECK(e.get() == was && e.capacity() == cap, "a move lost the block");
    d = std::move(e);
    CHECK(e.get() == nullptr && e.capacity() == 0 && d.get() == was, "(e) move assignment");
    d.reset();
    CHECK(d.get() == nullptr && d.capacity() == 0, "reset leaves a block");
    p.slots.clear();
  });

  // ---- the stores ---------------------------------------------------------------------------------------------------------
  sweep("InputStore", [&] {
    InputStore<Counting> s;
    Probe p;
    p.watch("d_off", s.d_off), p.watch("d_cones", s.d_cones), p.watch("d_poses", s.d_poses), p.watch("d_prev", s.d_prev);
    struct { size_t n, rows; bool prev; } reqs[] = {{3, 30, false}, {40, 500, true}, {5, 0, false}, {70, 400, true}, {70, 1200, false}, {2, 10, true}};
    for (auto r : reqs) {
      const bool fitted = s.fits(r.n, r.rows, r.prev);
      const long calls = g_allocs;
      request(p, at("InputStore", r.n, r.rows), [&] { return s.reserve(r.n, r.rows, r.prev); },
              {{"d_off", r.n + 1, r.n + 1}, {"d_poses", 4 * r.n, 4 * r.n}, {"d_cones", std::max<size_t>(3 * r.rows, 1), 3 * cones_rule(r.rows)}, {"d_prev", r.prev ? PREV * r.n : 0, PREV * r.n}});
      if (fitted) CHECK(g_allocs == calls, "fits() said yes and reserve allocated");
      CHECK(!s.fits(r.n, r.rows, r.prev) || (s.d_off && s.d_cones && s.d_poses && (!r.prev || s.d_prev)), "fits() with an empty buffer");
      const Inputs v = s.view();
      CHECK(v.d_off == s.d_off.get() && v.d_cones == s.d_cones.get() && v.d_poses == s.d_poses.get() && v.d_prev == s.d_prev.get(), "view() is not the store's buffers");
    }
  });
  sweep("PassStore", [&] {
    for (int skid = 0; skid < 2; skid++) {
      PassStore<Counting> s;
      Probe p;
      p.watch("d_sort", s.d_sort), p.watch("d_match", s.d_match), p.watch("d_path", s.d_path), p.watch("d_arena", s.d_arena), p.watch("d_big", s.d_big);
      p.watch("d_retry", s.d_retry), p.watch("d_mid", s.d_mid), p.watch("d_result", s.d_result), p.watch("d_skid_info", s.d_skid_info), p.watch("d_skid_status", s.d_skid_status);
      const size_t counts[] = {3, 40, 5, 70, 2, 70};  // (2: the small pass right after a growth that may have failed)
      for (size_t n : counts) {
        const size_t sk = skid ? n : 0;
        request(p, at(skid ? "PassStore skid" : "PassStore", n), [&] { return s.reserve(n, skid != 0); },
                {{"d_sort", n, n}, {"d_match", n, n}, {"d_path", n, n}, {"d_arena", (size_t)ARENA_DOUBLES * n, (size_t)ARENA_DOUBLES * n}, {"d_big", n + 1, n + 1},
                 {"d_retry", n + 1, n + 1}, {"d_mid", n, n}, {"d_result", n, n}, {"d_skid_info", sk, sk}, {"d_skid_status", sk, sk}});
        // the slot's one test in front of a pass: it may say "fits" only when every buffer does
        if (n <= s.frames())
          for (Slot& b : p.slots)
            CHECK((b.ptr() && b.cap() >= n) || (!skid && std::string(b.name).find("skid") != std::string::npos), std::string("frames() says the slot holds the pass, ") + b.name + " does not");
      }
    }
  });
  sweep("FilterStore", [&] {
    FilterStore<Counting> s;
    Probe p;
    p.watch("f_cnt", s.f_cnt), p.watch("f_off", s.f_off), p.watch("f_cones", s.f_cones), p.watch("f_map", s.f_map);
    struct { size_t n, rows; } reqs[] = {{3, cones_rule(30)}, {40, cones_rule(500)}, {5, cones_rule(30)}, {70, cones_rule(500)}, {70, cones_rule(1200)}, {2, cones_rule(10)}};
    for (auto r : reqs) {
      const bool fitted = s.fits(r.n, r.rows);
      const long calls = g_allocs;
      request(p, at("FilterStore", r.n, r.rows), [&] { return s.reserve(r.n, r.rows); }, {{"f_cnt", r.n, r.n}, {"f_off", r.n + 1, r.n + 1}, {"f_cones", 3 * r.rows, 3 * r.rows}, {"f_map", r.rows, r.rows}});
      if (fitted) CHECK(g_allocs == calls, "fits() said yes and reserve allocated");
      CHECK(!s.fits(r.n, r.rows) || (s.f_cnt && s.f_off && s.f_cones && s.f_map), "fits() with an empty buffer");
    }
  });
  sweep("SeqStore", [&] {
    SeqStore<Counting> s;
    Probe p;
    p.watch("d_seq", s.d_seq), p.watch("d_seq_init", s.d_seq_init), p.watch("d_seq_final", s.d_seq_final);
    struct { size_t planners, steps; } reqs[] = {{2, 3}, {5, 4}, {1, 2}, {3, 20}, {9, 2}, {2, 2}};
    for (auto r : reqs) {
      const size_t n = r.planners * r.steps;
      request(p, at("SeqStore", r.planners, r.steps), [&] { return s.reserve(n, r.planners); },
              {{"d_seq", (size_t)SEQ_LIST + 2 * n, (size_t)SEQ_LIST + 2 * n}, {"d_seq_init", PREV * r.planners, PREV * r.planners}, {"d_seq_final", PREV * r.planners, PREV * r.planners}});
      CHECK(!s.fits(n, r.planners) || (s.d_seq && s.d_seq_init && s.d_seq_final), "fits() with an empty buffer");
    }
  });
  sweep("SeqCacheStore", [&] {
    SeqCacheStore<Counting> s;
    Probe p;
    p.watch("d_seqc_rec", s.d_seqc_rec), p.watch("d_seqc_hits", s.d_seqc_hits), p.watch("d_seqc_resorted", s.d_seqc_resorted);
    struct { size_t planners, steps; } reqs[] = {{2, 3}, {5, 4}, {1, 2}, {3, 20}, {9, 2}, {2, 2}};
    for (auto r : reqs) {
      const size_t n = r.planners * r.steps;
      request(p, at("SeqCacheStore", r.planners, r.steps), [&] { return s.reserve(n, r.planners); }, {{"d_seqc_rec", n, n}, {"d_seqc_hits", 2 * n, 2 * n}, {"d_seqc_resorted", r.planners, r.planners}});
    }
  });
  sweep("SkidGroupStore", [&] {
    SkidGroupStore<Counting> s;
    Probe p;
    p.watch("d_g_arena", s.d_g_arena), p.watch("d_g_mid", s.d_g_mid), p.watch("d_g_out", s.d_g_out), p.watch("d_g_retry", s.d_g_retry), p.watch("d_g_sel", s.d_g_sel);
    struct { size_t frames, n, group; } reqs[] = {{4, 2, 2}, {10, 5, 4}, {3, 3, 1}, {30, 5, 4}, {64, 8, 16}, {6, 3, 2}};
    for (auto r : reqs) {
      const size_t m = std::max(r.frames, r.n * r.group);  // the skid group: max(frames, n * skid_group_size)
      request(p, at("SkidGroupStore", r.frames, r.n * r.group), [&] { return s.reserve(r.frames, r.n, r.group); },
              {{"d_g_arena", (size_t)ARENA_DOUBLES * r.frames, (size_t)ARENA_DOUBLES * m}, {"d_g_mid", r.frames, m}, {"d_g_out", r.frames, m}, {"d_g_retry", r.frames + 1, m + 1}, {"d_g_sel", r.frames, m}});
      if (r.frames <= s.frames())
        for (Slot& b : p.slots) CHECK(b.ptr(), std::string("frames() says the group fits, ") + b.name + " is empty");
    }
  });
  sweep("SortCacheStore", [&] {
    const size_t planners[] = {2, 5, 3};
    for (size_t n : planners) {  // fsdp_sort_cache_reset: a fresh store each time
      SortCacheStore<Counting> s;
      Probe p;
      p.watch("d_hdr0", s.d_hdr[0]), p.watch("d_hdr1", s.d_hdr[1]), p.watch("d_off0", s.d_off[0]), p.watch("d_off1", s.d_off[1]);
      p.watch("d_xyt0", s.d_xyt[0]), p.watch("d_xyt1", s.d_xyt[1]), p.watch("d_hits", s.d_hits);
      request(p, at("SortCacheStore", n), [&] { return s.reserve(n); },
              {{"d_hdr0", n, n}, {"d_hdr1", n, n}, {"d_off0", n + 1, n + 1}, {"d_off1", n + 1, n + 1}, {"d_xyt0", 3, 3}, {"d_xyt1", 3, 3}, {"d_hits", 2 * n, 2 * n}});
      if (!s.d_hits) continue;  // (the reset failed: the cache stays off)
      CHECK(s.rows(0) == 1 && s.rows(1) == 1 && s.layout[0].size() == n + 1 && s.region.size() == n, "a fresh cache's layout");
      const size_t rows[] = {1, 30, 7, 200, 200, 301};
      int b = 0;
      for (size_t need : rows) {
        const char* name = b ? "d_xyt1" : "d_xyt0";
        request(p, at("SortCacheStore rows", need, (size_t)b), [&] { return s.reserve_rows(b, need); }, {{name, 3 * need, 3 * cones_rule(need)}});
        CHECK(s.rows(b) * 3 == s.d_xyt[b].capacity(), "rows() against the cone store");
        b = 1 - b;
      }
    }
  });
  printf("host_buffers_probe: all scripts passed\n");
  return 0;
}
