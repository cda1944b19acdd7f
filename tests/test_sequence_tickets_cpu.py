"""CPU-side checks of the sequence tickets (fsdp_submit_sequence): the ABI's declarations against both built libraries and the
binding, the planner cut of MultiPlanner, and the slice index arithmetic of csrc/sequence_slice.h — the one helper the host library,
the staging kernels and this test share — against a NumPy restatement, through a small stand-alone host program."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("fsdp_submit_sequence", "fsdp_submit_sequence_compact")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge

    ge.build_hip()
    return importlib.import_module("ft-fsd-path-planning_amd")


def test_new_symbols_are_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "fsdp.h").read_text()
    declared = set(re.findall(r"\b(fsdp_[a-z0-9_]+)\s*\(", header))
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in pkg._capi.EXPORTED_SYMBOLS, sym
    for shapes in (pkg._capi.STANDARD, pkg._capi.WIDE):
        raw = ctypes.CDLL(str(shapes.lib_path))
        bound = pkg._capi.load(shapes)
        for sym in NEW_SYMBOLS:
            assert hasattr(raw, sym), (shapes.name, sym)
            # (ctx, n_planners, n_steps, planner_lo, planners_total, offsets, cones, poses, initial_prev, results, final_prev, n_replanned, ticket)
            assert len(getattr(bound, sym).argtypes) == 13, (shapes.name, sym)
    # the two calls take the arguments of fsdp_plan_sequence + the slice + the ticket
    proto = re.search(r"int fsdp_submit_sequence\((.*?)\);", header, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")]
    assert names == ["ctx", "n_planners", "n_steps", "planner_lo", "planners_total", "cone_offsets", "cones_xyt", "poses", "initial_prev", "results",
                     "final_prev", "n_replanned", "ticket"]
    assert callable(pkg.Context.submit_sequence) and callable(pkg.MultiPlanner.submit_sequence) and callable(pkg.MultiPlanner.plan_sequence)


def test_planner_slices_cover_disjoint_ordered_balanced(pkg):
    planner_slices = pkg.multi.planner_slices
    for n in list(range(0, 70)) + [127, 128, 130, 4096, 100003]:
        for parts in list(range(1, 20)) + [32, 33, 257]:
            cut = planner_slices(n, parts)
            assert len(cut) == parts
            assert cut[0][0] == 0 and cut[-1][1] == n
            assert all(lo <= hi for lo, hi in cut)
            assert all(cut[g][1] == cut[g + 1][0] for g in range(parts - 1))  # ordered, disjoint, no gap
            sizes = [hi - lo for lo, hi in cut]
            assert sum(sizes) == n and max(sizes) - min(sizes) <= 1
    assert planner_slices(130, 4) == [(0, 32), (32, 65), (65, 97), (97, 130)]
    with pytest.raises(ValueError):
        planner_slices(3, 0)


PROGRAM = r"""
// reads: n n_steps lo total, then n_steps * total + 1 offsets; prints what csrc/sequence_slice.h makes of them
#include <cstdio>
#include <vector>
#include "sequence_slice.h"
int main() {
  fsdp::SeqSlice s;
  if (scanf("%d %d %d %d", &s.n, &s.n_steps, &s.lo, &s.total) != 4) return 2;
  printf("valid %d\n", fsdp::seq_slice_valid(s) ? 1 : 0);
  if (!fsdp::seq_slice_valid(s)) return 0;
  const long long rec_frames = (long long)s.n_steps * s.total;
  std::vector<int32_t> off((size_t)rec_frames + 1);
  for (auto& o : off)
    if (scanf("%d", &o) != 1) return 2;
  printf("whole %d frames %lld\n", s.whole() ? 1 : 0, s.frames());
  for (long long f = 0; f < s.frames(); f++) printf("rec %lld\n", fsdp::seq_rec_of_call(s, f));
  for (long long r = -1; r <= rec_frames; r++) printf("call %lld\n", fsdp::seq_call_of_rec(s, r));
  std::vector<fsdp::SeqSeg> seg((size_t)s.n_steps + 1);
  int most = -1;
  const int rc = fsdp::seq_slice_segments(s, off.data(), seg.data(), &most);
  printf("segments %d\n", rc);
  if (rc != 0) return 0;
  printf("most %d\n", most);
  for (const fsdp::SeqSeg& g : seg) printf("seg %d %d\n", g.src, g.dst);
  for (long long f = 0; f < s.frames(); f++)
    printf("dense %lld\n", fsdp::seq_dense_offset(seg[(size_t)(f / s.n)], off[(size_t)fsdp::seq_rec_of_call(s, f)]));
  return 0;
}
"""


def restated(n, steps, lo, total, off):
    """what the program prints, from NumPy"""
    lines = [f"valid {int(n >= 1 and steps >= 1 and lo >= 0 and lo + n <= total)}"]
    if lines[0] == "valid 0":
        return lines
    lines.append(f"whole {int(lo == 0 and total == n)} frames {n * steps}")
    t, p = np.divmod(np.arange(n * steps), n)
    rec = t * total + lo + p
    lines += [f"rec {r}" for r in rec]
    back = np.full(steps * total + 2, -1, np.int64)  # index r + 1
    back[rec + 1] = np.arange(n * steps)
    lines += [f"call {c}" for c in back]
    off = np.asarray(off, np.int64)
    first = off[np.arange(steps) * total + lo]
    counts = off[rec + 1] - off[rec]
    if (first < 0).any() or (counts < 0).any():
        # (the helper reports the first fault it meets, step by step: a negative base of a step before a decrease inside it)
        for s in range(steps):
            if first[s] < 0:
                return lines + ["segments 1"]
            if (counts[s * n : (s + 1) * n] < 0).any():
                return lines + ["segments 2"]
    per_step = counts.reshape(steps, n).sum(axis=1)
    dst = np.concatenate([[0], np.cumsum(per_step)])
    if dst.max() > 2**31 - 1:
        return lines + ["segments 3"]
    lines += ["segments 0", f"most {counts.max()}"]
    lines += [f"seg {a} {b}" for a, b in zip(first, dst[:-1])] + [f"seg 0 {dst[-1]}"]
    dense = dst[t] + (off[rec] - first[t])
    assert (np.diff(np.concatenate([dense, [dst[-1]]])) == counts).all()  # the device CSR starts at 0 and has no gaps
    return lines + [f"dense {d}" for d in dense]


def cases():
    rng = np.random.default_rng(11)
    out = []
    for _ in range(60):
        total = int(rng.integers(1, 9))
        steps = int(rng.integers(1, 7))
        n = int(rng.integers(1, total + 1))
        lo = int(rng.integers(0, total - n + 1))
        counts = rng.integers(0, 6, steps * total) * rng.integers(0, 2, steps * total)  # ragged, many empty frames
        off = int(rng.integers(0, 50)) + np.concatenate([[0], np.cumsum(counts)])
        out.append((n, steps, lo, total, off))
    n, steps, lo, total, off = out[3]
    out.append((n, steps, total - n + 1, total, off))  # past the recording
    out.append((0, steps, 0, total, off))
    out.append((n, steps, -1, total, off))
    out.append((2, 3, 2**31 - 2, 2**31 - 1, off))  # lo + n beyond int
    bad = np.array(out[5][4])
    n, steps, lo, total = out[5][:4]
    bad[(steps - 1) * total + lo + 1] -= 7  # decreasing inside the last segment (or, for a frame without cones before it, a base below the segment's)
    out.append((n, steps, lo, total, bad))
    out.append((n, steps, lo, total, np.array(out[5][4]) - 10**6))  # negative offsets
    out.append((1, 2, 0, 1, np.array([0, 2**31 - 1000, 2**31 - 1000])))  # fits
    out.append((1, 2, 1, 2, np.array([0, 0, 2**31 - 10, 5, 2**31 - 10])))  # two segments of 2^31 - 10 rows each: too many for the device CSR
    return out


def host_compiler():
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    return cxx


def build_program(tmp_path, flags=()):
    src = tmp_path / "slice_program.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / ("slice_program" + "".join(f.replace("=", "_").replace(",", "_") for f in flags))
    done = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", str(ROOT / "ft-fsd-path-planning_amd" / "csrc"),
                           str(src), "-o", str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-3000:]
    return exe


SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def check_helper(exe):
    for n, steps, lo, total, off in cases():
        feed = f"{n} {steps} {lo} {total}\n" + " ".join(str(int(v)) for v in off) + "\n"
        run = subprocess.run([str(exe)], input=feed, capture_output=True, text=True)
        assert run.returncode == 0, (n, steps, lo, total, run.stderr[-2000:])
        assert run.stdout.split("\n")[:-1] == restated(n, steps, lo, total, off), (n, steps, lo, total)


def test_slice_index_helper_against_numpy(tmp_path):
    check_helper(build_program(tmp_path))


def test_slice_index_helper_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same stand-alone program (never code loaded into Python) with -fsanitize=address,undefined; whether this host can link
    and run such a program is found out first, with an empty one, and a host that cannot is a visible skip that says so"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    built = subprocess.run([host_compiler(), *SANITIZE, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if built.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this host's C++ compiler cannot link and run a program with -fsanitize=address,undefined (sanitizer runtime libraries missing): "
                    + (built.stderr.strip().splitlines() or ["the probe program did not run"])[-1][:200])
    exe = build_program(tmp_path, SANITIZE)
    symbols = subprocess.run(["nm", "-D", str(exe)], capture_output=True, text=True).stdout if shutil.which("nm") else "__asan_init"
    assert "__asan" in symbols or "asan" in subprocess.run(["ldd", str(exe)], capture_output=True, text=True).stdout, "the sanitized build is not linked to the sanitizer"
    check_helper(exe)
