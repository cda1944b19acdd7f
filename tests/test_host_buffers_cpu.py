"""The host library's owning buffers and stores (csrc/host_buffers.h) under allocation failure, on the CPU: tests/emu/host_buffers_probe.cpp
instantiates the library's own growth code with a counting allocator that fails the k-th allocation, for every k of every script
(grow, shrink, grow).  It asserts that after a failure a buffer is empty or still holds what was reserved, that the next successful
reserve leaves no null buffer, that a reserve within capacity never allocates, the headroom rules' exact counts, and that nothing
leaks, is freed twice or survives a move.  No GPU test exhausts device memory: this is where a failed growth is covered."""
import subprocess
from pathlib import Path

EMU_DIR = Path(__file__).resolve().parent / "emu"
ROOT = EMU_DIR.parent.parent
EXE = EMU_DIR / "host_buffers_probe"
STORES = ["buffers", "InputStore", "PassStore", "FilterStore", "SeqStore", "SeqCacheStore", "SkidGroupStore", "SortCacheStore"]


def build():
    src = EMU_DIR / "host_buffers_probe.cpp"
    deps = [src, EMU_DIR / "hip_emu.h", ROOT / "include" / "fsdp.h", *sorted((ROOT / "ft-fsd-path-planning_amd" / "csrc").glob("*.h"))]
    if not EXE.exists() or any(EXE.stat().st_mtime < d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-Wno-unknown-pragmas", "-Wno-sign-compare",
                        "-Wno-attributes", "-pthread", str(src), "-o", str(EXE)], check=True, cwd=str(EMU_DIR))
    return EXE


def test_every_store_survives_every_failed_allocation():
    run = subprocess.run([str(build())], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    for name in STORES:  # every script ran, and made allocations that could fail
        line = [l for l in run.stdout.splitlines() if l.startswith(f"ok {name} ")]
        assert len(line) == 1 and int(line[0].split()[2]) > 0, run.stdout
    assert run.stdout.rstrip().endswith("all scripts passed")
