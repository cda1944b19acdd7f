#!/usr/bin/env python3
"""Condense rocprofv3 (rocpd sqlite) outputs — kernel stats + separate PMC passes + the counter calibration — into a
short text summary that is committed under profiles/, and into pmc_traffic.json (read by bench.py, keyed by the library's
hash).  Usage: summarize_prof.py <gpurun_out/prof_TAG> [pmc_traffic.json]"""
import glob
import hashlib
import json
import re
import sqlite3
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sys
from pathlib import Path

out = sys.argv[1]
json_out = sys.argv[2] if len(sys.argv) > 2 else None
ROOT = Path(__file__).resolve().parent.parent
FRAMES = 4096
ALGO_BYTES = 4488  # SURVEY.md 8d, N = 128
SIMDS, CLOCK_GHZ = 1024, 2.4  # MI355X: 256 CUs x 4 SIMDs; peak engine clock (MI355X_MICROARCH.md)


def db(sub):
    files = glob.glob(f"{out}/{sub}/*.db")
    return sqlite3.connect(files[0]) if files else None


def short(name):
    """'void fsdp::fit_kernel<8, 16>(int, ...)' -> 'fit_kernel<8>', '...<8, 32>' -> 'fit_kernel<8,32>' (the names bench.py /
    fsdp_stage_names use: the second parameter, knots per fit, is spelled out only for the wide instantiations)"""
    s = name.split("(")[0].replace("void ", "").split("::")[-1].strip()
    s = re.sub(r"<(\d+), 16>", r"<\1>", s)
    return re.sub(r"<(\d+), (\d+)>", r"<\1,\2>", s)


durations = {}
for sub, label in (("trace", "python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-latency  [passes overlapped, as the bench runs: 5 warm-up + 5 priming passes, the 20 timed passes, their 20-pass repeat with every kernel bracketed, 10 passes one at a time]"),
                   ("trace_serial", "same command with --no-overlap  [one pass after the other]")):
    con = db(sub)
    print(f"== rocprofv3 --kernel-trace --stats ({label}) ==")
    if con:
        print(f"{'kernel':<30}{'calls':>6}{'avg_us':>12}{'total_ms':>11}{'pct':>7}")
        for name, calls, tot, avg, pct in con.execute("select name,total_calls,total_duration,average,percentage from top_kernels"):
            print(f"{short(name):<30}{calls:>6}{avg:>12.1f}{tot / 1e3:>11.2f}{pct:>7.2f}")
        # Registers / spills / LDS / scratch come from the code object of the library that ran (tools/kernel_resources.py: the
        # AMDGPU metadata of the gfx950 ELF inside the .so), NOT from rocprofv3's kernel records — their VGPR field saturates at
        # 128 on this stack (fit_kernel<4> printed 128, the compiler says 256).  Only the launch geometry
        # is taken from the trace.
        print("-- per-kernel resources (code object metadata of lib/libfsdp_hip.so; launch geometry of the 4096-frame launches from the trace) --")
        try:
            import kernel_resources as kr
            meta = {short(k["short"]): k for k in kr.kernels(kr.ROOT / "ft-fsd-path-planning_amd" / "lib" / "libfsdp_hip.so")}
        except Exception as e:  # noqa: BLE001
            meta = {}
            print("(code object metadata unavailable:", e, ")")

        def lookup(nm):
            if nm in meta:  # (same normalisation on both sides: <8, 16> -> <8>, <8, 32> -> <8,32>)
                return meta[nm]
            base = nm.split("<")[0]
            for k, v in meta.items():
                if k == nm or (k.split("<")[0] == base and nm.split("<")[-1].rstrip(">").split(",")[0] == k.split("<")[-1].rstrip(">").split(",")[0].strip()):
                    return v
            return None
        seen = set()
        for r in con.execute("select name, workgroup_x, grid_x from kernels order by grid_x desc"):
            if r[0] in seen:
                continue
            seen.add(r[0])
            m = lookup(short(r[0]))
            if m:
                regs, by_lds = kr.occupancy(int(m["vgpr_count"]), int(m.get("agpr_count", 0)), int(m["group_segment_fixed_size"]), int(r[1]))
                print(f"{short(r[0]):<30} regs={m['vgpr_count']} (agpr {m.get('agpr_count', 0)}) sgpr={m['sgpr_count']} vgpr_spill={m.get('vgpr_spill_count', 0)} "
                      f"sgpr_spill={m.get('sgpr_spill_count', 0)} lds={m['group_segment_fixed_size']}B scratch={m['private_segment_fixed_size']}B/lane "
                      f"waves/SIMD: {regs} by registers, {by_lds:.2f} by LDS   wg={r[1]} grid={r[2]}")
            else:
                print(f"{short(r[0]):<30} (not one of the library's kernels) wg={r[1]} grid={r[2]}")
        for name, avg, cnt in con.execute("select name, avg(duration), count(*) from kernels where grid_x >= 4096 group by name"):
            if "fsdp::" in name and "default" not in name:
                gbs = ALGO_BYTES * FRAMES / (avg * 1e-9) / 1e9
                durations.setdefault(sub, {})[short(name)] = avg
                print(f"roofline[{short(name)}]: avg {avg / 1e3:.1f} us over {cnt} launches -> algorithmic {gbs:.3f} GB/s = {gbs / 8000:.2e} of 8 TB/s HBM peak")
        if sub == "trace":
            # the launches bench.py's events bracket: the timed region = launches 11..30 of a kernel, its repeat = 31..50
            # (launches 1..10 are the warm-up and priming passes, which run with fewer passes in flight)
            for (name,) in list(con.execute("select distinct name from kernels where grid_x >= 4096")):
                if "fsdp::" not in name or "default" in name:
                    continue
                d = [r[0] for r in con.execute("select duration from kernels where name = ? and grid_x >= 4096 order by start", (name,))]
                if len(d) >= 50 and short(name).startswith(("fit_kernel", "path_kernel<64>")):
                    # the same launches as bench.py's own HIP events saw them, in this very process (its JSON line in trace.log)
                    try:
                        line = [l for l in open(f"{out}/trace.log") if l.startswith("{")][-1]
                        bj = json.loads(line)
                        print(f"bench.py in this run: value {bj['value']:.0f} frames/s, roofline.kernel {bj['roofline']['kernel']}, "
                              f"kernel_ms_timed_region {1e3 * bj['roofline']['kernel_ms_timed_region']:.1f} us (HIP events, launches 11-30)"
                              + (f", kernel_ms_device_clock {1e3 * bj['roofline']['kernel_ms_device_clock']:.1f} us (the kernel's own clock, same launches)"
                                 if bj['roofline'].get('kernel_ms_device_clock') else ""))
                    except Exception as e:  # noqa: BLE001
                        print("(no bench line in trace.log:", e, ")")
                if len(d) >= 50:
                    print(f"timed-region launches [{short(name)}]: avg {sum(d[10:30]) / 20e3:.1f} us (launches 11-30), repeat {sum(d[30:50]) / 20e3:.1f} us (31-50), "
                          f"warm-up / priming {sum(d[:10]) / 10e3:.1f} us (1-10)")

# counter calibration: 1 GiB moved per kernel
calib = {}
for sub, ctr in (("calib_fetch", "FETCH_SIZE"), ("calib_write", "WRITE_SIZE")):
    con = db(sub)
    if not con:
        continue
    print(f"== counter calibration ({ctr}, kernels that move exactly 1 048 576 KB; tools/ubench/fetch_calib.hip) ==")
    for k, c, v, n in con.execute("select kernel_name, counter_name, avg(value), count(*) from counters_collection group by kernel_name, counter_name"):
        if c != ctr:
            continue
        kn = short(k)
        if (ctr == "FETCH_SIZE") == kn.startswith("read"):
            calib[kn] = 1048576.0 / v if v else None
            print(f"{kn:<14}{c:<12}{v:>14.1f} KB reported  -> true/reported = {calib[kn]:.3f}")

pmc = {}
for sub in ("pmc_fetch", "pmc_write", "pmc_sq"):
    con = db(sub)
    if not con:
        continue
    print(f"== rocprofv3 --pmc pass: {sub} (per-dispatch averages of the 4096-frame launches) ==")
    # (dispatches of other sizes — the default-path kernel, flip-count frames — are excluded by their grid size)
    q = ("select c.kernel_name, c.counter_name, avg(c.value), count(*) from counters_collection c "
         "where c.grid_size >= 4096 * 4 group by c.kernel_name, c.counter_name")
    try:
        rows = list(con.execute(q))
    except sqlite3.OperationalError:
        rows = list(con.execute("select kernel_name, counter_name, avg(value), count(*) from counters_collection group by kernel_name, counter_name"))
    for k, c, v, n in rows:
        if "fsdp::" not in k or "default" in k or "selftest" in k:
            continue
        kn = short(k)
        print(f"{kn:<30}{c:<22}{v:>16.1f}  n={n}")
        pmc.setdefault(kn, {})[c] = v

if json_out and pmc:
    # no calibration run, no byte counts: FETCH_SIZE under-reports by 2 x on this stack, and a silent factor of 1 would halve every
    # traffic figure (the calibration binary is a build output: tools/profile_gpu.sh compiles it on the box when it is missing)
    have_calib = bool(calib.get("read_b64") and (calib.get("read_rec64") or calib.get("read_b128")) and calib.get("write_b64"))
    if not have_calib:
        print("!! counter calibration missing (tools/ubench/fetch_calib did not run): FETCH_SIZE / WRITE_SIZE are listed raw, "
              "hbm_bytes_per_launch is NOT written")
    f8 = calib.get("read_b64") or 1.0
    f16 = calib.get("read_rec64") or calib.get("read_b128") or 1.0
    fw = calib.get("write_b64") or 1.0
    doc = {"source": f"{out}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE / SQ_* (separate passes, per-dispatch averages of the "
                     "4096-frame launches; tools/profile_gpu.sh)",
           "lib_sha256_16": hashlib.sha256((ROOT / "ft-fsd-path-planning_amd" / "lib" / "libfsdp_hip.so").read_bytes()).hexdigest()[:16],
           "calibration_true_over_reported": calib,
           "note": "hbm_bytes_per_launch = FETCH_SIZE x calibration factor + WRITE_SIZE x factor.  The fit / prep / finish kernels "
                   "read their scratch mostly as 64-byte records (16 B per lane: factor of read_rec64), the sorting and "
                   "matching kernels read 8 B per lane (factor of read_b64)."}
    for kn, d in pmc.items():
        ff = f16 if ("fit" in kn or "prep" in kn or "finish" in kn or "path" in kn) else f8
        e = {}
        if "FETCH_SIZE" in d or "WRITE_SIZE" in d:
            e["FETCH_SIZE_KB"] = round(d.get("FETCH_SIZE", 0.0), 1)
            e["WRITE_SIZE_KB"] = round(d.get("WRITE_SIZE", 0.0), 1)
            if have_calib:
                e["fetch_factor"] = ff
                e["hbm_bytes_per_launch"] = int(1024 * (ff * d.get("FETCH_SIZE", 0.0) + fw * d.get("WRITE_SIZE", 0.0)))
        if "SQ_INSTS_VALU" in d:
            e["valu_insts_per_frame"] = round(d["SQ_INSTS_VALU"] / FRAMES, 1)
            dur = durations.get("trace_serial", {}).get(kn)
            if dur:
                # share of the chip's VALU issue slots the kernel's wave-instructions fill while it runs alone
                # (one wave64 FP64/VALU instruction = 4 issue cycles of one SIMD)
                e["valu_issue_util"] = round(d["SQ_INSTS_VALU"] * 4 / (dur * CLOCK_GHZ * SIMDS), 4)
            if d.get("SQ_WAVE_CYCLES"):
                e["valu_active_share_of_wave_cycles"] = round(d.get("SQ_ACTIVE_INST_VALU", 0) / d["SQ_WAVE_CYCLES"], 3)
                e["wait_share_of_wave_cycles"] = round(d.get("SQ_WAIT_ANY", 0) / d["SQ_WAVE_CYCLES"], 3)
        doc[kn] = e
    json.dump(doc, open(json_out, "w"), indent=1)
    print("== pmc_traffic.json ==")
    print(json.dumps(doc, indent=1))
