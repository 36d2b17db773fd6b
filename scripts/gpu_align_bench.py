"""Host alignment (dtw_align of yourmt3_amd/metrics.py, the specification) against the device call (Aligner.align; include/ymt3.h,
alignment) on the same inputs, 130 programs at 100 frames per second.

Three workloads, each a reference and the same music under a piecewise tempo curve with 10 ms jitter, 10 % misses, 5 % octave errors and
false alarms:
  tempo_curve  the case of tests/align_cases.py: 30 s against 27.5 s, 3000 x 2750 frames, band 400
  3_minutes    180 s against 165 s, 18 000 x 16 500 frames, band 1000 (10 pitched notes a second and a drum pattern, seed 20261018)
  10_minutes   600 s against 550 s, 60 000 x 55 000 frames, band 3000
Timed in one process per workload, the records already on the device, after a warm-up:
  host     dtw_align(ref, est, ...): a host clock; HOST_REPS runs (5 for tempo_curve, 1 for the long pairs: their one run takes long)
  device   Aligner.align with the path: device events around CALLS back-to-back calls, divided by CALLS; medians of REPS
The only comparison is host specification against device path: the parent commit has no such call.  No ratio is promised.

Run without arguments this file is the launcher: every workload is a fresh process under its own `timeout`; a step that fails ends the run.
`--workload NAME --profile` runs the device call once after a warm-up and nothing else: the process to put under a kernel trace.
`--trace` (the launcher's last step, or alone) puts that process for the 10-minute pair under `rocprofv3 --kernel-trace --stats`, a run
of its own under its own `timeout`, and reduces the trace's dispatches of the LAST call to profiles/align_bench_kernel_stats.csv: per
kernel the launches, the summed, mean, least and largest duration in ns and the least and largest number of workgroups (grid x /
workgroup x), then one row with the time from the first kernel's start to the last one's end.
Output: profiles/align_bench.json (OUT=... for another path; STATS=... for the kernel table)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 20261018
REPS = 5
CALLS = 10
N_PROGRAMS = 130
FPS = 100.0
# name -> (reference seconds, estimate seconds, band frames, largest distance from the straight line in seconds, host runs, timeout)
WORKLOADS = {"tempo_curve": (30.0, 27.5, 400, 3.5, 5, 300), "3_minutes": (180.0, 165.0, 1000, 8.0, 1, 600), "10_minutes": (600.0, 550.0, 3000, 25.0, 1, 1100)}


def pair(ref_sec, est_sec, dev, seed=SEED):
    """-> (ref, est) NOTE_RECORD arrays"""
    import numpy as np
    from align_cases import NAN, records
    rng = np.random.default_rng(seed)
    knots_ref = [ref_sec * k / 4 for k in range(5)]
    knots_est = [est_sec * k / 4 + d * dev for k, d in enumerate((0.0, 1.0, 0.2, -0.75, 0.0))]
    assert all(b > a for a, b in zip(knots_est, knots_est[1:]))
    curve = lambda t: float(np.interp(t, knots_ref, knots_est))
    ref = []
    for _ in range(int(10 * ref_sec)):
        on = float(rng.uniform(0.0, ref_sec - 0.5))
        ref.append((round(on, 3), round(on + float(rng.uniform(0.1, 1.2)), 3), int(rng.integers(0, 8)), int(rng.integers(36, 96)), False))
    ref += [(round(0.25 * k, 3), NAN, 128, (36, 42, 38, 42)[k % 4], True) for k in range(int(4 * ref_sec))]
    est = []
    for on, off, prog, pitch, drum in ref:
        u = rng.random()
        if u < 0.10:
            continue
        if u > 0.95 and not drum:
            pitch += 12
        est.append((curve(on) + float(rng.normal(0.0, 0.010)), NAN if drum else curve(off) + float(rng.normal(0.0, 0.010)), prog, pitch, drum))
    for _ in range(int(0.7 * ref_sec)):
        on = float(rng.uniform(0.0, est_sec - 0.5))
        est.append((on, on + 0.3, int(rng.integers(0, 8)), int(rng.integers(36, 96)), False))
    return records(ref), records([est[i] for i in rng.permutation(len(est))])


def workload(name):
    ref_sec, est_sec, band, dev, host_reps, _ = WORKLOADS[name]
    if name == "tempo_curve":
        import align_cases
        c = align_cases.tempo_curve_case()
        return c["ref"], c["est"], c["na"], c["nb"], c["band"], host_reps, align_cases.SEED + 1
    ref, est = pair(ref_sec, est_sec, dev)
    return ref, est, int(ref_sec * FPS), int(est_sec * FPS), band, host_reps, SEED


def band_cells(na, nb, band):
    from yourmt3_amd.metrics import _diag_range
    q, p = na - 1, nb - 1
    bm = band * max(p, q, 1)
    return sum(max(0, hi - lo + 1) for lo, hi in (_diag_range(d, p, q, bm) for d in range(p + q + 1)))


def child(name, profile):
    import numpy as np
    import torch
    from yourmt3_amd.config import YMT3Config
    from yourmt3_amd.metrics import dtw_align
    from yourmt3_amd.model import YourMT3
    ref, est, na, nb, band, host_reps, seed = workload(name)
    cfg = YMT3Config(segment_samples=8191, max_decode_len=16, n_enc_layers=1, n_dec_layers=1)    # only the handle matters here
    m = YourMT3(cfg, max_batch=1)
    al = m.compile_aligner(N_PROGRAMS, max(na, nb), FPS, band)
    rd, ed = (torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda() for r in (ref, est))
    call = lambda: al.align(rd, ed, na, nb, path=True)
    call()                                                        # warm-up: code objects, the allocator's blocks
    torch.cuda.synchronize()
    if profile:
        call()
        torch.cuda.synchronize()
        al.close()
        m.close()
        return 0
    reps = int(os.environ.get("REPS", REPS))
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            out = call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3 / CALLS)
    print(f"{name}: device {sorted(times)} s per call", flush=True)
    host = []
    for _ in range(int(os.environ.get("HOST_REPS", host_reps))):
        t0 = time.perf_counter()
        want = dtw_align(ref, est, na, nb, N_PROGRAMS, frames_per_second=FPS, band_frames=band)
        host.append(time.perf_counter() - t0)
        print(f"{name}: host {host[-1]:.2f} s", flush=True)
    warp, result, path = (t.cpu().numpy() for t in out)
    equal = (result.tolist() == [want.total, want.path_len] + want.skipped.tolist() and bool(np.array_equal(warp, want.warp))
             and bool(np.array_equal(path[:want.path_len], want.path)))
    cells = band_cells(na, nb, band)
    tr, tc = -(-min(na, nb) // 256), -(-max(na, nb) // 64)
    med = lambda v: float(np.median(v))
    res = {"workload": f"{na} x {nb} frames at {FPS:g} per second, band {band}, {N_PROGRAMS} programs, seed {seed}; device: events around {CALLS} calls, "
                       f"median of {reps}; host: median of {len(host)}",
           "n_ref": int(ref.size), "n_est": int(est.size), "n_ref_frames": na, "n_est_frames": nb, "band_frames": band, "band_cells": cells,
           "tile_antidiagonals": tr + tc - 1, "device_equals_host": equal, "total": want.total, "path_len": want.path_len,
           "host_s": round(med(host), 4), "device_s": round(med(times), 7), "device_cells_per_s": round(cells / med(times)),
           "host_cells_per_s": round(cells / med(host)), "host_s_all": [round(x, 4) for x in host], "device_s_all": [round(x, 7) for x in times]}
    al.close()
    m.close()
    print("RESULT " + json.dumps(res))
    return 0 if equal else 3


def trace():
    import csv, glob, sqlite3, tempfile
    stats_path = os.environ.get("STATS", os.path.join(ROOT, "profiles", "align_bench_kernel_stats.csv"))
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "align", "--", sys.executable, os.path.abspath(__file__),
               "--workload", "10_minutes", "--profile"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        found = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not found:
            print(r.stdout[-3000:], r.stderr[-3000:], sep="\n")
            print(f"trace: exit status {r.returncode}, {len(found)} database(s)")
            return r.returncode or 1
        db = sqlite3.connect(found[0])
        t0 = db.execute("select max(start) from kernels where name like '%align_clear_kernel%'").fetchone()[0]      # the call after the warm-up
        rows = db.execute("select name, count(*), sum(end - start), avg(end - start), min(end - start), max(end - start), min(grid_x / workgroup_x), "
                          "max(grid_x / workgroup_x) from kernels where start >= ? and name like '%align_%' group by name order by min(start)", (t0,)).fetchall()
        span = db.execute("select max(end) - min(start) from kernels where start >= ? and name like '%align_%'", (t0,)).fetchone()[0]
    os.makedirs(os.path.dirname(stats_path), exist_ok=True)
    with open(stats_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "MinWorkgroups", "MaxWorkgroups"])
        for r in rows:
            w.writerow([r[0].replace("(anonymous namespace)::", ""), r[1], r[2], round(r[3]), r[4], r[5], r[6], r[7]])
        w.writerow(["first start to last end of the call", 1, span, span, "", "", "", ""])
    print(open(stats_path).read())
    return 0


def launcher():
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "align_bench.json"))
    results = {}
    me = os.path.abspath(__file__)
    for name in os.environ.get("WORKLOADS", ",".join(WORKLOADS)).split(","):
        r = subprocess.Popen(["timeout", "-k", "10", str(WORKLOADS[name][5]), sys.executable, me, "--workload", name], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        line = None
        for out in r.stdout:                                      # passed on as it comes: the long pairs' host runs take minutes
            if out.startswith("RESULT "):
                line = out
            else:
                print(out, end="", flush=True)
        if r.wait() != 0 or line is None:
            print(f"{name}: exit status {r.returncode}; nothing further is started")
            return r.returncode or 1
        results[name] = json.loads(line[len("RESULT "):])
        print(name, json.dumps(results[name]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(results, open(out_path, "w"), indent=1)
    print("wrote", out_path, flush=True)
    return trace()


if __name__ == "__main__":
    if "--trace" in sys.argv:
        sys.exit(trace())
    if "--workload" in sys.argv:
        sys.exit(child(sys.argv[sys.argv.index("--workload") + 1], "--profile" in sys.argv))
    sys.exit(launcher())
