"""Segmented deposition on the MI355X: the fused ds scan against one fused call per run, and one profile per beam against
one profile per launch -> profiles/r05/measurements/scan_profiles.json.

    python tools/scan_profiles_bench.py --parent-lib PATH/librays_hip.so [--reps 11] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/scan_profiles_bench.py --kernels-only
    python tools/scan_profiles_bench.py --merge-kernel-stats DIR [--out FILE]

PATH: the library built from the parent commit (make -C rays_amd/csrc in a checkout of it).  ONE process holds both
libraries -- two handles with rays_amd.hip's declarations, each with its own tables -- so baseline and change are timed
in one session on one device, alternating.  Every figure is the median of `--reps` (>= 10) timed passes after a warm-up
pass, each pass between a pair of device events and ended by a synchronise.  configs/cfg5b_axisym256k_rk4_damp.in,
'Ptotal_psi' + 'Ptotal_rho' at 100 bins each:
  scan       the fan cut to 1024 rays, 64 values of ds: ONE call of rays_hip_scan_profiles_device (this library) against
             64 calls of rays_hip_trace_profiles_device one after another on one stream (the parent's library; and this
             library's, which must agree with the parent's).  Every run of the scan is asserted to equal its single call
             bit for bit.
  memory     device bytes held (hipMemGetInfo before the tensors exist and after the pass) by the fused scan, by the
             summary scan (rays_hip_scan_summary_device: no profile at all), and by the recording scan followed by the
             two-step deposition (trajectories + two work arrays).
  beams      the fan as it is (64 beams x 4096 rays): rays_hip_trace_profiles_segments_device (this library) against
             rays_hip_trace_profiles_device on the same rays (one profile per record; the parent's library).
--kernels-only runs one pass of each side of `beams` on this library and nothing else, for a kernel trace that collects
no counters; --merge-kernel-stats reads the trace's kernel statistics and adds the two sum kernels' own times to the file.
Nothing here is a pass / fail bar."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIG = os.path.join(ROOT, "configs", "cfg5b_axisym256k_rk4_damp.in")
SPECS = [("Ptotal_psi", 100), ("Ptotal_rho", 100)]
N_RUNS, SCAN_RAYS, N_BEAMS = 64, 1024, 64
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r05", "measurements", "scan_profiles.json")


class Libraries:
    """Two handles of librays_hip.so in one process; use(side) makes rays_amd.hip talk to one of them."""

    def __init__(self, paths):
        from rays_amd import hip
        self.hip, self.handles = hip, {}
        for side, path in paths.items():
            hip._lib, hip.LIB_PATH = None, path
            self.handles[side] = hip.load()
        self.zfun = {side: False for side in paths}

    def use(self, side):
        self.hip._lib, self.hip._zfun_set = self.handles[side], self.zfun[side]
        if not self.zfun[side]:
            self.hip.set_zfun_table()
            self.zfun[side] = True
        return self.hip


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=reps)


def fan():
    import numpy as np

    import bench
    nml, p, r0, n0 = bench.build_fan(CONFIG, 1)
    tab = bench.build_fan.tables
    w = getattr(bench.build_fan, "ray_pwr_wt", None)
    power = np.full(len(r0), 1.0 / len(r0)) if w is None or not np.any(w) else np.asarray(w, dtype=np.float64)
    return p, r0, n0, power, tab


def same_bits(torch, a, b):
    return bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def held(torch, build):
    """(object, device bytes it holds once launched): hipMemGetInfo before it exists and after its pass"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free_before, _ = torch.cuda.mem_get_info()
    obj = build()
    torch.cuda.synchronize()
    free_after, _ = torch.cuda.mem_get_info()
    return obj, int(free_before - free_after)


def measure(libs, reps):
    import numpy as np
    import torch

    from rays_amd.params import copy_params
    from rays_amd.scan import RayScan
    from rays_amd.trace import DeviceTrace

    p, r0, n0, power, tab = fan()
    for side in libs.handles:
        hip = libs.use(side)
        hip.set_numerics("exact")
        hip.set_axisym_tables(tab)
        hip.set_rho_table(tab["rho_grid"], tab["rho_fspl"])
    out = dict(config=os.path.basename(CONFIG), profiles=[w for w, _ in SPECS], n_bins=SPECS[0][1], reps=reps)

    # ---- the scan ----------------------------------------------------------------------------------------------------------
    step = len(r0) // SCAN_RAYS
    s_r0, s_n0, s_pw = r0[::step][:SCAN_RAYS].copy(), n0[::step][:SCAN_RAYS].copy(), power[::step][:SCAN_RAYS].copy()
    ds = np.linspace(0.5, 1.0, N_RUNS) * float(p.ds)
    row = dict(nray=SCAN_RAYS, n_runs=N_RUNS, ds_min=float(ds[0]), ds_max=float(ds[-1]))
    singles = []
    for d in ds:
        q = copy_params(p)
        q.ds = float(d)
        singles.append(DeviceTrace(q, s_r0, s_n0, trajectories=False, deposition=list(SPECS), ray_power=s_pw))

    def one_by_one():
        for s in singles:
            s.launch()
    hip = libs.use("change")
    scan, row["fused_scan_bytes_held"] = held(torch, lambda: _launched(RayScan(
        p, s_r0, s_n0, ds, trajectories=False, deposition=list(SPECS), ray_power=s_pw)))
    row["kernel"] = hip.profiles_kernel_name(p, N_RUNS * SCAN_RAYS, 2)
    for rnd in range(2):   # alternating: parent, change, parent, change
        libs.use("parent")
        row[f"parent_sequential_calls_{rnd}"] = timed(torch, one_by_one, reps)
        libs.use("change")
        row[f"change_sequential_calls_{rnd}"] = timed(torch, one_by_one, reps)
        row[f"change_one_scan_call_{rnd}"] = timed(torch, scan.launch, reps)
    one_by_one()
    scan.launch()
    torch.cuda.synchronize()
    same = True
    for r, s in enumerate(singles):
        for k, (_, nb) in enumerate(SPECS):
            same = same and same_bits(torch, scan.profiles[k][r], s.profiles[k])
            same = same and same_bits(torch, scan.works[k][:, r * SCAN_RAYS:(r + 1) * SCAN_RAYS], s.works[k])
        same = same and bool(torch.equal(scan.npoints[r], s.npoints))
    row["scan_equals_sequential_calls"] = same
    if not same:
        sys.exit("the fused scan does not reproduce the sequential calls")
    row["steps"] = int(torch.clamp(scan.npoints.to(torch.int64) - 1, min=0).sum())
    del scan, singles
    # ---- memory ------------------------------------------------------------------------------------------------------------
    summ, row["summary_scan_bytes_held"] = held(torch, lambda: _launched(RayScan(p, s_r0, s_n0, ds, trajectories=False)))
    del summ

    def recording():
        sc = _launched(RayScan(p, s_r0, s_n0, ds, trajectories=True))
        works = [torch.zeros((nb, N_RUNS * SCAN_RAYS), dtype=torch.float64, device="cuda") for _, nb in SPECS]
        return sc, works
    rec, row["recording_scan_and_two_step_bytes_held"] = held(torch, recording)
    row["nstep_max"] = int(p.nstep_max)
    del rec
    torch.cuda.empty_cache()
    out["scan"] = row

    # ---- the beams ---------------------------------------------------------------------------------------------------------
    nray = len(r0)
    per = nray // N_BEAMS
    row = dict(nray=nray, n_beams=N_BEAMS, rays_per_beam=per)
    one = DeviceTrace(p, r0, n0, trajectories=False, deposition=list(SPECS), ray_power=power)
    libs.use("change")
    beams = DeviceTrace(p, r0, n0, trajectories=False, deposition=list(SPECS), ray_power=power, segments=per)
    for rnd in range(2):
        libs.use("parent")
        row[f"parent_one_profile_{rnd}"] = timed(torch, one.launch, reps)
        libs.use("change")
        row[f"change_one_profile_{rnd}"] = timed(torch, one.launch, reps)
        row[f"change_profile_per_beam_{rnd}"] = timed(torch, beams.launch, reps)
    one.launch()
    beams.launch()
    torch.cuda.synchronize()
    row["work_equals_one_profile_call"] = all(same_bits(torch, a, b) for a, b in zip(beams.works, one.works))
    out["beams"] = row
    for side in libs.handles:
        libs.use(side).finalize()
    return out


def _launched(obj):
    import torch
    obj.launch()
    torch.cuda.synchronize()
    return obj


def kernels_only():
    import torch

    from rays_amd import hip
    from rays_amd.trace import DeviceTrace
    p, r0, n0, power, tab = fan()
    hip.set_numerics("exact")
    hip.set_rho_table(tab["rho_grid"], tab["rho_fspl"])
    per = len(r0) // N_BEAMS
    for segments in (None, per):
        tr = DeviceTrace(p, r0, n0, trajectories=False, deposition=list(SPECS), ray_power=power, segments=segments)
        for _ in range(3):
            tr.launch()
        torch.cuda.synchronize()
        del tr
    hip.finalize()


def merge_kernel_stats(directory, out_path):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Name", "")
                if "profile_sum" in name:
                    key = "profile_sum_segments_kernel" if "segments" in name else "profile_sum_kernel"
                    rows[key] = dict(calls=int(r["Calls"]), average_ns=float(r["AverageNs"]), min_ns=float(r["MinNs"]),
                                     max_ns=float(r["MaxNs"]), name=name)
    if not rows:
        sys.exit(f"no kernel statistics with the sum kernels under {directory}")
    with open(out_path) as f:
        doc = json.load(f)
    doc["beams"]["sum_kernels"] = dict(rows, note="per launch; 100 bins; profile_sum_kernel: 100 waves over 262144 rays each, "
                                       "profile_sum_segments_kernel: 64 x 100 waves over 4096 rays each")
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["beams"]["sum_kernels"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="librays_hip.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--merge-kernel-stats", metavar="DIR")
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a.merge_kernel_stats, a.out)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's librays_hip.so is needed (the comparison is made in one session)")
    if a.reps < 10:
        sys.exit("--reps: at least 10 timed passes")
    import torch  # noqa: F401  (before either library: rays_amd.hip's loading order)
    libs = Libraries({"parent": os.path.abspath(a.parent_lib), "change": os.path.join(ROOT, "rays_amd", "lib", "librays_hip.so")})
    doc = dict(tool="tools/scan_profiles_bench.py", **measure(libs, a.reps))
    doc["not_measured"] = ["make FULL=1 library", "the SG fan (cfg 5)", "more than one device"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
