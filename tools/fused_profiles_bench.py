"""Both axisym_toroid deposition profiles from ONE fused pass against two single-profile fused passes, on the MI355X
-> profiles/r05/measurements/fused_profiles.json.

    python tools/fused_profiles_bench.py --parent-lib PATH/librays_hip.so [--rounds 5] [--rounds-cfg5 3] [--reps 5] [--out FILE]

PATH: the library built from the parent commit (make -C rays_amd/csrc in a checkout of it).  Every measurement runs in
a child process of its own that loads ONE library (RAYS_HIP_LIB), under a time limit of its own; the children alternate
parent / change / parent / ... for `--rounds` rounds in one session, one process on the GPU at a time, and the first
child that fails ends the run.  Device events around work that ends in a synchronise; medians over the repetitions of
a child, then min / median / max over the rounds.  Per configuration (cfg 5b = configs/cfg5b_axisym256k_rk4_damp.in
every round; cfg 5 = configs/cfg5_axisym256k_sg_damp.in, the SG fan, in the first `--rounds-cfg5` rounds), 'Ptotal_psi'
+ 'Ptotal_rho' at 100 bins each:
  (a) two_passes    rays_hip_trace_deposition_device twice, zeroing of work included -- with the parent's library
  (b) two_passes    the same with this library, which must lie within the parent's spread
  (c) one_pass      rays_hip_trace_profiles_device with both records (this library only)
  (d) single        rays_hip_trace_deposition_device once: (c) - (d) is the price of the second profile
The two-profile pass traces once instead of twice, so the bar is: the median of (c) lies below the parent's MINIMUM of
(a) over the rounds.  Every round asserts that (c)'s two work arrays and two profiles equal (b)'s bit for bit.  For cfg 5b
the device memory in use per ray during (c) is recorded (hipMemGetInfo before the tensors exist and after the pass)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = {"cfg5b": "cfg5b_axisym256k_rk4_damp.in", "cfg5": "cfg5_axisym256k_sg_damp.in"}
N_BINS = 100
PROFILES = ("Ptotal_psi", "Ptotal_rho")


def worker(reps, names):
    import numpy as np
    import torch

    import bench
    from rays_amd import hip
    from rays_amd.trace import DeviceTrace

    have_profiles = hasattr(hip.load(), "rays_hip_trace_profiles_device")
    hip.set_numerics("exact")
    out = {"library": os.path.basename(os.path.dirname(os.path.dirname(hip.LIB_PATH))), "have_profiles": have_profiles}

    def timed(fn, n):
        """median / min / max of n device-event timings of fn() (ms), after one warm-up call"""
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=n)

    for name in names:
        nml, p, r0, n0 = bench.build_fan(os.path.join(ROOT, "configs", CONFIGS[name]), 1)
        tab = bench.build_fan.tables
        hip.set_rho_table(tab["rho_grid"], tab["rho_fspl"])
        nray = len(r0)
        w = getattr(bench.build_fan, "ray_pwr_wt", None)
        power = np.full(nray, 1.0 / nray) if w is None or not np.any(w) else np.asarray(w, dtype=np.float64)
        row = dict(nray=nray, n_bins=N_BINS, rho_spline_is_nan=bool(np.isnan(tab["rho_fspl"]).any()))
        singles = [DeviceTrace(p, r0, n0, trajectories=False, deposition=(which, N_BINS, power)) for which in PROFILES]

        def two_passes():
            for s in singles:
                s.launch()
        row["kernel_single"] = hip.deposition_kernel_name(p, nray)
        row["two_passes"] = timed(two_passes, reps)
        row["single"] = timed(singles[0].launch, reps)
        row["steps"] = int(torch.clamp(singles[0].npoints.to(torch.int64) - 1, min=0).sum())
        ref = [(s.work.clone(), s.profile.clone()) for s in singles]
        del singles
        torch.cuda.empty_cache()
        if have_profiles:
            torch.cuda.synchronize()
            free_before, _ = torch.cuda.mem_get_info()
            both = DeviceTrace(p, r0, n0, trajectories=False, deposition=[(which, N_BINS) for which in PROFILES],
                               ray_power=power)
            row["kernel_one_pass"] = hip.profiles_kernel_name(p, nray, 2)
            row["one_pass"] = timed(both.launch, reps)
            free_after, _ = torch.cuda.mem_get_info()
            row["one_pass_device_bytes_per_ray"] = (free_before - free_after) / nray
            same = all(torch.equal(wk.view(torch.int64), rw.view(torch.int64)) and
                       torch.equal(pf.view(torch.int64), rp.view(torch.int64))
                       for wk, pf, (rw, rp) in zip(both.works, both.profiles, ref))
            row["one_pass_equals_two_passes"] = bool(same)
            if not same:   # asserted in every round: a pass that bins something else is not a measurement
                print("RESULT " + json.dumps(out), flush=True)
                sys.exit(f"{name}: the two-profile pass does not reproduce the two single-profile passes")
            del both
        del ref
        torch.cuda.empty_cache()
        hip.finalize()
        out[name] = row
    print("RESULT " + json.dumps(out), flush=True)


def spread(rows, name, key):
    vals = [r[name][key]["median_ms"] for r in rows if name in r and key in r[name]]
    if not vals:
        return None
    return dict(min_ms=min(vals), median_ms=statistics.median(vals), max_ms=max(vals), rounds=len(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="librays_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rounds-cfg5", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05", "measurements", "fused_profiles.json"))
    ap.add_argument("--worker", default=None, help="(internal) comma-separated configurations to time in this process")
    a = ap.parse_args()
    if a.worker:
        return worker(a.reps, a.worker.split(","))
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's librays_hip.so is needed (the comparison is made in one session)")
    libs = {"parent": os.path.abspath(a.parent_lib), "change": os.path.join(ROOT, "rays_amd", "lib", "librays_hip.so")}
    rows = {"parent": [], "change": []}
    for rnd in range(a.rounds):
        names = "cfg5b,cfg5" if rnd < a.rounds_cfg5 else "cfg5b"
        for side in ("parent", "change"):
            env = dict(os.environ, RAYS_HIP_LIB=libs[side])
            r = subprocess.run(["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__),
                                "--worker", names, "--reps", str(a.reps)], env=env, capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:   # a measurement that did not run ends the session: nothing more is started
                sys.exit(f"round {rnd}, {side} library: worker failed ({r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            rows[side].append(json.loads(line[-1][7:]))
            print(f"round {rnd} {side}: cfg5b two passes {rows[side][-1]['cfg5b']['two_passes']['median_ms']:.3f} ms", flush=True)
    summary = {}
    for name in CONFIGS:
        s = dict(a_parent_two_passes=spread(rows["parent"], name, "two_passes"),
                 b_change_two_passes=spread(rows["change"], name, "two_passes"),
                 c_change_one_pass=spread(rows["change"], name, "one_pass"),
                 d_change_single=spread(rows["change"], name, "single"))
        if s["c_change_one_pass"] and s["d_change_single"]:
            s["second_profile_cost_ms"] = s["c_change_one_pass"]["median_ms"] - s["d_change_single"]["median_ms"]
        if s["a_parent_two_passes"] and s["c_change_one_pass"]:
            below = s["c_change_one_pass"]["median_ms"] < s["a_parent_two_passes"]["min_ms"]
            s["verdict"] = ("the two-profile pass's median lies below the parent's minimum of two single-profile passes" if below
                            else "DEFECT: the two-profile pass's median does NOT lie below the parent's minimum of two passes")
            s["two_passes_within_parent_spread"] = bool(s["a_parent_two_passes"]["min_ms"] <= s["b_change_two_passes"]["median_ms"]
                                                        <= s["a_parent_two_passes"]["max_ms"])
        s["one_pass_equals_two_passes"] = all(r[name].get("one_pass_equals_two_passes") for r in rows["change"] if name in r)
        mem = [r[name]["one_pass_device_bytes_per_ray"] for r in rows["change"] if name in r and "one_pass_device_bytes_per_ray" in r[name]]
        if mem:
            s["one_pass_device_bytes_per_ray"] = statistics.median(mem)
        summary[name] = s
    doc = dict(tool="tools/fused_profiles_bench.py", rounds=a.rounds, rounds_cfg5=a.rounds_cfg5, reps=a.reps, n_bins=N_BINS,
               profiles=list(PROFILES),
               not_measured=["make FULL=1 library", "multi-device host form (rays_hip_trace_profiles over several devices)",
                             "a fan whose rho(psiN) spline is finite at this size (both configurations use the 129 x 129 "
                             "table, whose rho spline is NaN: every rho segment lands in bin 1)"],
               summary=summary, rounds_raw=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
