"""Deposition windows against the one-shot two-profile fused pass, on the MI355X
-> profiles/r05/measurements/window_deposition.json.

    python tools/window_deposition_bench.py --parent-lib PATH/librays_hip.so [--rounds 3] [--rounds-cfg5 2] [--reps 5] [--out FILE]

PATH: the library built from the parent commit (make -C rays_amd/csrc in a checkout of it).  Every measurement runs in
a child process of its own that loads ONE library (RAYS_HIP_LIB), under a time limit of its own; the children alternate
parent / change / parent / ... for `--rounds` rounds in one session, one process on the GPU at a time, and the first
child that fails ends the run.  Device events around work that ends in a synchronise; medians over the repetitions of
a child, then min / median / max over the rounds.  Per configuration (cfg 5b = configs/cfg5b_axisym256k_rk4_damp.in
every round; cfg 5 = configs/cfg5_axisym256k_sg_damp.in, the SG fan, in the first `--rounds-cfg5` rounds), 'Ptotal_psi'
+ 'Ptotal_rho' at 100 bins each:
  (a) one_shot     rays_hip_trace_profiles_device with both records, zeroing of both works included -- with the parent's
                   library and with this one.  The one-shot kernels are the parent's instructions, so THE BAR is: the
                   median of this library's figure lies within the parent's min - max over the rounds.
  (b) windows_N    rays_hip_state_init_device + zeroing of both works + deposition windows of N = 1000, 100 and 10 steps
                   to the end of every ray, queued with no host synchronisation between them (their number is counted
                   once beforehand), the profiles summed in the last window only (this library only).  Reported, not
                   gated; the yardstick beside them is (a) on the parent in the same session.  Every child asserts that
                   the works and profiles of the windowed runs equal the one-shot pass's bit for bit."""
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
WINDOWS = (1000, 100, 10)


def worker(reps, names):
    import numpy as np
    import torch

    import bench
    from rays_amd import hip
    from rays_amd.trace import DeviceTrace

    have = hasattr(hip.load(), "rays_hip_trace_window_profiles_device")
    hip.set_numerics("exact")
    out = {"library": os.path.basename(os.path.dirname(os.path.dirname(hip.LIB_PATH))), "have_window_profiles": have}

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
        specs = [(which, N_BINS) for which in PROFILES]
        row = dict(nray=nray, n_bins=N_BINS, rho_spline_is_nan=bool(np.isnan(tab["rho_fspl"]).any()))
        both = DeviceTrace(p, r0, n0, trajectories=False, deposition=specs, ray_power=power)
        row["kernel_one_shot"] = hip.profiles_kernel_name(p, nray, 2)
        row["one_shot"] = timed(both.launch, reps)
        row["steps"] = int(torch.clamp(both.npoints.to(torch.int64) - 1, min=0).sum())
        if have:
            from rays_amd.trace import WindowedDeposition
            ref = [(wk.clone(), pf.clone()) for wk, pf in zip(both.works, both.profiles)]
            del both
            torch.cuda.empty_cache()
            row["kernel_windows"] = hip.window_profiles_kernel_name(p, nray, 2)
            for n_steps in WINDOWS:
                wd = WindowedDeposition(p, r0, n0, deposition=specs, ray_power=power)
                wd.launch()
                count = 0
                while wd.state.under_way:
                    wd.advance(n_steps, profiles=False)
                    count += 1

                def whole(wd=wd, count=count, n_steps=n_steps):
                    wd.launch()
                    for k in range(count):
                        wd.advance(n_steps, profiles=k == count - 1)
                row[f"windows_{n_steps}"] = dict(n_steps=n_steps, windows=count, **timed(whole, max(3, reps // 2)))
                same = all(torch.equal(wk.view(torch.int64), rw.view(torch.int64)) and
                           torch.equal(pf.view(torch.int64), rp.view(torch.int64))
                           for wk, pf, (rw, rp) in zip(wd.works, wd.profiles, ref))
                row[f"windows_{n_steps}"]["equals_one_shot"] = bool(same)
                if not same:   # a run that bins something else is not a measurement
                    print("RESULT " + json.dumps(out), flush=True)
                    sys.exit(f"{name}: windows of {n_steps} steps do not reproduce the one-shot pass")
                del wd
                torch.cuda.empty_cache()
            del ref
        else:
            del both
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rounds-cfg5", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05", "measurements", "window_deposition.json"))
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
            print(f"round {rnd} {side}: cfg5b one-shot {rows[side][-1]['cfg5b']['one_shot']['median_ms']:.3f} ms", flush=True)
    summary = {}
    for name in CONFIGS:
        pa, ch = spread(rows["parent"], name, "one_shot"), spread(rows["change"], name, "one_shot")
        s = dict(a_parent_one_shot=pa, a_change_one_shot=ch)
        if pa and ch:
            s["change_median_within_parent_spread"] = bool(pa["min_ms"] <= ch["median_ms"] <= pa["max_ms"])
        for n_steps in WINDOWS:
            key = f"windows_{n_steps}"
            s["b_" + key] = spread(rows["change"], name, key)
            first = [r[name][key] for r in rows["change"] if name in r and key in r[name]]
            if first:
                s["b_" + key]["windows"] = first[0]["windows"]
                s["b_" + key]["equals_one_shot"] = all(x["equals_one_shot"] for x in first)
        summary[name] = s
    doc = dict(tool="tools/window_deposition_bench.py", rounds=a.rounds, rounds_cfg5=a.rounds_cfg5, reps=a.reps, n_bins=N_BINS,
               profiles=list(PROFILES),
               not_measured=["make FULL=1 and FAST=1 libraries", "single-profile deposition windows (EQ + 224)",
                             "other window sizes and bin counts", "counters (rocprofv3 --pmc) of the new kernels",
                             "a fan whose rho(psiN) spline is finite at this size (both configurations use the 129 x 129 "
                             "table, whose rho spline is NaN: every rho segment lands in bin 1)",
                             "the cost of save() / load() between windows"],
               summary=summary, rounds_raw=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
