"""Fused trace + deposition against trace-then-deposit, on the MI355X -> profiles/r05/measurements/fused_deposition.json.

    python tools/fused_deposition_bench.py --parent-lib PATH/librays_hip.so [--rounds 5] [--reps 5] [--out FILE]

PATH: the library built from the parent commit (make -C rays_amd/csrc in a checkout of it).  Every measurement runs in
a child process of its own that loads ONE library (RAYS_HIP_LIB); the children alternate parent / change / parent / ...
for `--rounds` rounds in one session, so that both see the same machine.  Device events around work that ends in a
synchronise; medians over the repetitions of a child, then min / median / max over the rounds.  Per configuration
(cfg 5b = configs/cfg5b_axisym256k_rk4_damp.in every round; cfg 5 = configs/cfg5_axisym256k_sg_damp.in, the SG fan, in
the first round only), 'Ptotal_psi' at 100 bins:
  (a) two_step   rays_hip_trace_device INCLUDING its zero-fill of the trajectories, then rays_hip_deposition_device
                 -- with the parent's library and (b) with this one, which must lie within the parent's spread
  (c) fused      rays_hip_trace_deposition_device including its zeroing of work (this library only)
  (d) summary    rays_hip_trace_summary_device: (c) - (d) is the price of binning
The fused entry moves strictly fewer bytes than (a), so the bar is: the median of (c) lies below the parent's MINIMUM of
(a) over the rounds.  `verdict` says whether it does."""
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


def worker(reps, names):
    import numpy as np
    import torch

    import bench
    from rays_amd import hip
    from rays_amd.trace import DeviceTrace

    have_fused = hasattr(hip.load(), "rays_hip_trace_deposition_device")
    hip.set_numerics("exact")
    out = {"library": os.path.basename(os.path.dirname(os.path.dirname(hip.LIB_PATH))), "have_fused": have_fused}

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
        nray = len(r0)
        w = getattr(bench.build_fan, "ray_pwr_wt", None)
        power = np.full(nray, 1.0 / nray) if w is None or not np.any(w) else np.asarray(w, dtype=np.float64)
        row = dict(nray=nray, n_bins=N_BINS, kernel_full=hip.kernel_name(p, nray))
        stream = torch.cuda.current_stream().cuda_stream
        full = DeviceTrace(p, r0, n0)
        d_pw = torch.as_tensor(power).cuda()
        work = torch.zeros((N_BINS, nray), dtype=torch.float64, device="cuda")
        prof = torch.zeros(N_BINS, dtype=torch.float64, device="cuda")

        def two_step():
            full.launch(zero_fill=True)
            hip.deposition_device(p, "Ptotal_psi", N_BINS, nray, full.ray_vec.data_ptr(), full.npoints.data_ptr(),
                                  d_pw.data_ptr(), work.data_ptr(), None, prof.data_ptr(), stream=stream)
        row["two_step"] = timed(two_step, reps)
        row["trajectory_bytes"] = int(full.ray_vec.numel() + full.residual.numel()) * 8
        row["steps"] = int(torch.clamp(full.npoints.to(torch.int64) - 1, min=0).sum())
        ref_work, ref_prof = work.clone(), prof.clone()
        del full, work
        torch.cuda.empty_cache()
        if have_fused:
            fused = DeviceTrace(p, r0, n0, trajectories=False, deposition=("Ptotal_psi", N_BINS, power))
            row["kernel_fused"] = hip.deposition_kernel_name(p, nray)
            row["fused"] = timed(fused.launch, reps)
            row["fused_equals_two_step"] = bool(torch.equal(fused.work.view(torch.int64), ref_work.view(torch.int64)) and
                                                torch.equal(fused.profile.view(torch.int64), ref_prof.view(torch.int64)))
            del fused
            s = DeviceTrace(p, r0, n0, trajectories=False)
            row["kernel_summary"] = hip.summary_kernel_name(p, nray)
            row["summary"] = timed(s.launch, reps)
            del s
        del ref_work
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05", "measurements", "fused_deposition.json"))
    ap.add_argument("--worker", default=None, help="(internal) comma-separated configurations to time in this process")
    a = ap.parse_args()
    if a.worker:
        return worker(a.reps, a.worker.split(","))
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's librays_hip.so is needed (the comparison is made in one session)")
    libs = {"parent": os.path.abspath(a.parent_lib), "change": os.path.join(ROOT, "rays_amd", "lib", "librays_hip.so")}
    rows = {"parent": [], "change": []}
    for rnd in range(a.rounds):
        names = "cfg5b,cfg5" if rnd == 0 else "cfg5b"
        for side in ("parent", "change"):
            env = dict(os.environ, RAYS_HIP_LIB=libs[side])
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", names, "--reps", str(a.reps)],
                               env=env, capture_output=True, text=True, timeout=900)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:   # a measurement that did not run is an error, never a gap in the table
                sys.exit(f"round {rnd}, {side} library: worker failed ({r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            rows[side].append(json.loads(line[-1][7:]))
            print(f"round {rnd} {side}: cfg5b two-step {rows[side][-1]['cfg5b']['two_step']['median_ms']:.3f} ms", flush=True)
    summary = {}
    for name in CONFIGS:
        s = dict(a_parent_two_step=spread(rows["parent"], name, "two_step"),
                 b_change_two_step=spread(rows["change"], name, "two_step"),
                 c_change_fused=spread(rows["change"], name, "fused"),
                 d_change_summary=spread(rows["change"], name, "summary"))
        if s["c_change_fused"] and s["d_change_summary"]:
            s["binning_cost_ms"] = s["c_change_fused"]["median_ms"] - s["d_change_summary"]["median_ms"]
        if s["a_parent_two_step"] and s["c_change_fused"]:
            below = s["c_change_fused"]["median_ms"] < s["a_parent_two_step"]["min_ms"]
            s["verdict"] = ("the fused entry's median lies below the parent's minimum of trace + deposition" if below else
                            "DEFECT: the fused entry's median does NOT lie below the parent's minimum of trace + deposition")
            s["two_step_within_parent_spread"] = bool(s["a_parent_two_step"]["min_ms"] <= s["b_change_two_step"]["median_ms"]
                                                      <= s["a_parent_two_step"]["max_ms"])
        s["fused_equals_two_step"] = all(r[name].get("fused_equals_two_step") for r in rows["change"] if name in r)
        summary[name] = s
    doc = dict(tool="tools/fused_deposition_bench.py", rounds=a.rounds, reps=a.reps, n_bins=N_BINS, profile="Ptotal_psi",
               not_measured=["make FULL=1 library", "multi-device host form (rays_hip_trace_deposition over several devices)"],
               summary=summary, rounds_raw=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
