"""Summary-only tracing against the full trace, on the MI355X -> profiles/r05/measurements/summary_trace.json.

    python tools/summary_trace_bench.py --parent-lib PATH/librays_hip.so [--rounds 5] [--out FILE]

PATH: the library built from the parent commit (make -C rays_amd/csrc in a checkout of it).  Every measurement runs in
a child process of its own that loads ONE library (RAYS_HIP_LIB); the children alternate parent / change / parent / ...
for `--rounds` rounds in one session, so that both see the same machine.  Figures (device events around work that ends
in a synchronise; medians over the repetitions of a child, then min / median / max over the rounds):
  headline   the 64k-ray Solovev fan (configs/cfg3b_solovev64k_rk4.in), exact numerics: one pass of
             rays_hip_trace_device (no zero-fill, as bench.py times it) and one of rays_hip_trace_summary_device
  scan       64 runs x 1024 rays (configs/cfg2_solovev1024_rk4.in): rays_hip_scan_device incl. the zero-fill of its
             4.2 GB, the same without the zero-fill, and rays_hip_scan_summary_device (which has nothing to fill)
  host       rays_hip_trace against rays_hip_trace_summary per call on the 64k fan (resident host arrays)
The summary kernel does strictly less work than the exact full-trace kernel, so its pass is judged against the
PARENT's exact pass: `verdict` says whether the summary median lies above the parent's own min-max spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(reps):
    import numpy as np
    import torch

    import bench
    from rays_amd import hip
    from rays_amd.scan import RayScan, scan_values
    from rays_amd.trace import DeviceTrace

    have_summary = hasattr(hip.load(), "rays_hip_trace_summary_device")
    hip.set_numerics("exact")
    out = {"library": os.path.basename(hip.LIB_PATH), "have_summary": have_summary}

    def timed(fn, n):
        """median / min / max of n device-event timings of fn() (ms), after two warm-up calls"""
        for _ in range(2):
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

    # headline fan
    nml, p, r0, n0 = bench.build_fan(os.path.join(ROOT, "configs", "cfg3b_solovev64k_rk4.in"), 1)
    full = DeviceTrace(p, r0, n0)
    out["headline"] = dict(nray=len(r0), kernel_full=hip.kernel_name(p, len(r0)),
                           full_pass=timed(lambda: full.launch(zero_fill=False), reps))
    ref = {k: getattr(full, k).clone() for k in ("npoints", "stop_code", "end_ray_vec", "end_residuals", "max_residuals")}
    ref["start_ray_vec"] = full.ray_vec[:, 0, :].clone()
    out["headline"]["steps"] = int(torch.clamp(full.npoints.to(torch.int64) - 1, min=0).sum())
    del full
    torch.cuda.empty_cache()
    if have_summary:
        s = DeviceTrace(p, r0, n0, trajectories=False)
        out["headline"]["kernel_summary"] = hip.summary_kernel_name(p, len(r0))
        out["headline"]["summary_pass"] = timed(s.launch, reps)
        out["headline"]["summary_equals_full"] = all(
            torch.equal(getattr(s, k).view(torch.int64) if getattr(s, k).dtype == torch.float64 else getattr(s, k),
                        ref[k].view(torch.int64) if ref[k].dtype == torch.float64 else ref[k]) for k in ref)
        del s
    # host entries, resident arrays
    res = hip.trace_host(p, r0, n0, ngpu=1)

    def wall(fn, n):
        fn()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=n)
    out["host"] = dict(nray=len(r0), rays_hip_trace=wall(lambda: hip.trace_host(p, r0, n0, ngpu=1, out=res), max(3, reps // 2)))
    del res
    if have_summary:
        out["host"]["rays_hip_trace_summary"] = wall(lambda: hip.trace_summary_host(p, r0, n0, ngpu=1), max(3, reps // 2))
    hip.finalize()
    torch.cuda.empty_cache()
    # the 64 x 1024 scan
    nml, p, r0, n0 = bench.build_fan(os.path.join(ROOT, "configs", "cfg2_solovev1024_rk4.in"), 1)
    vals = scan_values("fixed_increment", 64, p_start=float(p.ds), p_incr=float(p.ds) / 64)
    scan = RayScan(p, r0, n0, vals)
    out["scan"] = dict(n_runs=64, nray=len(r0), trajectory_bytes=int(scan.ray_vec.numel() + scan.residual.numel()) * 8,
                       full_with_zero_fill=timed(lambda: scan.launch(zero_fill=True), reps),
                       full_no_zero_fill=timed(lambda: scan.launch(zero_fill=False), reps))
    del scan
    torch.cuda.empty_cache()
    if have_summary:
        s = RayScan(p, r0, n0, vals, trajectories=False)
        out["scan"]["summary"] = timed(s.launch, reps)
        del s
    print("RESULT " + json.dumps(out), flush=True)


def spread(rows, *path):
    vals = []
    for r in rows:
        x = r
        for k in path:
            x = x.get(k) if isinstance(x, dict) else None
            if x is None:
                break
        if x is not None:
            vals.append(x["median_ms"])
    if not vals:
        return None
    return dict(min_ms=min(vals), median_ms=statistics.median(vals), max_ms=max(vals), rounds=len(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="librays_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05", "measurements", "summary_trace.json"))
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.reps)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's librays_hip.so is needed (the comparison is made in one session)")
    libs = {"parent": os.path.abspath(a.parent_lib), "change": os.path.join(ROOT, "rays_amd", "lib", "librays_hip.so")}
    rows = {"parent": [], "change": []}
    for rnd in range(a.rounds):
        for side in ("parent", "change"):
            env = dict(os.environ, RAYS_HIP_LIB=libs[side])
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(a.reps)], env=env,
                               capture_output=True, text=True, timeout=900)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:   # a measurement that did not run is an error, never a gap in the table
                sys.exit(f"round {rnd}, {side} library: worker failed ({r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            rows[side].append(json.loads(line[-1][7:]))
            print(f"round {rnd} {side}: headline full {rows[side][-1]['headline']['full_pass']['median_ms']:.3f} ms", flush=True)
    summary = dict(
        headline=dict(parent_full_pass=spread(rows["parent"], "headline", "full_pass"),
                      change_full_pass=spread(rows["change"], "headline", "full_pass"),
                      change_summary_pass=spread(rows["change"], "headline", "summary_pass")),
        scan=dict(parent_full_with_zero_fill=spread(rows["parent"], "scan", "full_with_zero_fill"),
                  parent_full_no_zero_fill=spread(rows["parent"], "scan", "full_no_zero_fill"),
                  change_full_with_zero_fill=spread(rows["change"], "scan", "full_with_zero_fill"),
                  change_full_no_zero_fill=spread(rows["change"], "scan", "full_no_zero_fill"),
                  change_summary=spread(rows["change"], "scan", "summary")),
        host=dict(parent_rays_hip_trace=spread(rows["parent"], "host", "rays_hip_trace"),
                  change_rays_hip_trace=spread(rows["change"], "host", "rays_hip_trace"),
                  change_rays_hip_trace_summary=spread(rows["change"], "host", "rays_hip_trace_summary")))
    h = summary["headline"]
    above = h["change_summary_pass"]["median_ms"] > h["parent_full_pass"]["max_ms"]
    summary["verdict"] = ("DEFECT: the summary pass's median lies above the parent's exact pass's min-max spread" if above else
                          "the summary pass's median lies within or below the parent's exact pass's min-max spread")
    summary["summary_equals_full"] = all(r["headline"].get("summary_equals_full") for r in rows["change"])
    doc = dict(tool="tools/summary_trace_bench.py", rounds=a.rounds, reps=a.reps, summary=summary, rounds_raw=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
