"""Windowed tracing against the one-shot trace, on the MI355X -> profiles/r05/measurements/window_trace.json.

    python tools/window_trace_bench.py --parent-lib PATH/librays_hip.so [--rounds 3] [--out FILE]

PATH: the library built from the parent commit.  Every measurement runs in a child process of its own that loads ONE
library (RAYS_HIP_LIB); the children alternate parent / change / parent / ... for `--rounds` rounds in one session, so
that both see the same machine (as tools/summary_trace_bench.py does).  Figures (device events around work that ends in
a synchronise; medians over the repetitions of a child, then min / median / max over the rounds):
  one_shot   the exact headline pass (64k-ray Solovev fan, configs/cfg3b_solovev64k_rk4.in) and cfg 5b's exact pass, as
             bench.py times them (rays_hip_trace_device, no zero-fill): parent against change
  windows    the headline fan from rays_hip_state_init_device to the end of every ray in windows of 1000, 100 and 10
             steps, recording (one slab [nray][n_steps][nv + 1]) and summary-only, with no host synchronisation between
             the windows (their number is counted once beforehand), next to the one-shot exact and summary passes
  host       rays_hip_trace against rays_hip_trace_windowed per call on the 64k fan (resident host arrays), n_steps = 50
             and 200"""
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
    import torch

    import bench
    from rays_amd import hip
    from rays_amd.trace import DeviceTrace

    have = hasattr(hip.load(), "rays_hip_trace_window_device")
    hip.set_numerics("exact")
    out = {"library": os.path.basename(hip.LIB_PATH), "have_window": have}

    def timed(fn, n):
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

    def wall(fn, n):
        fn()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=n)

    out["one_shot"] = {}
    for cfg in ("cfg3b_solovev64k_rk4.in", "cfg5b_axisym256k_rk4_damp.in"):
        nml, p, r0, n0 = bench.build_fan(os.path.join(ROOT, "configs", cfg), 1)
        full = DeviceTrace(p, r0, n0)
        out["one_shot"][cfg] = dict(nray=len(r0), kernel=hip.kernel_name(p, len(r0)),
                                    exact_pass=timed(lambda: full.launch(zero_fill=False), reps))
        del full
        torch.cuda.empty_cache()
    nml, p, r0, n0 = bench.build_fan(os.path.join(ROOT, "configs", "cfg3b_solovev64k_rk4.in"), 1)
    s = DeviceTrace(p, r0, n0, trajectories=False)
    out["windows"] = dict(nray=len(r0), summary_pass=timed(s.launch, reps))
    del s
    torch.cuda.empty_cache()
    if have:
        for rec in (True, False):
            for w in (1000, 100, 10):
                tr = DeviceTrace(p, r0, n0, window=w, trajectories=rec)
                tr.launch()
                count = 0
                while tr.state.under_way:
                    tr.advance()
                    count += 1

                def whole(tr=tr, count=count):
                    tr.launch()
                    for _ in range(count):
                        tr.advance()
                key = f"{'recording' if rec else 'summary'}_{w}"
                out["windows"][key] = dict(n_steps=w, windows=count, kernel=hip.window_kernel_name(p, len(r0), rec),
                                           **timed(whole, max(3, reps // 2)))
                del tr
                torch.cuda.empty_cache()
    res = hip.trace_host(p, r0, n0, ngpu=1)
    out["host"] = dict(nray=len(r0), rays_hip_trace=wall(lambda: hip.trace_host(p, r0, n0, ngpu=1, out=res), 3))
    if have:
        for w in (50, 200):
            out["host"][f"rays_hip_trace_windowed_{w}"] = wall(
                lambda: hip.trace_windowed_host(p, r0, n0, w, ngpu=1, out=res), 3)
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05", "measurements", "window_trace.json"))
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
            print(f"round {rnd} {side} done", flush=True)
    summary = dict(one_shot={}, windows={}, host={})
    for cfg in ("cfg3b_solovev64k_rk4.in", "cfg5b_axisym256k_rk4_damp.in"):
        pa, ch = spread(rows["parent"], "one_shot", cfg, "exact_pass"), spread(rows["change"], "one_shot", cfg, "exact_pass")
        summary["one_shot"][cfg] = dict(parent=pa, change=ch,
                                        change_median_within_parent_spread=pa["min_ms"] <= ch["median_ms"] <= pa["max_ms"])
    for key in rows["change"][0]["windows"]:
        if key != "nray":
            summary["windows"][key] = spread(rows["change"], "windows", key)
            if key != "summary_pass":
                summary["windows"][key]["windows"] = rows["change"][0]["windows"][key]["windows"]
    summary["windows"]["exact_pass"] = summary["one_shot"]["cfg3b_solovev64k_rk4.in"]["change"]
    for key in rows["change"][0]["host"]:
        if key != "nray":
            summary["host"][key] = spread(rows["change"], "host", key)
    summary["host"]["parent_rays_hip_trace"] = spread(rows["parent"], "host", "rays_hip_trace")
    doc = dict(tool="tools/window_trace_bench.py", rounds=a.rounds, reps=a.reps, summary=summary, rounds_raw=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
