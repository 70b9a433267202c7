#!/usr/bin/env python
"""Times rays_hip_ray_diagnostics_device against the exact trace pass of the same fan, in the same process:

    python tools/diag_bench.py [--reps 30] [--warmup 3] [--out FILE.json]

For the headline fan (configs/cfg3b_solovev64k_rk4.in) and cfg 5b (configs/cfg5b_axisym256k_rk4_damp.in): trace on the
device (exact numerics), then HIP events around `reps` back-to-back launches of (a) the exact trace pass, (b) the
diagnostics with all nineteen fields, (c) the diagnostics without N_IMAG (no deriv_cold / damping), alternating the
three so that they see the same clocks, and with them the PACKED form (rays_hip_ray_diagnostics_packed_device, out_stride
= the total read once beforehand) in both input layouts -- (d), (e) on the padded trace arrays, (f), (g) on the arrays
packed once by rays_hip_pack_device -- with all nineteen fields and without N_IMAG.  Each figure is the median over the
repetitions of one launch's time; `packed_speedup` sets the packed form against the padded one of the same process and
against the ratio of their algorithmic bytes (the expectation: the stores dominate, so the time follows them).  Points/s
and the algorithmic bytes (what the kernel must read and write: nv + 1 doubles in per recorded point, one double out per
selected field per SLOT, npoints once) are computed from the shapes here; the FETCH_SIZE / WRITE_SIZE to set against
them come from a rocprofv3 --pmc run of --one CONFIG --pmc-pass (one launch of each variant, nothing timed).
Each configuration runs in a child process of its own under `timeout`; the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = ("cfg3b_solovev64k_rk4", "cfg5b_axisym256k_rk4_damp")


def one(cfg, reps, warmup, pmc_pass):
    import numpy as np
    import torch

    from rays_amd import hip
    from rays_amd.trace import DeviceTrace, RaysRun

    hip.set_numerics("exact")
    run = RaysRun.from_namelist(os.path.join(ROOT, "configs", cfg + ".in"))
    p = run.params
    tr = DeviceTrace(p, run.rvec0, run.rindex_vec0)
    tr.launch()
    torch.cuda.synchronize()
    npts = tr.npoints.cpu().numpy().astype(np.int64)
    points, slots = int(npts.sum()), int(tr.nray) * (p.nstep_max + 1)
    no_imag = tuple(f for f in hip.DIAG_FIELDS if f != "n_imag")
    out = torch.empty((19, tr.nray, p.nstep_max + 1), dtype=torch.float64, device="cuda")
    bad = torch.empty(tr.nray, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def diag(fields):
        hip.ray_diagnostics_device(p, tr.nray, tr.ray_vec.data_ptr(), tr.residual.data_ptr(), tr.npoints.data_ptr(),
                                   fields, out.data_ptr(), bad.data_ptr(), stream=stream)

    # the packed form: offsets and the total once, outside the timed launches; the packed input made once
    off = torch.empty(tr.nray + 1, dtype=torch.int64, device="cuda")
    hip.point_offsets_device(tr.nray, p.nstep_max, tr.npoints.data_ptr(), off.data_ptr(), stream)
    total = int(off[-1].item())
    assert total == points
    pv = torch.empty((total, p.nv), dtype=torch.float64, device="cuda")
    pr = torch.empty(total, dtype=torch.float64, device="cuda")
    hip.pack_device(tr.nray, p.nv, p.nstep_max, tr.npoints.data_ptr(), off.data_ptr(), tr.ray_vec.data_ptr(),
                    tr.residual.data_ptr(), pv.data_ptr(), pr.data_ptr(), stream)
    pout = torch.empty((19, total), dtype=torch.float64, device="cuda")

    def packed(fields, packed_input):
        rv, rs = (pv, pr) if packed_input else (tr.ray_vec, tr.residual)
        hip.ray_diagnostics_packed_device(p, tr.nray, rv.data_ptr(), rs.data_ptr(), tr.npoints.data_ptr(), off.data_ptr(),
                                          total, fields, pout.data_ptr(), bad.data_ptr(), stream, packed_input=packed_input)

    variants = {"trace_exact": lambda: tr.launch(), "diag_all": lambda: diag(None), "diag_no_n_imag": lambda: diag(no_imag),
                "packed_all": lambda: packed(None, False), "packed_no_n_imag": lambda: packed(no_imag, False),
                "packed_in_all": lambda: packed(None, True), "packed_in_no_n_imag": lambda: packed(no_imag, True),
                "point_offsets": lambda: hip.point_offsets_device(tr.nray, p.nstep_max, tr.npoints.data_ptr(),
                                                                  off.data_ptr(), stream)}
    if pmc_pass:
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        return dict(config=cfg, pmc_pass=True)
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    res = dict(config=cfg, nray=int(tr.nray), nv=int(p.nv), nstep_max=int(p.nstep_max), recorded_points=points, slots=slots,
               steps=int(np.maximum(npts - 1, 0).sum()), reps=reps, kernel=hip.kernel_name(p, tr.nray))
    for k, t in times.items():
        t = np.sort(np.array(t))
        res[k + "_ms"] = dict(median=float(np.median(t)), min=float(t[0]), max=float(t[-1]))
    for k, nf in (("diag_all", 19), ("diag_no_n_imag", 18)):
        ms = res[k + "_ms"]["median"]
        res[k + "_points_per_s"] = points / (ms * 1e-3)
        rd, wr = 8 * (p.nv + 1) * points + 4 * tr.nray, 8 * nf * slots
        res[k + "_algorithmic_bytes"] = dict(read=rd, write=wr, gb_per_s=(rd + wr) / (ms * 1e-3) / 1e9)
    for k, nf in (("packed_all", 19), ("packed_no_n_imag", 18), ("packed_in_all", 19), ("packed_in_no_n_imag", 18)):
        ms = res[k + "_ms"]["median"]
        res[k + "_points_per_s"] = points / (ms * 1e-3)
        rd = 8 * (p.nv + 1) * points + 8 * (tr.nray + 1) + (0 if "_in_" in k else 4 * tr.nray)
        wr = 8 * nf * points
        res[k + "_algorithmic_bytes"] = dict(read=rd, write=wr, gb_per_s=(rd + wr) / (ms * 1e-3) / 1e9)
        ref = "diag_all" if nf == 19 else "diag_no_n_imag"
        rb = res[ref + "_algorithmic_bytes"]
        speedup, expected = res[ref + "_ms"]["median"] / ms, (rb["read"] + rb["write"]) / (rd + wr)
        res[k + "_packed_speedup"] = dict(over=ref, measured=speedup, ratio_of_algorithmic_bytes=expected,
                                          achieved_fraction=speedup / expected)
    res["first_bad_points"] = int((bad != 0).sum().item())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(child) run this configuration in this process")
    ap.add_argument("--pmc-pass", action="store_true", help="with --one: one launch of each variant, nothing timed")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.reps, a.warmup, a.pmc_pass)))
        return 0
    results = []
    for cfg in CONFIGS:
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", cfg,
                            "--reps", str(a.reps), "--warmup", str(a.warmup)], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"diag_bench: {cfg} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
