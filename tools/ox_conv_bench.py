#!/usr/bin/env python
"""Times the O-X conversion analysis on the device (rays_hip_ox_conv_device) against what a user had before it existed,
in the same process:

    python tools/ox_conv_bench.py [--reps 30] [--warmup 3] [--out profiles/r05/measurements/ox_conv.json]

Two workloads: the headline fan (configs/cfg3b_solovev64k_rk4.in) traced on the device, and the slab case T.slab_ox of
tests/golden/ox_conv_cases.npz (48 rays, 253 points kept) tiled to 65 536 rays.  For each, HIP events around `reps`
launches, alternating, of
  (a) ox_conv          rays_hip_ox_conv_device on the padded arrays, every field wanted;
  (b) alpha_download   the yardstick: rays_hip_ray_diagnostics_packed_device with the alpha_e field alone (offsets and the
                       total read once beforehand) plus the copy of that field to pinned host memory -- what the host loop
                       of the reference's find_x_max_ray needs before it can start.  The host loop itself, the ascent
                       and the coefficient are NOT in the yardstick: it is a lower bound of the old way.
Each figure is the median over the repetitions of one launch's time.  No ratio is demanded of the two; both are
recorded, with the counts that explain them (recorded points, rays with a maximum, the points the scan has to visit:
step_number + 1 rounded up to whole chunks of 64).  Each workload runs in a child process of its own under `timeout`;
the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = ("cfg3b_solovev64k_rk4", "slab_ox_65536")


def one(which, reps, warmup):
    import numpy as np
    import torch

    from rays_amd import hip

    hip.set_numerics("exact")
    if which == "slab_ox_65536":
        from tests import ox_conv_expect as ox

        fx = ox.load_fixture("T.slab_ox")
        p0, _ = ox.load_params("T.slab_ox")
        p, rv, npts = ox.padded(p0, fx)
        copies = 65536 // len(npts) + 1
        rv, npts = np.tile(rv, (copies, 1, 1))[:65536], np.tile(npts, copies)[:65536]
        nray = len(npts)
        d_rv, d_res = torch.as_tensor(rv).cuda(), torch.zeros((nray, rv.shape[1]), dtype=torch.float64, device="cuda")
        d_np = torch.as_tensor(npts).cuda()
    else:
        from rays_amd.trace import DeviceTrace, RaysRun

        run = RaysRun.from_namelist(os.path.join(ROOT, "configs", which + ".in"))
        p = run.params
        tr = DeviceTrace(p, run.rvec0, run.rindex_vec0)
        tr.launch()
        torch.cuda.synchronize()
        nray, d_rv, d_res, d_np = tr.nray, tr.ray_vec, tr.residual, tr.npoints
    stream = torch.cuda.current_stream().cuda_stream
    out = {f: torch.empty((nray, w) if w > 1 else (nray,), dtype=torch.int32 if dt is np.int32 else torch.float64, device="cuda")
           for f, dt, w in hip.OX_FIELDS}
    ptrs = {f: t.data_ptr() for f, t in out.items()}
    off = torch.empty(nray + 1, dtype=torch.int64, device="cuda")
    hip.point_offsets_device(nray, p.nstep_max, d_np.data_ptr(), off.data_ptr(), stream)
    total = int(off[-1].item())
    alpha = torch.empty((1, total), dtype=torch.float64, device="cuda")
    bad = torch.empty(nray, dtype=torch.int32, device="cuda")
    host = torch.empty(total, dtype=torch.float64).pin_memory()

    def ox_conv():
        hip.ox_conv_device(p, nray, d_rv.data_ptr(), d_np.data_ptr(), ptrs, stream=stream)

    def alpha_download():
        hip.ray_diagnostics_packed_device(p, nray, d_rv.data_ptr(), d_res.data_ptr(), d_np.data_ptr(), off.data_ptr(), total,
                                          ("alpha_e",), alpha.data_ptr(), bad.data_ptr(), stream)
        host.copy_(alpha[0], non_blocking=True)

    variants = {"ox_conv": ox_conv, "alpha_download": alpha_download}
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
    status, step = out["status"].cpu().numpy(), out["step_number"].cpu().numpy().astype(np.int64)
    npts = d_np.cpu().numpy().astype(np.int64)
    found = (status & hip.OX_FOUND_MAX) != 0
    visited = np.where(found, np.minimum(((step + 1 + 63) // 64) * 64, npts), npts)
    res = dict(workload=which, nray=int(nray), nv=int(p.nv), nstep_max=int(p.nstep_max), recorded_points=int(npts.sum()),
               rays_with_maximum=int(found.sum()), rays_with_cutoff=int(((status & hip.OX_FOUND_CUTOFF) != 0).sum()),
               rays_converted=int(((status & hip.OX_CONVERTED) != 0).sum()),
               rays_refused=int(((status & hip.OX_EQ_REFUSED) != 0).sum()), points_the_scan_visits=int(visited.sum()),
               alpha_download_bytes=8 * total, reps=reps, kernel=hip.ox_conv_kernel_name(p))
    for k, t in times.items():
        t = np.sort(np.array(t))
        res[k + "_ms"] = dict(median=float(np.median(t)), min=float(t[0]), max=float(t[-1]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05", "measurements", "ox_conv.json"))
    ap.add_argument("--one", default=None, help="(child) run this workload in this process")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per workload")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.reps, a.warmup)))
        return 0
    results = []
    for w in WORKLOADS:
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", w,
                            "--reps", str(a.reps), "--warmup", str(a.warmup)], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"ox_conv_bench: {w} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
