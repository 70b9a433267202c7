"""Full-fan numerics survey of a trace kernel against the CPU oracle (test infrastructure; used by
tests/test_gpu_numerics_full_fans.py and tools/numerics_evidence.py).

Two measurements per fan, both against the oracle's trajectories (bit-identical to the reference CPU path):

  * per step: the HIP path restarted from EVERY recorded oracle point of the selected rays for one output step
    (`rays_hip_ode_step_device` = ode_solver + check_save), norm-wise relative error on r and k of the point it
    lands on against the oracle's next point (north_star: "within 1e-10 relative per step");
  * pointwise: the fan traced as a whole by the kernel the configuration dispatches, every recorded point against the
    oracle's point with the same index (accumulated deviation along the ray), and npoints / stop codes of every ray.

A third one looks at the traced fan alone (`own_step_errors`, survey(own_step=True)):

  * own step: the ORACLE's one output step (`oracle_lib.step` = the reference's RK4_ode + check_save) from the traced
    result's own point k against the traced result's point k + 1, for every recorded k of every ray -- what the
    persistent trace loop itself did on each of its steps (its stage state machine, the fused check_save, the record path
    and the hand-over to the resume kernel are another compilation context than the step kernel's), and whether the
    reference, standing on the kernel's last recorded point, ends the ray there with the same stop flag.

`restart` says what the arithmetic does on the reference's points, `own` what the benchmarked loop did on its own.

The oracle runs in chunks of rays (its padded arrays are nray x (nstep_max + 1) x nv doubles)."""
from __future__ import annotations

import numpy as np

from rays_amd import hip
from tests import oracle_lib

THRESHOLDS = (1e-10, 1e-11, 1e-12)
# stop codes that trace_rays decides between two steps ('sout > s_max', ' nstep > nstep_max': ray_tracing.f90:128-172)
OUTSIDE_THE_STEP = (1, 2)


def _rel(a, b, sl):
    num = np.linalg.norm(a[:, sl] - b[:, sl], axis=-1)
    den = np.linalg.norm(b[:, sl], axis=-1)
    out = np.zeros(len(a))
    m = den > 0
    out[m] = num[m] / den[m]
    return out


def s_of_point(p, n):
    """s of recorded point k = 0..n as trace_rays accumulates it: sout = sout + ds, k times (ray_tracing.f90:118-121)."""
    return np.concatenate([[0.0], np.cumsum(np.full(n, float(p.ds)))])


def own_step_errors(p, ray_vec, npoints, stop_code, residual=None, nthreads=0):
    """A traced result judged on its own steps (pure numpy + the CPU oracle; no GPU): for every ray and every recorded
    k < npoints - 1 the oracle's output step from ray_vec[ray, k] (at s = k running sums of ds) against
    ray_vec[ray, k + 1].  ray_vec[nray][>= max npoints][nv], residual[nray][>= max npoints] (optional).  RK4 only.

    Per step (arrays `ray`, `point`, `err`, one entry per step, ray-major): err = max of the norm-wise relative errors
    on r and on k (`_rel`); a mid-ray step the oracle comes back `stopped` from -- the kernel recorded a point the
    reference would not have -- is counted in `midray_stops` (listed in `midray_stop_steps`) and carries err = inf.
    Rows >= 6 by the rule of test_gpu_tolerance_flavour.test_per_step_within_1e10_of_the_reference: largest absolute
    difference of the row and the row's largest magnitude (`row_max_abs`, `row_scale`, to be combined over chunks;
    `max_other_rows` = their largest quotient over the rows held to 1e-10, `max_damping_row` the quotient of row 7 under
    damping, which the reference carries through single-precision COMPLEX and is held to 1e-6).
    `max_resid_diff`: largest |oracle residual - recorded residual| of the points landed on.
    Last point of each ray: the oracle's step from it must stop with the ray's stop code.  Judged for rays that end
    inside a step and took at least one (`terminal_judged`); not judged: 'sout > s_max' / ' nstep > nstep_max', decided
    between steps, and rays that never started (npoints = 1: stopped by the check_save of the launch point).
    `terminal_disagree` counts the others, `terminal_disagreements` lists (ray, npoints, code, oracle code, stopped)."""
    npts = np.asarray(npoints).astype(np.int64)
    codes = np.asarray(stop_code)
    nray, nv = len(npts), int(p.nv)
    nmax = int(npts.max()) if nray else 0
    assert ray_vec.shape[0] == nray and ray_vec.shape[1] >= nmax and ray_vec.shape[2] == nv
    s_tab = s_of_point(p, max(nmax, 1))
    damp = bool(p.damping_model)
    out = dict(steps=0, max_per_step=0.0, max_per_step_r=0.0, max_per_step_k=0.0, midray_stops=0, midray_stop_steps=[],
               row_max_abs=np.zeros(nv), row_scale=np.zeros(nv), max_other_rows=0.0, max_damping_row=0.0,
               max_resid_diff=0.0, ray=np.zeros(0, dtype=np.int64), point=np.zeros(0, dtype=np.int64), err=np.zeros(0),
               terminal_judged=0, terminal_disagree=0, terminal_disagreements=[])
    # ---- every recorded step ----
    cnt = np.maximum(npts - 1, 0)
    if cnt.sum():
        first = np.arange(nmax - 1)[None, :] < cnt[:, None]          # [ray][k]: point k has a successor
        kk = np.broadcast_to(np.arange(nmax - 1)[None, :], first.shape)[first]
        rr = np.broadcast_to(np.arange(nray)[:, None], first.shape)[first]
        got = ray_vec[:, 1:nmax][first]
        v1, resid, code, stopped = oracle_lib.step(p, ray_vec[:, :nmax - 1][first], s_tab[kk], nthreads=nthreads)
        er, ek = _rel(got, v1, slice(0, 3)), _rel(got, v1, slice(3, 6))
        bad = ~(np.isfinite(er) & np.isfinite(ek))                   # a NaN in either point is not "within" anything
        er[bad | stopped] = np.inf
        ek[bad | stopped] = np.inf
        err = np.maximum(er, ek)
        ok = ~stopped
        out.update(steps=int(len(err)), ray=rr, point=kk, err=err, midray_stops=int(stopped.sum()),
                   midray_stop_steps=[(int(rr[i]), int(kk[i]), int(code[i])) for i in np.flatnonzero(stopped)[:16]])
        if ok.any():
            out.update(max_per_step=float(err[ok].max()), max_per_step_r=float(er[ok].max()), max_per_step_k=float(ek[ok].max()))
            out["row_max_abs"][6:] = np.abs(v1[ok][:, 6:] - got[ok][:, 6:]).max(axis=0)
            out["row_scale"][6:] = np.abs(got[ok][:, 6:]).max(axis=0)
            if residual is not None:
                out["max_resid_diff"] = float(np.abs(resid[ok] - residual[:, 1:nmax][first][ok]).max())
        out["max_other_rows"], out["max_damping_row"] = rows_rule(out["row_max_abs"], out["row_scale"], damp)
    # ---- each ray's last recorded point ----
    judged = np.flatnonzero(~np.isin(codes, OUTSIDE_THE_STEP) & (npts >= 2))
    if len(judged):
        last = npts[judged] - 1
        _, _, code, stopped = oracle_lib.step(p, ray_vec[judged, last], s_tab[last], nthreads=nthreads)
        wrong = ~stopped | (code != codes[judged])
        out.update(terminal_judged=int(len(judged)), terminal_disagree=int(wrong.sum()),
                   terminal_disagreements=[(int(judged[i]), int(npts[judged[i]]), int(codes[judged[i]]), int(code[i]), bool(stopped[i]))
                                           for i in np.flatnonzero(wrong)[:16]])
    return out


def rows_rule(row_max_abs, row_scale, damp):
    """(largest quotient over the rows >= 6 held to 1e-10, quotient of the absorbed-power row held to 1e-6)"""
    q = np.asarray(row_max_abs) / np.maximum(np.asarray(row_scale), 1e-300)
    other = [float(q[c]) for c in range(6, len(q)) if not (damp and c == 7)]
    return (max(other) if other else 0.0), (float(q[7]) if damp and len(q) > 7 else 0.0)


def survey(p, r0, n0, ray_stride=1, chunk_rays=4096, restart_batch=65536, n_worst=8, progress=None, per_step=True,
           own_step=False, own_ray_stride=1):
    """Returns a dict of plain numbers (JSON-ready).  `restart_batch`: states per `ode_step` call -- below two waves per
    SIMD worth of states the one-wave-per-SIMD build of the kernel serves the call, from 131072 on the two-waves build:
    pick the one the fan itself dispatches (`hip.kernel_name(p, len(r0))`).  per_step=False: the pointwise comparison and
    the counts only (Shampine-Gordon fans: an output step there is a whole restarted integration whose tolerances the ray
    carries along, so a restart from a recorded point is not the reference's next step).
    own_step=True: `own_step_errors` on the fan just traced (every `own_ray_stride`-th of the surveyed rays), reported as
    own_steps, own_max_per_step, own_n_above_<threshold>, own_midray_stops, own_terminal_judged / _disagree,
    own_max_other_rows, own_max_damping_row, own_max_resid_diff, own_worst_steps.  The oracle runs with OpenMP's own
    thread count (OMP_NUM_THREADS is honoured)."""
    import torch
    from rays_amd.trace import DeviceTrace

    nthreads = 0
    sel = np.arange(0, len(r0), ray_stride)
    kernel = hip.kernel_name(p, len(r0))
    step_kernel = hip.kernel_name(p, restart_batch)
    tr = DeviceTrace(p, r0, n0)
    tr.launch()
    torch.cuda.synchronize()
    d_npts, d_codes = tr.npoints.cpu().numpy(), tr.stop_code.cpu().numpy()
    ds = float(p.ds)
    st = dict(steps_restarted=0, restarts_stopped=0, max_per_step=0.0, max_per_step_r=0.0, max_per_step_k=0.0,
              points_compared=0, points_not_identical=0, max_pointwise=0.0, rays_with_other_counts=0, rays_surveyed=int(len(sel)))
    n_step_above = {t: 0 for t in THRESHOLDS}
    n_point_above = {t: 0 for t in THRESHOLDS}
    worst = []   # (err, ray, point, npoints)
    med = []
    own = dict(steps=0, max_per_step=0.0, midray_stops=0, terminal_judged=0, terminal_disagree=0, max_resid_diff=0.0,
               row_max_abs=np.zeros(p.nv), row_scale=np.zeros(p.nv), rays=0)
    own_above = {t: 0 for t in THRESHOLDS}
    own_worst, own_stops, own_terminals = [], [], []
    for c0 in range(0, len(sel), chunk_rays):
        rays = sel[c0:c0 + chunk_rays]
        ora = oracle_lib.trace(p, r0[rays], n0[rays], nthreads=nthreads)
        npts = ora["npoints"].astype(np.int64)
        st["rays_with_other_counts"] += int(((d_npts[rays] != ora["npoints"]) | (d_codes[rays] != ora["stop_code"])).sum())
        # ---- pointwise: the traced fan against the oracle, point by point ----
        idx = torch.as_tensor(rays, device=tr.ray_vec.device)
        nmax = int(max(npts.max(), d_npts[rays].max()))
        got = tr.ray_vec.index_select(0, idx)[:, :nmax].cpu().numpy()
        ref = ora["ray_vec"][:, :nmax]
        live = np.arange(nmax)[None, :] < np.minimum(npts, d_npts[rays])[:, None]
        g2, r2 = got[live], ref[live]
        pe = np.maximum(_rel(g2, r2, slice(0, 3)), _rel(g2, r2, slice(3, 6)))
        st["points_compared"] += int(len(pe))
        st["points_not_identical"] += int(((g2 != r2) & ~(np.isnan(g2) & np.isnan(r2))).any(axis=-1).sum())  # all nv components
        if len(pe):
            st["max_pointwise"] = max(st["max_pointwise"], float(pe.max()))
            for t in THRESHOLDS:
                n_point_above[t] += int((pe > t).sum())
        if own_step:
            # ---- own step: the oracle's step from the traced fan's own points ----
            orays = np.arange(0, len(rays), own_ray_stride)
            got_res = tr.residual.index_select(0, idx)[:, :nmax].cpu().numpy()
            o = own_step_errors(p, got[orays], d_npts[rays][orays], d_codes[rays][orays], got_res[orays], nthreads=nthreads)
            own["rays"] += int(len(orays))
            for k in ("steps", "midray_stops", "terminal_judged", "terminal_disagree"):
                own[k] += o[k]
            for k in ("max_per_step", "max_resid_diff"):
                own[k] = max(own[k], o[k])
            for k in ("row_max_abs", "row_scale"):
                own[k] = np.maximum(own[k], o[k])
            for t in THRESHOLDS:
                own_above[t] += int((o["err"] > t).sum())        # (inf: a mid-ray stop or a NaN point -- above every bar)
            top = np.argsort(-o["err"])[:n_worst]
            own_worst += [(float(o["err"][i]), int(rays[orays[o["ray"][i]]]), int(o["point"][i]),
                           int(d_npts[rays[orays[o["ray"][i]]]])) for i in top]
            own_worst = sorted(own_worst, reverse=True)[:n_worst]
            own_stops += [(int(rays[orays[r]]), k, c) for r, k, c in o["midray_stop_steps"]]
            own_terminals += [(int(rays[orays[r]]),) + tuple(rest) for r, *rest in o["terminal_disagreements"]]
            del got_res, o
        del got, g2, r2
        if not per_step:
            if progress:
                progress(f"  rays {rays[0]}..{rays[-1]}: {st['points_compared']} points so far, max pointwise {st['max_pointwise']:.3e}")
            continue
        # ---- per step: one-step restarts from every oracle point ----
        has = npts >= 2
        cnt = np.where(has, npts - 1, 0)
        tot = int(cnt.sum())
        if tot == 0:
            continue
        first = np.arange(nmax - 1)[None, :] < cnt[:, None]          # [ray][k]: point k has a successor
        v0 = ora["ray_vec"][:, :nmax - 1][first]
        v1 = ora["ray_vec"][:, 1:nmax][first]
        kk = np.broadcast_to(np.arange(nmax - 1)[None, :], first.shape)[first]
        rr = np.broadcast_to(rays[:, None], first.shape)[first]
        # s of point k as trace_rays accumulates it: sout = sout + ds, k times (ray_tracing.f90:118-121)
        s_tab = np.concatenate([[0.0], np.cumsum(np.full(nmax, ds))])
        s0 = s_tab[kk]
        err = np.empty(tot)
        for b0 in range(0, tot, restart_batch):
            b1 = min(tot, b0 + restart_batch)
            g, _, code = hip.ode_step(p, v0[b0:b1], s0[b0:b1])
            ok = code == 0
            st["restarts_stopped"] += int((~ok).sum())
            er, ek = _rel(g, v1[b0:b1], slice(0, 3)), _rel(g, v1[b0:b1], slice(3, 6))
            er[~ok] = 0.0
            ek[~ok] = 0.0
            st["max_per_step_r"] = max(st["max_per_step_r"], float(er.max()))
            st["max_per_step_k"] = max(st["max_per_step_k"], float(ek.max()))
            err[b0:b1] = np.maximum(er, ek)
        st["steps_restarted"] += tot
        st["max_per_step"] = max(st["max_per_step"], float(err.max()))
        for t in THRESHOLDS:
            n_step_above[t] += int((err > t).sum())
        med.append(float(np.median(err)))
        top = np.argsort(-err)[:n_worst]
        nn = npts[np.searchsorted(rays, rr[top])]
        worst += [(float(err[i]), int(rr[i]), int(kk[i]), int(n)) for i, n in zip(top, nn)]
        worst = sorted(worst, reverse=True)[:n_worst]
        if progress:
            progress(f"  rays {rays[0]}..{rays[-1]}: {st['steps_restarted']} restarts so far, max per step {st['max_per_step']:.3e}, "
                     f"max pointwise {st['max_pointwise']:.3e}")
    del tr
    torch.cuda.empty_cache()
    out = dict(st)
    out.update(kernel=kernel, restart_kernel=step_kernel, ray_stride=int(ray_stride), rays_total=int(len(r0)),
               median_per_step=float(np.median(med)) if med else 0.0,
               worst_steps=[dict(rel_err=e, ray=r, point=k, npoints=n) for e, r, k, n in worst])
    if own_step:
        other, damping = rows_rule(own["row_max_abs"], own["row_scale"], bool(p.damping_model))
        out.update(own_steps=own["steps"], own_rays=own["rays"], own_ray_stride=int(own_ray_stride),
                   own_max_per_step=own["max_per_step"], own_midray_stops=own["midray_stops"],
                   own_terminal_judged=own["terminal_judged"], own_terminal_disagree=own["terminal_disagree"],
                   own_max_other_rows=other, own_max_damping_row=damping, own_max_resid_diff=own["max_resid_diff"],
                   own_worst_steps=[dict(rel_err=e, ray=r, point=k, npoints=n) for e, r, k, n in own_worst],
                   own_midray_stop_steps=[dict(ray=r, point=k, oracle_code=c) for r, k, c in own_stops[:16]],
                   own_terminal_disagreements=[dict(ray=r, npoints=n, code=c, oracle_code=oc, oracle_stopped=s)
                                               for r, n, c, oc, s in own_terminals[:16]])
        for t in THRESHOLDS:
            out[f"own_n_above_{t:g}"] = own_above[t]
    for t in THRESHOLDS:
        out[f"n_above_{t:g}"] = n_step_above[t]
        out[f"points_above_{t:g}"] = n_point_above[t]
    out["frac_points_above_1e-10"] = n_point_above[1e-10] / max(1, st["points_compared"])
    return out
