"""Fused `ray_scan`: the reference's scan driver re-initialises and calls
`trace_rays` once per scan value, serially (RAYS_project/ray_scan/ray_scan.f90:33-49, scanner_m.f90:
100-205; the scanned parameter is the step size `ds`).  A scan is just more independent rays: here
ALL runs go out as ONE launch of the trace kernel over n_runs x nray rays (rays_hip_scan_device): ray
i belongs to run i // nray, which sets its step `ds`; the persistent waves and their refill counter
treat the lot as one fan, so small fans (a 1024-ray fan occupies 16 of the GPU's 1024 SIMDs) fill the
machine together and 64 runs of a 1024-ray fan cost about one 64k-ray pass.  Results per run are
exactly those of a stand-alone trace.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from .params import ConfigError, RaysParams, copy_params

from .trace import (DeviceTrace, RayDeposition, RayResults, RaySummaries, _is_profile_list, _profile_list,
                    deposition_grid_limits)


def scan_values(scan_algorithm: str, n_runs: int, p_start: float = 0.0, p_incr: float = 0.0, p_max: float = 0.0,
                max_divide: int = 0, S_max: float = 0.0, n_max: int = 0, k_factor: int = 0,
                delta: float = float(np.float32(1.0e-14))) -> np.ndarray:  # scanner_m.f90:39 (single literal)
    """p_values(1:n_runs) of scanner_m.f90:115-160 (the algorithms that scan a real parameter)."""
    i = np.arange(1, n_runs + 1, dtype=np.float64)
    a = scan_algorithm.strip()
    if a == "fixed_increment":
        return p_start + (i - 1.0) * p_incr
    if a == "pwr_of_2":
        return p_max / np.float32(2.0) ** (n_runs - i) - delta
    if a == "integer_divide":
        return p_max / (max_divide - i + 1.0)
    if a == "algorithm_1":
        return S_max / (n_max + k_factor * (n_runs - i)) - delta
    raise ConfigError(f"initialize_scanner_m: unknown scan algorithm = {scan_algorithm!r}")


class RayScan:
    """All runs of a `ds` scan in one launch; outputs carry a leading run dimension.
    trajectories=False: summary-only (rays_hip_scan_summary_device) -- what scanner_m's aggregate_run_data keeps of a
    run, no trajectory tensor; results() returns one RaySummaries per run.
    trajectories=False, deposition=[(which, n_bins), ...] | "all" (with n_bins=n), ray_power=w: the fused ds scan
    (rays_hip_scan_profiles_device) -- every run binned into one or two deposition profiles while it is traced, still one
    launch and no trajectory.  ray_power: one weight per fan member.  .works[k] is [n_bins][n_runs * nray] (run r owns
    the columns r * nray ..), .profiles[k] and profile_in[k] (a tensor or None per profile) are [n_runs][n_bins].
    results() returns per run what DeviceTrace(..., trajectories=False, deposition=[...]) returns for that run alone: a
    list of RayDeposition sharing the run's RaySummaries."""

    def __init__(self, params: RaysParams, rvec0, rindex_vec0, ds_values: Sequence[float],
                 scan_parameter: str = "ds", device=None, trajectories: bool = True, deposition=None, ray_power=None,
                 profile_in=None, n_bins=None):
        import torch

        from . import hip

        if scan_parameter.strip() != "ds":  # scanner_m.f90:185-201 ('*_num_threads' has no meaning here)
            raise ConfigError(f"initialize_scanner_m: unknown scan parameter = {scan_parameter!r}")
        self.deposition = None
        if deposition is not None:
            if trajectories:
                raise ValueError("RayScan: deposition=... is the fused scan without trajectories -- pass "
                                 "trajectories=False (or bin the trajectories of a recording scan with "
                                 "hip.deposition_device and hip.profile_sum_segments)")
            if not _is_profile_list(deposition):
                raise ValueError('RayScan: deposition=[(which, n_bins), ...] or "all" (with n_bins=n)')
            self.deposition = _profile_list(params, deposition, n_bins, "RayScan")
            if ray_power is None or len(ray_power) != len(rvec0):
                raise ValueError("RayScan: deposition=[...] needs ray_power= with one weight per fan member")
            if profile_in is not None and (not isinstance(profile_in, (list, tuple)) or len(profile_in) != len(self.deposition)):
                raise ValueError("RayScan: profile_in is a list with one entry (a tensor [n_runs][n_bins] or None) per "
                                 "profile")
        elif ray_power is not None or profile_in is not None or n_bins is not None:
            raise ValueError("RayScan: ray_power= / profile_in= / n_bins= go with deposition=...")
        self.profile_in = profile_in
        self.works = self.profiles = self.power = None
        self.torch, self.hip = torch, hip
        self.params = params
        hip.check_params(params)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.ds_values = np.ascontiguousarray(ds_values, dtype=np.float64)
        self.n_runs, self.nray = len(self.ds_values), len(rvec0)
        nv, npt = params.nv, params.nstep_max + 1
        f64, i32 = torch.float64, torch.int32
        R, N = self.n_runs, self.nray
        self.trajectories = bool(trajectories)
        self.ray_vec = self.residual = self.start_ray_vec = None
        with torch.cuda.device(self.device):
            self.ds = torch.as_tensor(self.ds_values).to(self.device)
            self.rvec0 = torch.as_tensor(np.ascontiguousarray(rvec0), dtype=f64).to(self.device)
            self.rindex_vec0 = torch.as_tensor(np.ascontiguousarray(rindex_vec0), dtype=f64).to(self.device)
            if self.trajectories:
                self.ray_vec = torch.zeros((R, N, npt, nv), dtype=f64, device=self.device)
                self.residual = torch.zeros((R, N, npt), dtype=f64, device=self.device)
            else:
                self.start_ray_vec = torch.zeros((R, N, nv), dtype=f64, device=self.device)
            self.npoints = torch.zeros((R, N), dtype=i32, device=self.device)
            self.stop_code = torch.zeros((R, N), dtype=i32, device=self.device)
            self.end_ray_vec = torch.zeros((R, N, nv), dtype=f64, device=self.device)
            self.end_residuals = torch.zeros((R, N), dtype=f64, device=self.device)
            self.max_residuals = torch.zeros((R, N), dtype=f64, device=self.device)
            if self.deposition is not None:
                pw = ray_power
                self.power = (pw.to(device=self.device, dtype=f64).contiguous() if torch.is_tensor(pw)
                              else torch.as_tensor(np.ascontiguousarray(pw, dtype=np.float64)).to(self.device))
                self.works = [torch.zeros((nb, R * N), dtype=f64, device=self.device) for _, nb in self.deposition]
                self.profiles = [torch.zeros((R, nb), dtype=f64, device=self.device) for _, nb in self.deposition]

    def launch(self, zero_fill: bool = True):
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        if self.deposition is not None:
            pin = self.profile_in or [None] * len(self.deposition)
            records = [(w, nb, work.data_ptr(), None if c is None else c.data_ptr(), prof.data_ptr())
                       for (w, nb), work, c, prof in zip(self.deposition, self.works, pin, self.profiles)]
            self.hip.scan_profiles_device(self.params, self.n_runs, self.ds.data_ptr(), self.nray, self.rvec0.data_ptr(),
                                          self.rindex_vec0.data_ptr(), self.power.data_ptr(), records,
                                          self.npoints.data_ptr(), self.stop_code.data_ptr(), self.start_ray_vec.data_ptr(),
                                          self.end_ray_vec.data_ptr(), self.end_residuals.data_ptr(),
                                          self.max_residuals.data_ptr(), stream=stream)
            return
        if not self.trajectories:
            self.hip.scan_summary_device(self.params, self.n_runs, self.ds.data_ptr(), self.nray, self.rvec0.data_ptr(),
                                         self.rindex_vec0.data_ptr(), self.npoints.data_ptr(), self.stop_code.data_ptr(),
                                         self.start_ray_vec.data_ptr(), self.end_ray_vec.data_ptr(),
                                         self.end_residuals.data_ptr(), self.max_residuals.data_ptr(), stream=stream)
            return
        self.hip.scan_device(self.params, self.n_runs, self.ds.data_ptr(), self.nray, self.rvec0.data_ptr(),
                             self.rindex_vec0.data_ptr(), self.ray_vec.data_ptr(), self.residual.data_ptr(),
                             self.npoints.data_ptr(), self.stop_code.data_ptr(), self.end_ray_vec.data_ptr(),
                             self.end_residuals.data_ptr(), self.max_residuals.data_ptr(), stream=stream,
                             zero_fill=zero_fill)

    def synchronize(self):
        self.torch.cuda.synchronize(self.device)

    def results(self):
        self.synchronize()
        c = lambda x: x.cpu().numpy()
        if not self.trajectories:
            arrays = [c(a) for a in (self.npoints, self.stop_code, self.start_ray_vec, self.end_ray_vec,
                                     self.end_residuals, self.max_residuals)]
            summ = [RaySummaries(*(a[r] for a in arrays)) for r in range(self.n_runs)]
            if self.deposition is None:
                return summ
            N = self.nray
            works, profs = [c(w) for w in self.works], [c(q) for q in self.profiles]
            return [[RayDeposition(summ[r], w, nb, *deposition_grid_limits(self.params, w), prof[r],
                                   np.ascontiguousarray(work[:, r * N:(r + 1) * N].T))
                     for (w, nb), work, prof in zip(self.deposition, works, profs)] for r in range(self.n_runs)]
        arrays = [c(a) for a in (self.ray_vec, self.residual, self.npoints, self.stop_code, self.end_ray_vec,
                                 self.end_residuals, self.max_residuals)]
        return [RayResults(*(a[r] for a in arrays)) for r in range(self.n_runs)]
