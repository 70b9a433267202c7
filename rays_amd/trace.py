"""Host-side mirror of the reference's run contract for the hot path:

    call initialize(read_input)   ->  RaysRun.from_namelist(path)      (module state)
    call trace_rays               ->  run.trace_rays()                 (the HIP path)
    ray_results_m arrays          ->  RayResults

(RAYS_project/RAYS_code/RAYS.f90:10-16, RAYS_lib/ray_results_m.f90:44-58.)  PyTorch is used only
as plumbing for device memory / streams / torch.distributed; the computation is
librays_hip.so through the C ABI.
"""
from __future__ import annotations

import dataclasses
from typing import Any, Dict, Optional

import numpy as np

from . import hip
from .namelist import read_namelist
from .params import RaysParams, params_from_namelist
from .ray_init import initialize_ray_init


@dataclasses.dataclass
class RayResults:
    """Image of the ray_results_m module arrays (ray_results_m.f90:44-58), C order."""

    ray_vec: np.ndarray          # [nray][nstep_max+1][nv]
    residual: np.ndarray         # [nray][nstep_max+1]
    npoints: np.ndarray          # [nray]
    stop_code: np.ndarray        # [nray]   integer image of ray_stop_flag
    end_ray_vec: np.ndarray      # [nray][nv]
    end_residuals: np.ndarray    # [nray]
    max_residuals: np.ndarray    # [nray]
    elapsed_s: float = 0.0

    @property
    def ray_stop_flag(self):
        return [hip.stop_flag_text(int(c)) for c in self.stop_code]

    @property
    def start_ray_vec(self):      # ray_tracing.f90:259
        return self.ray_vec[:, 0, :]

    @property
    def end_ray_parameter(self):  # ray_tracing.f90:257
        return self.end_ray_vec[:, 6]

    @property
    def total_steps(self) -> int:
        return int(np.maximum(self.npoints.astype(np.int64) - 1, 0).sum())

    def diagnostics(self, params: RaysParams, fields=None, packed: bool = False) -> Dict[str, np.ndarray]:
        """The post-processors' ray_detailed_diagnostics (axisym_toroid_processor_m.f90:252-482) of these host arrays,
        evaluated on the GPU (hip.ray_diagnostics_host): {field name: array[nray][nstep_max+1]} for `fields`
        (hip.DIAG_FIELDS; None = all), plus "first_bad_point"[nray] (include/rays_hip.h).  `params`: the run's
        parameter block (a RayResults does not hold it).
        packed=True: {field name: array[sum(npoints)]}, the recorded points alone, rays in order, plus "offsets"
        (int64[nray + 1], hip.diag_offsets) and "first_bad_point" -- the packed device entry on the packed arrays
        (hip.ray_diagnostics_packed_device, one upload of the recorded points, no blocks)."""
        if packed:
            return self._diagnostics_packed(params, fields)
        out, bad = hip.ray_diagnostics_host(params, self.ray_vec, self.residual, self.npoints, fields)
        out["first_bad_point"] = bad
        return out

    def ox_conversion(self, params: RaysParams):
        """The post-processors' analyze_OX_conv (post_process_lib/OX_conv_analysis_m.f90:91-198) of these host arrays,
        evaluated on the GPU (hip.ox_conv_host): a results.OXConversion with one entry per ray in every array and the
        reference's compacted list of converted rays.  conv_coeff is the host libm's: bit-identical to the reference."""
        from .results import OXConversion

        return OXConversion.from_fields(hip.ox_conv_host(params, self.ray_vec, self.npoints))

    def _diagnostics_packed(self, params: RaysParams, fields) -> Dict[str, np.ndarray]:
        import torch

        _, names = hip.diag_field_mask(fields)
        nray, npt = len(self.npoints), params.nstep_max + 1
        if self.ray_vec.shape != (nray, npt, params.nv) or self.residual.shape != (nray, npt):
            raise ValueError("RayResults.diagnostics: arrays do not have the ray_results_m shapes of this run")
        off = hip.diag_offsets(self.npoints, params.nstep_max)
        total = int(off[-1])
        live = np.arange(npt)[None, :] < np.diff(off)[:, None]
        d_rv = torch.as_tensor(np.ascontiguousarray(self.ray_vec[live])).cuda()
        d_res = torch.as_tensor(np.ascontiguousarray(self.residual[live])).cuda()
        d_np = torch.as_tensor(np.ascontiguousarray(self.npoints, dtype=np.int32)).cuda()
        d_off = torch.empty(nray + 1, dtype=torch.int64, device="cuda")
        out = torch.empty((len(names), total), dtype=torch.float64, device="cuda")
        bad = torch.empty(nray, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        hip.point_offsets_device(nray, params.nstep_max, d_np.data_ptr(), d_off.data_ptr(), stream)
        if total:
            hip.ray_diagnostics_packed_device(params, nray, d_rv.data_ptr(), d_res.data_ptr(), d_np.data_ptr(),
                                              d_off.data_ptr(), total, names, out.data_ptr(), bad.data_ptr(), stream,
                                              packed_input=True)
        else:   # no recorded point: the arrays are empty, and the entry refuses their null pointers
            bad.zero_()
        h = out.cpu().numpy()
        res: Dict[str, np.ndarray] = {n: h[k] for k, n in enumerate(names)}
        res["offsets"] = d_off.cpu().numpy()
        res["first_bad_point"] = bad.cpu().numpy()
        return res


@dataclasses.dataclass
class RaySummaries:
    """What a summary-only trace keeps of every ray (rays_hip_trace_summary*): the per-ray rows of ray_results_m
    without ray_vec(:,:,:) and residual(:,:) -- the six things the reference's ray_scan aggregates per run
    (scanner_m.f90:213-227).  Always from the exact kernels (include/rays_hip.h)."""

    npoints: np.ndarray          # [nray]
    stop_code: np.ndarray        # [nray]   integer image of ray_stop_flag
    start_ray_vec: np.ndarray    # [nray][nv]   ray_vec(:, 1, iray)
    end_ray_vec: np.ndarray      # [nray][nv]
    end_residuals: np.ndarray    # [nray]
    max_residuals: np.ndarray    # [nray]
    elapsed_s: float = 0.0

    @property
    def ray_stop_flag(self):
        return [hip.stop_flag_text(int(c)) for c in self.stop_code]

    @property
    def end_ray_parameter(self):  # ray_tracing.f90:257
        return self.end_ray_vec[:, 6]

    @property
    def total_steps(self) -> int:
        return int(np.maximum(self.npoints.astype(np.int64) - 1, 0).sum())


class RayState:
    """The saved ray state of windowed tracing (include/rays_hip.h: rays_ray_state_t) as torch tensors: everything a
    fan needs to go on after a window -- v[nray][nv], s[nray], nstep[nray], stop_code[nray], resid[nray][3],
    sg_err[nray][2], flags[nray].  Nothing in it is an address or depends on a launch: save() / load() take it to an
    npz file and back, onto any device."""

    FIELDS = (("v", "float64"), ("s", "float64"), ("nstep", "int32"), ("stop_code", "int32"), ("resid", "float64"),
              ("sg_err", "float64"), ("flags", "int32"))

    def __init__(self, nray: int, nv: int, device=None):
        import torch

        self.nray, self.nv = int(nray), int(nv)
        shapes = dict(v=(nray, nv), s=(nray,), nstep=(nray,), stop_code=(nray,), resid=(nray, 3), sg_err=(nray, 2),
                      flags=(nray,))
        for name, dt in self.FIELDS:
            setattr(self, name, torch.zeros(shapes[name], dtype=getattr(torch, dt), device=device))

    @property
    def device(self):
        return self.v.device

    def numpy(self) -> Dict[str, np.ndarray]:
        return {name: getattr(self, name).cpu().numpy() for name, _ in self.FIELDS}

    def save(self, path: str):
        """np.savez of the seven arrays (blocking: the tensors are copied to the host)."""
        np.savez(path, **self.numpy())

    @classmethod
    def load(cls, path: str, device=None) -> "RayState":
        """A state saved by save(), in fresh tensors on `device`."""
        import torch

        with np.load(path, allow_pickle=False) as z:
            nray, nv = z["v"].shape
            st = cls(nray, nv, device=device)
            for name, dt in cls.FIELDS:
                a = np.ascontiguousarray(z[name], dtype=dt)
                if a.shape != tuple(getattr(st, name).shape):
                    raise ValueError(f"RayState.load: {name} has shape {a.shape}")
                getattr(st, name).copy_(torch.as_tensor(a))
        return st

    @property
    def under_way(self) -> int:
        """Rays that have not ended (a synchronising copy)."""
        return int((self.stop_code == 0).sum().item())


@dataclasses.dataclass
class RayDeposition:
    """What a fused trace + deposition returns (rays_hip_trace_deposition*): the per-ray summaries and one deposition
    profile, binned while the rays were traced -- no trajectory exists.  `profile_record` is the dictionary
    results.write_deposition_profiles_LD / _NC take."""

    summaries: RaySummaries
    profile_name: str            # 'Ptotal_psi' | 'Ptotal_rho' | 'Ptotal_x'
    n_bins: int
    grid_min: float
    grid_max: float
    profile: np.ndarray          # [n_bins]   sum(work, 2) in ray order ([n_seg][n_bins] of a trace with segments=)
    work: Optional[np.ndarray]   # [nray][n_bins]  the reference's work(n_bins, nray); None if not asked for

    @property
    def Q_sum(self):             # the ordered sum of the profile (deposition_profiles_m.f90:251); one per segment
        if np.ndim(self.profile) == 2:
            return np.array([RayDeposition(self.summaries, self.profile_name, self.n_bins, self.grid_min, self.grid_max,
                                           row, None).Q_sum for row in self.profile], dtype=np.float64)
        q = 0.0
        for x in self.profile:
            q = q + float(x)
        return q

    @property
    def profile_record(self) -> Dict[str, Any]:
        from .results import deposition_grid
        return dict(profile_name=self.profile_name, grid_name=self.profile_name.split("_")[1], profile=self.profile,
                    grid=deposition_grid(self.grid_min, self.grid_max, self.n_bins), Q_sum=self.Q_sum,
                    n_bins=self.n_bins, grid_min=self.grid_min, grid_max=self.grid_max)


def deposition_grid_limits(params: RaysParams, which: str):
    """(grid_min, grid_max) of a deposition profile: the slab box in x for 'Ptotal_x' (deposition_profiles_m.f90:136-137),
    0..1 for psiN and rho (:176-177)."""
    if which == "Ptotal_x":
        return float(params.slab.xmin), float(params.slab.xmax)
    return 0.0, 1.0


def _deposition_spec(deposition, with_power: bool):
    """(which, n_bins[, power]) of a `deposition=` argument."""
    want = 3 if with_power else 2
    if not isinstance(deposition, (tuple, list)) or len(deposition) != want:
        raise ValueError("deposition=(which, n_bins, power)" if with_power else "deposition=(which, n_bins)")
    if deposition[0] not in hip.DEP_PROFILES:
        raise ValueError(f"deposition profile {deposition[0]!r}: known are {tuple(hip.DEP_PROFILES)}")
    return deposition


def _is_profile_list(deposition) -> bool:
    """deposition=[(which, n_bins), ...] or "all": the several-profiles spelling (one trace pass, rays_hip_trace_profiles*)."""
    if isinstance(deposition, str):
        return True
    return isinstance(deposition, list) and (not deposition or isinstance(deposition[0], (tuple, list)))


def _profile_list(params: RaysParams, deposition, n_bins, who: str):
    """[(which, n_bins), ...] of the several-profiles spelling, checked: one or two different profiles of the
    configuration's equilibrium.  "all" with n_bins=n: the equilibrium's whole set in the reference's order
    (hip.deposition_profile_set), n bins each."""
    if isinstance(deposition, str):
        if deposition != "all":
            raise ValueError(f'{who}: deposition={deposition!r}: a string can only be "all" (with n_bins=n)')
        if n_bins is None:
            raise ValueError(f'{who}: deposition="all" needs n_bins=n')
        names = hip.deposition_profile_set(params)
        if not names:
            raise ValueError(f'{who}: deposition="all": this equilibrium has no deposition profile')
        return [(w, int(n_bins)) for w in names]
    if n_bins is not None:
        raise ValueError(f'{who}: n_bins=... goes with deposition="all" only; a list carries its own bin counts')
    specs = []
    for d in deposition:
        if not isinstance(d, (tuple, list)) or len(d) != 2:
            raise ValueError(f"{who}: deposition=[(which, n_bins), ...] takes pairs; the powers go in "
                             "ray_power= (DeviceTrace) or come from ray_pwr_wt (RaysRun) -- the tuple and the list "
                             "spelling do not mix")
        which, nb = _deposition_spec(d, False)
        specs.append((which, int(nb)))
    if not 1 <= len(specs) <= hip.DEP_MAX_PROFILES:
        raise ValueError(f"{who}: deposition=[...] takes 1..{hip.DEP_MAX_PROFILES} profiles, not {len(specs)}")
    if len({w for w, _ in specs}) != len(specs):
        raise ValueError(f"{who}: deposition=[...] names the profile {specs[0][0]!r} twice")
    slab = int(params.equilib_model) == 0
    for w, _ in specs:
        if (w == "Ptotal_x") != slab:
            raise ValueError(f"{who}: deposition profile {w!r} does not exist for this equilib_model (slab: Ptotal_x; "
                             "axisym_toroid: Ptotal_psi, Ptotal_rho)")
    return specs


def check_segments(segments, nray: int, who: str):
    """A `segments=` argument: (n_seg, offsets or None, rays_per_seg).  A host sequence of offsets is checked here --
    non-decreasing, within 0..nray -- and returned as an int32 array; an int k means uniform segments of k rays, the last
    one as long as the fan allows; an int32 torch tensor on the device is taken as it is (the kernel clamps what it reads)."""
    if isinstance(segments, (int, np.integer)) and not isinstance(segments, bool):
        k = int(segments)
        if k < 1:
            raise ValueError(f"{who}: segments={k}: a uniform segment holds at least one ray")
        return (int(nray) + k - 1) // k, None, k
    if hasattr(segments, "data_ptr"):
        if str(segments.dtype) != "torch.int32" or segments.dim() != 1 or len(segments) < 1:
            raise ValueError(f"{who}: segments= as a tensor is int32[n_seg + 1]")
        return len(segments) - 1, segments, 0
    off = np.asarray(segments)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"{who}: segments= is a sequence of n_seg + 1 integer offsets, or an int (rays per segment)")
    if (np.diff(off) < 0).any():
        raise ValueError(f"{who}: segments= offsets must be non-decreasing")
    if off[0] < 0 or off[-1] > nray:
        raise ValueError(f"{who}: segments= offsets must lie within 0..nray = {int(nray)}")
    return off.size - 1, np.ascontiguousarray(off, dtype=np.int32), 0


class WindowedDeposition:
    """Deposition windows (rays_hip_trace_window_profiles_device): a damped fan advanced in windows of at most n_steps
    recorded steps per ray, every accepted point binned into one or two profiles, no trajectory anywhere.  The saved
    RayState and the work rows are all a run needs to go on -- in this process or, through save() / load(), in another.
    deposition=[(which, n_bins), ...] or "all" with n_bins=n, as DeviceTrace takes them; ray_power: one weight per ray.
    .works[k] is [n_bins][nray] (bin-major), an accumulator zeroed by launch() alone; .profiles[k] is the ray-ordered sum
    over works[k] so far, continued from profile_in[k] (None = from zero), as of the last advance(profiles=True).
    state= / works= continue tensors the caller holds instead of allocating them (then do not call launch()).
    All launches are asynchronous on the current torch stream.  Once every ray has ended, advance() changes nothing."""

    def __init__(self, params: RaysParams, rvec0, rindex_vec0, deposition=None, ray_power=None,
                 n_bins: Optional[int] = None, state: Optional[RayState] = None, works=None, profile_in=None, device=None):
        import torch

        self.torch = torch
        self.params = params
        hip.check_params(params)
        if deposition is None or not _is_profile_list(deposition):
            raise ValueError('WindowedDeposition: deposition=[(which, n_bins), ...] or "all" (with n_bins=n)')
        self.deposition = _profile_list(params, deposition, n_bins, "WindowedDeposition")
        self.nray = len(rvec0)
        if ray_power is None:
            raise ValueError("WindowedDeposition: needs ray_power= (one weight per ray)")
        if len(ray_power) != self.nray:
            raise ValueError("WindowedDeposition: ray_power must hold one weight per ray")
        k = len(self.deposition)
        if profile_in is not None and (not isinstance(profile_in, (list, tuple)) or len(profile_in) != k):
            raise ValueError("WindowedDeposition: profile_in is a list with one entry (a tensor or None) per profile")
        if works is not None and (not isinstance(works, (list, tuple)) or len(works) != k or any(
                tuple(w.shape) != (nb, self.nray) for w, (_, nb) in zip(works, self.deposition))):
            raise ValueError("WindowedDeposition: works= is a list with one tensor [n_bins][nray] per profile")
        nv = params.nv
        if state is not None and (state.nray != self.nray or state.nv != nv):
            raise ValueError("WindowedDeposition: state= does not match this fan")
        self.profile_in = profile_in
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        f64, i32, dev = torch.float64, torch.int32, self.device
        put = lambda a: (a.to(device=dev, dtype=f64).contiguous() if torch.is_tensor(a)
                         else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev))
        self.rvec0, self.rindex_vec0, self.power = put(rvec0), put(rindex_vec0), put(ray_power)
        self.state = state if state is not None else RayState(self.nray, nv, device=dev)
        self.works = (list(works) if works is not None
                      else [torch.zeros((nb, self.nray), dtype=f64, device=dev) for _, nb in self.deposition])
        self.profiles = [torch.zeros(nb, dtype=f64, device=dev) for _, nb in self.deposition]
        self.npoints_win = torch.zeros(self.nray, dtype=i32, device=dev)
        self.start_ray_vec = torch.zeros((self.nray, nv), dtype=f64, device=dev)
        self._start_known = False   # launch() fills start_ray_vec; a continued state gets it in results()
        self.npoints = torch.zeros(self.nray, dtype=i32, device=dev)
        self.stop_code = torch.zeros(self.nray, dtype=i32, device=dev)
        self.end_ray_vec = torch.zeros((self.nray, nv), dtype=f64, device=dev)
        self.end_residuals = torch.zeros(self.nray, dtype=f64, device=dev)
        self.max_residuals = torch.zeros(self.nray, dtype=f64, device=dev)

    def _stream(self, who: str) -> int:
        if self.device.type != "cuda":
            raise RuntimeError(f"WindowedDeposition.{who}: this object lives on {self.device}; the kernels need a GPU "
                               "(there is no CPU fallback)")
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def launch(self):
        """Every ray at its launch point (rays_hip_state_init_device) and every work row zero."""
        stream = self._stream("launch")
        hip.state_init_device(self.params, self.nray, self.rvec0.data_ptr(), self.rindex_vec0.data_ptr(), self.state,
                              self.start_ray_vec.data_ptr(), stream=stream)
        self._start_known = True
        for w in self.works:
            w.zero_()

    def advance(self, n_steps: int, profiles: bool = True):
        """One deposition window of at most n_steps recorded steps per ray; profiles=False leaves the profile sums out
        (an intermediate window need not pay for them).  Returns npoints_win[nray], overwritten by the next advance()."""
        n = int(n_steps)
        if n < 1:
            raise ValueError("WindowedDeposition.advance: n_steps must be >= 1")
        stream = self._stream("advance")
        pin = self.profile_in or [None] * len(self.deposition)
        records = [(w, nb, work.data_ptr(), None if c is None else c.data_ptr(), prof.data_ptr() if profiles else None)
                   for (w, nb), work, c, prof in zip(self.deposition, self.works, pin, self.profiles)]
        hip.trace_window_profiles_device(self.params, self.nray, self.state, n, self.power.data_ptr(), records,
                                         self.npoints_win.data_ptr(), stream=stream)
        return self.npoints_win

    def results(self):
        """A list of RayDeposition (one per profile) on the state's RaySummaries; rays under way are included as they
        stand.  The profiles are those of the last advance(profiles=True).  Blocking."""
        t = self.torch
        stream = self._stream("results")
        if not self._start_known:   # a continued state: point 1 of every ray, from a scratch state
            scratch = RayState(self.nray, self.params.nv, device=self.device)
            hip.state_init_device(self.params, self.nray, self.rvec0.data_ptr(), self.rindex_vec0.data_ptr(), scratch,
                                  self.start_ray_vec.data_ptr(), stream=stream)
            self._start_known = True
        hip.state_summary_device(self.params, self.nray, self.state, self.npoints.data_ptr(), self.stop_code.data_ptr(),
                                 self.end_ray_vec.data_ptr(), self.end_residuals.data_ptr(),
                                 self.max_residuals.data_ptr(), stream=stream)
        t.cuda.synchronize(self.device)
        c = lambda x: x.cpu().numpy()
        summ = RaySummaries(c(self.npoints), c(self.stop_code), c(self.start_ray_vec), c(self.end_ray_vec),
                            c(self.end_residuals), c(self.max_residuals))
        return [RayDeposition(summ, w, nb, *deposition_grid_limits(self.params, w), c(prof),
                              np.ascontiguousarray(c(work).T))
                for (w, nb), work, prof in zip(self.deposition, self.works, self.profiles)]

    def save(self, path: str):
        """One npz file: the seven state arrays, every work (work_0, work_1), ray_power and the (which, n_bins) list
        (blocking: the tensors are copied to the host)."""
        arrays = self.state.numpy()
        for k, w in enumerate(self.works):
            arrays[f"work_{k}"] = w.cpu().numpy()
        arrays["ray_power"] = self.power.cpu().numpy()
        arrays["which"] = np.array([w for w, _ in self.deposition])
        arrays["n_bins"] = np.array([nb for _, nb in self.deposition], dtype=np.int32)
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path: str, params: RaysParams, rvec0, rindex_vec0, device=None) -> "WindowedDeposition":
        """A run saved by save(), in fresh tensors on `device`, ready for advance()."""
        import torch

        with np.load(path, allow_pickle=False) as z:
            specs = [(str(w), int(nb)) for w, nb in zip(z["which"], z["n_bins"])]
            wd = cls(params, rvec0, rindex_vec0, deposition=specs, ray_power=z["ray_power"], device=device)
            for name, dt in RayState.FIELDS:
                a = np.ascontiguousarray(z[name], dtype=dt)
                if a.shape != tuple(getattr(wd.state, name).shape):
                    raise ValueError(f"WindowedDeposition.load: {name} has shape {a.shape}")
                getattr(wd.state, name).copy_(torch.as_tensor(a))
            for k, w in enumerate(wd.works):
                a = np.ascontiguousarray(z[f"work_{k}"], dtype=np.float64)
                if a.shape != tuple(w.shape):
                    raise ValueError(f"WindowedDeposition.load: work_{k} has shape {a.shape}")
                w.copy_(torch.as_tensor(a))
        return wd


def load_axisym_tables(namelist_path: str, nml: Dict[str, Dict[str, Any]]) -> Optional[Dict[str, Any]]:
    """Host-built spline tables of an eqdsk equilibrium: `<eqdsk_file_name>.tables.npz` next to the
    namelist (None for the analytic equilibria)."""
    import os

    if str(nml.get("equilibrium_list", {}).get("equilib_model", "")).strip() != "axisym_toroid":
        return None
    if str(nml.get("axisym_toroid_eq_list", {}).get("magnetics_model", "")).strip() == "solovev_magnetics":
        return None   # analytic magnetics: nothing to load (spline PROFILE models would still need their tables)
    here = os.path.dirname(os.path.abspath(namelist_path))
    if str(nml.get("axisym_toroid_eq_list", {}).get("magnetics_model", "")).strip() == "eqdsk_magnetics_lin_interp":
        # bilinear eqdsk model: no spline fit, the host mirror reads the g-eqdsk itself (rays_amd/eqdsk.py); splined
        # PROFILES still come from the RAYS host's tables file when there is one
        from .eqdsk import eqdsk_lin_tables
        eq = str(nml.get("eqdsk_magnetics_lin_interp_list", {}).get("eqdsk_file_name", "")).strip()
        tab = eqdsk_lin_tables(os.path.join(here, eq))
        f = os.path.join(here, eq + ".tables.npz")
        if os.path.exists(f):
            z = np.load(f)
            tab.update({k: z[k] for k in z.files if k[:3] in ("ne_", "te_", "ti_")})
        return tab
    eq = str(nml.get("eqdsk_magnetics_spline_interp_list", {}).get("eqdsk_file_name", "")).strip()
    f = os.path.join(here, eq + ".tables.npz")
    if not os.path.exists(f):
        raise FileNotFoundError(f"{f}: spline tables of the eqdsk equilibrium (built by the RAYS host)")
    z = np.load(f)
    return {k: (float(z[k]) if z[k].ndim == 0 else z[k]) for k in z.files}


class RaysRun:
    """Module state after `initialize`: parameters + launched fan."""

    def __init__(self, params: RaysParams, rvec0, rindex_vec0, ray_pwr_wt=None,
                 namelist: Optional[Dict[str, Dict[str, Any]]] = None):
        self.params = params
        self.rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
        self.rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
        self.ray_pwr_wt = ray_pwr_wt
        self.namelist = namelist
        hip.check_params(params)

    @classmethod
    def from_namelist(cls, path: str, axisym_tables: Optional[Dict[str, Any]] = None) -> "RaysRun":
        """`initialize(read_input=.true.)`.  For equilib_model = 'axisym_toroid' the host-built spline
        tables are taken from `axisym_tables` or from `<eqdsk_file_name>.tables.npz` next to the
        namelist (written by a RAYS host, see tests/golden/make_golden.py)."""
        nml = read_namelist(path)
        tab = axisym_tables if axisym_tables is not None else load_axisym_tables(path, nml)
        p = params_from_namelist(nml, tab)
        if tab is not None:
            hip.set_axisym_tables(tab)
            if "rho_grid" in tab:
                hip.set_rho_table(tab["rho_grid"], tab["rho_fspl"])
        import os
        r0, n0, w = initialize_ray_init(p, nml, tab, base_dir=os.path.dirname(os.path.abspath(path)))
        return cls(p, r0, n0, w, nml)

    @property
    def nray(self) -> int:
        return len(self.rvec0)

    def trace_rays(self, ngpu: int = 1, trajectories: bool = True, deposition=None, want_work: bool = False,
                   window: Optional[int] = None, n_bins: Optional[int] = None):
        """window=n_steps: the same RayResults, traced in windows of n_steps on one device (hip.trace_windowed_host):
        the device holds the ray state and two window slabs, and each window's points reach the host arrays through
        pinned memory while the next window runs -- the way to trace a fan whose trajectories exceed the card.
        trajectories=False: the summary-only trace (RaySummaries; no trajectory array on the device or the host).
        trajectories=False, deposition=(which, n_bins): the fused trace + deposition (RayDeposition: the summaries and
        the profile `which` of the launcher's power weights ray_pwr_wt -- initial_ray_power of the run's results -- with
        work[nray][n_bins] if want_work).
        trajectories=False, deposition=[(which, n_bins), ...]: one or two profiles from ONE trace pass
        (rays_hip_trace_profiles): a list of RayDeposition that share one RaySummaries.  deposition="all", n_bins=n: the
        whole set of the equilibrium in the reference's order (calculate_deposition_profiles bins every one), whose
        profile_records go straight into results.write_deposition_profiles_LD / _NC."""
        if n_bins is not None and not isinstance(deposition, str):
            raise ValueError('RaysRun.trace_rays: n_bins=... goes with deposition="all" only')
        if window is not None:
            if deposition is not None or not trajectories:
                raise ValueError("RaysRun.trace_rays: window=... assembles the full trajectories; it goes with neither "
                                 "trajectories=False nor deposition=...")
            return RayResults(**hip.trace_windowed_host(self.params, self.rvec0, self.rindex_vec0, int(window), ngpu=ngpu))
        if deposition is not None:
            if trajectories:
                raise ValueError("RaysRun.trace_rays: deposition=... is the fused trace without trajectories -- pass "
                                 "trajectories=False (or bin a full trace with hip.deposition_host)")
            specs = _profile_list(self.params, deposition, n_bins, "RaysRun.trace_rays") if _is_profile_list(deposition) else None
            if specs is None:
                which, n_bins = _deposition_spec(deposition, False)
            if self.ray_pwr_wt is None:
                raise ValueError("RaysRun.trace_rays: deposition=... needs the launcher's power weights (ray_pwr_wt); this "
                                 "run has none")
            power = np.asarray(self.ray_pwr_wt, dtype=np.float64)
            if specs is not None:
                out = hip.trace_profiles_host(self.params, self.rvec0, self.rindex_vec0, power, specs, ngpu=ngpu,
                                              want_work=want_work)
                works, profs = out.pop("works"), out.pop("profiles")
                summ = RaySummaries(**out)
                return [RayDeposition(summ, w, nb, *deposition_grid_limits(self.params, w), prof, work)
                        for (w, nb), prof, work in zip(specs, profs, works)]
            out = hip.trace_deposition_host(self.params, self.rvec0, self.rindex_vec0, power, which, int(n_bins),
                                            ngpu=ngpu, want_work=want_work)
            work, prof = out.pop("work"), out.pop("profile")
            lo, hi = deposition_grid_limits(self.params, which)
            return RayDeposition(RaySummaries(**out), which, int(n_bins), lo, hi, prof, work)
        if not trajectories:
            return RaySummaries(**hip.trace_summary_host(self.params, self.rvec0, self.rindex_vec0, ngpu=ngpu))
        out = hip.trace_host(self.params, self.rvec0, self.rindex_vec0, ngpu=ngpu)
        return RayResults(**out)

    def finalize_run(self, res: RayResults, directory: str = ".", list_directed: bool = True, netcdf: bool = True):
        """finalize_run.f90:20-28: write run_results.<run_label> (list-directed) and/or
        run_results.<run_label>.nc from the results of this run (rays_amd/results.py)."""
        import os

        from . import results as rf

        label = str((self.namelist or {}).get("diagnostics_list", {}).get("run_label", "")).strip()
        rr = rf.RunResults(res, self.ray_pwr_wt, label)
        base = os.path.join(directory, "run_results." + label)
        if list_directed:
            rf.write_results_LD(base, rr)
        if netcdf:
            rf.write_results_NC(base + ".nc", rr)
        return rr


class DeviceTrace:
    """Device-resident trace: inputs/outputs are torch CUDA tensors, launches are asynchronous on
    the current torch stream (used by bench.py and by multi-GPU runs).
    trajectories=False: summary-only (rays_hip_trace_summary_device) -- ray_vec and residual are None, no trajectory
    tensor is allocated, start_ray_vec exists instead, results() returns a RaySummaries.
    trajectories=False, deposition=(which, n_bins, power): the fused trace + deposition (rays_hip_trace_deposition_device)
    -- additionally .work[n_bins][nray] (bin-major, zeroed by every launch) and .profile[n_bins] of the profile `which`
    with the per-ray power weights `power`; profile_in: a tensor[n_bins] of running sums the profile continues (the
    block of rays before this one), None = from zero.
    window=n_steps: windowed tracing (rays_hip_state_init_device / rays_hip_trace_window_device).  No tensor with an
    nstep_max + 1 axis exists: .state is the saved RayState, .ray_vec / .residual are ONE window slab
    [nray][n_steps][nv] / [nray][n_steps] (None with trajectories=False) and .npoints_win[nray] says how many points of
    it each ray recorded in the last window.  launch() puts every ray at its launch point (start_ray_vec = point 1,
    residual 0); advance() runs one window and returns (ray_vec_win, residual_win, npoints_win) -- the object's own
    tensors, overwritten by the next advance(); results() gives the state's RaySummaries, rays under way included as
    they stand.  state= continues a RayState saved earlier instead of allocating one.
    trajectories=False, deposition=[(which, n_bins), ...], ray_power=power: one or two profiles from ONE trace pass
    (rays_hip_trace_profiles_device) -- .works, .profiles and .deposition are lists in the order asked, profile_in a
    list of tensors / None of the same length, and results() returns a list of RayDeposition that share one
    RaySummaries.  deposition="all", n_bins=n: the equilibrium's whole set (hip.deposition_profile_set).
    ... segments=offsets | int (with the list spelling): one profile per SEGMENT of rays -- the beams of an aiming survey
    (rays_hip_trace_profiles_segments_device).  offsets: n_seg + 1 ray indices, segment s being the rays offsets[s] ..
    offsets[s + 1] - 1 (a host sequence is checked: non-decreasing, within 0..nray); an int k: uniform segments of k
    rays.  Every .profiles[i], profile_in[i] and RayDeposition.profile is then [n_seg][n_bins], and Q_sum has one value
    per segment; .works are unchanged."""

    def __init__(self, params: RaysParams, rvec0, rindex_vec0, device=None, trajectories: bool = True, deposition=None,
                 profile_in=None, window: Optional[int] = None, state: Optional[RayState] = None, ray_power=None,
                 n_bins: Optional[int] = None, segments=None):
        import torch

        self.torch = torch
        self.params = params
        hip.check_params(params)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.nray = len(rvec0)
        self.trajectories = bool(trajectories)
        self.deposition = None
        self.work = self.profile = self.power = None
        self.profile_in = profile_in
        self.works = self.profiles = None
        self.profile_list = deposition is not None and _is_profile_list(deposition)
        self.segments = None
        if segments is not None:
            if not self.profile_list:
                raise ValueError("DeviceTrace: segments= goes with the list spelling deposition=[(which, n_bins), ...] "
                                 'or "all"')
            self.segments = check_segments(segments, self.nray, "DeviceTrace")
        if self.profile_list:
            if self.trajectories:
                raise ValueError("DeviceTrace: deposition=... is the fused trace without trajectories -- pass "
                                 "trajectories=False (or bin a full trace with hip.deposition_device)")
            self.deposition = _profile_list(params, deposition, n_bins, "DeviceTrace")
            if ray_power is None:
                raise ValueError("DeviceTrace: deposition=[...] needs ray_power= (one weight per ray)")
            if len(ray_power) != self.nray:
                raise ValueError("DeviceTrace: ray_power must hold one weight per ray")
            if profile_in is not None and (not isinstance(profile_in, (list, tuple)) or len(profile_in) != len(self.deposition)):
                raise ValueError("DeviceTrace: profile_in of deposition=[...] is a list with one entry (a tensor or None) "
                                 "per profile")
        elif ray_power is not None or n_bins is not None:
            raise ValueError("DeviceTrace: ray_power= / n_bins= go with the list spelling deposition=[(which, n_bins), ...] "
                             'or "all"; the tuple spelling carries its power: deposition=(which, n_bins, power)')
        elif deposition is not None:
            if self.trajectories:
                raise ValueError("DeviceTrace: deposition=... is the fused trace without trajectories -- pass "
                                 "trajectories=False (or bin a full trace with hip.deposition_device)")
            which, n_bins, power = _deposition_spec(deposition, True)
            if len(power) != self.nray:
                raise ValueError("DeviceTrace: deposition power must hold one weight per ray")
            self.deposition = (which, int(n_bins))
        elif profile_in is not None:
            raise ValueError("DeviceTrace: profile_in without deposition=...")
        nv, npt = params.nv, params.nstep_max + 1
        f64, i32 = torch.float64, torch.int32
        self.ray_vec = self.residual = self.start_ray_vec = None
        self.window = None if window is None else int(window)
        self.state = self.npoints_win = None
        if self.window is not None:
            if deposition is not None:
                raise ValueError("DeviceTrace: window=... does not go with deposition=... (deposition windows are a class "
                                 "of their own: WindowedDeposition)")
            if self.window < 1:
                raise ValueError("DeviceTrace: window must be >= 1")
        elif state is not None:
            raise ValueError("DeviceTrace: state= without window=...")
        with torch.cuda.device(self.device):
            self.rvec0 = torch.as_tensor(np.ascontiguousarray(rvec0), dtype=f64).to(self.device)
            self.rindex_vec0 = torch.as_tensor(np.ascontiguousarray(rindex_vec0), dtype=f64).to(self.device)
            if self.window is not None:
                if state is not None and (state.nray != self.nray or state.nv != nv):
                    raise ValueError("DeviceTrace: state= does not match this fan")
                self.state = state if state is not None else RayState(self.nray, nv, device=self.device)
                if self.trajectories:
                    self.ray_vec = torch.zeros((self.nray, self.window, nv), dtype=f64, device=self.device)
                    self.residual = torch.zeros((self.nray, self.window), dtype=f64, device=self.device)
                self.npoints_win = torch.zeros(self.nray, dtype=i32, device=self.device)
                self.start_ray_vec = torch.zeros((self.nray, nv), dtype=f64, device=self.device)
            elif self.trajectories:
                # zero-filled once, like initialize_ray_results_m (ray_results_m.f90:154-164)
                self.ray_vec = torch.zeros((self.nray, npt, nv), dtype=f64, device=self.device)
                self.residual = torch.zeros((self.nray, npt), dtype=f64, device=self.device)
            else:
                self.start_ray_vec = torch.zeros((self.nray, nv), dtype=f64, device=self.device)
            self.npoints = torch.zeros(self.nray, dtype=i32, device=self.device)
            self.stop_code = torch.zeros(self.nray, dtype=i32, device=self.device)
            self.end_ray_vec = torch.zeros((self.nray, nv), dtype=f64, device=self.device)
            self.end_residuals = torch.zeros(self.nray, dtype=f64, device=self.device)
            self.max_residuals = torch.zeros(self.nray, dtype=f64, device=self.device)
            if self.profile_list:
                pw = ray_power
                self.power = (pw.to(device=self.device, dtype=f64).contiguous() if torch.is_tensor(pw)
                              else torch.as_tensor(np.ascontiguousarray(pw, dtype=np.float64)).to(self.device))
                self.works = [torch.zeros((max(nb, 0), self.nray), dtype=f64, device=self.device)
                              for _, nb in self.deposition]
                self.profiles = [torch.zeros(max(nb, 0), dtype=f64, device=self.device) for _, nb in self.deposition]
                if self.segments is not None:
                    n_seg, off, per = self.segments
                    self.profiles = [torch.zeros((n_seg, max(nb, 0)), dtype=f64, device=self.device)
                                     for _, nb in self.deposition]
                    if off is not None:
                        off = off.to(self.device).contiguous() if torch.is_tensor(off) else torch.as_tensor(off).to(self.device)
                    self.segments = (n_seg, off, per)
            elif self.deposition is not None:
                nb = max(self.deposition[1], 0)
                pw = deposition[2]
                self.power = (pw.to(device=self.device, dtype=f64).contiguous() if torch.is_tensor(pw)
                              else torch.as_tensor(np.ascontiguousarray(pw, dtype=np.float64)).to(self.device))
                self.work = torch.zeros((nb, self.nray), dtype=f64, device=self.device)
                self.profile = torch.zeros(nb, dtype=f64, device=self.device)

    def launch(self, zero_fill: bool = True):
        t = self.torch
        stream = t.cuda.current_stream(self.device).cuda_stream
        if self.window is not None:
            hip.state_init_device(self.params, self.nray, self.rvec0.data_ptr(), self.rindex_vec0.data_ptr(), self.state,
                                  self.start_ray_vec.data_ptr(), stream=stream)
            return
        if self.profile_list:
            pin = self.profile_in or [None] * len(self.deposition)
            records = [(w, nb, work.data_ptr(), None if c is None else c.data_ptr(), prof.data_ptr())
                       for (w, nb), work, c, prof in zip(self.deposition, self.works, pin, self.profiles)]
            if self.segments is not None:
                n_seg, off, per = self.segments
                hip.trace_profiles_segments_device(
                    self.params, self.nray, self.rvec0.data_ptr(), self.rindex_vec0.data_ptr(), self.power.data_ptr(),
                    records, n_seg, None if off is None else off.data_ptr(), per, self.npoints.data_ptr(),
                    self.stop_code.data_ptr(), self.start_ray_vec.data_ptr(), self.end_ray_vec.data_ptr(),
                    self.end_residuals.data_ptr(), self.max_residuals.data_ptr(), stream=stream)
                return
            hip.trace_profiles_device(self.params, self.nray, self.rvec0.data_ptr(), self.rindex_vec0.data_ptr(),
                                      self.power.data_ptr(), records, self.npoints.data_ptr(), self.stop_code.data_ptr(),
                                      self.start_ray_vec.data_ptr(), self.end_ray_vec.data_ptr(),
                                      self.end_residuals.data_ptr(), self.max_residuals.data_ptr(), stream=stream)
            return
        if self.deposition is not None:
            hip.trace_deposition_device(self.params, self.nray, self.rvec0.data_ptr(), self.rindex_vec0.data_ptr(),
                                        self.power.data_ptr(), self.deposition[0], self.deposition[1],
                                        self.npoints.data_ptr(), self.stop_code.data_ptr(), self.start_ray_vec.data_ptr(),
                                        self.end_ray_vec.data_ptr(), self.end_residuals.data_ptr(),
                                        self.max_residuals.data_ptr(), self.work.data_ptr(),
                                        None if self.profile_in is None else self.profile_in.data_ptr(),
                                        self.profile.data_ptr(), stream=stream)
            return
        if not self.trajectories:
            hip.trace_summary_device(self.params, self.nray, self.rvec0.data_ptr(), self.rindex_vec0.data_ptr(),
                                     self.npoints.data_ptr(), self.stop_code.data_ptr(), self.start_ray_vec.data_ptr(),
                                     self.end_ray_vec.data_ptr(), self.end_residuals.data_ptr(),
                                     self.max_residuals.data_ptr(), stream=stream)
            return
        hip.trace_device(self.params, self.nray, self.rvec0.data_ptr(), self.rindex_vec0.data_ptr(),
                         self.ray_vec.data_ptr(), self.residual.data_ptr(), self.npoints.data_ptr(),
                         self.stop_code.data_ptr(), self.end_ray_vec.data_ptr(),
                         self.end_residuals.data_ptr(), self.max_residuals.data_ptr(),
                         stream=stream, zero_fill=zero_fill)

    def advance(self, n_steps: Optional[int] = None, recording: Optional[bool] = None):
        """One window: every ray under way advances by at most n_steps (default: the window length) recorded steps, and
        .state is updated in place.  recording=False: a summary window (nothing is stored; possible at any time).
        Returns (ray_vec_win, residual_win, npoints_win): the window's new points -- ray_vec_win[r, :npoints_win[r]] --
        or (None, None, npoints_win).  Asynchronous on the current torch stream."""
        if self.window is None:
            raise RuntimeError("DeviceTrace.advance: this trace has no window (pass window=n_steps)")
        n = self.window if n_steps is None else int(n_steps)
        rec = self.trajectories if recording is None else bool(recording)
        if rec and not self.trajectories:
            raise ValueError("DeviceTrace.advance: recording=True on a trace built with trajectories=False")
        if rec and n > self.window:
            raise ValueError("DeviceTrace.advance: n_steps exceeds the window slab this trace allocated")
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        hip.trace_window_device(self.params, self.nray, self.state, n, self.ray_vec.data_ptr() if rec else 0,
                                self.residual.data_ptr() if rec else 0, self.npoints_win.data_ptr(), stream=stream)
        if not rec:
            return None, None, self.npoints_win
        # the slab of a shorter window is laid out with ITS stride: [nray][n][nv]
        rv = self.ray_vec.view(-1)[:self.nray * n * self.params.nv].view(self.nray, n, self.params.nv)
        res = self.residual.view(-1)[:self.nray * n].view(self.nray, n)
        return rv, res, self.npoints_win

    def diagnostics(self, fields=None, packed: bool = False) -> Dict[str, Any]:
        """ray_detailed_diagnostics of the trace as it lies on the device (hip.ray_diagnostics_device): {field name:
        tensor[nray][nstep_max+1]} for `fields` (hip.DIAG_FIELDS; None = all) -- views of one [k][nray][nstep_max+1]
        block -- plus "first_bad_point"[nray] (int32).  Asynchronous on the current torch stream, behind launch().
        packed=True (hip.ray_diagnostics_packed_device on the padded trace arrays): {field name: tensor[total]}, the
        recorded points alone, rays in order -- views of one [k][total] block, no zero slots -- plus "offsets"
        (int64[nray + 1] on the device: point j of ray i is element offsets[i] + j) and "first_bad_point".  To
        allocate k * total doubles instead of k * nray * (nstep_max + 1) it reads offsets[nray] once before
        allocating: ONE 8-BYTE SYNCHRONISING COPY behind launch(); the diagnostics kernel itself is asynchronous."""
        t = self.torch
        if self.window is not None:
            raise RuntimeError("DeviceTrace.diagnostics: a windowed trace holds one window of points, not the trajectories")
        if not self.trajectories:
            raise RuntimeError("DeviceTrace.diagnostics: this trace is summary-only (trajectories=False) -- the per-point "
                               "diagnostics need the recorded points; trace with trajectories=True")
        _, names = hip.diag_field_mask(fields)
        if packed:
            with t.cuda.device(self.device):
                stream = t.cuda.current_stream(self.device).cuda_stream
                off = t.empty(self.nray + 1, dtype=t.int64, device=self.device)
                hip.point_offsets_device(self.nray, self.params.nstep_max, self.npoints.data_ptr(), off.data_ptr(), stream)
                total = int(off[self.nray].item())   # the one synchronising copy
                out = t.empty((len(names), total), dtype=t.float64, device=self.device)
                bad = t.empty(self.nray, dtype=t.int32, device=self.device)
                if total:
                    hip.ray_diagnostics_packed_device(self.params, self.nray, self.ray_vec.data_ptr(),
                                                      self.residual.data_ptr(), self.npoints.data_ptr(), off.data_ptr(),
                                                      total, names, out.data_ptr(), bad.data_ptr(), stream)
                else:   # no recorded point: `out` is empty, and the entry refuses its null pointer
                    bad.zero_()
            res = {n: out[k] for k, n in enumerate(names)}
            res["offsets"] = off
            res["first_bad_point"] = bad
            return res
        with t.cuda.device(self.device):
            out = t.empty((len(names), self.nray, self.params.nstep_max + 1), dtype=t.float64, device=self.device)
            bad = t.empty(self.nray, dtype=t.int32, device=self.device)
            hip.ray_diagnostics_device(self.params, self.nray, self.ray_vec.data_ptr(), self.residual.data_ptr(),
                                       self.npoints.data_ptr(), names, out.data_ptr(), bad.data_ptr(),
                                       stream=t.cuda.current_stream(self.device).cuda_stream)
        res: Dict[str, Any] = {n: out[k] for k, n in enumerate(names)}
        res["first_bad_point"] = bad
        return res

    def ox_conversion(self, fields=None) -> Dict[str, Any]:
        """analyze_OX_conv of the trace as it lies on the device (hip.ox_conv_device): {field name: tensor} for
        `fields` (names of hip.OX_FIELDS; None = all) -- status, step_number, iterations int32[nray]; alpha_max,
        conv_coeff float64[nray]; x_max, k_max, x_cut, nvecx_c, nvecy_c, nvecz_c [nray][3]; aux [nray][5]
        (hip.OX_AUX).  No trajectory leaves the device.  conv_coeff and the CONVERTED bit of status come from the
        device library's acos / sin / cos (include/rays_hip.h); everything else is bit-identical to the reference.
        Asynchronous on the current torch stream, behind launch()."""
        t = self.torch
        if self.window is not None:
            raise RuntimeError("DeviceTrace.ox_conversion: a windowed trace holds one window of points, not the trajectories")
        if not self.trajectories:
            raise RuntimeError("DeviceTrace.ox_conversion: this trace is summary-only (trajectories=False) -- the analysis "
                               "scans the recorded points; trace with trajectories=True")
        known = [f for f, _, _ in hip.OX_FIELDS]
        fields = known if fields is None else list(fields)
        unknown = [f for f in fields if f not in known]
        if unknown:
            raise ValueError(f"DeviceTrace.ox_conversion: unknown fields {unknown}; known: {known}")
        with t.cuda.device(self.device):
            out = {f: t.empty((self.nray, w) if w > 1 else (self.nray,), dtype=t.int32 if dt is np.int32 else t.float64,
                              device=self.device) for f, dt, w in hip.OX_FIELDS if f in fields}
            hip.ox_conv_device(self.params, self.nray, self.ray_vec.data_ptr(), self.npoints.data_ptr(),
                               {f: v.data_ptr() for f, v in out.items()},
                               stream=t.cuda.current_stream(self.device).cuda_stream)
        return out

    def results(self):
        if self.window is not None:
            stream = self.torch.cuda.current_stream(self.device).cuda_stream
            hip.state_summary_device(self.params, self.nray, self.state, self.npoints.data_ptr(), self.stop_code.data_ptr(),
                                     self.end_ray_vec.data_ptr(), self.end_residuals.data_ptr(),
                                     self.max_residuals.data_ptr(), stream=stream)
        self.torch.cuda.synchronize(self.device)
        c = lambda x: x.cpu().numpy()
        if self.window is not None:
            return RaySummaries(c(self.npoints), c(self.stop_code), c(self.start_ray_vec), c(self.end_ray_vec),
                                c(self.end_residuals), c(self.max_residuals))
        if self.profile_list:
            summ = RaySummaries(c(self.npoints), c(self.stop_code), c(self.start_ray_vec), c(self.end_ray_vec),
                                c(self.end_residuals), c(self.max_residuals))
            return [RayDeposition(summ, w, nb, *deposition_grid_limits(self.params, w), c(prof),
                                  np.ascontiguousarray(c(work).T))
                    for (w, nb), work, prof in zip(self.deposition, self.works, self.profiles)]
        if not self.trajectories:
            return RaySummaries(c(self.npoints), c(self.stop_code), c(self.start_ray_vec), c(self.end_ray_vec),
                                c(self.end_residuals), c(self.max_residuals))
        return RayResults(c(self.ray_vec), c(self.residual), c(self.npoints), c(self.stop_code),
                          c(self.end_ray_vec), c(self.end_residuals), c(self.max_residuals))
