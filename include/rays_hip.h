/*
 * rays_hip.h -- C ABI of the MI355X-native RAYS ray-trajectory integrator (librays_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path of ORNL-Fusion/RAYS:
 *
 *     call trace_rays            RAYS_project/RAYS_code/RAYS.f90:13
 *                                RAYS_project/RAYS_lib/ray_tracing.f90:1-290
 *
 * i.e. the per-ray ODE march  ode_solver(RK4_ode | SG_ode) -> eqn_ray ->
 * equilibrium(slab | solovev) + deriv_cold | deriv_num -> check_save, for all rays of a fan.
 * The reference has no process/device boundary (module state in, ray_results_m arrays out);
 * the binding a RAYS maintainer adds is the iso_c_binding interface in fortran/rays_hip_m.f90
 * plus the replacement trace_rays in fortran/trace_rays_hip.f90.
 *
 * Conventions
 *   - plain C types only; every array is caller-owned; the library never keeps a host pointer
 *     after a call returns.
 *   - return 0 on success; non-zero = HIP failure / bad configuration, message via
 *     rays_hip_last_error().  A ray that stops is NOT an error: it gets a stop code
 *     (RAYS_STOP_*), mapped to the reference's ode_stop_flag text by rays_hip_stop_flag_text().
 *   - all reals are IEEE binary64 (reference rkind = selected_real_kind(15,307),
 *     constants_m.f90:14), counters are 32-bit.
 *   - array layouts are exactly the reference's Fortran arrays (ray_results_m.f90:44-58):
 *       ray_vec (nv, nstep_max+1, nray)  column-major == C [nray][nstep_max+1][nv]
 *       residual(nstep_max+1, nray)      column-major == C [nray][nstep_max+1]
 *       rvec0(3,nray), rindex_vec0(3,nray)             == C [nray][3]   (ray_init_m.f90:47-53)
 *     Entries past npoints(iray) are zero, as after initialize_ray_results_m (154-164).
 */
#ifndef RAYS_HIP_H
#define RAYS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAYS_ABI_VERSION 3
#define RAYS_NSPEC0 5 /* species_m.f90:25  nspec0; arrays are dimensioned 0:nspec0 */
#define RAYS_NS0 (RAYS_NSPEC0 + 1)

/* ---- selectors: integer images of the reference's string switches ----------------------- */
enum { RAYS_ODE_RK4 = 0, RAYS_ODE_SG = 1 };           /* ode_m.f90:238  'RK4_ODE' | 'SG_ODE'   */
enum { RAYS_DERIV_COLD = 0, RAYS_DERIV_NUM = 1 };     /* eqn_ray.f90:106 'cold' | 'numerical'  */
enum { RAYS_PARAM_ARCL = 0, RAYS_PARAM_TIME = 1 };    /* eqn_ray.f90:148 'arcl' | 'time'       */
enum { RAYS_EQ_SLAB = 0, RAYS_EQ_SOLOVEV = 1, RAYS_EQ_AXISYM = 2 }; /* equilibrium_m.f90:177-189 */
enum { RAYS_DAMP_NONE = 0, RAYS_DAMP_FUND_ECH = 1 };  /* damping_m.f90:94-101 'no_damp' | 'damp_fund_ECH' */

/* slab_eq_m.f90:172-300 profile-model strings */
enum { RAYS_SLAB_BX_ZERO = 0 };
enum { RAYS_SLAB_BY_ZERO = 0, RAYS_SLAB_BY_CONSTANT, RAYS_SLAB_BY_TOROID, RAYS_SLAB_BY_LINEAR_SHEAR };
enum { RAYS_SLAB_BZ_CONSTANT = 0, RAYS_SLAB_BZ_TOROID, RAYS_SLAB_BZ_LINEAR, RAYS_SLAB_BZ_LINEAR_2 };
enum { RAYS_SLAB_N_CONSTANT = 0, RAYS_SLAB_N_LINEAR, RAYS_SLAB_N_LINEAR_2, RAYS_SLAB_N_PARABOLIC,
       RAYS_SLAB_N_GAUSSIAN };
enum { RAYS_SLAB_T_ZERO = 0, RAYS_SLAB_T_CONSTANT, RAYS_SLAB_T_LINEAR, RAYS_SLAB_T_LINEAR_2,
       RAYS_SLAB_T_PARABOLIC };
/* solovev_eq_m.f90:208-267 */
enum { RAYS_SOLOVEV_N_CONSTANT = 0, RAYS_SOLOVEV_N_PARABOLIC };
enum { RAYS_SOLOVEV_T_ZERO = 0, RAYS_SOLOVEV_T_PARABOLIC = 2 };

/* axisym_toroid_eq_m.f90:56-100: magnetics / profile model strings */
enum { RAYS_AXI_MAG_EQDSK_SPLINE = 0, /* 'eqdsk_magnetics_spline_interp' */
       RAYS_AXI_MAG_SOLOVEV = 1 };    /* 'solovev_magnetics' (solovev_magnetics_m.f90): the analytic Solovev field under
                                         the axisym_toroid profile models; its /solovev_magnetics_list/ travels in
                                         rays_params_t.solovev (rmaj, kappa, bphi0, iota0, outer_bound = outer_boundary,
                                         psiB, box_*), and axisym.box_* / psiB repeat the box and psiB */
enum { RAYS_AXI_MAG_EQDSK_LIN = 2 };  /* 'eqdsk_magnetics_lin_interp' (eqdsk_magnetics_lin_interp_m.f90): bilinear
                                         interpolation of the raw eqdsk Psi(NRBOX, NZBOX) and linear interpolation of
                                         T(NRBOX), derivatives by the reference's central differences over +-dR, +-dZ
                                         (eqdsk_utilities_m.f90:144-306); tables: rays_hip_set_eqdsk_lin_tables */
enum { RAYS_AXI_N_CONSTANT = 0, RAYS_AXI_N_PARABOLIC, RAYS_AXI_N_SPLINE };
enum { RAYS_AXI_T_ZERO = 0, RAYS_AXI_T_CONSTANT, RAYS_AXI_T_PARABOLIC, RAYS_AXI_T_SPLINE };

/* ---- per-ray stop codes  <->  reference ode_stop_flag strings ---------------------------- */
enum {
  RAYS_STOP_NONE = 0,
  RAYS_STOP_SOUT_GT_SMAX = 1,      /* 'sout > s_max'            ray_tracing.f90:144 */
  RAYS_STOP_NSTEP_MAX = 2,         /* ' nstep > nstep_max'      ray_tracing.f90:152 (leading blank) */
  RAYS_STOP_X_OUT_OF_BOUNDS = 10,  /* 'x out_of_bounds'         slab_eq_m.f90:163 */
  RAYS_STOP_Y_OUT_OF_BOUNDS = 11,  /* 'y out_of_bounds'         slab_eq_m.f90:164 */
  RAYS_STOP_Z_OUT_OF_BOUNDS = 12,  /* 'z out_of_bounds'         slab_eq_m.f90:165 */
  RAYS_STOP_NEGATIVE_DENS = 13,    /* 'negative_dens'           slab_eq_m.f90:305, solovev_eq_m.f90:272 */
  RAYS_STOP_NEGATIVE_TEMP = 14,    /* 'negative_temp'           slab_eq_m.f90:306, solovev_eq_m.f90:273 */
  RAYS_STOP_R_OUT_OF_BOX = 20,     /* 'R out_of_box'            solovev_eq_m.f90:155 */
  RAYS_STOP_Z_OUT_OF_BOX = 21,     /* 'z out_of_box'            solovev_eq_m.f90:156 */
  RAYS_STOP_AXI_R_OUT_OF_BOX = 22, /* 'R_out_of_box'            axisym_toroid_eq_m.f90:263 */
  RAYS_STOP_AXI_Z_OUT_OF_BOX = 23, /* 'Z_out_of_box'            axisym_toroid_eq_m.f90:267 */
  RAYS_STOP_OUT_OF_PLASMA = 24,    /* 'out_of_plasma'           axisym_toroid_eq_m.f90:288 */
  RAYS_STOP_SOLMAG_R_OUT_OF_BOUNDS = 25, /* 'R out_of_bounds'   solovev_magnetics_m.f90:147 */
  RAYS_STOP_SOLMAG_Z_OUT_OF_BOUNDS = 26, /* 'z out_of_bounds'   solovev_magnetics_m.f90:148 */
  RAYS_STOP_INFINITE_VG_RHS = 30,  /* 'infinite Vg'             eqn_ray.f90:142 */
  RAYS_STOP_RAY_STALLED = 31,      /* 'ray stalled'             eqn_ray.f90:168 */
  RAYS_STOP_DISP_RESIDUAL = 40,    /* 'dispersion_residual'     check_save.f90:70 */
  RAYS_STOP_INFINITE_VG_CHECK = 41,/* 'infinite_Vg'             check_save.f90:108 */
  RAYS_STOP_TOTAL_ABSORPTION = 42, /* 'total_absorption'        check_save.f90:123 */
  RAYS_STOP_ODE_TOTAL_ERROR = 50,  /* 'ODE total error'         SG_ode_m.f90:144 */
  RAYS_STOP_SG_MAXNUM = 51,        /* 'step number .ge. maxnum' ode_RAYS.f90:538 */
  RAYS_STOP_SG_STIFF = 52,         /* 'equations stiff'         ode_RAYS.f90:541 */
  RAYS_STOP_SG_T_EQ_TOUT = 53,     /* 't == tout'               ode_RAYS.f90:433 */
  RAYS_STOP_SG_NEG_ERR = 54,       /* 'relerr or abserr < 0'    ode_RAYS.f90:439 */
  RAYS_STOP_SG_EPS_LE_0 = 55       /* 'eps <= 0'                ode_RAYS.f90:447 */
};

/* ---- slab_eq_m.f90:35-85 namelist /slab_eq_list/ ------------------------------------------ */
typedef struct rays_slab_params {
  int32_t bx_prof_model, by_prof_model, bz_prof_model, dens_prof_model;
  int32_t t_prof_model[RAYS_NS0];
  int32_t pad_[2];
  double xmin, xmax, ymin, ymax, zmin, zmax;
  double rmaj, rmin, x0;
  double bx0, by0, bz0, LBy_shear_scale, LBz_scale, dBzdx;
  double Ln_scale, dndx, alphan1, alphan2, n_min;
  double LT_scale, dtdx;
  double alphat1[RAYS_NS0], alphat2[RAYS_NS0], T_min[RAYS_NS0];
} rays_slab_params_t;

/* ---- solovev_eq_m.f90:17-45 namelist /solovev_eq_list/ + derived psiB (:92) --------------- */
typedef struct rays_solovev_params {
  int32_t dens_prof_model;
  int32_t t_prof_model[RAYS_NS0];
  int32_t pad_[1];
  double rmaj, kappa, bphi0, iota0, outer_bound;
  double psiB; /* computed by the host exactly as solovev_eq_m.f90:89-92 */
  double alphan1, alphan2;
  double alphat1[RAYS_NS0], alphat2[RAYS_NS0];
  double box_rmin, box_rmax, box_zmin, box_zmax;
} rays_solovev_params_t;

/* ---- axisym_toroid_eq_m.f90:56-100 namelist /axisym_toroid_eq_list/ + eqdsk-derived scalars ---- */
typedef struct rays_axisym_params {
  int32_t magnetics_model, density_prof_model;
  int32_t t_prof_model[RAYS_NS0];
  double box_rmin, box_rmax, box_zmin, box_zmax; /* from the eqdsk (eqdsk_magnetics_spline_interp_m.f90:115-118) */
  double plasma_psi_limit;
  double psiB; /* PSIBOUND - PSIAXIS (eqdsk_magnetics_spline_interp_m.f90:171-173) */
  double alphan1, alphan2, d_scrape_off, T_scrape_off;
  double alphat1[RAYS_NS0], alphat2[RAYS_NS0];
} rays_axisym_params_t;

/* ---- everything trace_rays reads from module state ----------------------- */
typedef struct rays_params {
  int32_t abi_version;  /* RAYS_ABI_VERSION */
  int32_t nv;           /* ode_m.f90:160-173: 7, +1 with damping, +1+nspec with multi_spec_damping, +5 with
                           integrate_eq_gradients */
  int32_t nspec;        /* species_m.f90:27 number of ion species (electrons are species 0) */
  int32_t nstep_max;    /* ode_m.f90:104 */
  int32_t ode_solver;   /* RAYS_ODE_* */
  int32_t ray_deriv;    /* RAYS_DERIV_* */
  int32_t ray_param;    /* RAYS_PARAM_* */
  int32_t equilib_model;/* RAYS_EQ_* */
  int32_t integrate_eq_gradients; /* diagnostics_m.f90:101 */
  int32_t pad_[3];
  double ds, s_max;                    /* ode_m.f90:98-101 */
  double omgrf, k0;                    /* rf_m.f90:18-21 (passed by value: never re-derived) */
  double clight, eps0;                 /* constants_m.f90:42-44 (single-precision literals!) */
  double dispersion_resid_limit;       /* rf_m.f90:48 */
  double rel_err0, abs_err0, SG_error_limit; /* SG_ode_m.f90:26-31 */
  double qs[RAYS_NS0], ms[RAYS_NS0];   /* species_m.f90:71-72, SI units after init (155-157) */
  double n0s[RAYS_NS0], t0s[RAYS_NS0]; /* species_m.f90:42-44 */
  double eta[RAYS_NS0];                /* species_m.f90:73 */
  rays_slab_params_t slab;
  rays_solovev_params_t solovev;
  /* damping_m.f90:30-40 (appended in ABI version 2) */
  int32_t damping_model;      /* RAYS_DAMP_* */
  int32_t multi_spec_damping; /* damping_m.f90:35: one absorbed-power row per species behind the total */
  double total_damping_limit; /* damping_m.f90:38 */
  /* appended in ABI version 3 */
  rays_axisym_params_t axisym;
} rays_params_t;

/* ---- library control ----------------------------------------------------------------------- */
/* Select up to ngpu visible devices for rays_hip_trace (0 = all).  Returns the number in use,
 * or a negative value on failure.  Optional: rays_hip_trace initialises lazily. */
int rays_hip_init(int ngpu);
/* Explicit device list for rays_hip_trace: slot i of the ray partition runs on device_ids[i]
 * (1 <= n <= 16).  A device may be listed more than once: its slots then run concurrently on that
 * device, each with its own host thread, stream and staging buffers, so one slot's device-to-host
 * copy overlaps another's trace.  Returns n, or a negative value on failure. */
int rays_hip_init_devices(int n, const int* device_ids);
/* Returns everything the library holds on the devices and in pinned host memory to the driver: the RCCL
 * communicators, the kept and the gathered result (their pointers are invalid from here on), the per-stream
 * workspaces and scratch blocks, the device copies of the tables, the staging buffers, the cached blocks and
 * streams, the device list.  Call it with no other entry running.  The library may be used again afterwards and
 * then behaves as on first use: the tables set so far are uploaded again from their host copies, and the
 * numerics setting and the rays_hip_keep_last_result switch are unchanged.  Returns 0. */
int rays_hip_finalize(void);
int rays_hip_device_count(void);
/* sizeof(rays_params_t) as compiled into the library: lets a foreign-language binding (ctypes,
 * iso_c_binding) verify its mirror of the struct. */
int rays_hip_sizeof_params(void);
/* Copies the last error message (NUL-terminated, truncated to len) and returns its length. */
int rays_hip_last_error(char* buf, int len);
/* Reference ode_stop_flag text for a stop code (e.g. " nstep > nstep_max"); "" if unknown. */
const char* rays_hip_stop_flag_text(int stop_code);
/* Z-function spline table for damping_model = 'damp_fund_ECH' (zfunctions_m.f90:436-466): the host
 * owns the table (the reference builds it in initialize_spline_coeffs); fspl_re is the PPPL-pspline
 * compact cubic spline fsplRe(4, nx) in Fortran order == C [nx][4], on the uniform grid
 * x_min .. x_max.  The library copies it; it must be set before tracing with damping. */
int rays_hip_set_zfun_table(const double* fspl_re, int nx, double x_min, double x_max);

/* Spline tables of equilib_model = 'axisym_toroid' with magnetics_model =
 * 'eqdsk_magnetics_spline_interp'.  Coefficient generation (PPPL pspline bcspline/cspline, not-a-knot)
 * stays on the host -- in RAYS it is initialize_eqdsk_magnetics_spline_interp /
 * initialize_density_spline_interp / initialize_temperature_spline_interp -- and only evaluation
 * (bcspeval / cspeval on uniform grids) runs on the device.  All arrays are the host objects'
 * own storage (type cube_spline_function_1D/2D, quick_cube_splines_m.f90:36-56):
 *   psi_fspl(4,4,nr,nz) Fortran order, on r_grid(nr) x z_grid(nz);   Psi - PSIAXIS
 *   rb_fspl(4,n_rb) on rb_grid:   T = R*Bphi
 *   ne/te/ti_fspl(4,n) on *_grid (psiN 0..1): profiles normalised to 1 on axis; n = 0 if unused.
 * magnetics_model = 'solovev_magnetics' (analytic field) has no psi / R*Bphi tables: the call is needed only
 * when n or T are splined, with nr = nz = n_rb = 0 and the profile tables alone.
 * The library copies everything; set before tracing. */
typedef struct rays_axisym_tables {
  int32_t nr, nz, n_rb, n_ne, n_te, n_ti;
  const double *r_grid, *z_grid, *psi_fspl;
  const double *rb_grid, *rb_fspl;
  const double *ne_grid, *ne_fspl;
  const double *te_grid, *te_fspl;
  const double *ti_grid, *ti_fspl;
} rays_axisym_tables_t;
int rays_hip_set_axisym_tables(const rays_axisym_tables_t* t);

/* Tables of magnetics_model = 'eqdsk_magnetics_lin_interp' (instead of rays_hip_set_axisym_tables): the host's
 * eqdsk_utilities_m arrays after initialize_eqdsk_magnetics_lin_interp (eqdsk_magnetics_lin_interp_m.f90:121-141),
 * in the same struct with this meaning:
 *   r_grid(nr) = R_grid, z_grid(nz) = Z_grid;   psi_fspl = Psi(nr, nz) Fortran order, PSIAXIS already subtracted;
 *   rb_fspl = T(nr) (= R*Bphi on R_grid), n_rb = nr, rb_grid unused (may be NULL);
 *   ne/te/ti_*: the splined profiles as in rays_hip_set_axisym_tables (n = 0 if unused);
 *   dR, dZ = eqdsk_utilities_m's dR, dZ (HALF the grid spacing, :137-138) -- the steps of GetPsiR .. GetRBphiR.
 * axisym.box_* and axisym.psiB (= PSIBOUND - PSIAXIS) travel in rays_params_t as for the spline model.
 * Where the reference's central differences index one cell beyond R_grid / Z_grid (a point in the outermost cells)
 * it reads the neighbouring column of Psi through Fortran's storage order; the library does the same and clamps only
 * what would leave the array altogether (undefined in the reference). */
int rays_hip_set_eqdsk_lin_tables(const rays_axisym_tables_t* t, double dR, double dZ);

/* Numerics of the trace kernels (process-wide; read when a trace is launched).
 *   RAYS_NUMERICS_EXACT (default): IEEE binary64 in the reference's operation order, no FMA contraction,
 *     correctly rounded quotients and roots -- trajectories bit-identical to the reference CPU path.
 *   RAYS_NUMERICS_TOLERANCE: NOT bit-identical -- the kernels fuse a*b+c, re-associate, use once-refined reciprocals
 *     and roots and algebraic short cuts.  What it is was measured on the full BASELINE fans against the reference
 *     (tests/test_gpu_numerics_full_fans.py, profiles/numerics_evidence.json): restarted from every recorded reference
 *     point, every step lands within 1e-10 relative (norm-wise on r and k) of the reference's next point -- the bar of
 *     BASELINE.json's north_star; measured 4.4e-15 over the headline fan's 12 873 661 steps, 1e-12 over 32.8 M steps of
 *     the slab fan -- and ray counts / step indices / stop flags are exactly the reference's on every ray surveyed;
 *     ACCUMULATED along a ray the trajectory deviates by up to 1.6e-8.  The steps where that bar cannot hold for any
 *     arithmetic but the reference's own (a ray's last recorded step before two modes coalesce) are handed over to a
 *     kernel of the exact build.  Built for ode_solver = RK4 with ray_deriv = cold (without
 *     multi_spec_damping); every other configuration runs its exact kernel under either setting (finite-difference
 *     dD amplifies an ulp by 1e8, and the adaptive solver then takes another step sequence).  The two-waves-per-SIMD
 *     build, which has no hand-over, serves slab fans only under this setting (they have no such step); Solovev and
 *     axisym fans of every size run the kernel with the hand-over.
 * The environment variable RAYS_HIP_NUMERICS = exact | tolerance sets the initial value.  Returns the previous
 * setting, or -1 for an unknown mode. */
enum { RAYS_NUMERICS_EXACT = 0, RAYS_NUMERICS_TOLERANCE = 1 };
int rays_hip_set_numerics(int mode);
int rays_hip_get_numerics(void);

/* Validates a parameter block exactly as the reference's `stop 1` configuration checks would;
 * 0 if the device path supports it. */
int rays_hip_check_params(const rays_params_t* p);

/* ---- the hot path, host-pointer form: replaces `call trace_rays` ---------------------------
 * Blocking.  Shards rays in contiguous blocks over the selected GPUs (the reference's
 * OpenMP `schedule(static)`, ray_tracing.f90:62), copies each device's contiguous output slab
 * straight into the caller's arrays.  Optional outputs may be NULL.
 * ray_vec / residual: points 1..npoints(i) of every ray are written; entries beyond are left as the
 * caller passed them -- as in the reference, whose arrays are zero-filled by
 * initialize_ray_results_m (ray_results_m.f90:154-164) before trace_rays runs.  (Only the
 * recorded points cross PCIe: packed on the device, unpacked by host threads.)  One caller thread at a
 * time, like the reference's trace_rays; the entry keeps its device buffers, pinned staging and stream
 * between calls until rays_hip_finalize().
 *   stop_code[nray]          integer image of ray_stop_flag(iray)          (ray_tracing.f90:258)
 *   end_ray_vec[nray][nv]    v at the last valid step                       (ray_tracing.f90:260)
 *   end_residuals[nray]      residual(nstep,iray)                           (ray_tracing.f90:255)
 *   max_residuals[nray]      maxval(abs(residual(1:nstep,iray)))            (ray_tracing.f90:256)
 *   elapsed_s                wall seconds of the device work incl. copies
 */
int rays_hip_trace(const rays_params_t* p, int nray,
                   const double* rvec0, const double* rindex_vec0,
                   double* ray_vec, double* residual, int32_t* npoints, int32_t* stop_code,
                   double* end_ray_vec, double* end_residuals, double* max_residuals,
                   double* elapsed_s);

/* ---- the hot path, device-pointer form ------------------------------------------------------
 * All pointers are device memory on the CURRENT HIP device; the launch is asynchronous on
 * `hip_stream` (a hipStream_t, NULL = default stream).  ray_vec/residual are zero-filled by the
 * call (hipMemsetAsync on the same stream) unless RAYS_TRACE_NO_ZERO_FILL is set in flags.
 * Used by the Python host (torch tensors), by bench.py, and by rays_hip_trace itself.
 */
enum { RAYS_TRACE_NO_ZERO_FILL = 1 };
int rays_hip_trace_device(const rays_params_t* p, int nray,
                          const double* d_rvec0, const double* d_rindex_vec0,
                          double* d_ray_vec, double* d_residual, int32_t* d_npoints,
                          int32_t* d_stop_code, double* d_end_ray_vec, double* d_end_residuals,
                          double* d_max_residuals, void* hip_stream, int flags);

/* ---- ray_scan fused into ONE launch ---------------------------------------
 * Replaces the reference's serial scan loop (ray_scan/ray_scan.f90:33-49: update_scan_parameter +
 * initialize + trace_rays per run; scanner_m.f90:174-205: scan_parameter = 'ds', the only physical one)
 * by one launch over n_runs x nray rays: run r traces the fan rvec0/rindex_vec0[nray][3] with
 * ds = d_ds_values[r]; everything else comes from p.  Outputs are the arrays of rays_hip_trace_device
 * with a leading run dimension: ray_vec[n_runs][nray][nstep_max+1][nv], npoints[n_runs][nray], ...
 * Each run's results are those of a stand-alone trace with that ds, bit for bit. */
int rays_hip_scan_device(const rays_params_t* p, int n_runs, const double* d_ds_values, int nray,
                         const double* d_rvec0, const double* d_rindex_vec0, double* d_ray_vec,
                         double* d_residual, int32_t* d_npoints, int32_t* d_stop_code,
                         double* d_end_ray_vec, double* d_end_residuals, double* d_max_residuals,
                         void* hip_stream, int flags);

/* ---- summary-only tracing: ray ends and residual statistics, no trajectories --------------------
 * For callers that never look at a trajectory -- the reference's own ray_scan, which keeps six things per run
 * (scanner_m.f90:213-227, :236-284: end_ray_parameter, end_residuals, max_residuals, start_ray_vec, end_ray_vec,
 * ray_stop_flag), aiming and absorbed-fraction surveys (end_ray_vec(8)), a Fortran host that would otherwise pull
 * every recorded point over PCIe.  The same rays, steps and stop logic as rays_hip_trace_device, from kernels compiled
 * without the recording path (EQ + 32 in their names): ray_vec(:,:,:) and residual(:,:) do not exist, on the device
 * or anywhere else, and the library allocates nothing that scales with nstep_max.  Per ray:
 *   npoints[nray], stop_code[nray], end_ray_vec[nray][nv], end_residuals[nray], max_residuals[nray]
 *                            exactly what rays_hip_trace_device puts there, bit for bit (all required)
 *   start_ray_vec[nray][nv]  ray_vec(:, 1, iray) of the full trace (ray_tracing.f90:259) -- also for a ray the initial
 *                            check_save refuses; may be NULL
 *   end_ray_parameter is end_ray_vec(7, iray); a ray's steps are npoints - 1.
 * NUMERICS: these entries always run the EXACT kernels, whatever rays_hip_set_numerics says.  The tolerance setting
 * is a permission, and exact results satisfy it; a tolerance variant would need recorded points both to evidence its
 * per-step bar and for its hand-over, which reads residual(:).
 * Built for every shape the library traces (the same lists; all of them under make FULL=1); another is refused by
 * the message of rays_hip_check_params.  Refused by name: a null required pointer, nray < 0, n_runs * nray > 2^31 - 1.
 * The device forms are asynchronous on hip_stream like rays_hip_trace_device. */
int rays_hip_trace_summary_device(const rays_params_t* p, int nray, const double* d_rvec0,
                                  const double* d_rindex_vec0, int32_t* d_npoints, int32_t* d_stop_code,
                                  double* d_start_ray_vec /* may be NULL */, double* d_end_ray_vec,
                                  double* d_end_residuals, double* d_max_residuals, void* hip_stream);
/* The fused scan of rays_hip_scan_device, summary-only: outputs with a leading run dimension, npoints[n_runs][nray],
 * start_ray_vec[n_runs][nray][nv], ...; each run equals a stand-alone summary trace with its ds. */
int rays_hip_scan_summary_device(const rays_params_t* p, int n_runs, const double* d_ds_values, int nray,
                                 const double* d_rvec0, const double* d_rindex_vec0, int32_t* d_npoints,
                                 int32_t* d_stop_code, double* d_start_ray_vec /* may be NULL */,
                                 double* d_end_ray_vec, double* d_end_residuals, double* d_max_residuals,
                                 void* hip_stream);
/* Host pointers, blocking.  Shards the rays over the devices of rays_hip_init[_devices] exactly as rays_hip_trace
 * does (contiguous blocks, one host thread per device) with that entry's resource owners, and copies only the
 * summaries: 16 + 8 (2 nv + 2) bytes per ray.  A device image kept by rays_hip_keep_last_result is dropped (it is not
 * this call's result) and none is left. */
int rays_hip_trace_summary(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                           int32_t* npoints, int32_t* stop_code, double* start_ray_vec /* may be NULL */,
                           double* end_ray_vec, double* end_residuals, double* max_residuals,
                           double* elapsed_s /* may be NULL */);
/* Name of the kernel the summary entries launch for a fan of nray rays ("" when p is refused). */
const char* rays_hip_summary_kernel_name_for(const rays_params_t* p, int nray);

/* ---- fused trace and deposition: the absorbed-power profile without trajectories ---------------------------------
 * A heating run needs one thing from a fan of damped rays: the deposition profile.  These entries trace the rays with
 * the summary-only kernels' twins that ALSO bin every accepted point (EQ + 96 in their names: the summary-only bit 32
 * and the deposition bit 64): the binner reads the grid value of a point (psiN, rho(psiN) or x) and ray_vec(8) *
 * initial_ray_power at two consecutive recorded points, and both are in the lane's registers when check_save accepts a
 * point.  The statements are the post-processor's own (one device function shared with rays_hip_deposition_device), a
 * step check_save refuses is neither recorded nor binned, and a ray refused at its initial check has one point and no
 * segment.  So:
 *   npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals
 *                            exactly those of rays_hip_trace_summary_device, bit for bit
 *   work[n_bins][nray], profile[n_bins]
 *                            exactly those of rays_hip_trace_device followed by rays_hip_deposition_device, bit for bit
 * and nothing that scales with nstep_max is allocated anywhere.
 * Device form: asynchronous on hip_stream.  d_work (required: it is the kernels' accumulator, bin-major like
 * rays_hip_deposition_device's) is zeroed by the call; the profile is the ray-ordered sum over d_work continued from
 * d_profile_in (NULL = from zero), so consecutive ray blocks chain bit for bit.  d_profile_in == d_profile_out is allowed.
 * One caller thread per (device, stream), as for rays_hip_ode_step_device (a 64-byte argument block per stream is kept
 * and released by rays_hip_finalize).
 * NUMERICS: always the EXACT kernels, whatever rays_hip_set_numerics says (see the summary entries).
 * Refused by name, before anything is allocated or launched: damping_model = no_damp or nv without the absorbed-power
 * row; equilib_model = solovev; Ptotal_psi / Ptotal_rho on a slab, Ptotal_x on axisym_toroid; Ptotal_rho without
 * rays_hip_set_rho_table or for the two magnetics models without rho; n_bins outside 1..RAYS_DEP_MAX_BINS; a null
 * required pointer; nray < 0; a shape that is not built (the message of rays_hip_check_params).
 * OUT OF SCOPE here: a tolerance variant, more than RAYS_DEP_MAX_BINS (320) bins.  (Several profiles in one pass:
 * rays_hip_trace_profiles* below; the fused ds scan and one profile per beam: rays_hip_scan_profiles_device and
 * rays_hip_trace_profiles_segments_device further below.) */
int rays_hip_trace_deposition_device(const rays_params_t* p, int nray, const double* d_rvec0,
                                     const double* d_rindex_vec0, const double* d_initial_ray_power, int which,
                                     int n_bins, int32_t* d_npoints, int32_t* d_stop_code,
                                     double* d_start_ray_vec /* may be NULL */, double* d_end_ray_vec,
                                     double* d_end_residuals, double* d_max_residuals,
                                     double* d_work /* [n_bins][nray] */, const double* d_profile_in /* may be NULL */,
                                     double* d_profile_out, void* hip_stream);
/* Host pointers, blocking.  Shards the rays like rays_hip_trace_summary (the devices of rays_hip_init[_devices],
 * contiguous blocks, that entry's resource owners), carries the running sums from block to block in ray order as
 * rays_hip_deposition_last does -- the profile is the single-block result bit for bit, whatever the device list -- and
 * copies the summaries, profile[n_bins] and, if asked, work in the reference's layout work(n_bins, nray) =
 * C [nray][n_bins] (may be NULL).  A device image kept by rays_hip_keep_last_result is dropped and none is left. */
int rays_hip_trace_deposition(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                              const double* initial_ray_power, int which, int n_bins, int32_t* npoints,
                              int32_t* stop_code, double* start_ray_vec /* may be NULL */, double* end_ray_vec,
                              double* end_residuals, double* max_residuals, double* work /* may be NULL */,
                              double* profile, double* elapsed_s /* may be NULL */);
/* Name of the kernel the fused entries launch for a fan of nray rays ("" when p is refused or has no such kernel). */
const char* rays_hip_deposition_kernel_name_for(const rays_params_t* p, int nray);

/* ---- fused deposition into every profile of the equilibrium, in one trace pass -----------------------------------
 * The reference post-processor never bins one profile: calculate_deposition_profiles loops over all profiles of the
 * equilibrium (deposition_profiles_m.f90:228-260) -- Ptotal_psi and Ptotal_rho for axisym_toroid on the eqdsk splines,
 * Ptotal_x alone for the slab.  These entries take the list.
 *   n_profiles == 1   rays_hip_trace_deposition[_device] itself: the same kernel (EQ + 96), the same bytes
 *   n_profiles == 2   ONE launch of the two-profile kernel (EQ + 352 in its name: + the bit 256): the grid value is
 *                     evaluated once per accepted point -- psiN, then rho(psiN) from it -- and the segment is binned
 *                     into both rows, with the post-processor's statements.  Each work / profile is bit for bit what
 *                     the single-profile entry gives for that record; the two bin counts are independent.
 * Device form: asynchronous on hip_stream; `profiles` is a HOST array of records that hold DEVICE pointers.  Each work
 * (required, [n_bins][nray] bin-major) is zeroed by the call; each profile is the ray-ordered sum over its work
 * continued from its own profile_in (NULL = from zero; profile_in == profile is allowed).  One caller thread per
 * (device, stream); a 96-byte argument block per stream is kept and released by rays_hip_finalize.  Always the EXACT
 * kernels.
 * Host form: blocking, sharded and chained in ray order like rays_hip_trace_deposition; work is the reference's layout
 * [nray][n_bins] and may be NULL; profile_in must be NULL.  A kept device image is dropped.
 * Refused by name, before anything is allocated or launched: everything rays_hip_trace_deposition_device refuses, for
 * each record; n_profiles outside 1..RAYS_DEP_MAX_PROFILES; the same `which` twice; two profiles on a configuration
 * that has one (the single-profile refusal's message); a null work or profile in the device form; a non-null
 * profile_in in the host form.
 * OUT OF SCOPE: more than two profiles, the same profile at two bin counts, a tolerance variant.  (In windows:
 * rays_hip_trace_window_profiles_device below.) */
#define RAYS_DEP_MAX_PROFILES 2
typedef struct rays_dep_profile {
  int which, n_bins;          /* RAYS_DEP_PTOTAL_*; 1..RAYS_DEP_MAX_BINS */
  double* work;               /* device form: [n_bins][nray], required.  host form: [nray][n_bins], may be NULL */
  const double* profile_in;   /* device form: running sums to continue, may be NULL; host form: must be NULL */
  double* profile;            /* [n_bins] */
} rays_dep_profile_t;
int rays_hip_trace_profiles_device(const rays_params_t* p, int nray, const double* d_rvec0,
                                   const double* d_rindex_vec0, const double* d_initial_ray_power, int n_profiles,
                                   const rays_dep_profile_t* profiles /* host array of device pointers */,
                                   int32_t* d_npoints, int32_t* d_stop_code, double* d_start_ray_vec /* may be NULL */,
                                   double* d_end_ray_vec, double* d_end_residuals, double* d_max_residuals,
                                   void* hip_stream);
int rays_hip_trace_profiles(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                            const double* initial_ray_power, int n_profiles, const rays_dep_profile_t* profiles,
                            int32_t* npoints, int32_t* stop_code, double* start_ray_vec /* may be NULL */,
                            double* end_ray_vec, double* end_residuals, double* max_residuals,
                            double* elapsed_s /* may be NULL */);
/* Name of the kernel rays_hip_trace_profiles* launch for n_profiles records ("" when p is refused or has no such
 * kernel: two profiles on a slab or Solovev configuration). */
const char* rays_hip_profiles_kernel_name_for(const rays_params_t* p, int nray, int n_profiles);
/* The profiles of the configuration's equilibrium in the reference's order, as RAYS_DEP_PTOTAL_* in
 * which[RAYS_DEP_MAX_PROFILES]; returns their number.  Slab: x.  axisym_toroid on the eqdsk splines with a rho table
 * set: psi, rho; the other two magnetics models, or no rho table: psi.  Solovev (or p refused): 0. */
int rays_hip_deposition_profile_set(const rays_params_t* p, int* which);

/* ---- segmented deposition: the fused ds scan and one profile per beam, in one pass --------------------------------
 * The fused entries above sum every ray of a launch into ONE profile per record.  Two users want more than one from a
 * launch: the ds scan (ray_scan: the same fan at n_runs step sizes, each run with a profile of its own, e.g. to see
 * whether the deposition profile has converged in ds) and the aiming survey (many beams at one ds -- steering angles,
 * launch positions, the ragged blocks rays_hip_ray_init_device returns -- each beam with its own profile).  The trace
 * kernels need nothing new for either: every ray owns its column of work, and the step of a ray was already
 * ds_values[ray / rays_per_run] in a scan launch.  What these entries add is the ray-ordered sum PER SEGMENT of rays.
 *   A segment s is the rays off[s] .. off[s+1]-1, off an int32 DEVICE array of n_seg + 1 entries; or, with
 *   d_seg_offsets == NULL, the rays s * rays_per_seg .. (s + 1) * rays_per_seg - 1.
 *   profile[s][b] = carry[s][b] + work[b][off[s]] + work[b][off[s]+1] + ... + work[b][off[s+1]-1]
 * with the adds in exactly that order and nothing else added.  An empty segment gives carry[s][b], or +0.0 without a
 * carry (d_profile_in == NULL starts every sum from +0.0; d_profile_in == d_profile_out is allowed).  Every offset is
 * clamped to [0, nray] on the device and end < start counts as empty, so no offset value makes the sum read outside
 * work; rays before off[0] and from off[n_seg] on belong to no profile.
 * RELATION TO THE SINGLE SUM: the kernel of the entries above pads its last chunk of rays with +0.0, which shows only
 * when a caller's profile_in holds -0.0 (-0.0 + +0.0 = +0.0); the segmented sum adds nothing but the segment's rays.  For
 * carries that are not -0.0, one segment [0, nray] equals those entries' profile bit for bit.
 * All three entries are asynchronous on hip_stream, always run the EXACT kernels, and follow the fused entries' rule:
 * one caller thread per (device, stream).
 *
 * rays_hip_profile_sum_segments_device: the sum on its own, e.g. behind rays_hip_deposition_device on the trajectories of
 * a scan or of a many-beam fan, from the work it already wrote.  d_work is [n_bins][nray]; d_profile_in (may be NULL)
 * and d_profile_out are [n_seg][n_bins].  n_seg == 0 does nothing.
 *
 * rays_hip_scan_profiles_device: the fused ds scan.  d_rvec0, d_rindex_vec0 and d_initial_ray_power are per fan member
 * ([nray]), as in rays_hip_scan_summary_device; ray r * nray + i is member i at step d_ds_values[r].  Each record's
 * work is [n_bins][n_runs * nray] (run r owns the columns r * nray ..), its profile and profile_in [n_runs][n_bins]; the
 * summaries are [n_runs * nray].  The call zeroes each work, tiles the power to one weight per ray in a workspace kept
 * per (device, stream) (grown on demand, released by rays_hip_finalize), launches the fused kernel of one or two
 * profiles with the per-run steps, and sums per run.  Run r is bit for bit what rays_hip_trace_profiles_device gives
 * with ds = d_ds_values[r]; profile_in chains the member blocks of a fan per run.  n_runs == 0 does nothing; nray == 0
 * writes profile_in, or zeros.
 *
 * rays_hip_trace_profiles_segments_device: the arguments of rays_hip_trace_profiles_device and the segments: the same
 * fused pass at the run's one ds, with profile and profile_in of each record [n_seg][n_bins].  work is that entry's.
 *
 * Refused by name, before anything is allocated or launched: everything rays_hip_trace_profiles_device refuses; n_runs
 * < 0; n_runs * nray beyond 2^31 - 1; a null d_ds_values; n_seg < 0; neither offsets nor a positive rays_per_seg when
 * n_seg > 0; (the sum alone) n_bins < 1, nray < 0, a null work or profile.
 * OUT OF SCOPE: host-pointer (sharded) forms, windows over a scan, a tolerance variant, a scan parameter other than ds. */
int rays_hip_profile_sum_segments_device(int n_bins, int nray, int n_seg, const int32_t* d_seg_offsets /* may be NULL */,
                                         int rays_per_seg, const double* d_work /* [n_bins][nray] */,
                                         const double* d_profile_in /* [n_seg][n_bins] or NULL */,
                                         double* d_profile_out /* [n_seg][n_bins] */, void* hip_stream);
int rays_hip_scan_profiles_device(const rays_params_t* p, int n_runs, const double* d_ds_values, int nray,
                                  const double* d_rvec0, const double* d_rindex_vec0,
                                  const double* d_initial_ray_power /* [nray], per fan member */, int n_profiles,
                                  const rays_dep_profile_t* profiles /* host array of device pointers */,
                                  int32_t* d_npoints, int32_t* d_stop_code, double* d_start_ray_vec /* may be NULL */,
                                  double* d_end_ray_vec, double* d_end_residuals, double* d_max_residuals,
                                  void* hip_stream);
int rays_hip_trace_profiles_segments_device(const rays_params_t* p, int nray, const double* d_rvec0,
                                            const double* d_rindex_vec0, const double* d_initial_ray_power,
                                            int n_profiles,
                                            const rays_dep_profile_t* profiles /* host array of device pointers */,
                                            int n_seg, const int32_t* d_seg_offsets /* may be NULL */, int rays_per_seg,
                                            int32_t* d_npoints, int32_t* d_stop_code,
                                            double* d_start_ray_vec /* may be NULL */, double* d_end_ray_vec,
                                            double* d_end_residuals, double* d_max_residuals, void* hip_stream);

/* ---- windowed tracing: pause rays after n steps, continue from a saved state ---------------------------------------
 * Every entry above runs a ray from its launch point to its end in one launch, so whoever wants trajectories holds
 * ray_vec[nray][nstep_max+1][nv] on the device at once.  These entries advance a fan in WINDOWS of at most n_steps
 * recorded steps per ray: between two windows everything a ray needs to go on is in a saved state, a struct of device
 * arrays the caller owns (and may copy to disk and back: nothing in it is an address or depends on the launch):
 *   v[nray][nv]        the ray's last recorded point (of an ended ray: the state the reference leaves in v)
 *   s[nray]            sout as ray_tracing.f90:118 finds it at the top of the next trip, not yet advanced
 *   nstep[nray]        steps taken and recorded so far (npoints - 1)
 *   stop_code[nray]    RAYS_STOP_NONE: under way; else the ray has ended with this code
 *   resid[nray][3]     residual of the last recorded point, of the one before, running max |residual|
 *                      (ray_tracing.f90:252-260: end_residuals, max_residuals)
 *   sg_err[nray][2]    SG_ODE: ray_stop%rel_err, %abs_err, which persist and grow across output steps
 *                      (SG_ode_m.f90:115-126) and are reset only by ray_init_ode_solver.  Required for SG_ODE; may be
 *                      NULL for RK4_ODE.
 *   flags[nray]        bit 0 (RAYS_STATE_REFUSED): the initial check_save refused the ray -- npoints 1 and every summary
 *                      field zero, unlike a ray that started and ended on its first step (npoints 1, end_ray_vec = v)
 * A ray that is under way is exactly where trace_rays stands at ray_tracing.f90:116, before any of the three tests of
 * the next trip: nstep steps taken and recorded, v the last recorded point, s not yet advanced.
 *
 * rays_hip_state_init_device   initialize_ode_vector and the initial check_save (ray_tracing.f90:77-112) for every ray;
 *                              a refused ray gets its stop code here.  d_start_ray_vec[nray][nv] (may be NULL) is point
 *                              1 of every ray; its residual is 0.
 * rays_hip_trace_window_device advances every ray under way by at most n_steps recorded steps and updates the state in
 *                              place.  d_ray_vec_win[nray][n_steps][nv], d_residual_win[nray][n_steps] receive only the
 *                              points recorded by this call (not zero-filled beyond them), d_npoints_win[nray] their
 *                              number: 0 for a ray that had ended before.  Both window arrays NULL: the summary policy
 *                              -- nothing that scales with n_steps or nstep_max exists anywhere.  p->nstep_max and
 *                              p->s_max stay limits of the WHOLE ray: ' nstep > nstep_max' is given when the ray's own
 *                              count reaches nstep_max, never at a window's end.
 * rays_hip_state_summary_device the five per-ray summary arrays of rays_hip_trace_device from the state; rays under
 *                              way are included as they stand.
 * CONTRACT: point 1 followed by the windows' points equals one rays_hip_trace_device call bit for bit -- ray_vec,
 * residual, npoints, stop_code -- for any sequence of n_steps >= 1, recording and summary windows mixed freely, and the
 * summaries after the last window equal rays_hip_trace_summary_device's.  Once every ray has ended, further calls
 * change no byte of the state and return npoints_win = 0.
 * KERNELS: the one-ray-per-lane trace kernel of the shape, compiled with the continuation bit (EQ + 128 in the name;
 * EQ + 160 for the summary policy), whatever the fan size -- bit-identical to the two-waves-per-SIMD and lane-group
 * kernels.  Always exact, whatever rays_hip_set_numerics says (see the summary entries).  Built for every shape the
 * library traces.
 * Asynchronous on hip_stream.  Refused by name, before anything is launched: n_steps < 1, nray < 0, a null required
 * pointer, sg_err == NULL with SG_ODE, only one of the two window arrays, a shape that is not built.
 * OUT OF SCOPE: continuing the fused ds scan; a tolerance flavour; re-opening a ray that ended with
 * ' nstep > nstep_max' under a larger nstep_max (its s has been advanced).  (Continuing the fused deposition variant:
 * rays_hip_trace_window_profiles_device below.) */
#define RAYS_STATE_REFUSED 1
typedef struct rays_ray_state {
  double* v;          /* [nray][nv] */
  double* s;          /* [nray] */
  int32_t* nstep;     /* [nray] */
  int32_t* stop_code; /* [nray] */
  double* resid;      /* [nray][3] */
  double* sg_err;     /* [nray][2]; may be NULL for RK4_ODE */
  int32_t* flags;     /* [nray] */
} rays_ray_state_t;
int rays_hip_state_init_device(const rays_params_t* p, int nray, const double* d_rvec0, const double* d_rindex_vec0,
                               const rays_ray_state_t* state, double* d_start_ray_vec /* may be NULL */,
                               void* hip_stream);
int rays_hip_trace_window_device(const rays_params_t* p, int nray, const rays_ray_state_t* state, int n_steps,
                                 double* d_ray_vec_win /* NULL with d_residual_win: summary policy */,
                                 double* d_residual_win, int32_t* d_npoints_win, void* hip_stream);
int rays_hip_state_summary_device(const rays_params_t* p, int nray, const rays_ray_state_t* state, int32_t* d_npoints,
                                  int32_t* d_stop_code, double* d_end_ray_vec, double* d_end_residuals,
                                  double* d_max_residuals, void* hip_stream);
/* Name of the kernel rays_hip_trace_window_device launches (recording != 0: with window arrays; 0: summary policy);
 * "" when p is refused or has no such kernel. */
const char* rays_hip_window_kernel_name_for(const rays_params_t* p, int nray, int recording);
/* ---- deposition windows: the fused deposition kernels continued from the saved state --------------------------------
 * rays_hip_trace_window_profiles_device advances the state exactly as a summary-policy rays_hip_trace_window_device
 * call does (no trajectory exists) and bins every point the window accepts into the rows of `profiles`, a HOST array of
 * 1..RAYS_DEP_MAX_PROFILES records holding DEVICE pointers:
 *   n_profiles == 1   the continuation variant of the fused deposition kernel (EQ + 224 in its name)
 *   n_profiles == 2   that of the two-profile kernel (EQ + 480), axisym_toroid with a rho table only
 *   work              [n_bins][nray] bin-major, required.  An ACCUMULATOR: the call never zeroes it.  The caller zeroes
 *                     it once, when it calls rays_hip_state_init_device, and hands the same array to every window.
 *   profile           may be NULL: then no sum is run (an intermediate window need not pay for it).  Otherwise the
 *                     ray-ordered sum over the work SO FAR, continued from profile_in (NULL = from zero).
 * d_initial_ray_power[nray] is required.  d_npoints_win[nray]: the points this call accepted, 0 for a ray that had ended.
 * A paused ray's saved v is its last recorded point and the last point binned: the launch that continues it evaluates
 * the grid value(s) and v(8) * power there again, which are the values the one-shot kernel carries in registers.
 * CONTRACT: start from rays_hip_state_init_device with zeroed works and run any sequence of deposition windows with
 * n_steps >= 1 until every ray has ended.  Then each work and profile equals rays_hip_trace_profiles_device's on the
 * same rays bit for bit, and rays_hip_state_summary_device gives the one-shot summaries.  After any prefix of the
 * sequence each work equals rays_hip_deposition_device on the one-shot trajectories with npoints clipped to
 * state.nstep + 1.  Once every ray has ended, further calls change no byte of the state or the works and return
 * npoints_win = 0.
 * THE CALLER'S CHOICE, not detectable: steps taken by a plain rays_hip_trace_window_device call in between are not
 * binned (the next deposition window starts its segments from the point that call left).
 * Asynchronous on hip_stream; one caller thread per (device, stream); the argument block is the one the one-shot
 * entries keep per stream, released by rays_hip_finalize.  Always the EXACT kernels.
 * Refused by name, before anything is launched: everything rays_hip_trace_profiles_device refuses, for each record
 * (but a null profile is allowed); everything rays_hip_trace_window_device refuses; a null d_initial_ray_power.
 * OUT OF SCOPE: a host form; recording windows that also bin; the fused ds scan; a tolerance variant. */
int rays_hip_trace_window_profiles_device(const rays_params_t* p, int nray, const rays_ray_state_t* state, int n_steps,
                                          const double* d_initial_ray_power, int n_profiles,
                                          const rays_dep_profile_t* profiles /* host array of device pointers */,
                                          int32_t* d_npoints_win, void* hip_stream);
/* Name of the kernel rays_hip_trace_window_profiles_device launches for n_profiles records ("" when p is refused or
 * has no such kernel). */
const char* rays_hip_window_profiles_kernel_name_for(const rays_params_t* p, int nray, int n_profiles);

/* Host pointers, blocking: the arguments and the results of rays_hip_trace, bit for bit (entries past npoints are left
 * as the caller passed them), traced in windows of n_steps.  Device memory is the ray state, two window slabs
 * [nray][n_steps][nv + 1] and the inputs, whatever nstep_max is; window k is copied out (whole slabs, through pinned
 * staging buffers of one slab each) and scattered into the caller's arrays while window k + 1 runs.  One device: the
 * first of rays_hip_init[_devices].  Uses rays_hip_trace's resource owners -- everything is freed by
 * rays_hip_finalize.  A device image kept by rays_hip_keep_last_result is dropped and none is left. */
int rays_hip_trace_windowed(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                            int n_steps, double* ray_vec, double* residual, int32_t* npoints, int32_t* stop_code,
                            double* end_ray_vec /* may be NULL */, double* end_residuals /* may be NULL */,
                            double* max_residuals /* may be NULL */, double* elapsed_s /* may be NULL */);

/* ---- one output step from arbitrary states: the ode_m interface --------------------------------
 * Batched image of `call ode_solver(eqn_ray, nv, v, s, sout, ray_stop)` (ode_m.f90:218-254, with
 * sout = s + ds and, for SG_ODE, ray_stop%rel_err/abs_err at rel_err0/abs_err0 as after
 * ray_init_ode_solver, ode_m.f90:182-214) followed by the check_save trace_rays applies to the new point
 * (ray_tracing.f90:212-243).  d_v0[n][nv] states, d_s0[n] ray parameters (NULL = 0) -> d_v1[n][nv],
 * d_resid[n] (may be NULL), d_stop_code[n]: RAYS_STOP_NONE when the step was taken and kept, then v1 is the new
 * state.  Otherwise v1 is what ode_solver left in v: the advanced state when check_save refused the step
 * (ray_tracing.f90:214-234), v0 when the solver itself stopped (RK4_ode_m.f90:83-89), zeros when v0 already failed
 * the initial check_save (such a ray never starts: ray_tracing.f90:100-112) -- a recorded trajectory point always
 * passes it.  ASYNCHRONOUS on hip_stream like rays_hip_trace_device (it was blocking before round 3): synchronise the
 * stream -- hipStreamSynchronize, or hipDeviceSynchronize for the null stream -- before reading d_v1 / d_resid /
 * d_stop_code on the host or from another stream.  Its scratch (one block per device and stream) is kept between
 * calls and released by rays_hip_finalize; ONE caller thread per (device, stream): a second thread that asks the same
 * stream for a larger block frees the first one's behind hipStreamSynchronize, which does not cover work the first
 * thread has not enqueued yet. */
int rays_hip_ode_step_device(const rays_params_t* p, int n, const double* d_v0, const double* d_s0,
                             double* d_v1, double* d_resid, int32_t* d_stop_code, void* hip_stream);

/* Name of the kernel specialisation rays_hip_trace_device would launch for p (for profiling
 * scripts: matches the rocprofv3 kernel-trace name prefix). */
const char* rays_hip_kernel_name(const rays_params_t* p);
/* Same for a fan of nray rays: large fans may get a differently tuned build of the kernel. */
const char* rays_hip_kernel_name_for(const rays_params_t* p, int nray);
/* Which step loop that kernel runs for p: the one-wave-per-SIMD RK4 kernels of the Solovev equilibrium (analytic
 * derivatives, up to two species) hold their step loop twice under ONE name -- 1: the lean loop, compiled for a run whose
 * density model is not 'constant', whose species have no parabolic temperature profile and whose ray_param is not
 * 'arcl'; 0: the general loop (every other kernel and parameter set; every launch while the developer switch
 * RAYS_HIP_RK4_LOOP=general is set in the environment).  -1: p is refused or is not an RK4 configuration.  Summary-only,
 * fused-deposition and rays_hip_ode_step_device launches of p take the same loop. */
int rays_hip_rk4_loop_for(const rays_params_t* p, int nray);

/* ---- multi-GPU trace with a device-resident result: the final trajectory gather over RCCL -------
 * (north_star: "RCCL over xGMI used only for the final trajectory gather".)
 * Shards the rays in contiguous blocks over the devices chosen by rays_hip_init[_devices] (distinct devices;
 * one host thread per device, like rays_hip_trace), traces every block on its device, then gathers the blocks'
 * PACKED trajectories and per-ray summaries on the root (= the first device of the list) with one grouped batch of
 * ncclSend/ncclRecv -- every peer uses its own xGMI link to the root -- and unpacks them there into the padded
 * reference layout.  The result stays in device memory on the root, owned by the library and valid until the
 * next rays_hip_trace_gather call or rays_hip_finalize; follow-on device work (rays_hip_deposition_device) can
 * consume it in place, rays_hip_result_to_host copies it out.  librccl.so is loaded on the first call with more
 * than one device.  rvec0 / rindex_vec0 are host arrays ([nray][3]). */
typedef struct rays_device_result {
  int32_t device, nray;
  double* ray_vec;       /* [nray][nstep_max+1][nv], zero past npoints */
  double* residual;      /* [nray][nstep_max+1] */
  int32_t* npoints;      /* [nray] */
  int32_t* stop_code;    /* [nray] */
  double* end_ray_vec;   /* [nray][nv] */
  double* end_residuals; /* [nray] */
  double* max_residuals; /* [nray] */
} rays_device_result_t;
int rays_hip_trace_gather(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                          rays_device_result_t* result);
int rays_hip_result_to_host(const rays_params_t* p, const rays_device_result_t* result, double* ray_vec,
                            double* residual, int32_t* npoints, int32_t* stop_code, double* end_ray_vec,
                            double* end_residuals, double* max_residuals);

/* ---- multi-GPU trajectory exchange helpers ---------------------------------
 * The padded reference layout is mostly zeros (a ray uses npoints of nstep_max+1 slots).  Before
 * the RCCL gather a rank packs its slab to packed_vec[sum(npoints)][nv], packed_res[sum(npoints)]
 * (d_offsets = exclusive prefix sum of npoints, int64); the root unpacks a peer's block into its
 * slab of the padded global arrays (which must be zero-filled beforehand).  Device pointers,
 * asynchronous on hip_stream. */
int rays_hip_pack_device(int nray, int nv, int nstep_max, const int32_t* d_npoints,
                         const int64_t* d_offsets, const double* d_ray_vec, const double* d_residual,
                         double* d_packed_vec, double* d_packed_res, void* hip_stream);
int rays_hip_unpack_device(int nray, int nv, int nstep_max, const int32_t* d_npoints,
                           const int64_t* d_offsets, const double* d_packed_vec,
                           const double* d_packed_res, double* d_ray_vec, double* d_residual,
                           void* hip_stream);

/* ---- ray initialisation on the device (the step before the hot path) -------
 * Replaces the reference's serial launch loops
 *   ray_init_solovev_nphi_ntheta            solovev_ray_init_nphi_ntheta_m.f90:60-198
 *   ray_init_axisym_toroid_R_Z_nphi_ntheta  axisym_toroid_ray_init_R_Z_nphi_ntheta_m.f90:67-244
 *   simple_slab_ray_init                    simple_slab_ray_init_m.f90:59-187
 * (each: equilibrium at the launch point + cold dispersion root solve_n1_vs_n2_n3 per fan member,
 * dispersion_solvers_m.f90:49-112; evanescent launches are dropped and the survivors numbered in
 * loop order).  rays_fan_t mirrors the launcher's namelist
 * (/solovev_ray_init_nphi_ktheta_list/, /axisym_toroid_ray_init_R_Z_nphi_ntheta_list/,
 * /simple_slab_ray_init_list/) plus wave_mode / k0_sign of /rf_list/ (rf_m.f90:28-34). */
enum { RAYS_RAY_INIT_SOLOVEV_NPHI_NTHETA = 0, RAYS_RAY_INIT_AXISYM_R_Z_NPHI_NTHETA = 1,
       RAYS_RAY_INIT_SIMPLE_SLAB = 2 };
enum { RAYS_WAVE_PLUS = 0, RAYS_WAVE_MINUS = 1, RAYS_WAVE_FAST = 2, RAYS_WAVE_SLOW = 3 };
typedef struct rays_fan {
  int32_t model;      /* RAYS_RAY_INIT_* ; must match rays_params_t.equilib_model */
  int32_t wave_mode;  /* RAYS_WAVE_* */
  int32_t k0_sign;    /* +1 | -1 */
  /* solovev / axisym_toroid fans */
  int32_t n_r_launch, n_theta_launch; /* solovev: minor radius x poloidal angle; axisym: n_R x n_Z */
  int32_t n_rindex_theta, n_rindex_phi;
  double r_launch0, dr_launch, theta_launch0, dtheta_launch; /* axisym: r_launch0 = R, z_launch0 = Z */
  double z_launch0;
  double rindex_theta0, delta_rindex_theta, rindex_phi0, delta_rindex_phi;
  /* simple slab */
  int32_t n_x_launch, n_y_launch, n_z_launch, n_ky_launch, n_kz_launch, pad_;
  double x_launch0, dx_launch, y_launch0, dy_launch, slab_z_launch0;
  double rindex_y0, delta_rindex_y0, rindex_z0, delta_rindex_z0;
} rays_fan_t;
int rays_hip_sizeof_fan(void);

/* Host-pointer form: fills rvec0[nray_max][3], rindex_vec0[nray_max][3], ray_pwr_wt[nray_max]
 * (= the reference's allocatable module arrays of ray_init_m.f90:47-53, C order) and *nray.
 * Returns non-zero with the reference's message when the launcher would `stop 1`
 * (improper number of rays, no successful initialisation). */
int rays_hip_ray_init(const rays_params_t* p, const rays_fan_t* fan, int nray_max, double* rvec0,
                      double* rindex_vec0, double* ray_pwr_wt, int32_t* nray);
/* Device-pointer form (current device; d_* hold nray_max x 3 doubles): the fan never visits the
 * host.  Synchronises `hip_stream` once to return *nray. */
int rays_hip_ray_init_device(const rays_params_t* p, const rays_fan_t* fan, int nray_max,
                             double* d_rvec0, double* d_rindex_vec0, int32_t* nray, void* hip_stream);

/* ---- deposition profiles on the device (the step after the hot path) --------
 * Replaces calculate_deposition_profiles / bin_a_ray (post_process_lib/deposition_profiles_m.f90:
 * 228-292) with its evaluators Ptotal_axisym_psi / Ptotal_axisym_rho (:458-503) and the uniform
 * grid binner (math_functions_lib/bin_to_uniform_grid_m.f90: binner_real), for
 * equilib_model = 'axisym_toroid' runs with damping (nv >= 8), and the slab's Ptotal_x (evaluator
 * Ptotal_x_slab_evaluator :438-452, grid [xmin, xmax] of the slab box :134-137), applied to the
 * trajectory arrays where rays_hip_trace_device left them.
 *   d_work[n_bins][nray]   per-ray binned power: the reference's work(n_bins, nray), stored bin-major
 *                          (scratch of the call; transposed so that the reduction reads coalesce)
 *   d_profile_out[n_bins]  = d_profile_in (or 0) + sum over rays IN RAY ORDER, the order of the
 *                          reference's sum(work, 2): ranks that hold consecutive ray blocks chain
 *                          their partial sums through d_profile_in and obtain the single-process
 *                          result bit for bit (a few-KB exchange instead of the trajectory gather).
 * Grid = [0, 1] in psiN or rho, [xmin, xmax] for Ptotal_x; the reference's default is n_bins = 100.
 * LIMIT: 1 <= n_bins <= RAYS_DEP_MAX_BINS = 320 (the binning kernel keeps the rows of one wave, 64 x n_bins doubles,
 * in the 160 KB of LDS of a compute unit).  All three entries refuse a larger n_bins with an error that names the
 * limit, before anything is allocated or launched.
 * Bins 1..n_bins receive exactly what the reference's statements give them; the one update the reference makes to
 * binned_Q(n_bins + 1) -- an upper segment end just below the grid maximum whose real-number index rounds up to
 * n_bins; undefined there -- is not made. */
#define RAYS_DEP_MAX_BINS 320
enum { RAYS_DEP_PTOTAL_PSI = 0, RAYS_DEP_PTOTAL_RHO = 1, RAYS_DEP_PTOTAL_X = 2 };
/* rho(psiN) spline of the eqdsk equilibrium (rho_profile of eqdsk_magnetics_spline_interp_m.f90:42,
 * 190-193; fspl(4, n) on grid(n)); needed for RAYS_DEP_PTOTAL_RHO.  Copied. */
int rays_hip_set_rho_table(const double* grid, const double* fspl, int n);
int rays_hip_deposition_device(const rays_params_t* p, int which, int n_bins, int nray,
                               const double* d_ray_vec, const int32_t* d_npoints,
                               const double* d_initial_ray_power, double* d_work,
                               const double* d_profile_in, double* d_profile_out, void* hip_stream);

/* Host-pointer form: ray_vec[nray][nstep_max+1][nv], npoints[nray], initial_ray_power[nray] are the
 * ray_results_m arrays; work[nray][n_bins] (= the reference's work(n_bins, nray), may be NULL) and
 * profile[n_bins] are filled.  Only points 1..maxval(npoints) of each ray cross PCIe. */
int rays_hip_deposition(const rays_params_t* p, int which, int n_bins, int nray, const double* ray_vec,
                        const int32_t* npoints, const double* initial_ray_power, double* work, double* profile);

/* The same profiles WITHOUT handing the trajectories back: the reference's drivers trace and post-process in one
 * process (RAYS_P.f90:19-44 -- trace_rays, then calculate_deposition_profiles on the same ray_results_m arrays,
 * deposition_profiles_m.f90:228-292).  rays_hip_keep_last_result(1) makes every later rays_hip_trace call leave the
 * device-resident image of its result (the padded ray_vec slabs and npoints of its blocks, on the devices that traced
 * them) in place until the next rays_hip_trace call, rays_hip_keep_last_result(0) or rays_hip_finalize; returns the
 * previous setting.  rays_hip_deposition_last bins that image: same arguments and results as rays_hip_deposition
 * minus the two arrays, blocks binned in ray order with the running sums carried from block to block (bit-identical
 * to the reference's ray-ordered sum for any number of blocks / devices).  Returns RAYS_HIP_NO_KEPT_RESULT (and
 * changes nothing) when no image of a trace with this nray / nv / nstep_max is held -- e.g. a post-processor that read
 * its arrays from a results file: call rays_hip_deposition then. */
#define RAYS_HIP_NO_KEPT_RESULT 5
int rays_hip_keep_last_result(int on);
int rays_hip_deposition_last(const rays_params_t* p, int which, int n_bins, int nray, const double* initial_ray_power,
                             double* work, double* profile);

/* ---- per-point ray diagnostics on the device (the post-processors' ray_detailed_diagnostics) ---------
 * Replaces the serial loop over every recorded point of every ray of
 *   ray_detailed_diagnostics        post_process_lib/axisym_toroid_processor_m.f90:252-482 (loop :351-419)
 *   ray_detailed_diagnostics_slab   post_process_lib/slab_processor_m.f90
 * (calculate_ray_diag = .true. is the processors' default): equilibrium + axisym_toroid_psi at the point and, with
 * damping, deriv_cold + damping for the imaginary index -- one GPU lane per recorded POINT.  Fields, per point:
 *   S, X, Y, Z, P_ABSORBED, RESIDUAL   copies: v(7), v(1), v(2), v(3), v(8) (0 when damping_model = 'no_damp'),
 *                                      residual(istep, iray)
 *   R                                  sqrt(x**2 + y**2)
 *   NE, MODB, ALPHA_E                  eq%ns(0), eq%bmag, eq%alpha(0)
 *   GAMMA_E                            abs(eq%gamma(0))
 *   TE_KEV                             eq%Ts(0)/e/1000.
 *   PSI                                psiN of axisym_toroid_psi (all three magnetics models); 0 for the slab.
 *                                      equilib_model = 'solovev' has no processor in the reference: an extension, PSI
 *                                      is then psiN of solovev_psi (solovev_eq_m.f90:308-318)
 *   N_PAR, N_PERP                      k3/k0, k1/k0 with k3 = sum(kvec*bunit), k1 = sqrt(sum((kvec - k3*bunit)**2))
 *   N_IMAG                             ki/k0, ki from damping(eq, v, vg = -dddk/dddw) with the COLD derivatives at
 *                                      nvec = kvec/k0 whatever ray_deriv is (the reference tests ray_dispersion_model);
 *                                      0 without damping
 *   XI_0, XI_1, XI_2                   (omgrf + m omgc(0))/(k3*vth), vth = sqrt(2.*ts(0)/ms(0)), m = 0, 1, 2, where
 *                                      ts(0) > 0 and abs(k3) > 0; else 0
 * The union of the axisym set and the slab set (X, Y there in place of Psi, R).  `fields` selects by bit
 * (1u << RAYS_DIAG_*); a field that is not selected costs neither its store nor, where separable, its arithmetic (no
 * equilibrium for the copies and R, no deriv_cold / damping without N_IMAG).  Always the exact arithmetic
 * (bit-identical to the reference's loop); rays_hip_set_numerics does not affect it.  Built for the species counts and
 * equilibria of the trace kernels (all of them under make FULL=1); another shape is refused by name.
 * The one behavioural difference: where the reference stops the program ('infinite group velocity',
 * abs(dddw) <= tiny(dddw), :395-400) the point gets N_IMAG = 0, first_bad_point[iray] is set to the 1-based index of
 * the ray's first such point (0 = none) and the call still returns 0. */
enum { RAYS_DIAG_S = 0, RAYS_DIAG_NE, RAYS_DIAG_TE_KEV, RAYS_DIAG_MODB, RAYS_DIAG_ALPHA_E, RAYS_DIAG_GAMMA_E,
       RAYS_DIAG_PSI, RAYS_DIAG_R, RAYS_DIAG_X, RAYS_DIAG_Y, RAYS_DIAG_Z, RAYS_DIAG_N_PAR, RAYS_DIAG_N_PERP,
       RAYS_DIAG_P_ABSORBED, RAYS_DIAG_N_IMAG, RAYS_DIAG_XI_0, RAYS_DIAG_XI_1, RAYS_DIAG_XI_2, RAYS_DIAG_RESIDUAL,
       RAYS_DIAG_NFIELDS };
/* Device-pointer form, on the arrays as rays_hip_trace_device left them (current device).
 * d_out[k][nray][nstep_max+1]: k counts the set bits of `fields` in enum order (== the reference's
 * field(max_number_of_points, number_of_rays) arrays, one after another); slots past npoints(iray) are written as
 * +0.0 by the call (the reference allocates with source = 0).  Asynchronous on hip_stream. */
int rays_hip_ray_diagnostics_device(const rays_params_t* p, int nray, const double* d_ray_vec,
                                    const double* d_residual, const int32_t* d_npoints, uint32_t fields,
                                    double* d_out, int32_t* d_first_bad_point /* may be NULL */, void* hip_stream);
/* The packed layout on the device: only recorded points, rays in order, points in order -- ray_vec[total][nv],
 * residual[total], one field [total] -- with the exclusive prefix sum of the rays' point counts to find a ray's run
 * (what rays_hip_pack_device / rays_hip_unpack_device and the RCCL gather already move).
 * rays_hip_point_offsets_device computes that prefix sum on the device: d_offsets[i] = sum over the rays before i of
 * clamp(npoints, 0, nstep_max + 1), i = 0 .. nray, so d_offsets[nray] is the total and the first nray entries are
 * what rays_hip_pack_device takes; nray = 0 writes the single 0.  Integer sums: exact.  Asynchronous on hip_stream, no
 * host synchronisation, no memory besides d_offsets (the current device). */
int rays_hip_point_offsets_device(int nray, int nstep_max, const int32_t* d_npoints,
                                  int64_t* d_offsets /* [nray + 1] */, void* hip_stream);
/* The diagnostics in the packed layout: point j (0-based) of ray i lands at d_out[k * out_stride + d_offsets[i] + j],
 * k counting the set bits of `fields` in enum order as above, and nothing else of d_out is written: there are no zero
 * slots, and the launched work follows the recorded points (one wave per 64 consecutive packed points).
 *   in_layout    RAYS_DIAG_IN_PADDED: d_ray_vec / d_residual are the arrays as rays_hip_trace_device left them;
 *                RAYS_DIAG_IN_PACKED: they are [total][nv] / [total] as rays_hip_pack_device wrote them
 *   d_offsets    [nray + 1], of rays_hip_point_offsets_device for this d_npoints
 *   out_stride   the caller's capacity per field, in doubles.  The call does not synchronise, so it cannot compare
 *                out_stride with d_offsets[nray]: THE KERNEL NEVER STORES AT AN INDEX >= out_stride OF A FIELD, points
 *                beyond it are dropped.  A caller that does not know the total passes its allocation size per field
 *                (nray * (nstep_max + 1) always suffices); one that has read d_offsets[nray] passes that.
 * Same fields, same `fields` semantics, same refusals and same first_bad_point as the padded entry; exact arithmetic
 * only.  Asynchronous on hip_stream (current device). */
enum { RAYS_DIAG_IN_PADDED = 0, RAYS_DIAG_IN_PACKED = 1 };
int rays_hip_ray_diagnostics_packed_device(const rays_params_t* p, int nray, int in_layout,
        const double* d_ray_vec, const double* d_residual, const int32_t* d_npoints,
        const int64_t* d_offsets /* [nray + 1] */, int64_t out_stride, uint32_t fields,
        double* d_out /* [k][out_stride] */, int32_t* d_first_bad_point /* may be NULL */,
        void* hip_stream);
/* Host-pointer form: ray_results_m arrays in, out[k][nray][nstep_max+1]; processes the rays in blocks so that the
 * device footprint is bounded whatever nray is (at most 2**21 trajectory slots per block; the environment variable
 * RAYS_HIP_DIAG_BLOCK_RAYS sets the rays per block instead); only recorded points cross PCIe in either direction
 * (packed on the host, evaluated in the packed layout, scattered back by the host, which zero-fills the rest).
 * Blocking, and plain: it runs on the CURRENT HIP device (the device list of rays_hip_init[_devices] is not used),
 * block after block without overlapping copies and kernels, through pageable copies and device buffers allocated and
 * freed per call.  Its time has not been measured; the figures quoted for the kernel are the device-pointer form's. */
int rays_hip_ray_diagnostics(const rays_params_t* p, int nray, const double* ray_vec, const double* residual,
                             const int32_t* npoints, uint32_t fields, double* out, int32_t* first_bad_point);

/* ---- O-X mode conversion analysis on the device (the post-processors' analyze_OX_conv) -----------------
 * Replaces the serial ray loop of post_process_lib/OX_conv_analysis_m.f90:91-198, which calls `equilibrium` at every
 * recorded point of every ray until alpha = omega_pe**2/omega**2 first decreases.  Per ray:
 *   find_x_max_ray (:202-252)     the first point j >= 2 with alpha(j) < alpha(j-1): step_number = j - 1, alpha_max,
 *                                 x_max = ray_vec(1:3, j-1), k_max = ray_vec(4:6, j-1); none: no maximum
 *   find_x_cutoff_ray (:256-311)  steepest ascent from x_max to abs(alpha - 1) <= 1e-4, at most 10 iterations, no step
 *                                 longer than a quarter of the distance from the z axis; `iterations` is the
 *                                 reference's `iteration` on exit: 1 .. 10, or 11 when no cutoff was found
 *   OX_conv_coeff (:315-407)      unit vectors xc (along grad ne), yc, zc at x_cut; cos_theta = xc . bunit,
 *                                 gamma = abs(gamma(0)), L = ne / |grad ne|; ny_c, nz_c and the vectors nvec*_c of
 *                                 k_max / k0 in that frame; conv_coeff, Mjolhus' formula
 *   converted                     conv_coeff > conversion_threshold = 0.0001 (a default-real literal)
 * status holds RAYS_OX_FOUND_MAX, RAYS_OX_FOUND_CUTOFF, RAYS_OX_CONVERTED or, alone, RAYS_OX_EQ_REFUSED.
 *   - A ray without a maximum holds the reference's zeros (:126-129) in every field.
 *   - A ray with a maximum and no cutoff holds step_number, alpha_max, x_max, k_max, iterations = 11 and zeros
 *     elsewhere (:143).
 *   - A ray with a cutoff holds everything, CONVERTED or not: the reference stores conv_coeff and the three vectors of
 *     converted rays only and leaves them UNDEFINED for the others; here they are the computed values.
 *   - The reference never looks at equib_err in this module.  Here a ray for which `equilibrium` refuses a point the
 *     analysis needs -- a recorded point up to and including the one that shows the first decrease (any point of a
 *     ray without one), an ascent iterate, x_cut -- gets status = RAYS_OX_EQ_REFUSED and zeros in every other field.
 *     Points behind the first decrease are never evaluated by the reference and influence nothing here.
 * Everything but conv_coeff is bit-identical to the reference's arithmetic (products, sums, quotients, square roots;
 * norm2, minval and dot_product as its compiler evaluates them).  conv_coeff passes through acos, sin and cos: the
 * device-pointer form computes it with the device library's (within 1e-10 relative of the reference's per unit of the
 * exponent, measured far below: DESIGN.md 4.11), the host-pointer form recomputes it on the host with libm from
 * aux[5] and is bit-identical.  Exact arithmetic only: the numerics setting does not reach this analysis.  Built for
 * the species counts and equilibria of the trace kernels; another shape is refused by name. */
enum { RAYS_OX_FOUND_MAX = 1, RAYS_OX_FOUND_CUTOFF = 2, RAYS_OX_CONVERTED = 4, RAYS_OX_EQ_REFUSED = 8 };
enum { RAYS_OX_AUX_COS_THETA = 0, RAYS_OX_AUX_GAMMA, RAYS_OX_AUX_L, RAYS_OX_AUX_NY_C, RAYS_OX_AUX_NZ_C, RAYS_OX_NAUX };
/* One array per field, indexed by ray (0-based; vectors [nray][3], aux [nray][RAYS_OX_NAUX]).  A null pointer: the
 * field is not wanted. */
typedef struct rays_ox_result_t {
  int32_t* status;
  int32_t* step_number;  /* 1-based index of the point of x_max */
  int32_t* iterations;
  double* alpha_max;
  double* x_max;
  double* k_max;
  double* x_cut;
  double* conv_coeff;
  double* nvecx_c;
  double* nvecy_c;
  double* nvecz_c;
  double* aux;
} rays_ox_result_t;
/* Device-pointer form (current device, asynchronous on hip_stream): two kernels, a scan with one wave per ray that
 * leaves at the chunk of 64 points holding the first decrease, and the ascent with one lane per ray.
 *   in_layout   RAYS_DIAG_IN_PADDED: d_ray_vec[nray][nstep_max+1][nv] as the trace entries leave it, d_offsets unused
 *               (may be NULL); RAYS_DIAG_IN_PACKED: d_ray_vec[total][nv] with d_offsets[nray + 1], the prefix sum of
 *               the point counts (the point offsets entry above)
 *   d_npoints   clamped to 0 .. nstep_max + 1 (packed: and to the ray's own run) whatever it holds
 *   out         device pointers.  The call keeps 8 bytes per ray of its own per (device, stream). */
int rays_hip_ox_conv_device(const rays_params_t* p, int nray, int in_layout, const double* d_ray_vec,
                            const int32_t* d_npoints, const int64_t* d_offsets /* may be NULL (padded) */,
                            const rays_ox_result_t* out, void* hip_stream);
/* Host-pointer form: the ray_results_m arrays in (ray_vec[nray][nstep_max+1][nv], npoints[nray]), host arrays out.
 * Blocking, on the CURRENT device, in blocks of rays of bounded device footprint (at most 2**21 trajectory slots; the
 * environment variable RAYS_HIP_OX_BLOCK_RAYS sets the rays per block instead); only the points up to each ray's end
 * are uploaded.  conv_coeff and RAYS_OX_CONVERTED are finished on the host with libm (bit-identical to the reference).
 * *number_of_rays_converted and converted_ray_number[0 .. *number_of_rays_converted - 1] (1-based ray numbers in ray
 * order, capacity nray) are the reference's compacted list; either may be NULL. */
int rays_hip_ox_conv(const rays_params_t* p, int nray, const double* ray_vec, const int32_t* npoints,
                     const rays_ox_result_t* out, int32_t* number_of_rays_converted, int32_t* converted_ray_number);
/* The scan kernel's name for p's shape, "ox_scan_kernel<EQ, NS>"; "" (and the last-error text) when it is not built. */
const char* rays_hip_ox_conv_kernel_name_for(const rays_params_t* p);

/* Diagnostic entry used by the parity tests: evaluates equilibrium + deriv_cold + deriv_num +
 * eqn_ray + check_save at n states on the current device (host pointers; nv must be 7, nspec 1|2).
 * cold7/num7[n][7] = dddx(3) dddk(3) dddw; dvds[n][7]; resid[n]; codes[n][4] = equilibrium err,
 * eqn_ray stop code, check_save flag, check_save stop_ode. */
int rays_hip_probe(const rays_params_t* p, int n, const double* v, double* cold7, double* num7,
                   double* dvds, double* resid, int32_t* codes);

#ifdef __cplusplus
}
#endif
#endif /* RAYS_HIP_H */
