 module rays_hip_m
! iso_c_binding interface to librays_hip.so (include/rays_hip.h) -- the thin Fortran shim through
! which the RAYS host calls the MI355X ray-trajectory integrator.
!
! type(rays_params_t) mirrors the C struct field for field; the integer selectors are the images
! of the reference's string switches (see the enums in rays_hip.h).  Every real constant is passed
! by value from the host's own module variables (constants_m, rf_m, species_m ...), never
! re-derived on the device side: several of them are single-precision literals widened to double
! (constants_m.f90:39-48) and must reach the GPU bit for bit.

    use, intrinsic :: iso_c_binding
    implicit none

    integer(c_int), parameter :: RAYS_HIP_NO_KEPT_RESULT = 5   ! rays_hip_deposition_last: no device-resident image held

    integer(c_int), parameter :: RAYS_ABI_VERSION = 3
    integer, parameter :: RAYS_NS0 = 6   ! species_m nspec0 + 1

    ! selectors
    integer(c_int32_t), parameter :: RAYS_ODE_RK4 = 0, RAYS_ODE_SG = 1
    integer(c_int32_t), parameter :: RAYS_DERIV_COLD = 0, RAYS_DERIV_NUM = 1
    integer(c_int32_t), parameter :: RAYS_PARAM_ARCL = 0, RAYS_PARAM_TIME = 1
    integer(c_int32_t), parameter :: RAYS_EQ_SLAB = 0, RAYS_EQ_SOLOVEV = 1, RAYS_EQ_AXISYM = 2
    integer(c_int32_t), parameter :: RAYS_DAMP_NONE = 0, RAYS_DAMP_FUND_ECH = 1

    type, bind(C) :: rays_slab_params_t
        integer(c_int32_t) :: bx_prof_model, by_prof_model, bz_prof_model, dens_prof_model
        integer(c_int32_t) :: t_prof_model(RAYS_NS0)
        integer(c_int32_t) :: pad_(2)
        real(c_double) :: xmin, xmax, ymin, ymax, zmin, zmax
        real(c_double) :: rmaj, rmin, x0
        real(c_double) :: bx0, by0, bz0, LBy_shear_scale, LBz_scale, dBzdx
        real(c_double) :: Ln_scale, dndx, alphan1, alphan2, n_min
        real(c_double) :: LT_scale, dtdx
        real(c_double) :: alphat1(RAYS_NS0), alphat2(RAYS_NS0), T_min(RAYS_NS0)
    end type rays_slab_params_t

    type, bind(C) :: rays_solovev_params_t
        integer(c_int32_t) :: dens_prof_model
        integer(c_int32_t) :: t_prof_model(RAYS_NS0)
        integer(c_int32_t) :: pad_(1)
        real(c_double) :: rmaj, kappa, bphi0, iota0, outer_bound
        real(c_double) :: psiB
        real(c_double) :: alphan1, alphan2
        real(c_double) :: alphat1(RAYS_NS0), alphat2(RAYS_NS0)
        real(c_double) :: box_rmin, box_rmax, box_zmin, box_zmax
    end type rays_solovev_params_t

    type, bind(C) :: rays_axisym_params_t
        integer(c_int32_t) :: magnetics_model, density_prof_model
        integer(c_int32_t) :: t_prof_model(RAYS_NS0)
        real(c_double) :: box_rmin, box_rmax, box_zmin, box_zmax
        real(c_double) :: plasma_psi_limit
        real(c_double) :: psiB
        real(c_double) :: alphan1, alphan2, d_scrape_off, T_scrape_off
        real(c_double) :: alphat1(RAYS_NS0), alphat2(RAYS_NS0)
    end type rays_axisym_params_t

    ! spline tables of the eqdsk equilibrium: pointers to the host's own (contiguous) arrays
    type, bind(C) :: rays_axisym_tables_t
        integer(c_int32_t) :: nr, nz, n_rb, n_ne, n_te, n_ti
        type(c_ptr) :: r_grid, z_grid, psi_fspl
        type(c_ptr) :: rb_grid, rb_fspl
        type(c_ptr) :: ne_grid, ne_fspl
        type(c_ptr) :: te_grid, te_fspl
        type(c_ptr) :: ti_grid, ti_fspl
    end type rays_axisym_tables_t

    ! The saved ray state of windowed tracing (include/rays_hip.h: rays_ray_state_t): device pointers, in Fortran order
    ! v(nv, nray), s(nray), nstep(nray), stop_code(nray), resid(3, nray), sg_err(2, nray) (c_null_ptr allowed for RK4_ODE),
    ! flags(nray).  The caller owns the arrays and may copy them to disk and back.
    integer(c_int32_t), parameter :: RAYS_STATE_REFUSED = 1
    type, bind(C) :: rays_ray_state_t
        type(c_ptr) :: v, s, nstep, stop_code, resid, sg_err, flags
    end type rays_ray_state_t

    ! One record of rays_hip_trace_profiles[_device] (include/rays_hip.h: rays_dep_profile_t).  which: RAYS_DEP_PTOTAL_PSI
    ! = 0 | _RHO = 1 | _X = 2.  Host form: work = c_loc(work(n_bins, nray)) or c_null_ptr, profile_in = c_null_ptr,
    ! profile = c_loc(profile(n_bins)); device form: device pointers, work(nray, n_bins) in Fortran order (bin-major).
    integer(c_int), parameter :: RAYS_DEP_MAX_PROFILES = 2
    type, bind(C) :: rays_dep_profile_t
        integer(c_int) :: which, n_bins
        type(c_ptr) :: work, profile_in, profile
    end type rays_dep_profile_t

    ! The result block of the O-X conversion analysis (include/rays_hip.h: rays_ox_result_t): one array per field,
    ! indexed by ray -- status, step_number, iterations (int32); alpha_max, conv_coeff; x_max, k_max, x_cut, nvecx_c,
    ! nvecy_c, nvecz_c (3, nray); aux (5, nray) = cos_theta, gamma, L, ny_c, nz_c.  c_null_ptr: the field is not wanted.
    integer(c_int32_t), parameter :: RAYS_OX_FOUND_MAX = 1, RAYS_OX_FOUND_CUTOFF = 2, RAYS_OX_CONVERTED = 4, &
         & RAYS_OX_EQ_REFUSED = 8
    integer(c_int), parameter :: RAYS_OX_NAUX = 5
    type, bind(C) :: rays_ox_result_t
        type(c_ptr) :: status, step_number, iterations
        type(c_ptr) :: alpha_max, x_max, k_max, x_cut, conv_coeff, nvecx_c, nvecy_c, nvecz_c, aux
    end type rays_ox_result_t

    type, bind(C) :: rays_params_t
        integer(c_int32_t) :: abi_version
        integer(c_int32_t) :: nv, nspec, nstep_max
        integer(c_int32_t) :: ode_solver, ray_deriv, ray_param, equilib_model
        integer(c_int32_t) :: integrate_eq_gradients
        integer(c_int32_t) :: pad_(3)
        real(c_double) :: ds, s_max
        real(c_double) :: omgrf, k0
        real(c_double) :: clight, eps0
        real(c_double) :: dispersion_resid_limit
        real(c_double) :: rel_err0, abs_err0, SG_error_limit
        real(c_double) :: qs(RAYS_NS0), ms(RAYS_NS0)
        real(c_double) :: n0s(RAYS_NS0), t0s(RAYS_NS0)
        real(c_double) :: eta(RAYS_NS0)
        type(rays_slab_params_t) :: slab
        type(rays_solovev_params_t) :: solovev
        integer(c_int32_t) :: damping_model, multi_spec_damping
        real(c_double) :: total_damping_limit
        type(rays_axisym_params_t) :: axisym
    end type rays_params_t

    ! ray launchers on the device (rays_fan_t of rays_hip.h; SURVEY 8(f) f1)
    integer(c_int32_t), parameter :: RAYS_RAY_INIT_SOLOVEV_NPHI_NTHETA = 0, &
         & RAYS_RAY_INIT_AXISYM_R_Z_NPHI_NTHETA = 1, RAYS_RAY_INIT_SIMPLE_SLAB = 2
    integer(c_int32_t), parameter :: RAYS_WAVE_PLUS = 0, RAYS_WAVE_MINUS = 1, RAYS_WAVE_FAST = 2, RAYS_WAVE_SLOW = 3
    type, bind(C) :: rays_fan_t
       integer(c_int32_t) :: model, wave_mode, k0_sign
       integer(c_int32_t) :: n_r_launch, n_theta_launch, n_rindex_theta, n_rindex_phi
       real(c_double) :: r_launch0, dr_launch, theta_launch0, dtheta_launch, z_launch0
       real(c_double) :: rindex_theta0, delta_rindex_theta, rindex_phi0, delta_rindex_phi
       integer(c_int32_t) :: n_x_launch, n_y_launch, n_z_launch, n_ky_launch, n_kz_launch, pad_
       real(c_double) :: x_launch0, dx_launch, y_launch0, dy_launch, slab_z_launch0
       real(c_double) :: rindex_y0, delta_rindex_y0, rindex_z0, delta_rindex_z0
    end type rays_fan_t

    ! device-resident result of rays_hip_trace_gather (rays_device_result_t of rays_hip.h)
    type, bind(C) :: rays_device_result_t
       integer(c_int32_t) :: device, nray
       type(c_ptr) :: ray_vec, residual, npoints, stop_code, end_ray_vec, end_residuals, max_residuals
    end type rays_device_result_t

    integer(c_int), parameter :: RAYS_TRACE_NO_ZERO_FILL = 1
    integer(c_int), parameter :: RAYS_NUMERICS_EXACT = 0, RAYS_NUMERICS_TOLERANCE = 1
    integer(c_int), parameter :: RAYS_DEP_PTOTAL_PSI = 0, RAYS_DEP_PTOTAL_RHO = 1, RAYS_DEP_PTOTAL_X = 2
    ! fields of the per-point ray diagnostics (bit numbers of `fields`; the order of the output's leading dimension)
    integer(c_int), parameter :: RAYS_DIAG_S = 0, RAYS_DIAG_NE = 1, RAYS_DIAG_TE_KEV = 2, RAYS_DIAG_MODB = 3, &
         & RAYS_DIAG_ALPHA_E = 4, RAYS_DIAG_GAMMA_E = 5, RAYS_DIAG_PSI = 6, RAYS_DIAG_R = 7, RAYS_DIAG_X = 8, &
         & RAYS_DIAG_Y = 9, RAYS_DIAG_Z = 10, RAYS_DIAG_N_PAR = 11, RAYS_DIAG_N_PERP = 12, RAYS_DIAG_P_ABSORBED = 13, &
         & RAYS_DIAG_N_IMAG = 14, RAYS_DIAG_XI_0 = 15, RAYS_DIAG_XI_1 = 16, RAYS_DIAG_XI_2 = 17, RAYS_DIAG_RESIDUAL = 18, &
         & RAYS_DIAG_NFIELDS = 19
    ! layouts of the trajectory arrays handed to rays_hip_ray_diagnostics_packed_device
    integer(c_int), parameter :: RAYS_DIAG_IN_PADDED = 0, RAYS_DIAG_IN_PACKED = 1

    interface

       integer(c_int) function rays_hip_init(ngpu) bind(C, name='rays_hip_init')
          import :: c_int
          integer(c_int), value :: ngpu
       end function rays_hip_init

       ! explicit slot -> device list for rays_hip_trace / rays_hip_trace_gather
       integer(c_int) function rays_hip_init_devices(n, device_ids) bind(C, name='rays_hip_init_devices')
          import :: c_int
          integer(c_int), value :: n
          integer(c_int), intent(in) :: device_ids(*)
       end function rays_hip_init_devices

       integer(c_int) function rays_hip_finalize() bind(C, name='rays_hip_finalize')
          import :: c_int
       end function rays_hip_finalize

       ! numerics of the trace kernels: RAYS_NUMERICS_EXACT (0, default: bit-identical to the CPU path) or
       ! RAYS_NUMERICS_TOLERANCE (1: every step within 1e-10 relative, counts and stop flags exact; cold RK4 kernels)
       integer(c_int) function rays_hip_set_numerics(mode) bind(C, name='rays_hip_set_numerics')
          import :: c_int
          integer(c_int), value :: mode
       end function rays_hip_set_numerics

       integer(c_int) function rays_hip_get_numerics() bind(C, name='rays_hip_get_numerics')
          import :: c_int
       end function rays_hip_get_numerics

       integer(c_int) function rays_hip_last_error(buf, len) bind(C, name='rays_hip_last_error')
          import :: c_int, c_char
          character(kind=c_char) :: buf(*)
          integer(c_int), value :: len
       end function rays_hip_last_error

       type(c_ptr) function rays_hip_stop_flag_text(stop_code) bind(C, name='rays_hip_stop_flag_text')
          import :: c_int, c_ptr
          integer(c_int), value :: stop_code
       end function rays_hip_stop_flag_text

       integer(c_int) function rays_hip_set_zfun_table(fspl_re, nx, x_min, x_max) &
                    & bind(C, name='rays_hip_set_zfun_table')
          import :: c_int, c_double
          real(c_double), intent(in) :: fspl_re(4,*)
          integer(c_int), value :: nx
          real(c_double), value :: x_min, x_max
       end function rays_hip_set_zfun_table

       integer(c_int) function rays_hip_set_axisym_tables(t) bind(C, name='rays_hip_set_axisym_tables')
          import :: c_int, rays_axisym_tables_t
          type(rays_axisym_tables_t), intent(in) :: t
       end function rays_hip_set_axisym_tables

       ! magnetics_model = 'eqdsk_magnetics_lin_interp': eqdsk_utilities_m's R_grid, Z_grid, Psi, T (rb_fspl), dR, dZ
       integer(c_int) function rays_hip_set_eqdsk_lin_tables(t, dR, dZ) bind(C, name='rays_hip_set_eqdsk_lin_tables')
          import :: c_int, c_double, rays_axisym_tables_t
          type(rays_axisym_tables_t), intent(in) :: t
          real(c_double), value :: dR, dZ
       end function rays_hip_set_eqdsk_lin_tables

       integer(c_int) function rays_hip_check_params(p) bind(C, name='rays_hip_check_params')
          import :: c_int, rays_params_t
          type(rays_params_t), intent(in) :: p
       end function rays_hip_check_params

       ! Replaces `call trace_rays`: blocking, host arrays in the reference's own layouts.
       integer(c_int) function rays_hip_trace(p, nray, rvec0, rindex_vec0, ray_vec, residual, &
                    & npoints, stop_code, end_ray_vec, end_residuals, max_residuals, elapsed_s) &
                    & bind(C, name='rays_hip_trace')
          import :: c_int, c_int32_t, c_double, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray
          real(c_double), intent(in) :: rvec0(3,*), rindex_vec0(3,*)
          real(c_double), intent(inout) :: ray_vec(*), residual(*)
          integer(c_int32_t), intent(inout) :: npoints(*), stop_code(*)
          real(c_double), intent(inout) :: end_ray_vec(*), end_residuals(*), max_residuals(*)
          real(c_double), intent(out) :: elapsed_s
       end function rays_hip_trace

       ! Multi-GPU trace whose result stays in device memory on the root device (RCCL gather of the blocks'
       ! packed trajectories: SURVEY 8(e)); rays_hip_result_to_host copies it into ray_results_m's arrays,
       ! rays_hip_deposition_device consumes it in place.
       integer(c_int) function rays_hip_trace_gather(p, nray, rvec0, rindex_vec0, result) &
                    & bind(C, name='rays_hip_trace_gather')
          import :: c_int, c_double, rays_params_t, rays_device_result_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray
          real(c_double), intent(in) :: rvec0(3,*), rindex_vec0(3,*)
          type(rays_device_result_t), intent(out) :: result
       end function rays_hip_trace_gather

       integer(c_int) function rays_hip_result_to_host(p, result, ray_vec, residual, npoints, stop_code, &
                    & end_ray_vec, end_residuals, max_residuals) bind(C, name='rays_hip_result_to_host')
          import :: c_int, c_int32_t, c_double, rays_params_t, rays_device_result_t
          type(rays_params_t), intent(in) :: p
          type(rays_device_result_t), intent(in) :: result
          real(c_double), intent(inout) :: ray_vec(*), residual(*)
          integer(c_int32_t), intent(inout) :: npoints(*), stop_code(*)
          real(c_double), intent(inout) :: end_ray_vec(*), end_residuals(*), max_residuals(*)
       end function rays_hip_result_to_host

       ! Device-pointer forms (type(c_ptr) = device memory on the current HIP device; hip_stream = a hipStream_t
       ! or c_null_ptr): the trace, the fused `ds` scan (ray_scan.f90:33-49), one ode_solver step from arbitrary
       ! states (ode_m.f90:218-254), the device ray launcher and the deposition profiles.
       integer(c_int) function rays_hip_trace_device(p, nray, d_rvec0, d_rindex_vec0, d_ray_vec, d_residual, &
                    & d_npoints, d_stop_code, d_end_ray_vec, d_end_residuals, d_max_residuals, hip_stream, flags) &
                    & bind(C, name='rays_hip_trace_device')
          import :: c_int, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray
          type(c_ptr), value :: d_rvec0, d_rindex_vec0, d_ray_vec, d_residual, d_npoints, d_stop_code
          type(c_ptr), value :: d_end_ray_vec, d_end_residuals, d_max_residuals, hip_stream
          integer(c_int), value :: flags
       end function rays_hip_trace_device

       integer(c_int) function rays_hip_scan_device(p, n_runs, d_ds_values, nray, d_rvec0, d_rindex_vec0, &
                    & d_ray_vec, d_residual, d_npoints, d_stop_code, d_end_ray_vec, d_end_residuals, &
                    & d_max_residuals, hip_stream, flags) bind(C, name='rays_hip_scan_device')
          import :: c_int, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: n_runs, nray
          type(c_ptr), value :: d_ds_values, d_rvec0, d_rindex_vec0, d_ray_vec, d_residual, d_npoints, d_stop_code
          type(c_ptr), value :: d_end_ray_vec, d_end_residuals, d_max_residuals, hip_stream
          integer(c_int), value :: flags
       end function rays_hip_scan_device

       ! Summary-only tracing (include/rays_hip.h): the per-ray rows of ray_results_m without ray_vec(:,:,:) and
       ! residual(:,:) -- what scanner_m's aggregate_run_data keeps of a run.  Always the exact kernels.  The device
       ! forms are asynchronous on hip_stream; d_start_ray_vec may be c_null_ptr.
       integer(c_int) function rays_hip_trace_summary_device(p, nray, d_rvec0, d_rindex_vec0, d_npoints, d_stop_code, &
                    & d_start_ray_vec, d_end_ray_vec, d_end_residuals, d_max_residuals, hip_stream) &
                    & bind(C, name='rays_hip_trace_summary_device')
          import :: c_int, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray
          type(c_ptr), value :: d_rvec0, d_rindex_vec0, d_npoints, d_stop_code, d_start_ray_vec
          type(c_ptr), value :: d_end_ray_vec, d_end_residuals, d_max_residuals, hip_stream
       end function rays_hip_trace_summary_device

       ! outputs with a leading (slowest) run dimension: npoints(nray, n_runs), end_ray_vec(nv, nray, n_runs), ...
       integer(c_int) function rays_hip_scan_summary_device(p, n_runs, d_ds_values, nray, d_rvec0, d_rindex_vec0, &
                    & d_npoints, d_stop_code, d_start_ray_vec, d_end_ray_vec, d_end_residuals, d_max_residuals, &
                    & hip_stream) bind(C, name='rays_hip_scan_summary_device')
          import :: c_int, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: n_runs, nray
          type(c_ptr), value :: d_ds_values, d_rvec0, d_rindex_vec0, d_npoints, d_stop_code, d_start_ray_vec
          type(c_ptr), value :: d_end_ray_vec, d_end_residuals, d_max_residuals, hip_stream
       end function rays_hip_scan_summary_device

       ! Blocking, host arrays: rays_hip_trace without the trajectories (only the summaries cross PCIe).
       integer(c_int) function rays_hip_trace_summary(p, nray, rvec0, rindex_vec0, npoints, stop_code, &
                    & start_ray_vec, end_ray_vec, end_residuals, max_residuals, elapsed_s) &
                    & bind(C, name='rays_hip_trace_summary')
          import :: c_int, c_int32_t, c_double, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray
          real(c_double), intent(in) :: rvec0(3,*), rindex_vec0(3,*)
          integer(c_int32_t), intent(inout) :: npoints(*), stop_code(*)
          real(c_double), intent(inout) :: start_ray_vec(*), end_ray_vec(*), end_residuals(*), max_residuals(*)
          real(c_double), intent(out) :: elapsed_s
       end function rays_hip_trace_summary

       ! Windowed tracing (include/rays_hip.h): rays are paused after n_steps recorded steps and continued from the saved
       ! state.  Device pointers, asynchronous on hip_stream.  state_init: initialize_ode_vector and the initial check_save
       ! for every ray, point 1 into d_start_ray_vec(nv, nray) (c_null_ptr: not wanted).
       integer(c_int) function rays_hip_state_init_device(p, nray, d_rvec0, d_rindex_vec0, state, d_start_ray_vec, &
                    & hip_stream) bind(C, name='rays_hip_state_init_device')
          import :: c_int, c_ptr, rays_params_t, rays_ray_state_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray
          type(c_ptr), value :: d_rvec0, d_rindex_vec0
          type(rays_ray_state_t), intent(in) :: state
          type(c_ptr), value :: d_start_ray_vec, hip_stream
       end function rays_hip_state_init_device

       ! One window: d_ray_vec_win(nv, n_steps, nray), d_residual_win(n_steps, nray) receive the points recorded by this
       ! call alone, d_npoints_win(nray) their number (0 for a ray that had ended); both window arrays c_null_ptr: a summary
       ! window.  The state is updated in place.  nstep_max and s_max stay limits of the whole ray.
       integer(c_int) function rays_hip_trace_window_device(p, nray, state, n_steps, d_ray_vec_win, d_residual_win, &
                    & d_npoints_win, hip_stream) bind(C, name='rays_hip_trace_window_device')
          import :: c_int, c_ptr, rays_params_t, rays_ray_state_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, n_steps
          type(rays_ray_state_t), intent(in) :: state
          type(c_ptr), value :: d_ray_vec_win, d_residual_win, d_npoints_win, hip_stream
       end function rays_hip_trace_window_device

       ! The five per-ray summary arrays of ray_results_m from the state (rays under way as they stand).
       integer(c_int) function rays_hip_state_summary_device(p, nray, state, d_npoints, d_stop_code, d_end_ray_vec, &
                    & d_end_residuals, d_max_residuals, hip_stream) bind(C, name='rays_hip_state_summary_device')
          import :: c_int, c_ptr, rays_params_t, rays_ray_state_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray
          type(rays_ray_state_t), intent(in) :: state
          type(c_ptr), value :: d_npoints, d_stop_code, d_end_ray_vec, d_end_residuals, d_max_residuals, hip_stream
       end function rays_hip_state_summary_device

       ! Blocking, host arrays: rays_hip_trace's arguments and results, traced in windows of n_steps on one device (the
       ! device holds the state and two window slabs, whatever nstep_max is).  The three summary arrays are type(c_ptr)
       ! so that c_null_ptr can stand for "not wanted" (else c_loc(array)).
       integer(c_int) function rays_hip_trace_windowed(p, nray, rvec0, rindex_vec0, n_steps, ray_vec, residual, npoints, &
                    & stop_code, end_ray_vec, end_residuals, max_residuals, elapsed_s) &
                    & bind(C, name='rays_hip_trace_windowed')
          import :: c_int, c_int32_t, c_double, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, n_steps
          real(c_double), intent(in) :: rvec0(3,*), rindex_vec0(3,*)
          real(c_double), intent(inout) :: ray_vec(*), residual(*)
          integer(c_int32_t), intent(inout) :: npoints(*), stop_code(*)
          type(c_ptr), value :: end_ray_vec, end_residuals, max_residuals
          real(c_double), intent(out) :: elapsed_s
       end function rays_hip_trace_windowed

       ! Name of the kernel a window launches (recording /= 0: with window arrays); c_null_char-terminated C string.
       type(c_ptr) function rays_hip_window_kernel_name_for(p, nray, recording) &
                    & bind(C, name='rays_hip_window_kernel_name_for')
          import :: c_int, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, recording
       end function rays_hip_window_kernel_name_for

       ! Fused trace and deposition (include/rays_hip.h): the summary-only trace that also bins every accepted point, so
       ! the absorbed-power profile exists without ray_vec(:,:,:).  Device pointers, asynchronous on hip_stream; d_work is
       ! work(nray, n_bins) in Fortran order (bin-major), zeroed by the call; the profile continues d_profile_in
       ! (c_null_ptr: from zero).  which: RAYS_DEP_PTOTAL_PSI = 0 | _RHO = 1 | _X = 2.
       integer(c_int) function rays_hip_trace_deposition_device(p, nray, d_rvec0, d_rindex_vec0, d_initial_ray_power, &
                    & which, n_bins, d_npoints, d_stop_code, d_start_ray_vec, d_end_ray_vec, d_end_residuals, &
                    & d_max_residuals, d_work, d_profile_in, d_profile_out, hip_stream) &
                    & bind(C, name='rays_hip_trace_deposition_device')
          import :: c_int, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, which, n_bins
          type(c_ptr), value :: d_rvec0, d_rindex_vec0, d_initial_ray_power, d_npoints, d_stop_code, d_start_ray_vec
          type(c_ptr), value :: d_end_ray_vec, d_end_residuals, d_max_residuals, d_work, d_profile_in, d_profile_out
          type(c_ptr), value :: hip_stream
       end function rays_hip_trace_deposition_device

       ! Blocking, host arrays: what `call trace_rays` followed by calculate_deposition_profiles gives for ONE profile --
       ! the per-ray summaries, work(n_bins, nray) (the reference's layout) and profile(n_bins) -- without the
       ! trajectories.  work is a type(c_ptr) so that c_null_ptr can stand for "not wanted" (else c_loc(work)).
       integer(c_int) function rays_hip_trace_deposition(p, nray, rvec0, rindex_vec0, initial_ray_power, which, n_bins, &
                    & npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals, work, profile, &
                    & elapsed_s) bind(C, name='rays_hip_trace_deposition')
          import :: c_int, c_int32_t, c_double, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, which, n_bins
          real(c_double), intent(in) :: rvec0(3,*), rindex_vec0(3,*), initial_ray_power(*)
          integer(c_int32_t), intent(inout) :: npoints(*), stop_code(*)
          real(c_double), intent(inout) :: start_ray_vec(*), end_ray_vec(*), end_residuals(*), max_residuals(*)
          type(c_ptr), value :: work
          real(c_double), intent(inout) :: profile(*)
          real(c_double), intent(out) :: elapsed_s
       end function rays_hip_trace_deposition

       ! Fused deposition into every profile of the equilibrium in ONE trace pass (include/rays_hip.h): what `call
       ! trace_rays` followed by calculate_deposition_profiles gives for axisym_toroid -- Ptotal_psi and Ptotal_rho --
       ! without the trajectories and without tracing twice.  profiles(n_profiles): one or two records.
       integer(c_int) function rays_hip_trace_profiles_device(p, nray, d_rvec0, d_rindex_vec0, d_initial_ray_power, &
                    & n_profiles, profiles, d_npoints, d_stop_code, d_start_ray_vec, d_end_ray_vec, d_end_residuals, &
                    & d_max_residuals, hip_stream) bind(C, name='rays_hip_trace_profiles_device')
          import :: c_int, c_ptr, rays_params_t, rays_dep_profile_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, n_profiles
          type(rays_dep_profile_t), intent(in) :: profiles(*)
          type(c_ptr), value :: d_rvec0, d_rindex_vec0, d_initial_ray_power, d_npoints, d_stop_code, d_start_ray_vec
          type(c_ptr), value :: d_end_ray_vec, d_end_residuals, d_max_residuals, hip_stream
       end function rays_hip_trace_profiles_device

       integer(c_int) function rays_hip_trace_profiles(p, nray, rvec0, rindex_vec0, initial_ray_power, n_profiles, &
                    & profiles, npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals, elapsed_s) &
                    & bind(C, name='rays_hip_trace_profiles')
          import :: c_int, c_int32_t, c_double, rays_params_t, rays_dep_profile_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, n_profiles
          real(c_double), intent(in) :: rvec0(3,*), rindex_vec0(3,*), initial_ray_power(*)
          type(rays_dep_profile_t), intent(in) :: profiles(*)
          integer(c_int32_t), intent(inout) :: npoints(*), stop_code(*)
          real(c_double), intent(inout) :: start_ray_vec(*), end_ray_vec(*), end_residuals(*), max_residuals(*)
          real(c_double), intent(out) :: elapsed_s
       end function rays_hip_trace_profiles

       ! the profiles of p's equilibrium in the reference's order, into which(RAYS_DEP_MAX_PROFILES); returns their number
       integer(c_int) function rays_hip_deposition_profile_set(p, which) bind(C, name='rays_hip_deposition_profile_set')
          import :: c_int, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), intent(out) :: which(*)
       end function rays_hip_deposition_profile_set

       ! Segmented deposition (include/rays_hip.h): the ray-ordered profile sum per SEGMENT of rays -- segment s is the
       ! rays off(s) .. off(s+1)-1 (zero-based, int32 on the device), or s*rays_per_seg .. with d_seg_offsets = c_null_ptr
       ! -- on its own, behind the fused ds scan (ray_scan: every run binned while it is traced, one launch), and behind a
       ! fused pass over many beams.  Device pointers; asynchronous on hip_stream.
       integer(c_int) function rays_hip_profile_sum_segments_device(n_bins, nray, n_seg, d_seg_offsets, rays_per_seg, &
                    & d_work, d_profile_in, d_profile_out, hip_stream) bind(C, name='rays_hip_profile_sum_segments_device')
          import :: c_int, c_ptr
          integer(c_int), value :: n_bins, nray, n_seg, rays_per_seg
          type(c_ptr), value :: d_seg_offsets, d_work, d_profile_in, d_profile_out, hip_stream
       end function rays_hip_profile_sum_segments_device

       ! d_rvec0, d_rindex_vec0, d_initial_ray_power: per fan member (nray); each record's work is [n_bins][n_runs*nray],
       ! its profile and profile_in [n_runs][n_bins]; the summaries are [n_runs*nray]
       integer(c_int) function rays_hip_scan_profiles_device(p, n_runs, d_ds_values, nray, d_rvec0, d_rindex_vec0, &
                    & d_initial_ray_power, n_profiles, profiles, d_npoints, d_stop_code, d_start_ray_vec, d_end_ray_vec, &
                    & d_end_residuals, d_max_residuals, hip_stream) bind(C, name='rays_hip_scan_profiles_device')
          import :: c_int, c_ptr, rays_params_t, rays_dep_profile_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: n_runs, nray, n_profiles
          type(rays_dep_profile_t), intent(in) :: profiles(*)
          type(c_ptr), value :: d_ds_values, d_rvec0, d_rindex_vec0, d_initial_ray_power, d_npoints, d_stop_code
          type(c_ptr), value :: d_start_ray_vec, d_end_ray_vec, d_end_residuals, d_max_residuals, hip_stream
       end function rays_hip_scan_profiles_device

       ! rays_hip_trace_profiles_device with one profile per segment: profile and profile_in are [n_seg][n_bins]
       integer(c_int) function rays_hip_trace_profiles_segments_device(p, nray, d_rvec0, d_rindex_vec0, &
                    & d_initial_ray_power, n_profiles, profiles, n_seg, d_seg_offsets, rays_per_seg, d_npoints, &
                    & d_stop_code, d_start_ray_vec, d_end_ray_vec, d_end_residuals, d_max_residuals, hip_stream) &
                    & bind(C, name='rays_hip_trace_profiles_segments_device')
          import :: c_int, c_ptr, rays_params_t, rays_dep_profile_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, n_profiles, n_seg, rays_per_seg
          type(rays_dep_profile_t), intent(in) :: profiles(*)
          type(c_ptr), value :: d_rvec0, d_rindex_vec0, d_initial_ray_power, d_seg_offsets, d_npoints, d_stop_code
          type(c_ptr), value :: d_start_ray_vec, d_end_ray_vec, d_end_residuals, d_max_residuals, hip_stream
       end function rays_hip_trace_profiles_segments_device

       ! (c_ptr to a NUL-terminated name, as the other *_kernel_name_for)
       type(c_ptr) function rays_hip_profiles_kernel_name_for(p, nray, n_profiles) &
                    & bind(C, name='rays_hip_profiles_kernel_name_for')
          import :: c_int, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, n_profiles
       end function rays_hip_profiles_kernel_name_for

       ! One deposition window: the state advances as in a summary-policy rays_hip_trace_window_device call, and every point
       ! the window accepts is binned into the records' work(nray, n_bins) (device pointers, bin-major) -- ACCUMULATORS the
       ! call never zeroes: zero them once, when rays_hip_state_init_device is called.  A record's profile may be
       ! c_null_ptr (no sum in this window); otherwise it is the ray-ordered sum over the work so far, continued from
       ! profile_in.  d_initial_ray_power(nray) is required; d_npoints_win(nray): the points this call accepted.
       ! Asynchronous on hip_stream; one caller thread per (device, stream).
       integer(c_int) function rays_hip_trace_window_profiles_device(p, nray, state, n_steps, d_initial_ray_power, &
                    & n_profiles, profiles, d_npoints_win, hip_stream) &
                    & bind(C, name='rays_hip_trace_window_profiles_device')
          import :: c_int, c_ptr, rays_params_t, rays_ray_state_t, rays_dep_profile_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, n_steps, n_profiles
          type(rays_ray_state_t), intent(in) :: state
          type(rays_dep_profile_t), intent(in) :: profiles(*)
          type(c_ptr), value :: d_initial_ray_power, d_npoints_win, hip_stream
       end function rays_hip_trace_window_profiles_device

       ! (c_ptr to a NUL-terminated name, as the other *_kernel_name_for)
       type(c_ptr) function rays_hip_window_profiles_kernel_name_for(p, nray, n_profiles) &
                    & bind(C, name='rays_hip_window_profiles_kernel_name_for')
          import :: c_int, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, n_profiles
       end function rays_hip_window_profiles_kernel_name_for

       ! ASYNCHRONOUS on hip_stream (blocking before round 3): synchronise the stream before d_v1 / d_resid /
       ! d_stop_code are read on the host or from another stream; one caller thread per (device, stream).
       integer(c_int) function rays_hip_ode_step_device(p, n, d_v0, d_s0, d_v1, d_resid, d_stop_code, hip_stream) &
                    & bind(C, name='rays_hip_ode_step_device')
          import :: c_int, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: n
          type(c_ptr), value :: d_v0, d_s0, d_v1, d_resid, d_stop_code, hip_stream
       end function rays_hip_ode_step_device

       integer(c_int) function rays_hip_ray_init_device(p, fan, nray_max, d_rvec0, d_rindex_vec0, nray, hip_stream) &
                    & bind(C, name='rays_hip_ray_init_device')
          import :: c_int, c_int32_t, c_ptr, rays_params_t, rays_fan_t
          type(rays_params_t), intent(in) :: p
          type(rays_fan_t), intent(in) :: fan
          integer(c_int), value :: nray_max
          type(c_ptr), value :: d_rvec0, d_rindex_vec0, hip_stream
          integer(c_int32_t), intent(out) :: nray
       end function rays_hip_ray_init_device

       ! Deposition profiles (post_process_lib/deposition_profiles_m.f90:228-292).  rho(psiN) spline for 'Ptotal_rho':
       integer(c_int) function rays_hip_set_rho_table(grid, fspl, n) bind(C, name='rays_hip_set_rho_table')
          import :: c_int, c_double
          real(c_double), intent(in) :: grid(*), fspl(4,*)
          integer(c_int), value :: n
       end function rays_hip_set_rho_table

       integer(c_int) function rays_hip_deposition_device(p, which, n_bins, nray, d_ray_vec, d_npoints, &
                    & d_initial_ray_power, d_work, d_profile_in, d_profile_out, hip_stream) &
                    & bind(C, name='rays_hip_deposition_device')
          import :: c_int, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: which, n_bins, nray
          type(c_ptr), value :: d_ray_vec, d_npoints, d_initial_ray_power, d_work, d_profile_in, d_profile_out, hip_stream
       end function rays_hip_deposition_device

       ! host arrays in the reference's layouts: ray_vec(nv, nstep_max+1, nray), work(n_bins, nray), profile(n_bins)
       integer(c_int) function rays_hip_deposition(p, which, n_bins, nray, ray_vec, npoints, initial_ray_power, &
                    & work, profile) bind(C, name='rays_hip_deposition')
          import :: c_int, c_int32_t, c_double, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: which, n_bins, nray
          real(c_double), intent(in) :: ray_vec(*), initial_ray_power(*)
          integer(c_int32_t), intent(in) :: npoints(*)
          real(c_double), intent(inout) :: work(*), profile(*)
       end function rays_hip_deposition

       ! The same profiles of the rays the LAST rays_hip_trace call traced, binned from the image that call left on
       ! the device(s) (rays_hip_keep_last_result(1) before the trace): no trajectory upload.  Returns
       ! RAYS_HIP_NO_KEPT_RESULT when no image of a trace with this nray / nv / nstep_max is held.
       integer(c_int) function rays_hip_keep_last_result(on) bind(C, name='rays_hip_keep_last_result')
          import :: c_int
          integer(c_int), value :: on
       end function rays_hip_keep_last_result
       integer(c_int) function rays_hip_deposition_last(p, which, n_bins, nray, initial_ray_power, work, profile) &
                    & bind(C, name='rays_hip_deposition_last')
          import :: c_int, c_double, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: which, n_bins, nray
          real(c_double), intent(in) :: initial_ray_power(*)
          real(c_double), intent(inout) :: work(*), profile(*)
       end function rays_hip_deposition_last

       ! The post-processors' ray_detailed_diagnostics loop (axisym_toroid_processor_m.f90:351-419) on the GPU: host
       ! arrays in the reference's layouts, out(nstep_max+1, nray, k) with k over the set bits of `fields` in
       ! RAYS_DIAG_* order; first_bad_point(nray) (fortran/ray_diagnostics_hip.f90 is the caller)
       integer(c_int) function rays_hip_ray_diagnostics(p, nray, ray_vec, residual, npoints, fields, out, &
                    & first_bad_point) bind(C, name='rays_hip_ray_diagnostics')
          import :: c_int, c_int32_t, c_double, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray
          real(c_double), intent(in) :: ray_vec(*), residual(*)
          integer(c_int32_t), intent(in) :: npoints(*)
          integer(c_int32_t), value :: fields
          real(c_double), intent(inout) :: out(*)
          integer(c_int32_t), intent(inout) :: first_bad_point(*)
       end function rays_hip_ray_diagnostics

       ! The packed layout on the device (include/rays_hip.h): d_offsets(0:nray) (int64) = exclusive prefix sum of
       ! the rays' point counts, the total in d_offsets(nray); asynchronous on hip_stream
       integer(c_int) function rays_hip_point_offsets_device(nray, nstep_max, d_npoints, d_offsets, hip_stream) &
                    & bind(C, name='rays_hip_point_offsets_device')
          import :: c_int, c_ptr
          integer(c_int), value :: nray, nstep_max
          type(c_ptr), value :: d_npoints, d_offsets, hip_stream
       end function rays_hip_point_offsets_device

       ! The diagnostics of the recorded points alone: d_out(out_stride, k), point j (1-based) of ray i at
       ! d_out(d_offsets(i) + j, k); in_layout = RAYS_DIAG_IN_PADDED (the trace's arrays) or RAYS_DIAG_IN_PACKED
       ! (ray_vec(nv, total), residual(total)); nothing at or beyond out_stride of a field is written
       integer(c_int) function rays_hip_ray_diagnostics_packed_device(p, nray, in_layout, d_ray_vec, d_residual, &
                    & d_npoints, d_offsets, out_stride, fields, d_out, d_first_bad_point, hip_stream) &
                    & bind(C, name='rays_hip_ray_diagnostics_packed_device')
          import :: c_int, c_int32_t, c_int64_t, c_ptr, rays_params_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, in_layout
          type(c_ptr), value :: d_ray_vec, d_residual, d_npoints, d_offsets
          integer(c_int64_t), value :: out_stride
          integer(c_int32_t), value :: fields
          type(c_ptr), value :: d_out, d_first_bad_point, hip_stream
       end function rays_hip_ray_diagnostics_packed_device

       ! The post-processors' analyze_OX_conv (post_process_lib/OX_conv_analysis_m.f90:91-198) on the GPU: host arrays in
       ! the reference's layouts in, the host arrays `res` points to out (one element per ray, vectors (3, nray), aux
       ! (5, nray)); number_of_rays_converted and converted_ray_number(1:number_of_rays_converted), 1-based ray numbers in
       ! ray order (fortran/ox_conv_analysis_hip.f90 is the caller)
       integer(c_int) function rays_hip_ox_conv(p, nray, ray_vec, npoints, res, number_of_rays_converted, &
                    & converted_ray_number) bind(C, name='rays_hip_ox_conv')
          import :: c_int, c_int32_t, c_double, rays_params_t, rays_ox_result_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray
          real(c_double), intent(in) :: ray_vec(*)
          integer(c_int32_t), intent(in) :: npoints(*)
          type(rays_ox_result_t), intent(in) :: res
          integer(c_int32_t), intent(out) :: number_of_rays_converted
          integer(c_int32_t), intent(inout) :: converted_ray_number(*)
       end function rays_hip_ox_conv

       ! The same on device arrays (include/rays_hip.h): in_layout = RAYS_DIAG_IN_PADDED (the trace's ray_vec, d_offsets
       ! may be c_null_ptr) or RAYS_DIAG_IN_PACKED (ray_vec(nv, total) with d_offsets(0:nray)); `res` holds device
       ! pointers; asynchronous on hip_stream
       integer(c_int) function rays_hip_ox_conv_device(p, nray, in_layout, d_ray_vec, d_npoints, d_offsets, res, &
                    & hip_stream) bind(C, name='rays_hip_ox_conv_device')
          import :: c_int, c_ptr, rays_params_t, rays_ox_result_t
          type(rays_params_t), intent(in) :: p
          integer(c_int), value :: nray, in_layout
          type(c_ptr), value :: d_ray_vec, d_npoints, d_offsets
          type(rays_ox_result_t), intent(in) :: res
          type(c_ptr), value :: hip_stream
       end function rays_hip_ox_conv_device

       ! Replaces the serial launch loops of ray_init_m's launchers (solovev_ray_init_nphi_ntheta_m.f90:
       ! 60-198 etc.): fills rvec0(3,nray_max), rindex_vec0(3,nray_max), ray_pwr_wt(nray_max), nray.
       integer(c_int) function rays_hip_ray_init(p, fan, nray_max, rvec0, rindex_vec0, ray_pwr_wt, nray) &
                    & bind(C, name='rays_hip_ray_init')
          import :: c_int, c_int32_t, c_double, rays_params_t, rays_fan_t
          type(rays_params_t), intent(in) :: p
          type(rays_fan_t), intent(in) :: fan
          integer(c_int), value :: nray_max
          real(c_double), intent(inout) :: rvec0(3,*), rindex_vec0(3,*), ray_pwr_wt(*)
          integer(c_int32_t), intent(out) :: nray
       end function rays_hip_ray_init

    end interface

 contains

    integer(c_int32_t) function wave_mode_code(wave_mode)
    ! rf_m's wave_mode string -> RAYS_WAVE_* (dispersion_solvers_m.f90:86-101 stops on anything else)
       character(len=*), intent(in) :: wave_mode
       select case (trim(wave_mode))
          case ('plus');  wave_mode_code = RAYS_WAVE_PLUS
          case ('minus'); wave_mode_code = RAYS_WAVE_MINUS
          case ('fast');  wave_mode_code = RAYS_WAVE_FAST
          case ('slow');  wave_mode_code = RAYS_WAVE_SLOW
          case default
             write(0,*) 'solve_disp: improper wave_mode = ', trim(wave_mode); stop 1
       end select
    end function wave_mode_code

    subroutine clear_fan(fan)
       type(rays_fan_t), intent(out) :: fan
       fan%model = 0 ; fan%wave_mode = 0 ; fan%k0_sign = 1
       fan%n_r_launch = 0 ; fan%n_theta_launch = 0 ; fan%n_rindex_theta = 0 ; fan%n_rindex_phi = 0
       fan%r_launch0 = 0. ; fan%dr_launch = 0. ; fan%theta_launch0 = 0. ; fan%dtheta_launch = 0. ; fan%z_launch0 = 0.
       fan%rindex_theta0 = 0. ; fan%delta_rindex_theta = 0. ; fan%rindex_phi0 = 0. ; fan%delta_rindex_phi = 0.
       fan%n_x_launch = 0 ; fan%n_y_launch = 0 ; fan%n_z_launch = 0 ; fan%n_ky_launch = 0
       fan%n_kz_launch = 0 ; fan%pad_ = 0
       fan%x_launch0 = 0. ; fan%dx_launch = 0. ; fan%y_launch0 = 0. ; fan%dy_launch = 0.
       fan%slab_z_launch0 = 0. ; fan%rindex_y0 = 0. ; fan%delta_rindex_y0 = 0.
       fan%rindex_z0 = 0. ; fan%delta_rindex_z0 = 0.
    end subroutine clear_fan

    function stop_flag_string(stop_code) result(flag)
    ! integer stop code -> the reference's ode_stop_flag text (e.g. ' nstep > nstep_max')
       integer(c_int), intent(in) :: stop_code
       character(len=60) :: flag
       type(c_ptr) :: cp
       character(kind=c_char), pointer :: cs(:)
       integer :: i
       flag = ''
       cp = rays_hip_stop_flag_text(stop_code)
       if (.not. c_associated(cp)) return
       call c_f_pointer(cp, cs, [60])
       do i = 1, 60
          if (cs(i) == c_null_char) exit
          flag(i:i) = cs(i)
       end do
    end function stop_flag_string

    subroutine last_error_string(msg)
       character(len=*), intent(out) :: msg
       character(kind=c_char) :: buf(512)
       integer :: i, n
       msg = ''
       n = rays_hip_last_error(buf, 512_c_int)
       do i = 1, min(len(msg), 511)
          if (buf(i) == c_null_char) exit
          msg(i:i) = buf(i)
       end do
    end subroutine last_error_string

 end module rays_hip_m
