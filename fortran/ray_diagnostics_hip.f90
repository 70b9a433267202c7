 module ray_diagnostics_hip_m
! GPU form of the loop of the reference post-processors' ray_detailed_diagnostics
!     ray_loop / step_loop        post_process_lib/axisym_toroid_processor_m.f90:351-419
!                                 (slab_processor_m.f90: the same body with X, Y in place of Psi, R)
! for a host that holds the ray_results_m arrays.  In ray_detailed_diagnostics, in place of the two loops:
!
!     use rays_hip_state_m, only : rays_hip_pack_physics
!     use ray_diagnostics_hip_m
!     type(rays_params_t) :: p
!     integer :: first_bad(number_of_rays)
!     call rays_hip_pack_physics(p, 'ray_detailed_diagnostics')
!     call ray_detailed_diagnostics_hip(p, number_of_rays, max_number_of_points, dim_v_vector, ray_vec, &
!          & residual_results, npoints, s, ne, Te_kev, modB, alpha_e, gamma_e, Psi, R, Z, n_par, n_perp, &
!          & P_absorbed, n_imag, xi_0, xi_1, xi_2, residual, first_bad)
!
! The seventeen arrays come back as the loop leaves them, bit for bit, zero where no point was recorded (the
! reference allocates them with source = 0).  The slab processor passes its X and Y for Psi and R and sets
! slab = .true..  Where the reference stops with 'infinite group velocity' (:395-400) the point gets n_imag = 0
! and first_bad(iray) the index of the ray's first such point (0 = none); the caller decides whether to stop.
! The module depends on rays_hip_m alone: the parameter block is the caller's (rays_hip_state_m builds it
! from the reference's module state; nv, nstep_max and the damping options are set here from the arrays).

    use, intrinsic :: iso_c_binding
    use rays_hip_m

    implicit none

 contains

    subroutine ray_detailed_diagnostics_hip(p, number_of_rays, max_number_of_points, dim_v_vector, ray_vec, &
         & residual_results, npoints, s, ne, Te_kev, modB, alpha_e, gamma_e, Psi, R, Z, n_par, n_perp, &
         & P_absorbed, n_imag, xi_0, xi_1, xi_2, residual, first_bad, slab)

    type(rays_params_t), intent(in) :: p
    integer, intent(in) :: number_of_rays, max_number_of_points, dim_v_vector
    real(c_double), intent(in) :: ray_vec(dim_v_vector, max_number_of_points, number_of_rays)
    real(c_double), intent(in) :: residual_results(max_number_of_points, number_of_rays)
    integer, intent(in) :: npoints(number_of_rays)
    real(c_double), dimension(max_number_of_points, number_of_rays), intent(out) :: s, ne, Te_kev, modB, alpha_e, &
         & gamma_e, Psi, R, Z, n_par, n_perp, P_absorbed, n_imag, xi_0, xi_1, xi_2, residual
    integer, intent(out) :: first_bad(number_of_rays)
    logical, intent(in), optional :: slab   ! .true.: Psi, R receive the slab processor's X, Y

    type(rays_params_t) :: q
    integer(c_int32_t), allocatable :: np32(:), bad32(:)
    real(c_double), allocatable :: out(:,:,:)
    integer(c_int32_t) :: fields
    character(len=512) :: msg
    integer(c_int) :: rc
    integer :: m, g
    logical :: found, is_slab

    is_slab = .false.
    if (present(slab)) is_slab = slab

    ! the run's ODE vector length and array extent, from the arrays themselves (a post-processor has read them from
    ! the results file); the damping options are recovered from nv as in deposition_profile_hip
    q = p
    q%nv = dim_v_vector
    q%nstep_max = max_number_of_points - 1
    found = .false.
    do m = 0, 1
       do g = 0, 1
          if (.not. found .and. 7 + min(q%damping_model, 1)*(1 + m*(1 + q%nspec)) + 5*g == q%nv) then
             q%multi_spec_damping = m*min(q%damping_model, 1)
             q%integrate_eq_gradients = g
             found = .true.
          end if
       end do
    end do
    if (.not. found) then
       write(0,*) 'ray_detailed_diagnostics_hip: dim_v_vector =', q%nv, ' matches no combination of options for nspec =', q%nspec
       stop 1
    end if

    ! every field but the two coordinates this processor does not write (enum order = order of out's last dimension)
    fields = int(2**RAYS_DIAG_NFIELDS - 1, c_int32_t)
    if (is_slab) then
       fields = fields - int(2**RAYS_DIAG_PSI + 2**RAYS_DIAG_R, c_int32_t)
    else
       fields = fields - int(2**RAYS_DIAG_X + 2**RAYS_DIAG_Y, c_int32_t)
    end if

    allocate(np32(number_of_rays), bad32(number_of_rays), out(max_number_of_points, number_of_rays, 17))
    np32 = npoints
    rc = rays_hip_ray_diagnostics(q, int(number_of_rays, c_int), ray_vec, residual_results, np32, fields, out, bad32)
    if (rc /= 0) then
       call last_error_string(msg)
       write(0,*) 'ray_detailed_diagnostics_hip: ', trim(msg) ; stop 1
    end if
    first_bad = bad32

    s = out(:,:,1) ; ne = out(:,:,2) ; Te_kev = out(:,:,3) ; modB = out(:,:,4) ; alpha_e = out(:,:,5)
    gamma_e = out(:,:,6)
    Psi = out(:,:,7) ; R = out(:,:,8)       ! Psi, R | X, Y
    Z = out(:,:,9) ; n_par = out(:,:,10) ; n_perp = out(:,:,11) ; P_absorbed = out(:,:,12) ; n_imag = out(:,:,13)
    xi_0 = out(:,:,14) ; xi_1 = out(:,:,15) ; xi_2 = out(:,:,16) ; residual = out(:,:,17)
    deallocate(np32, bad32, out)

    end subroutine ray_detailed_diagnostics_hip

 end module ray_diagnostics_hip_m
