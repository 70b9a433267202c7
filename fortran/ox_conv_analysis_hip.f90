 module OX_conv_analysis_m
! GPU form of the reference post-processor's O-X mode conversion analysis
!     analyze_OX_conv             post_process_lib/OX_conv_analysis_m.f90:91-198
!     write_OX_conversion_data_LD :411-444
! under the reference's module name and with its public names (OX_conv, OX_conv_data, number_of_rays_converted,
! conversion_threshold, analyze_OX_conv, write_OX_conversion_data_LD), for a host that holds the ray_results_m arrays.
! The ray loop -- find_x_max_ray, find_x_cutoff_ray, OX_conv_coeff, one `equilibrium` per recorded point until alpha
! first decreases -- runs on the device (rays_hip_ox_conv, include/rays_hip.h); what comes back is loaded into
! OX_conv_data as the reference loads it.  In post_process_RAYS, in place of `call analyze_OX_conv`:
!
!     use rays_hip_state_m, only : rays_hip_pack_physics
!     use ray_results_m, only : number_of_rays, max_number_of_points, dim_v_vector, ray_vec, npoints
!     use diagnostics_m, only : run_label
!     type(rays_params_t) :: p
!     call rays_hip_pack_physics(p, 'analyze_OX_conv')
!     call analyze_OX_conv(p, number_of_rays, max_number_of_points, dim_v_vector, ray_vec, npoints, run_label)
!
! The module depends on rays_hip_m alone: the parameter block and the arrays are the caller's (nv, nstep_max and the
! damping options are set here from the arrays, as in ray_diagnostics_hip_m).  Every number is the reference's bit for
! bit: conv_coeff is finished on the host with the libm the reference calls.  The per-ray prints of the reference
! (write(*,*) 'ray ', ...) are not repeated.  Differences, all where the reference is undefined:
!   - OX_conv_data holds the converted rays only, like the reference's; ray_status(number_of_rays) keeps every ray's
!     RAYS_OX_* bits for a caller that wants to know why a ray is missing (no maximum, no cutoff, below the threshold,
!     or a point the equilibrium refused -- the reference computes on with an undefined eq_point there).

    use, intrinsic :: iso_c_binding
    use rays_hip_m

    implicit none

    integer, parameter, private :: rkind = selected_real_kind(15,307)

    integer :: number_of_rays_converted
    real(KIND=rkind), parameter :: conversion_threshold = 0.0001

! One converted ray.  Field names and kinds are those the reference's users read (:35-47).
    type OX_conv
        real(KIND=rkind) :: x_max(3)      ! ray point at which alpha stops rising
        real(KIND=rkind) :: k_max(3)      ! wave vector there
        real(KIND=rkind) :: alpha_max     ! alpha there
        real(KIND=rkind) :: x_cut(3)      ! end point of the ascent: on the O-mode cutoff
        real(KIND=rkind) :: conv_coeff    ! O-X conversion coefficient
        real(KIND=rkind) :: nvecx_c(3)    ! k_max/k0 along grad(ne) at x_cut
        real(KIND=rkind) :: nvecy_c(3)    ! ... along B x grad(ne)
        real(KIND=rkind) :: nvecz_c(3)    ! ... along the third direction of that frame
        integer :: ray_number             ! 1-based number of the ray in the fan
        integer :: step_number            ! 1-based index of the point of x_max
    end type OX_conv

    type(OX_conv), allocatable :: OX_conv_data(:)
    integer, allocatable :: ray_status(:)   ! RAYS_OX_* bits of every ray (an addition)

 contains

    subroutine analyze_OX_conv(p, number_of_rays, max_number_of_points, dim_v_vector, ray_vec, npoints, run_label)

    type(rays_params_t), intent(in) :: p
    integer, intent(in) :: number_of_rays, max_number_of_points, dim_v_vector
    real(c_double), intent(in) :: ray_vec(dim_v_vector, max_number_of_points, number_of_rays)
    integer, intent(in) :: npoints(number_of_rays)
    character(len=*), intent(in), optional :: run_label   ! present: write OX_conv_data.<run_label>.dat like the reference

    type(rays_params_t) :: q
    type(rays_ox_result_t) :: res
    integer(c_int32_t), allocatable, target :: np32(:), status(:), step_number(:), converted(:)
    real(c_double), allocatable, target :: alpha_max(:), conv_coeff(:), x_max(:,:), k_max(:,:), x_cut(:,:), &
         & nvecx_c(:,:), nvecy_c(:,:), nvecz_c(:,:)
    integer(c_int32_t) :: n_conv
    character(len=512) :: msg
    integer(c_int) :: rc
    integer :: m, g, i, i_ray
    logical :: found

    ! the run's ODE vector length and array extent, from the arrays themselves; the damping options are recovered from
    ! nv as in ray_detailed_diagnostics_hip (the analysis reads ray_vec(1:6) only)
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
       write(0,*) 'analyze_OX_conv: dim_v_vector =', q%nv, ' matches no combination of options for nspec =', q%nspec
       stop 1
    end if

    m = max(number_of_rays, 1)
    allocate(np32(m), status(m), step_number(m), converted(m), alpha_max(m), conv_coeff(m))
    allocate(x_max(3,m), k_max(3,m), x_cut(3,m), nvecx_c(3,m), nvecy_c(3,m), nvecz_c(3,m))
    np32(1:number_of_rays) = npoints
    res%status = c_loc(status) ; res%step_number = c_loc(step_number) ; res%iterations = c_null_ptr
    res%alpha_max = c_loc(alpha_max) ; res%conv_coeff = c_loc(conv_coeff)
    res%x_max = c_loc(x_max) ; res%k_max = c_loc(k_max) ; res%x_cut = c_loc(x_cut)
    res%nvecx_c = c_loc(nvecx_c) ; res%nvecy_c = c_loc(nvecy_c) ; res%nvecz_c = c_loc(nvecz_c)
    res%aux = c_null_ptr

    n_conv = 0
    rc = rays_hip_ox_conv(q, int(number_of_rays, c_int), ray_vec, np32, res, n_conv, converted)
    if (rc /= 0) then
       call last_error_string(msg)
       write(0,*) 'analyze_OX_conv: ', trim(msg) ; stop 1
    end if

    ! the compacted list (:170-191): entry i is ray converted(i)
    number_of_rays_converted = n_conv
    if (allocated(OX_conv_data)) deallocate(OX_conv_data)
    if (allocated(ray_status)) deallocate(ray_status)
    allocate(OX_conv_data(number_of_rays_converted), ray_status(number_of_rays))
    ray_status = status(1:number_of_rays)
    do i = 1, number_of_rays_converted
       i_ray = converted(i)
       OX_conv_data(i)%x_max = x_max(:, i_ray)
       OX_conv_data(i)%k_max = k_max(:, i_ray)
       OX_conv_data(i)%alpha_max = alpha_max(i_ray)
       OX_conv_data(i)%x_cut = x_cut(:, i_ray)
       OX_conv_data(i)%conv_coeff = conv_coeff(i_ray)
       OX_conv_data(i)%nvecx_c = nvecx_c(:, i_ray)
       OX_conv_data(i)%nvecy_c = nvecy_c(:, i_ray)
       OX_conv_data(i)%nvecz_c = nvecz_c(:, i_ray)
       OX_conv_data(i)%ray_number = i_ray
       OX_conv_data(i)%step_number = step_number(i_ray)
    end do
    deallocate(np32, status, step_number, converted, alpha_max, conv_coeff, x_max, k_max, x_cut, nvecx_c, nvecy_c, nvecz_c)

    if (number_of_rays_converted > 0 .and. present(run_label)) then
       call write_OX_conversion_data_LD(run_label)
    end if

    end subroutine analyze_OX_conv

!****************************************************************************

    subroutine write_OX_conversion_data_LD(run_label)
    ! One list-directed record group per converted ray, the items of the reference's file in its order (:434-437): the
    ! label 'ray ', the position in the list, then three labelled reals.  Nothing is copied to standard output.

    character(len=*), intent(in) :: run_label
    integer :: OX_conv_unit, i_ray
    real(KIND=rkind) :: nz, ny
    character(len=80) :: out_file

    out_file = 'OX_conv_data.'//trim(run_label)//'.dat'
    open(newunit=OX_conv_unit, file=out_file, action='write', status='replace', form='formatted')
    do i_ray = 1, number_of_rays_converted
       nz = norm2(OX_conv_data(i_ray)%nvecz_c)
       ny = norm2(OX_conv_data(i_ray)%nvecy_c)
       write(OX_conv_unit,*) 'ray ', i_ray, '  conv coeff = ', OX_conv_data(i_ray)%conv_coeff, 'nz_c = ', nz, 'ny_c = ', ny
    end do
    close(unit = OX_conv_unit)

    end subroutine write_OX_conversion_data_LD

!****************************************************************************

    subroutine deallocate_OX_conv_analysis_m
        if (allocated(OX_conv_data)) deallocate(OX_conv_data)
        if (allocated(ray_status)) deallocate(ray_status)
    end subroutine deallocate_OX_conv_analysis_m

 end module OX_conv_analysis_m
