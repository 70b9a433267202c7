 program fused_deposition_driver
! TEST INFRASTRUCTURE ONLY (tests/test_gpu_fused_deposition.py): calls the fused trace + deposition host entry through
! fortran/rays_hip_m.f90 -- rays_hip_trace_deposition on host arrays -- and writes what came back to a flat file.
!     fused_deposition_driver IN ZFUN OUT
! IN (stream, native): int32 nray, nv, n_bins, which; the bytes of rays_params_t; real64 rvec0(3, nray),
!   rindex_vec0(3, nray), initial_ray_power(nray).
! ZFUN: int32 nx; real64 x_min, x_max, fspl_re(4, nx) -- the Z-function spline table the damping needs.
! OUT: int32 npoints(nray), stop_code(nray), real64 start_ray_vec(nv, nray), end_ray_vec(nv, nray), end_residuals(nray),
!   max_residuals(nray), work(n_bins, nray), profile(n_bins).

    use, intrinsic :: iso_c_binding
    use rays_hip_m

    implicit none

    character(len=1024) :: fin, fzf, fout
    integer(c_int32_t) :: nray, nv, n_bins, which, nx
    type(rays_params_t) :: p
    real(c_double) :: x_min, x_max, elapsed
    real(c_double), allocatable, target :: rvec0(:,:), rindex_vec0(:,:), power(:), fspl(:,:)
    integer(c_int32_t), allocatable, target :: npoints(:), stop_code(:)
    real(c_double), allocatable, target :: start_ray_vec(:,:), end_ray_vec(:,:), end_residuals(:), max_residuals(:)
    real(c_double), allocatable, target :: work(:,:), profile(:), profile2(:)
    integer :: u

    call get_command_argument(1, fin)
    call get_command_argument(2, fzf)
    call get_command_argument(3, fout)
    open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
    read(u) nray, nv, n_bins, which
    read(u) p
    if (nray < 1 .or. n_bins < 1 .or. nv /= p%nv) stop 3
    allocate(rvec0(3, nray), rindex_vec0(3, nray), power(nray))
    read(u) rvec0, rindex_vec0, power
    close(u)
    open(newunit=u, file=trim(fzf), access='stream', form='unformatted', status='old', action='read')
    read(u) nx
    read(u) x_min, x_max
    allocate(fspl(4, nx))
    read(u) fspl
    close(u)
    if (rays_hip_set_zfun_table(fspl, nx, x_min, x_max) /= 0) stop 4

    ! every element must come back written
    allocate(npoints(nray), stop_code(nray), start_ray_vec(nv, nray), end_ray_vec(nv, nray), end_residuals(nray), &
           & max_residuals(nray), work(n_bins, nray), profile(n_bins), profile2(n_bins))
    npoints = -7; stop_code = -7; start_ray_vec = -7.; end_ray_vec = -7.; end_residuals = -7.; max_residuals = -7.
    work = -7.; profile = -7.; profile2 = -7.
    if (rays_hip_trace_deposition(p, nray, rvec0, rindex_vec0, power, which, n_bins, npoints, stop_code, start_ray_vec, &
         & end_ray_vec, end_residuals, max_residuals, c_loc(work), profile, elapsed) /= 0) stop 5
    ! work is optional
    if (rays_hip_trace_deposition(p, nray, rvec0, rindex_vec0, power, which, n_bins, npoints, stop_code, start_ray_vec, &
         & end_ray_vec, end_residuals, max_residuals, c_null_ptr, profile2, elapsed) /= 0) stop 6
    if (any(profile2 /= profile)) stop 8

    open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace', action='write')
    write(u) npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals, work, profile
    close(u)

 end program fused_deposition_driver
