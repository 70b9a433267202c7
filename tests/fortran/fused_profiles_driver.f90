 program fused_profiles_driver
! TEST INFRASTRUCTURE ONLY (tests/test_gpu_fused_profiles.py): calls the host entry of the fused deposition into two
! profiles through fortran/rays_hip_m.f90 -- rays_hip_trace_profiles on host arrays -- and writes what came back to a
! flat file.
!     fused_profiles_driver IN OUT
! IN (stream, native): int32 nray, nv, n_bins_a, n_bins_b, which_a, which_b, nx, n_rho; the bytes of rays_params_t;
!   real64 x_min, x_max, fspl_re(4, nx) -- the Z-function spline table; int32 nr, nz, n_rb, n_ne, n_te, n_ti and the
!   eleven arrays of rays_axisym_tables_t, each behind its int32 length; real64 rho_grid(n_rho), rho_fspl(4, n_rho);
!   rvec0(3, nray), rindex_vec0(3, nray), initial_ray_power(nray).
! OUT: int32 npoints(nray), stop_code(nray), real64 start_ray_vec(nv, nray), end_ray_vec(nv, nray), end_residuals(nray),
!   max_residuals(nray), work_a(n_bins_a, nray), profile_a(n_bins_a), work_b(n_bins_b, nray), profile_b(n_bins_b).

    use, intrinsic :: iso_c_binding
    use rays_hip_m

    implicit none

    type table_t
        real(c_double), allocatable :: a(:)
    end type table_t

    character(len=1024) :: fin, fout
    integer(c_int32_t) :: nray, nv, nb(2), which(2), nx, n_rho, tn(6), n
    type(rays_params_t) :: p
    type(rays_axisym_tables_t) :: t
    type(rays_dep_profile_t) :: rec(2)
    type(table_t), target :: tab(11)
    real(c_double) :: x_min, x_max, elapsed
    real(c_double), allocatable, target :: rvec0(:,:), rindex_vec0(:,:), power(:), fspl(:,:), rho_grid(:), rho_fspl(:,:)
    integer(c_int32_t), allocatable, target :: npoints(:), stop_code(:)
    real(c_double), allocatable, target :: start_ray_vec(:,:), end_ray_vec(:,:), end_residuals(:), max_residuals(:)
    real(c_double), allocatable, target :: work_a(:,:), work_b(:,:), profile_a(:), profile_b(:), again_a(:), again_b(:)
    integer(c_int) :: set(RAYS_DEP_MAX_PROFILES)
    integer :: u, k

    call get_command_argument(1, fin)
    call get_command_argument(2, fout)
    open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
    read(u) nray, nv, nb, which, nx, n_rho
    read(u) p
    if (nray < 1 .or. any(nb < 1) .or. nv /= p%nv) stop 3
    read(u) x_min, x_max
    allocate(fspl(4, nx))
    read(u) fspl
    read(u) tn
    do k = 1, 11
        read(u) n
        allocate(tab(k)%a(n))
        read(u) tab(k)%a
    end do
    allocate(rho_grid(n_rho), rho_fspl(4, n_rho), rvec0(3, nray), rindex_vec0(3, nray), power(nray))
    read(u) rho_grid, rho_fspl, rvec0, rindex_vec0, power
    close(u)
    if (rays_hip_set_zfun_table(fspl, nx, x_min, x_max) /= 0) stop 4
    t%nr = tn(1); t%nz = tn(2); t%n_rb = tn(3); t%n_ne = tn(4); t%n_te = tn(5); t%n_ti = tn(6)
    t%r_grid = ptr(1); t%z_grid = ptr(2); t%psi_fspl = ptr(3); t%rb_grid = ptr(4); t%rb_fspl = ptr(5); t%ne_grid = ptr(6)
    t%ne_fspl = ptr(7); t%te_grid = ptr(8); t%te_fspl = ptr(9); t%ti_grid = ptr(10); t%ti_fspl = ptr(11)
    if (rays_hip_set_axisym_tables(t) /= 0) stop 5
    if (rays_hip_set_rho_table(rho_grid, rho_fspl, n_rho) /= 0) stop 6
    if (rays_hip_deposition_profile_set(p, set) /= 2) stop 7

    ! every element must come back written
    allocate(npoints(nray), stop_code(nray), start_ray_vec(nv, nray), end_ray_vec(nv, nray), end_residuals(nray), &
           & max_residuals(nray), work_a(nb(1), nray), work_b(nb(2), nray), profile_a(nb(1)), profile_b(nb(2)), &
           & again_a(nb(1)), again_b(nb(2)))
    npoints = -7; stop_code = -7; start_ray_vec = -7.; end_ray_vec = -7.; end_residuals = -7.; max_residuals = -7.
    work_a = -7.; work_b = -7.; profile_a = -7.; profile_b = -7.; again_a = -7.; again_b = -7.
    rec(1) = rays_dep_profile_t(which(1), nb(1), c_loc(work_a), c_null_ptr, c_loc(profile_a))
    rec(2) = rays_dep_profile_t(which(2), nb(2), c_loc(work_b), c_null_ptr, c_loc(profile_b))
    if (rays_hip_trace_profiles(p, nray, rvec0, rindex_vec0, power, 2, rec, npoints, stop_code, start_ray_vec, &
         & end_ray_vec, end_residuals, max_residuals, elapsed) /= 0) stop 8
    ! work is optional
    rec(1) = rays_dep_profile_t(which(1), nb(1), c_null_ptr, c_null_ptr, c_loc(again_a))
    rec(2) = rays_dep_profile_t(which(2), nb(2), c_null_ptr, c_null_ptr, c_loc(again_b))
    if (rays_hip_trace_profiles(p, nray, rvec0, rindex_vec0, power, 2, rec, npoints, stop_code, start_ray_vec, &
         & end_ray_vec, end_residuals, max_residuals, elapsed) /= 0) stop 9
    if (any(again_a /= profile_a) .or. any(again_b /= profile_b)) stop 10

    open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace', action='write')
    write(u) npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals, work_a, profile_a, work_b, profile_b
    close(u)

 contains

    function ptr(k) result(c)
        integer, intent(in) :: k
        type(c_ptr) :: c
        c = c_null_ptr
        if (size(tab(k)%a) > 0) c = c_loc(tab(k)%a)
    end function ptr

 end program fused_profiles_driver
