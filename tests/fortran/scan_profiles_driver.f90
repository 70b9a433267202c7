 program scan_profiles_driver
! TEST INFRASTRUCTURE ONLY (tests/test_gpu_scan_profiles.py): the fused ds scan through fortran/rays_hip_m.f90 --
! rays_hip_scan_profiles_device with two records, then rays_hip_profile_sum_segments_device on the first record's work
! with the runs as uniform segments -- on device arrays it allocates through the HIP runtime; writes what came back to a
! flat file.
!     scan_profiles_driver IN OUT
! IN: the file of fused_profiles_driver.f90 (int32 nray, nv, n_bins_a, n_bins_b, which_a, which_b, nx, n_rho; the bytes
!   of rays_params_t; the Z-function table; the axisym tables; the rho table; rvec0, rindex_vec0, initial_ray_power),
!   then int32 n_runs and real64 ds(n_runs).
! OUT (total = n_runs * nray): int32 npoints(total), stop_code(total), real64 start_ray_vec(nv, total),
!   end_ray_vec(nv, total), end_residuals(total), max_residuals(total), work_a(total, n_bins_a) (bin-major, as on the
!   device), profile_a(n_bins_a, n_runs), work_b(total, n_bins_b), profile_b(n_bins_b, n_runs), and profile_a once more
!   from the sum alone.

    use, intrinsic :: iso_c_binding
    use rays_hip_m

    implicit none

    interface
       integer(c_int) function hipMalloc(ptr, bytes) bind(C, name='hipMalloc')
          import :: c_int, c_ptr, c_size_t
          type(c_ptr), intent(out) :: ptr
          integer(c_size_t), value :: bytes
       end function hipMalloc
       integer(c_int) function hipFree(ptr) bind(C, name='hipFree')
          import :: c_int, c_ptr
          type(c_ptr), value :: ptr
       end function hipFree
       integer(c_int) function hipMemcpy(dst, src, bytes, kind) bind(C, name='hipMemcpy')
          import :: c_int, c_ptr, c_size_t
          type(c_ptr), value :: dst, src
          integer(c_size_t), value :: bytes
          integer(c_int), value :: kind
       end function hipMemcpy
       integer(c_int) function hipMemset(dst, val, bytes) bind(C, name='hipMemset')
          import :: c_int, c_ptr, c_size_t
          type(c_ptr), value :: dst
          integer(c_int), value :: val
          integer(c_size_t), value :: bytes
       end function hipMemset
       integer(c_int) function hipDeviceSynchronize() bind(C, name='hipDeviceSynchronize')
          import :: c_int
       end function hipDeviceSynchronize
    end interface
    integer(c_int), parameter :: H2D = 1, D2H = 2

    type table_t
        real(c_double), allocatable :: a(:)
    end type table_t

    character(len=1024) :: fin, fout
    integer(c_int32_t) :: nray, nv, nb(2), which(2), nx, n_rho, tn(6), n, n_runs, total
    type(rays_params_t) :: p
    type(rays_axisym_tables_t) :: t
    type(rays_dep_profile_t) :: rec(2)
    type(table_t), target :: tab(11)
    real(c_double) :: x_min, x_max
    real(c_double), allocatable, target :: rvec0(:,:), rindex_vec0(:,:), power(:), fspl(:,:), rho_grid(:), rho_fspl(:,:), ds(:)
    integer(c_int32_t), allocatable, target :: npoints(:), stop_code(:)
    real(c_double), allocatable, target :: start_ray_vec(:,:), end_ray_vec(:,:), end_residuals(:), max_residuals(:)
    real(c_double), allocatable, target :: work_a(:,:), work_b(:,:), profile_a(:,:), profile_b(:,:), profile_again(:,:)
    type(c_ptr) :: d_r0, d_n0, d_pw, d_ds, d_work(2), d_prof(2), d_again, d_start, d_np, d_sc, d_end, d_er, d_mr
    integer(c_size_t) :: nr8, tot8, run8
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
    read(u) n_runs
    if (n_runs < 1) stop 3
    allocate(ds(n_runs))
    read(u) ds
    close(u)
    if (rays_hip_set_zfun_table(fspl, nx, x_min, x_max) /= 0) stop 4
    t%nr = tn(1); t%nz = tn(2); t%n_rb = tn(3); t%n_ne = tn(4); t%n_te = tn(5); t%n_ti = tn(6)
    t%r_grid = ptr(1); t%z_grid = ptr(2); t%psi_fspl = ptr(3); t%rb_grid = ptr(4); t%rb_fspl = ptr(5); t%ne_grid = ptr(6)
    t%ne_fspl = ptr(7); t%te_grid = ptr(8); t%te_fspl = ptr(9); t%ti_grid = ptr(10); t%ti_fspl = ptr(11)
    if (rays_hip_set_axisym_tables(t) /= 0) stop 5
    if (rays_hip_set_rho_table(rho_grid, rho_fspl, n_rho) /= 0) stop 6
    if (rays_hip_init(1) < 1) stop 7

    total = n_runs * nray
    nr8 = 8_c_size_t * int(nray, c_size_t)
    tot8 = 8_c_size_t * int(total, c_size_t)
    run8 = 8_c_size_t * int(n_runs, c_size_t)
    d_r0 = dev(3 * nr8); d_n0 = dev(3 * nr8); d_pw = dev(nr8); d_ds = dev(run8)
    d_start = dev(nv * tot8); d_np = dev(tot8 / 2); d_sc = dev(tot8 / 2); d_end = dev(nv * tot8); d_er = dev(tot8); d_mr = dev(tot8)
    do k = 1, 2
        d_work(k) = dev(nb(k) * tot8)
        d_prof(k) = dev(nb(k) * run8)
        rec(k) = rays_dep_profile_t(which(k), nb(k), d_work(k), c_null_ptr, d_prof(k))
    end do
    d_again = dev(nb(1) * run8)
    if (hipMemcpy(d_r0, c_loc(rvec0), 3 * nr8, H2D) /= 0) stop 9
    if (hipMemcpy(d_n0, c_loc(rindex_vec0), 3 * nr8, H2D) /= 0) stop 9
    if (hipMemcpy(d_pw, c_loc(power), nr8, H2D) /= 0) stop 9
    if (hipMemcpy(d_ds, c_loc(ds), run8, H2D) /= 0) stop 9
    if (rays_hip_scan_profiles_device(p, n_runs, d_ds, nray, d_r0, d_n0, d_pw, 2, rec, d_np, d_sc, d_start, d_end, d_er, &
         & d_mr, c_null_ptr) /= 0) stop 10
    if (rays_hip_profile_sum_segments_device(nb(1), total, n_runs, c_null_ptr, nray, d_work(1), c_null_ptr, d_again, &
         & c_null_ptr) /= 0) stop 11

    allocate(npoints(total), stop_code(total), start_ray_vec(nv, total), end_ray_vec(nv, total), end_residuals(total), &
           & max_residuals(total), work_a(total, nb(1)), work_b(total, nb(2)), profile_a(nb(1), n_runs), &
           & profile_b(nb(2), n_runs), profile_again(nb(1), n_runs))
    if (hipDeviceSynchronize() /= 0) stop 15
    if (hipMemcpy(c_loc(npoints), d_np, tot8 / 2, D2H) /= 0) stop 16
    if (hipMemcpy(c_loc(stop_code), d_sc, tot8 / 2, D2H) /= 0) stop 16
    if (hipMemcpy(c_loc(start_ray_vec), d_start, nv * tot8, D2H) /= 0) stop 16
    if (hipMemcpy(c_loc(end_ray_vec), d_end, nv * tot8, D2H) /= 0) stop 16
    if (hipMemcpy(c_loc(end_residuals), d_er, tot8, D2H) /= 0) stop 16
    if (hipMemcpy(c_loc(max_residuals), d_mr, tot8, D2H) /= 0) stop 16
    if (hipMemcpy(c_loc(work_a), d_work(1), nb(1) * tot8, D2H) /= 0) stop 16
    if (hipMemcpy(c_loc(work_b), d_work(2), nb(2) * tot8, D2H) /= 0) stop 16
    if (hipMemcpy(c_loc(profile_a), d_prof(1), nb(1) * run8, D2H) /= 0) stop 16
    if (hipMemcpy(c_loc(profile_b), d_prof(2), nb(2) * run8, D2H) /= 0) stop 16
    if (hipMemcpy(c_loc(profile_again), d_again, nb(1) * run8, D2H) /= 0) stop 16

    open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace', action='write')
    write(u) npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals, work_a, profile_a, work_b, &
           & profile_b, profile_again
    close(u)
    if (rays_hip_finalize() /= 0) stop 17

 contains

    function ptr(k) result(c)
        integer, intent(in) :: k
        type(c_ptr) :: c
        c = c_null_ptr
        if (size(tab(k)%a) > 0) c = c_loc(tab(k)%a)
    end function ptr

    function dev(bytes) result(c)
        integer(c_size_t), intent(in) :: bytes
        type(c_ptr) :: c
        if (hipMalloc(c, bytes) /= 0) stop 20
    end function dev

 end program scan_profiles_driver
