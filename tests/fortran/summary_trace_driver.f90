 program summary_trace_driver
! TEST INFRASTRUCTURE ONLY (tests/test_gpu_summary_trace.py): calls the summary-only entries through
! fortran/rays_hip_m.f90 -- rays_hip_trace_summary on host arrays, then rays_hip_scan_summary_device, one launch for all
! runs of a `ds` scan, whose outputs are what scanner_m's aggregate_run_data keeps of every run -- and writes what came
! back to a flat file.
!     summary_trace_driver IN OUT
! IN (stream, native): int32 nray, nv, n_runs; the bytes of rays_params_t; real64 rvec0(3, nray), rindex_vec0(3, nray),
!   ds_values(n_runs).
! OUT: the host entry's int32 npoints(nray), stop_code(nray), real64 start_ray_vec(nv, nray), end_ray_vec(nv, nray),
!   end_residuals(nray), max_residuals(nray); then the scan's, the same six arrays with a trailing run dimension.
! The device memory comes from the HIP runtime's C entry points, declared below.

    use, intrinsic :: iso_c_binding
    use rays_hip_m

    implicit none

    integer(c_int), parameter :: H2D = 1, D2H = 2   ! hipMemcpyHostToDevice, hipMemcpyDeviceToHost

    interface
       integer(c_int) function hipMalloc(ptr, nbytes) bind(C, name='hipMalloc')
          import :: c_int, c_ptr, c_size_t
          type(c_ptr), intent(out) :: ptr
          integer(c_size_t), value :: nbytes
       end function hipMalloc
       integer(c_int) function hipMemcpy(dst, src, nbytes, kind) bind(C, name='hipMemcpy')
          import :: c_int, c_ptr, c_size_t
          type(c_ptr), value :: dst, src
          integer(c_size_t), value :: nbytes
          integer(c_int), value :: kind
       end function hipMemcpy
       integer(c_int) function hipFree(ptr) bind(C, name='hipFree')
          import :: c_int, c_ptr
          type(c_ptr), value :: ptr
       end function hipFree
    end interface

    character(len=1024) :: fin, fout
    integer(c_int32_t) :: nray, nv, n_runs
    type(rays_params_t) :: p
    real(c_double), allocatable, target :: rvec0(:,:), rindex_vec0(:,:), ds_values(:)
    integer(c_int32_t), allocatable, target :: npoints(:), stop_code(:), s_npoints(:,:), s_stop_code(:,:)
    real(c_double), allocatable, target :: start_ray_vec(:,:), end_ray_vec(:,:), end_residuals(:), max_residuals(:)
    real(c_double), allocatable, target :: s_start(:,:,:), s_end(:,:,:), s_end_residuals(:,:), s_max_residuals(:,:)
    type(c_ptr) :: d_r, d_n, d_ds, d_np, d_sc, d_sv, d_ev, d_er, d_mr
    real(c_double) :: elapsed
    integer(c_size_t) :: n1, nt
    integer :: u

    call get_command_argument(1, fin)
    call get_command_argument(2, fout)
    open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
    read(u) nray, nv, n_runs
    read(u) p
    if (nray < 1 .or. n_runs < 1 .or. nv /= p%nv) stop 3
    allocate(rvec0(3, nray), rindex_vec0(3, nray), ds_values(n_runs))
    read(u) rvec0, rindex_vec0, ds_values
    close(u)

    ! the host entry: every element must come back written
    allocate(npoints(nray), stop_code(nray), start_ray_vec(nv, nray), end_ray_vec(nv, nray), end_residuals(nray), &
           & max_residuals(nray))
    npoints = -7; stop_code = -7; start_ray_vec = -7.; end_ray_vec = -7.; end_residuals = -7.; max_residuals = -7.
    if (rays_hip_trace_summary(p, nray, rvec0, rindex_vec0, npoints, stop_code, start_ray_vec, end_ray_vec, &
         & end_residuals, max_residuals, elapsed) /= 0) stop 4

    ! all runs of the scan in one launch, on device memory
    n1 = int(nray, c_size_t)
    nt = n1 * int(n_runs, c_size_t)
    allocate(s_npoints(nray, n_runs), s_stop_code(nray, n_runs), s_start(nv, nray, n_runs), s_end(nv, nray, n_runs), &
           & s_end_residuals(nray, n_runs), s_max_residuals(nray, n_runs))
    call chk(hipMalloc(d_r, 24 * n1)); call chk(hipMalloc(d_n, 24 * n1)); call chk(hipMalloc(d_ds, 8 * int(n_runs, c_size_t)))
    call chk(hipMalloc(d_np, 4 * nt)); call chk(hipMalloc(d_sc, 4 * nt))
    call chk(hipMalloc(d_sv, 8 * nv * nt)); call chk(hipMalloc(d_ev, 8 * nv * nt))
    call chk(hipMalloc(d_er, 8 * nt)); call chk(hipMalloc(d_mr, 8 * nt))
    call chk(hipMemcpy(d_r, c_loc(rvec0), 24 * n1, H2D))
    call chk(hipMemcpy(d_n, c_loc(rindex_vec0), 24 * n1, H2D))
    call chk(hipMemcpy(d_ds, c_loc(ds_values), 8 * int(n_runs, c_size_t), H2D))
    if (rays_hip_scan_summary_device(p, n_runs, d_ds, nray, d_r, d_n, d_np, d_sc, d_sv, d_ev, d_er, d_mr, &
         & c_null_ptr) /= 0) stop 5
    call chk(hipMemcpy(c_loc(s_npoints), d_np, 4 * nt, D2H))   ! (waits for the kernel)
    call chk(hipMemcpy(c_loc(s_stop_code), d_sc, 4 * nt, D2H))
    call chk(hipMemcpy(c_loc(s_start), d_sv, 8 * nv * nt, D2H))
    call chk(hipMemcpy(c_loc(s_end), d_ev, 8 * nv * nt, D2H))
    call chk(hipMemcpy(c_loc(s_end_residuals), d_er, 8 * nt, D2H))
    call chk(hipMemcpy(c_loc(s_max_residuals), d_mr, 8 * nt, D2H))
    call chk(hipFree(d_r)); call chk(hipFree(d_n)); call chk(hipFree(d_ds)); call chk(hipFree(d_np)); call chk(hipFree(d_sc))
    call chk(hipFree(d_sv)); call chk(hipFree(d_ev)); call chk(hipFree(d_er)); call chk(hipFree(d_mr))

    open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace', action='write')
    write(u) npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals
    write(u) s_npoints, s_stop_code, s_start, s_end, s_end_residuals, s_max_residuals
    close(u)

 contains

    subroutine chk(rc)
       integer(c_int), intent(in) :: rc
       if (rc /= 0) then
          write(*,*) 'summary_trace_driver: HIP runtime error ', rc
          stop 7
       end if
    end subroutine chk

 end program summary_trace_driver
