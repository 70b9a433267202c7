 program ray_diagnostics_packed_driver
! TEST INFRASTRUCTURE ONLY (tests/test_gpu_ray_diagnostics_packed.py): calls rays_hip_point_offsets_device and
! rays_hip_ray_diagnostics_packed_device through fortran/rays_hip_m.f90 on one fixture's ray_results_m arrays read from
! a flat file, with all nineteen fields, and writes what came back to another.
!     ray_diagnostics_packed_driver IN OUT
! IN (stream, native): int32 nray, npt, nv, in_layout (RAYS_DIAG_IN_*), nx of the Z-function table (0 = none); the
!   bytes of rays_params_t; [real64 x_min, x_max, fspl_re(4, nx)]; ray_vec(nv, npt, nray), residual(npt, nray), int32
!   npoints(nray).  With in_layout = RAYS_DIAG_IN_PACKED the arrays are packed here on the host before the upload.
! OUT: int64 offsets(0:nray); real64 out(total, 19); int32 first_bad(nray).
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
    integer(c_int32_t) :: nray, npt, nv, in_layout, nx
    type(rays_params_t) :: p
    real(c_double) :: x_min, x_max
    real(c_double), allocatable, target :: fspl(:,:), ray_vec(:,:,:), residual_results(:,:), pv(:,:), pr(:), out(:,:)
    integer(c_int32_t), allocatable, target :: npoints(:), first_bad(:)
    integer(c_int64_t), allocatable, target :: offsets(:)
    type(c_ptr) :: d_rv, d_res, d_np, d_off, d_out, d_bad
    integer(c_int64_t) :: total, o
    integer(c_int32_t) :: fields
    integer :: u, i, n

    call get_command_argument(1, fin)
    call get_command_argument(2, fout)
    open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
    read(u) nray, npt, nv, in_layout, nx
    read(u) p
    if (nx > 0) then
       allocate(fspl(4, nx))
       read(u) x_min, x_max, fspl
       if (rays_hip_set_zfun_table(fspl, nx, x_min, x_max) /= 0) stop 2
    end if
    allocate(ray_vec(nv, npt, nray), residual_results(npt, nray), npoints(nray), first_bad(nray), offsets(0:nray))
    read(u) ray_vec, residual_results, npoints
    close(u)
    if (nray < 1) stop 3

    ! the offsets, on the device; the total comes back with them
    call chk(hipMalloc(d_np, int(4 * nray, c_size_t)))
    call chk(hipMalloc(d_off, int(8 * (nray + 1), c_size_t)))
    call chk(hipMemcpy(d_np, c_loc(npoints), int(4 * nray, c_size_t), H2D))
    if (rays_hip_point_offsets_device(nray, npt - 1, d_np, d_off, c_null_ptr) /= 0) stop 4
    call chk(hipMemcpy(c_loc(offsets), d_off, int(8 * (nray + 1), c_size_t), D2H))
    total = offsets(nray)
    if (total < 1) stop 5

    if (in_layout == RAYS_DIAG_IN_PACKED) then
       allocate(pv(nv, total), pr(total))
       do i = 1, nray
          o = offsets(i - 1)
          n = int(offsets(i) - o)
          pv(:, o + 1 : o + n) = ray_vec(:, 1:n, i)
          pr(o + 1 : o + n) = residual_results(1:n, i)
       end do
       call chk(hipMalloc(d_rv, int(8, c_size_t) * nv * total))
       call chk(hipMalloc(d_res, int(8, c_size_t) * total))
       call chk(hipMemcpy(d_rv, c_loc(pv), int(8, c_size_t) * nv * total, H2D))
       call chk(hipMemcpy(d_res, c_loc(pr), int(8, c_size_t) * total, H2D))
    else
       call chk(hipMalloc(d_rv, int(8, c_size_t) * nv * npt * nray))
       call chk(hipMalloc(d_res, int(8, c_size_t) * npt * nray))
       call chk(hipMemcpy(d_rv, c_loc(ray_vec), int(8, c_size_t) * nv * npt * nray, H2D))
       call chk(hipMemcpy(d_res, c_loc(residual_results), int(8, c_size_t) * npt * nray, H2D))
    end if

    allocate(out(total, RAYS_DIAG_NFIELDS))
    out = -1.   ! every element must come back written
    first_bad = -1
    call chk(hipMalloc(d_out, int(8, c_size_t) * total * RAYS_DIAG_NFIELDS))
    call chk(hipMalloc(d_bad, int(4 * nray, c_size_t)))
    call chk(hipMemcpy(d_out, c_loc(out), int(8, c_size_t) * total * RAYS_DIAG_NFIELDS, H2D))
    fields = int(ishft(1, RAYS_DIAG_NFIELDS) - 1, c_int32_t)
    if (rays_hip_ray_diagnostics_packed_device(p, nray, in_layout, d_rv, d_res, d_np, d_off, total, fields, d_out, &
         & d_bad, c_null_ptr) /= 0) stop 6
    call chk(hipMemcpy(c_loc(out), d_out, int(8, c_size_t) * total * RAYS_DIAG_NFIELDS, D2H))   ! (waits for the kernel)
    call chk(hipMemcpy(c_loc(first_bad), d_bad, int(4 * nray, c_size_t), D2H))
    call chk(hipFree(d_rv)); call chk(hipFree(d_res)); call chk(hipFree(d_np)); call chk(hipFree(d_off))
    call chk(hipFree(d_out)); call chk(hipFree(d_bad))

    open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace', action='write')
    write(u) offsets
    write(u) out
    write(u) first_bad
    close(u)

 contains

    subroutine chk(rc)
       integer(c_int), intent(in) :: rc
       if (rc /= 0) then
          write(*,*) 'ray_diagnostics_packed_driver: HIP runtime error ', rc
          stop 7
       end if
    end subroutine chk

 end program ray_diagnostics_packed_driver
