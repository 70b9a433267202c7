 program ray_diagnostics_driver
! TEST INFRASTRUCTURE ONLY (tests/test_gpu_ray_diagnostics.py): runs fortran/ray_diagnostics_hip.f90's
! ray_detailed_diagnostics_hip on one fixture's ray_results_m arrays read from a flat file and writes the
! seventeen arrays and first_bad to another.
!     ray_diagnostics_driver IN OUT
! IN (stream, native): int32 nray, npt, nv, slab, nx of the Z-function table (0 = none); the bytes of rays_params_t;
!   [real64 x_min, x_max, fspl_re(4, nx)]; ray_vec(nv, npt, nray), residual(npt, nray), int32 npoints(nray).
! OUT: the seventeen arrays in the module procedure's argument order, each (npt, nray); int32 first_bad(nray).

    use, intrinsic :: iso_c_binding
    use rays_hip_m
    use ray_diagnostics_hip_m

    implicit none

    character(len=1024) :: fin, fout
    integer(c_int32_t) :: nray, npt, nv, slab, nx
    type(rays_params_t) :: p
    real(c_double) :: x_min, x_max
    real(c_double), allocatable :: fspl(:,:), ray_vec(:,:,:), residual_results(:,:), a(:,:,:)
    integer(c_int32_t), allocatable :: np32(:)
    integer, allocatable :: npoints(:), first_bad(:)
    integer :: u, k

    call get_command_argument(1, fin)
    call get_command_argument(2, fout)
    open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
    read(u) nray, npt, nv, slab, nx
    read(u) p
    if (nx > 0) then
       allocate(fspl(4, nx))
       read(u) x_min, x_max, fspl
       if (rays_hip_set_zfun_table(fspl, nx, x_min, x_max) /= 0) stop 2
    end if
    allocate(ray_vec(nv, npt, nray), residual_results(npt, nray), np32(nray), npoints(nray), first_bad(nray))
    allocate(a(npt, nray, 17))
    read(u) ray_vec, residual_results, np32
    close(u)
    npoints = np32
    a = -1.   ! intent(out): every element must come back written

    call ray_detailed_diagnostics_hip(p, int(nray), int(npt), int(nv), ray_vec, residual_results, npoints, &
         & a(:,:,1), a(:,:,2), a(:,:,3), a(:,:,4), a(:,:,5), a(:,:,6), a(:,:,7), a(:,:,8), a(:,:,9), a(:,:,10), &
         & a(:,:,11), a(:,:,12), a(:,:,13), a(:,:,14), a(:,:,15), a(:,:,16), a(:,:,17), first_bad, slab = (slab /= 0))

    open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace', action='write')
    do k = 1, 17
       write(u) a(:,:,k)
    end do
    np32 = first_bad
    write(u) np32
    close(u)

 end program ray_diagnostics_driver
