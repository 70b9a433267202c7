! TEST INFRASTRUCTURE ONLY.
! Driver written for this repo (not reference code): links against the reference RAYS_lib objects built by
! oracle/build_ref.sh, runs the reference's own initialize on the namelist in the working directory (rays.in) and writes
! the fan its ray launcher left in ray_init_m -- the reference for tests/golden/launch_cases.npz (the launches of
! tests/launch_cases.py: every wave mode and sign, fans of every compaction shape, members on either side of the
! evanescent thresholds, degenerate launch points).  It traces nothing.
!
!   RAYS_LAUNCH_OUT   output path, a raw little-endian stream: int32 magic, int32 nray, then rvec0(1:3,1:nray),
!                     rindex_vec0(1:3,1:nray) and ray_pwr_wt(1:nray) as doubles
!
! When every launch is dropped the reference's launcher stops the program ("No successful ray initializations") inside
! initialize: nothing is written, and the generator records the exit status and the text instead.
!
! The Solovev launcher sets ray_pwr_wt(count) after each r loop and nothing else: the other entries of the array are
! whatever the allocation held.  The driver writes them as they are; the reader keeps only the entries that were set.
program ref_launch_driver
    use constants_m, only : rkind
    use ray_init_m, only : nray, rvec0, rindex_vec0, ray_pwr_wt
    implicit none

    logical :: read_input = .true.
    character(len=256) :: fout
    integer :: uout, stat

    call get_environment_variable('RAYS_LAUNCH_OUT', fout, status=stat)
    if (stat /= 0 .or. len_trim(fout) == 0) then
       write(0,*) 'ref_launch_driver: RAYS_LAUNCH_OUT not set'
       stop 1
    end if

    call initialize(read_input)

    open(newunit=uout, file=trim(fout), access='stream', form='unformatted', status='replace')
    write(uout) int(z'4c41554e'), nray
    write(uout) rvec0(1:3,1:nray)
    write(uout) rindex_vec0(1:3,1:nray)
    write(uout) ray_pwr_wt(1:nray)
    close(uout)
    write(*,'(a,i0)') 'RAYS_REF_LAUNCH nray = ', nray
end program ref_launch_driver
