! TEST INFRASTRUCTURE ONLY.
! Driver written for this repo (not reference code): links against the reference's
! bin_to_uniform_grid_m object built by oracle/build_ref.sh and runs the reference's own
!     binner_real      (RAYS_project/math_functions_lib/bin_to_uniform_grid_m.f90)
! -- the uniform grid binner under calculate_deposition_profiles / bin_a_ray -- on synthetic rays, so
! that tests/golden/deposition_binner_cases.npz (tests/golden/make_golden.py) can be cut from the
! reference itself for the binner branches that no traced fixture reaches.
!
!     ref_binner <case file> <result file>          (both raw little-endian stream files)
!
! case file:    int32 ncase, then per case: real64 xmin, xmax; int32 n_bins, nx; real64 xQ(1:nx), Q(1:nx)
! result file:  per case: int32 ierr; real64 binned_Q(1:n_bins)
!
! The caller keeps every case inside what the reference defines: a segment whose upper end lies below
! xmax while floor((x_high - xmin)/x_bin_width) >= n_bins makes binner_real update binned_Q(n_bins + 1)
! (DESIGN.md section 2 (vi)); tests/deposition_cases.py asserts that no case here has one.
program ref_binner_driver
    use bin_to_uniform_grid_m, only : rkind, binner_real
    implicit none

    character(len=1024) :: fin, fout
    integer :: uin, uout, ncase, icase, n_bins, nx, ierr
    real(kind=rkind) :: xmin, xmax
    real(kind=rkind), allocatable :: xQ(:), Q(:), binned_Q(:)

    if (command_argument_count() /= 2) then
        write(*,*) 'usage: ref_binner <case file> <result file>'
        stop 1
    end if
    call get_command_argument(1, fin)
    call get_command_argument(2, fout)
    open(newunit=uin, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
    open(newunit=uout, file=trim(fout), access='stream', form='unformatted', status='replace', action='write')

    read(uin) ncase
    do icase = 1, ncase
        read(uin) xmin, xmax
        read(uin) n_bins, nx
        if (n_bins < 1 .or. nx < 0) then
            write(*,*) 'ref_binner: bad case ', icase, n_bins, nx
            stop 1
        end if
        allocate(xQ(nx), Q(nx), binned_Q(n_bins))
        read(uin) xQ
        read(uin) Q
        call binner_real(Q, xQ, xmin, xmax, binned_Q, ierr)
        write(uout) ierr
        write(uout) binned_Q
        deallocate(xQ, Q, binned_Q)
    end do
    close(uin)
    close(uout)
end program ref_binner_driver
