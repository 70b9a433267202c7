! TEST INFRASTRUCTURE ONLY.  What the compiler makes of norm2 on 3- and 2-element arrays and of minval on a two-element
! array constructor, in the forms post_process_lib/OX_conv_analysis_m.f90 uses them (a section of a derived type's
! component, an array constructor); tests/test_cpu_ox_conv.py holds tests/ox_conv_expect.py's restatement to it.
!   argument 1: raw stream of int32 n, then n times (a, b, c) as doubles
!   argument 2: output, n times (norm2 of (a, b, c), norm2 of (a, b), minval of (a, b)) as doubles
program norm2_minval_probe
    implicit none
    integer, parameter :: rkind = selected_real_kind(15, 307)
    type vecs
        real(kind=rkind) :: g(3, 0:1)
    end type vecs
    type(vecs) :: e
    character(len=256) :: fin, fout
    integer :: uin, uout, n, i
    real(kind=rkind) :: v(3), r, m
    call get_command_argument(1, fin)
    call get_command_argument(2, fout)
    open(newunit=uin, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
    open(newunit=uout, file=trim(fout), access='stream', form='unformatted', status='replace')
    read(uin) n
    do i = 1, n
        read(uin) v
        e%g(:, 0) = v
        e%g(:, 1) = 0.
        r = norm2((/v(1), v(2)/))
        m = minval((/v(1), 0.25_rkind*v(2)/))
        write(uout) norm2(e%g(:, 0)), r, m
    end do
    close(uin)
    close(uout)
end program norm2_minval_probe
