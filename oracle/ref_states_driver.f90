! TEST INFRASTRUCTURE ONLY.
! Driver written for this repo (not reference code): links against the reference RAYS_lib objects built by
! oracle/build_ref.sh, runs the reference's own initialize, and then evaluates the reference's right-hand side at
! STATES READ FROM A FILE instead of tracing rays -- the reference for tests/golden/rhs_state_cases.npz (synthetic
! states of tests/rhs_state_cases.py: thresholds of the box tests, the plasma edge, the damping argument, check_save).
!
!   RAYS_STATES_IN    raw little-endian stream: int32 n, int32 nv, then n times (s, v(1:nv)) as doubles
!   RAYS_STATES_OUT   output path: int32 magic, n, nv, nspec, rk4 (1 = the step records follow each probe record), then
!                     per state the probe record of oracle/ref_dump_driver.f90 (equilibrium, deriv_cold, deriv_num,
!                     eqn_ray with dvds zeroed first, check_save with the stop record cleared before each) with the
!                     flag text equilibrium, eqn_ray and check_save each left, and for RK4 configurations the step
!                         call ode_solver(eqn_ray, nv, v, s, s + ds, ray_stop) ; call check_save(s, nv, v, resid, ray_stop)
!                     as trace_rays has them (check_save only if the solver did not stop), plus the flag equilibrium
!                     leaves at the new state.
!
! deriv_num evaluates equilibrium at the six points r +- 1.e-6 e_i (deriv_num.f90:37-57) and uses what comes back without
! looking at equib_err: where one of them errs, its dD/dx is undefined too.  The driver asks the reference's equilibrium
! at those points and writes the number that err (num_undef); for a configuration that integrates with the numerical
! derivatives it does the same at the stage states of the step (step_num_undef).
!
! Where equilibrium returns with an error the reference's eq_point is undefined (equilibrium_m.f90:198-202 returns
! before anything is stored): the values of such a record are whatever the previous state left, and only the
! equilibrium and eqn_ray flags are facts.  The reader (tests/refdump.py: read_states) blanks the rest.
program ref_states_driver
    use constants_m, only : rkind
    use species_m, only : nspec
    use rf_m, only : k0
    use ode_m, only : nv, ds, ode_stop, ode_solver, ode_solver_name, ray_deriv_name
    use equilibrium_m, only : equilibrium, eq_point
    implicit none

    logical :: read_input = .true.
    character(len=256) :: fin, fout
    integer :: uin, uout, stat, n, nv_file, i, is, rk4
    real(kind=rkind) :: s, s1, sout, resid
    real(kind=rkind), allocatable :: v(:), dvds(:), v1(:)
    real(kind=rkind) :: dddx(3), dddk(3), dddw, ndx(3), ndk(3), ndw, nvec(3)
    type(eq_point) :: eq, eq1
    type(ode_stop) :: rs
    character(len=30) :: flag_eqn, flag_cs, flag_step, flag_cs1
    integer :: stop_eqn, stop_cs, stop_step, stop_cs1, num_undef, step_num_undef, j
    real(kind=rkind), allocatable :: x(:), f(:)
    type(ode_stop) :: rs2

    interface
       subroutine deriv_cold(eq, nvec, dddx, dddk, dddw)
          use constants_m, only : rkind
          use equilibrium_m, only : eq_point
          type(eq_point), intent(in) :: eq
          real(KIND=rkind), intent(in) :: nvec(3)
          real(KIND=rkind), intent(out) :: dddx(3), dddk(3), dddw
       end subroutine deriv_cold
       subroutine deriv_num(eq, v, dddx, dddk, dddw)
          use constants_m, only : rkind
          use equilibrium_m, only : eq_point
          use ode_m, only : nv
          type(eq_point), intent(in) :: eq
          real(KIND=rkind), intent(in) :: v(nv)
          real(KIND=rkind), intent(out) :: dddx(3), dddk(3), dddw
       end subroutine deriv_num
       subroutine eqn_ray(s, v, dvds, ray_stop)
          use constants_m, only : rkind
          use ode_m, only : nv, ode_stop
          real(KIND=rkind), intent(in) :: s
          real(KIND=rkind), intent(in) :: v(nv)
          real(KIND=rkind), intent(out) :: dvds(nv)
          type(ode_stop) :: ray_stop
       end subroutine eqn_ray
       subroutine check_save(s, nv, v, resid, ray_stop)
          use constants_m, only : rkind
          use ode_m, only : ode_stop
          real(KIND=rkind), intent(in) :: s
          integer, intent(in) :: nv
          real(KIND=rkind), intent(in) :: v(nv)
          real(KIND=rkind), intent(out) :: resid
          type(ode_stop) :: ray_stop
       end subroutine check_save
    end interface

    call get_environment_variable('RAYS_STATES_IN', fin, status=stat)
    if (stat /= 0 .or. len_trim(fin) == 0) then
       write(0,*) 'ref_states_driver: RAYS_STATES_IN not set'
       stop 1
    end if
    call get_environment_variable('RAYS_STATES_OUT', fout, status=stat)
    if (stat /= 0 .or. len_trim(fout) == 0) then
       write(0,*) 'ref_states_driver: RAYS_STATES_OUT not set'
       stop 1
    end if

    call initialize(read_input)

    open(newunit=uin, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
    read(uin) n, nv_file
    if (nv_file /= nv) then
       write(0,*) 'ref_states_driver: the states have nv = ', nv_file, ', the configuration nv = ', nv
       stop 1
    end if
    rk4 = 0
    if (trim(ode_solver_name) == 'RK4_ODE') rk4 = 1
    allocate(v(nv), dvds(nv), v1(nv), x(nv), f(nv))

    open(newunit=uout, file=trim(fout), access='stream', form='unformatted', status='replace')
    write(uout) int(z'52485353'), n, nv, nspec, rk4
    do i = 1, n
       read(uin) s, v
       call equilibrium(v(1:3), eq)
       nvec = v(4:6)/k0
       call deriv_cold(eq, nvec, dddx, dddk, dddw)
       call deriv_num(eq, v, ndx, ndk, ndw)
       rs%stop_ode = .false. ; rs%ode_stop_flag = ''
       dvds = 0.
       call eqn_ray(s, v, dvds, rs)
       flag_eqn = rs%ode_stop_flag ; stop_eqn = merge(1, 0, rs%stop_ode)
       rs%stop_ode = .false. ; rs%ode_stop_flag = ''
       call check_save(s, nv, v, resid, rs)
       flag_cs = rs%ode_stop_flag ; stop_cs = merge(1, 0, rs%stop_ode)
       write(uout) v
       write(uout) eq%equib_err
       write(uout) eq%bvec, eq%bmag, eq%gradbmag, eq%bunit, eq%gradbunit, eq%gradbtensor
       do is = 0, nspec
          write(uout) eq%ns(is), eq%gradns(:,is), eq%ts(is), eq%gradts(:,is), &
                    & eq%omgc(is), eq%omgp2(is), eq%alpha(is), eq%gamma(is)
       end do
       write(uout) dddx, dddk, dddw
       write(uout) ndx, ndk, ndw
       write(uout) dvds
       write(uout) resid
       num_undef = displaced_errors(v(1:3))
       write(uout) flag_eqn, stop_eqn, flag_cs, stop_cs, num_undef
       if (rk4 == 1) then
          v1 = v ; s1 = s ; sout = s1 + ds
          resid = 0.
          rs%stop_ode = .false. ; rs%ode_stop_flag = ''
          call ode_solver(eqn_ray, nv, v1, s1, sout, rs)
          flag_step = rs%ode_stop_flag ; stop_step = merge(1, 0, rs%stop_ode)
          flag_cs1 = '' ; stop_cs1 = 0
          if (.not. rs%stop_ode) then
             call check_save(s1, nv, v1, resid, rs)
             flag_cs1 = rs%ode_stop_flag ; stop_cs1 = merge(1, 0, rs%stop_ode)
          end if
          call equilibrium(v1(1:3), eq1)
          step_num_undef = 0
          if (trim(ray_deriv_name) == 'numerical') then   ! the stage states of RK4_ode (RK4_ode_m.f90:81-89)
             x = v
             do j = 1, 4
                rs2%stop_ode = .false. ; rs2%ode_stop_flag = ''
                call eqn_ray(s, x, f, rs2)
                if (trim(rs2%ode_stop_flag) /= '' .and. trim(rs2%ode_stop_flag) /= 'infinite Vg' .and. &
                  & trim(rs2%ode_stop_flag) /= 'ray stalled') exit    ! refused by equilibrium: deriv_num was not reached
                step_num_undef = step_num_undef + displaced_errors(x(1:3))
                if (rs2%stop_ode .or. j == 4) exit
                if (j < 3) then
                   x = v + (sout - s)*f/2.0
                else
                   x = v + (sout - s)*f
                end if
             end do
          end if
          write(uout) v1
          write(uout) resid
          write(uout) flag_step, stop_step, flag_cs1, stop_cs1, step_num_undef
          write(uout) eq1%equib_err
       end if
    end do
    close(uin)
    close(uout)
    write(*,'(a,i0)') 'RAYS_REF_STATES records = ', n
contains

    ! how many of the six points deriv_num displaces r to are refused by the reference's equilibrium
    integer function displaced_errors(r)
       real(kind=rkind), intent(in) :: r(3)
       real(kind=rkind) :: q(3), delta
       type(eq_point) :: e
       integer :: i, sgn
       delta = 1.e-6
       displaced_errors = 0
       do i = 1, 3
          do sgn = -1, 1, 2
             q = r
             q(i) = r(i) + sgn*delta
             call equilibrium(q, e)
             if (e%equib_err /= '') displaced_errors = displaced_errors + 1
          end do
       end do
    end function displaced_errors
end program ref_states_driver
