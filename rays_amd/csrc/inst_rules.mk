# inst_rules.mk -- the variants of rays_inst.hip, once, for every build that compiles it: the product library
# (Makefile here), the emulated C ABI of the CPU tier (tests/hip_emul/Makefile.capi) and the developer tools
# (print-defs below).
#
# A variant is the same source compiled with other -DRAYS_INST_* switches and another offset in the kernels' EQ template
# argument (rays_device.hpp, rays_device_arith.inc: kEqTol 16, kEqNoTraj 32, kEqDeposit 64, kEqContinue 128); its
# objects are <variant>_<group>.o.  One line each:
#                          variant  EQ offset  switches
INST_VARIANTS :=
inst_variant = $(eval INST_VARIANTS += $1)$(eval INST_EQT_$1 := $2)$(eval INST_DEFS_$1 := $3)
$(call inst_variant,inst,0,)
$(call inst_variant,sum,32,-DRAYS_INST_NOTRAJ=1)
$(call inst_variant,dep,96,-DRAYS_INST_NOTRAJ=1 -DRAYS_INST_DEPOSIT=1)
$(call inst_variant,win,128,-DRAYS_INST_CONTINUE=1)
$(call inst_variant,wsum,160,-DRAYS_INST_CONTINUE=1 -DRAYS_INST_NOTRAJ=1)
$(call inst_variant,tol,16,-DRAYS_INST_TOL=1)
$(call inst_variant,dep2,352,-DRAYS_INST_NOTRAJ=1 -DRAYS_INST_DEPOSIT=1 -DRAYS_INST_DEPOSIT2=1)
$(call inst_variant,wdep,224,-DRAYS_INST_CONTINUE=1 -DRAYS_INST_NOTRAJ=1 -DRAYS_INST_DEPOSIT=1)
$(call inst_variant,wdep2,480,-DRAYS_INST_CONTINUE=1 -DRAYS_INST_NOTRAJ=1 -DRAYS_INST_DEPOSIT=1 -DRAYS_INST_DEPOSIT2=1)
# (inst: the kernels record the trajectories; sum: summary-only; dep: fused deposition; win, wsum: the continuation
# kernels of windowed tracing, recording and summary-only; tol: the tolerance flavour of the cold RK4 groups; dep2: fused
# deposition into two profiles, kEqDeposit2 256, of the axisym_toroid groups; wdep, wdep2: the continuation kernels of
# dep and dep2, windowed tracing that bins what it accepts.  Which
# kernels of the shape lists a variant keeps: rays_inst.hip.)
#
# The including Makefile supplies
#   INST_COMPILE         the compiler command with its flags (expanded in the recipe, so target-specific flags work)
#   INST_COMPILE_<v>     the same for variant <v>, where it differs (tol: the tolerance flags)
#   INST_BUILD           the build directory
#   INST_SRC             the path of rays_inst.hip
#   INST_DEPS            the objects' other prerequisites
# and lists the objects it links.

# A group is solver_equilibrium_derivative_unitexp_multispec.  A stem of two numbers, <equilibrium>_<unitexp>, names the
# cold RK4 group 0_<equilibrium>_0_<unitexp>_0: the tolerance objects are tol_<e>_<u>.o.
inst_group = $(if $(word 5,$(subst _, ,$1)),$(subst _, ,$1),0 $(word 1,$(subst _, ,$1)) 0 $(word 2,$(subst _, ,$1)) 0)
# The -D set of (variant, stem).  RAYS_INST_EQT, the kernels' EQ argument as a literal for their names, is computed here
# and nowhere else; the static_assert of rays_inst.hip cross-checks it.
inst_defs = $(INST_DEFS_$1) $(call inst_group_defs,$(call inst_group,$2),$(INST_EQT_$1))
inst_group_defs = -DRAYS_INST_SOLVER=$(word 1,$1) -DRAYS_INST_EQ=$(word 2,$1) -DRAYS_INST_DERIV=$(word 3,$1) \
  -DRAYS_INST_UE=$(word 4,$1) -DRAYS_INST_MS=$(word 5,$1) \
  -DRAYS_INST_EQT=$(shell echo $$(( $(word 2,$1) + 4 * $(word 4,$1) + 8 * $(word 5,$1) + $2 )))

define inst_rule
$$(INST_BUILD)/$1_%.o: $$(INST_SRC) $$(INST_DEPS)
	$$(or $$(INST_COMPILE_$1),$$(INST_COMPILE)) $$(call inst_defs,$1,$$*) -c $$(INST_SRC) -o $$@
endef
$(foreach v,$(INST_VARIANTS),$(eval $(call inst_rule,$(v))))

# make -s -f inst_rules.mk print-defs VARIANT=sum GROUP=0_1_0_1_0   ->   the -D set of that object
print-defs:
	@echo $(call inst_defs,$(VARIANT),$(GROUP))
.PHONY: print-defs
