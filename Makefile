# Top-level build.  Default target mirrors the reference's Makefile target name (nbody-sim-new/Makefile:7):
#   make            -> libnbody_hip.so (HIP, gfx950) + oracle + nbody_sim harness
#   make lib        -> nbody-simulation-parallel_amd/libnbody_hip.so only
PKG      := nbody-simulation-parallel_amd
CSRC     := $(PKG)/csrc
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
# -fvisibility=hidden: the shared library exports the entry points of include/nbody_hip.h and nothing else
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function -Iinclude
LIB      := $(PKG)/libnbody_hip.so
# A/B builds (tools/build_ab_*.sh): `make lib LIB=<other .so> O=<suffix>.o <defines>` compiles every object again under another
# name and links it into another library; this file stays the only list of objects
O        := .o

# host side: the reference's own flags (nbody-sim-new/Makefile:1-3)
CXX      ?= g++
CXXFLAGS := -std=c++17 -O3 -fopenmp -Iinclude -I$(PKG)/host
LDFLAGS  := -fopenmp

all: lib oracle nbody_sim

lib: $(LIB)

OBJS := $(addprefix $(CSRC)/,$(addsuffix $(O),force_kernel force_sym_kernel force_launch state_kernels nbx_api nbx_node leaf_pair_kernel \
          leaf_plan_api leaf_far_kernel leaf_phi_kernel octree_device close_hash measure_kernels active_kernel active_jerk_kernel))
# name of the force-kernel variant used when the caller does not pick one
# (round 4: the three-level summation build -- same pair arithmetic, fp32 errors ~3x smaller for +1.5 % time)
DEFAULT_VARIANT ?= fastpk3l_t8_w3_u4
# 1: a single-shard context that was not given a variant runs the symmetric own-shard pass (sympk3l_t8_w3) where its
# decomposition applies; 0: only on request.  The default variant's name above does not change.
SYM_DEFAULT ?= 1
# exact (self-contained, guarded) variant used when the fast path's preconditions do not hold
DEFAULT_EXACT_VARIANT ?= lds_t1_w8_exact_u8

# -fno-slp-vectorize: the packed arithmetic is written by hand on float2 values (see force_kernel.hip)
$(CSRC)/force_kernel$(O): $(CSRC)/force_kernel.hip $(CSRC)/nbx_internal.h
	$(HIPCC) $(HIPFLAGS) $(FORCE_KERNEL_DEFS) -fno-slp-vectorize -c $< -o $@

# the symmetric own-shard pass: same flags as the one-sided force kernels
$(CSRC)/force_sym_kernel$(O): $(CSRC)/force_sym_kernel.hip $(CSRC)/sym_plan.h $(CSRC)/nbx_internal.h
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

$(CSRC)/force_launch$(O): $(CSRC)/force_launch.hip $(CSRC)/nbx_internal.h $(CSRC)/sym_plan.h Makefile
	$(HIPCC) $(HIPFLAGS) -DNBX_DEFAULT_VARIANT='"$(DEFAULT_VARIANT)"' -DNBX_DEFAULT_EXACT_VARIANT='"$(DEFAULT_EXACT_VARIANT)"' -c $< -o $@

# -ffp-contract=off: the fp64 kick/drift must round like the reference's two-step arithmetic
$(CSRC)/state_kernels$(O): $(CSRC)/state_kernels.hip $(CSRC)/nbx_internal.h $(CSRC)/device_sort.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $< -o $@

# forces on a device-resident list of targets: the force kernels' flags
$(CSRC)/active_kernel$(O): $(CSRC)/active_kernel.hip $(CSRC)/nbx_internal.h
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

# the same evaluation with the jerk (fourth-order Hermite): active_kernel's flags
$(CSRC)/active_jerk_kernel$(O): $(CSRC)/active_jerk_kernel.hip $(CSRC)/nbx_internal.h
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

$(CSRC)/nbx_api$(O): $(CSRC)/nbx_api.hip $(CSRC)/nbx_internal.h $(CSRC)/nbx_ctx.h $(CSRC)/device_block.h include/nbody_hip.h Makefile
	$(HIPCC) $(HIPFLAGS) -DNBX_SYM_DEFAULT=$(SYM_DEFAULT) -c $< -o $@

$(CSRC)/nbx_node$(O): $(CSRC)/nbx_node.hip $(CSRC)/nbx_internal.h $(CSRC)/nbx_ctx.h include/nbody_hip.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/measure_kernels$(O): $(CSRC)/measure_kernels.hip $(CSRC)/nbx_internal.h $(CSRC)/nbx_ctx.h include/nbody_hip.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/close_hash$(O): $(CSRC)/close_hash.hip $(CSRC)/nbx_internal.h $(CSRC)/device_sort.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the near field of a leaf plan: the pair kernels and their launches (leaf_near.h) ...
$(CSRC)/leaf_pair_kernel$(O): $(CSRC)/leaf_pair_kernel.hip $(CSRC)/leaf_near.h $(CSRC)/leaf_plan.h $(CSRC)/leaf_law.h $(CSRC)/nbx_internal.h include/nbody_hip.h
	$(HIPCC) $(HIPFLAGS) $(LEAF_DEFS) -c $< -o $@

# ... and the host side behind the C ABI: the one-shot call and nbx_leaf_plan_* (with the device planner's kernels, leaf_plan_device.h)
$(CSRC)/leaf_plan_api$(O): $(CSRC)/leaf_plan_api.hip $(CSRC)/leaf_near.h $(CSRC)/leaf_plan.h $(CSRC)/leaf_plan_device.h $(CSRC)/leaf_far.h $(CSRC)/leaf_phi.h $(CSRC)/octree_device.h $(CSRC)/device_sort.h $(CSRC)/device_block.h $(CSRC)/nbx_internal.h $(CSRC)/nbx_ctx.h include/nbody_hip.h
	$(HIPCC) $(HIPFLAGS) $(LEAF_DEFS) -c $< -o $@

# the far field of a leaf plan: moment and far kernels
$(CSRC)/leaf_far_kernel$(O): $(CSRC)/leaf_far_kernel.hip $(CSRC)/leaf_far.h $(CSRC)/leaf_law.h $(CSRC)/nbx_internal.h include/nbody_hip.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the potential of a leaf plan: near, far and reduction kernels (the flags of the other leaf kernels)
$(CSRC)/leaf_phi_kernel$(O): $(CSRC)/leaf_phi_kernel.hip $(CSRC)/leaf_phi.h $(CSRC)/leaf_far.h $(CSRC)/leaf_plan.h $(CSRC)/leaf_law.h $(CSRC)/nbx_internal.h include/nbody_hip.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the octree built on the device.  -ffp-contract=off: a body's cell index must round like the host builder's two-step arithmetic
$(CSRC)/octree_device$(O): $(CSRC)/octree_device.hip $(CSRC)/octree_device.h $(CSRC)/leaf_far.h $(CSRC)/device_sort.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $< -o $@

$(LIB): $(OBJS) $(CSRC)/libnbody_hip.map
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $(OBJS) -ldl -Wl,--version-script=$(CSRC)/libnbody_hip.map

oracle:
	$(MAKE) -C oracle

HOST_SRCS := $(wildcard $(PKG)/host/*.cpp)
HOST_HDRS := $(wildcard $(PKG)/host/*.h) include/nbody_hip.h
nbody_sim: $(LIB) $(HOST_SRCS) $(HOST_HDRS)
	@if [ -n "$(HOST_SRCS)" ]; then \
	  $(CXX) $(CXXFLAGS) $(HOST_SRCS) -o $@ $(LDFLAGS) -L$(PKG) -lnbody_hip -Wl,-rpath,'$$ORIGIN/$(PKG)'; \
	else echo "host harness not built yet"; fi

tools/ubench_valu: tools/ubench_valu.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 $< -o $@

tools/ubench_banks: tools/ubench_banks.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 $< -o $@

clean:
	rm -f $(OBJS) $(LIB) nbody_sim tools/ubench_valu tools/ubench_banks $(CSRC)/*_ab.o $(CSRC)/*_leafab.o $(PKG)/libnbody_hip_ab.so $(PKG)/libnbody_hip_leafab.so
	$(MAKE) -C oracle clean

.PHONY: all lib oracle clean
