# Builds libxlbhip.so (HIP, gfx950) and the C oracle.  No cmake: hipcc/gcc directly.
HIPCC     ?= /opt/rocm/bin/hipcc
ARCH      ?= gfx950
CSRC      := xlb_amd/csrc
OBJDIR    ?= build/obj
LIB       ?= xlb_amd/lib/libxlbhip.so
# -ffp-contract=off: fp32/fp64 results are bit-identical to the oracle's operation order
EXTRA     ?=
HIPFLAGS  := $(EXTRA) --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -fPIC -Wall -Wno-unused-function -Iinclude
SRCS      := api.hip masker.hip stepper.hip ibm.hip stats.hip comm.cpp step_d2q9_bgk.hip step_d2q9_kbc.hip step_d3q19_bgk.hip step_d3q27_bgk.hip step_d3q27_kbc.hip step_d3q27_kbc_fast.hip \
             step_d2q9_ext.hip step_d3q19_ext.hip step_d3q27_ext.hip step_d2q9_reg.hip step_d3q19_reg.hip step_d3q27_reg.hip step2_d3q19.hip step2_d3q19_strips.hip step2_d3q27.hip yardstick.hip \
             scalar.hip scalar_d2q9.hip scalar_d3q19.hip scalar_d3q27.hip \
             adjoint.hip adjoint_d2q9.hip adjoint_d3q19.hip adjoint_d3q27.hip \
             multiphase.hip multiphase_d2q9.hip multiphase_d3q19.hip multiphase_d3q27.hip \
             multicomponent.hip multicomponent_d2q9.hip multicomponent_d3q19.hip multicomponent_d3q27.hip \
             porous.hip porous_d2q9.hip porous_d3q19.hip porous_d3q27.hip
OBJS      := $(addprefix $(OBJDIR)/,$(addsuffix .o,$(basename $(SRCS))))
HDRS      := $(wildcard $(CSRC)/*.hpp) include/xlbhip.h

all: $(LIB) oracle

# the two-step kernel packs its fp32 pairs by hand (cell.hpp: bgk_packed_pairs); hipcc's SLP vectorizer on top of that
# scrambles the sequential moment sums into packed adds + moves (measured +2 % kernel time)
$(OBJDIR)/step2_d3q19.o $(OBJDIR)/step2_d3q19_strips.o $(OBJDIR)/step2_d3q27.o: HIPFLAGS += -fno-slp-vectorize

# the regularised units (tests/test_regularized_build.py compiles with the same flags and requires that no FP32FP32 kernel reserves
# a private segment): the loop over the cells of a thread must unroll in the extended-boundary variants too — at VEC = 4 its body exceeds
# the default pragma-unroll threshold, and f[4][q] would live in scratch —, and with the spiller placing spills for size the forced
# extended-boundary kernels keep no dead stack slot for a kernel-argument tuple that is re-loaded instead of spilled (36 B otherwise)
REGFLAGS  := -mllvm -pragma-unroll-threshold=200000 -mllvm -split-spill-mode=size
$(OBJDIR)/step_d2q9_reg.o $(OBJDIR)/step_d3q19_reg.o $(OBJDIR)/step_d3q27_reg.o: HIPFLAGS += $(REGFLAGS)

# the sample kernel's moment sums are sequential by contract; packed adds only cost it moves and registers
$(OBJDIR)/stats.o: HIPFLAGS += -fno-slp-vectorize

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p xlb_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -ldl

oracle: oracle/liblbmref.so

oracle/liblbmref.so: oracle/lbm_ref.c oracle/lbm_ref_body.inc
	gcc -O2 -fPIC -shared -fopenmp -ffp-contract=off -fno-fast-math -o $@ $< -lm

# Host-side AddressSanitizer / UBSan build (tools/asan_host.py): only the translation units with host logic (api, masker, stepper,
# comm) are instrumented, for the host compilation only; the kernel objects are the ordinary ones.  Their device passes are compiled
# again (minutes each; run with -j to overlap them).
ASANDIR := build/asan
ASANFLAGS := --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -fPIC -Iinclude -fsanitize=address,undefined -fno-gpu-sanitize -fno-omit-frame-pointer
ASANSRCS := api.hip masker.hip stepper.hip comm.cpp
ASANOBJS := $(addprefix $(ASANDIR)/,$(addsuffix .o,$(basename $(ASANSRCS))))
HOSTOBJS := $(addprefix $(OBJDIR)/,$(addsuffix .o,$(basename $(ASANSRCS))))

$(ASANDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(ASANDIR)
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

$(ASANDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(ASANDIR)
	$(HIPCC) $(ASANFLAGS) -x hip -c $< -o $@

asan: $(LIB) $(ASANOBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -fsanitize=address,undefined -o $(ASANDIR)/libxlbhip_asan.so $(ASANOBJS) $(filter-out $(HOSTOBJS),$(OBJS)) -ldl

clean:
	rm -rf build xlb_amd/lib/libxlbhip.so oracle/liblbmref.so

.PHONY: all oracle clean asan
