# Builds (in-tree, so the .so files travel to the GPU box with gpurun):
#   sycl-ray-tracing_amd/lib/librt_hip.so      product: gfx950 kernel + C ABI (hipcc)
#   sycl-ray-tracing_amd/lib/librt_hostsim.so  CPU build of the same device code (tests only)
#   oracle/liboracle.so                        CPU restatement oracle (tests / cpu_baseline only)
#   build/libm_check                           libm restatement vs glibc checker
#
# Numerics: every object is built with -ffp-contract=off and without
# -ffast-math / -march, because the reference (g++ -O2, baseline x86-64) never
# fuses a*b+c and keeps IEEE division, sqrt, denormals and infinities.
HIPCC ?= /opt/rocm/bin/hipcc
CXX ?= g++
ARCH ?= gfx950
PKG := sycl-ray-tracing_amd
SRC := $(PKG)/csrc
LIB := $(PKG)/lib
OBJ := build/obj

CXXFLAGS := -std=c++17 -O2 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unknown-pragmas
HIPFLAGS := -std=c++17 -O3 -fPIC --offload-arch=$(ARCH) -ffp-contract=off -fno-fast-math \
            -fno-gpu-flush-denormals-to-zero -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function -Wno-unknown-pragmas

HDRS := $(wildcard $(SRC)/*.h) include/rt_hip.h
# the kernel sources' hash, compiled into each library (rt_build_id) so a run reports the build it loaded
SRC_HASH := $(shell cat $(SRC)/* include/*.h 2>/dev/null | sha256sum | cut -c1-12)

all: $(LIB)/librt_hip.so $(LIB)/librt_hostsim.so oracle/liboracle.so build/libm_check build/cdf_check build/plan_check stamp

$(OBJ)/%.host.o: $(SRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJ)
	$(CXX) $(CXXFLAGS) -c $< -o $@

# (the two objects that compile SRC_HASH in as rt_build_id, rt_hostsim.o and rt_backend.o, depend on every file it hashes,
# so a change to a host-only source cannot leave a stale build id in the library)
ALL_SRC := $(wildcard $(SRC)/*) $(wildcard include/*.h)

$(OBJ)/rt_hostsim.o: $(SRC)/rt_hostsim.cpp $(HDRS) $(ALL_SRC)
	@mkdir -p $(OBJ)
	$(CXX) $(CXXFLAGS) -fopenmp -DRT_BUILD_SRC='"$(SRC_HASH)"' -c $< -o $@

# The gfx950 units. rt_render holds the render kernels and nothing else; each of the others is a
# translation unit of its own so that the render kernels' code generation does not depend on it:
#   rt_wave_run  the host loop that launches them (run_wave; no device code)
#   rt_probe     the kernels no render calls (rt_intersect's walk, query benchmark, self-tests)
#   rt_denoise   the post stage (feature pass + rt_denoise's entry points to the à-trous filter)
#   rt_query     the ray queries (rt_query / rt_query_device)
#   rt_display   the display stage (tone-map + 8-bit conversion, linear resolve)
#   rt_noise     a tracked progression's fold and noise estimate
#   rt_adapt     an adaptive progression's selection, gather / scatter and resolves
#   rt_dnv       the absolute noise figure and rt_denoise_var's entry points to the same filter
#                (rt_atrous_hip.h holds the filter's device side once; each of the two units compiles its own mode of it)
#   rt_temporal  temporal accumulation: the previous frame reprojected into the new camera and blended in
#   rt_firefly   firefly rejection: a pixel's luminance limited by a rank of its neighbours'
#   rt_meter     exposure metering: the luminance histogram of a linear frame
#   rt_upscale   guided upscale: a low-resolution frame taken to the output size along the full-size guides
#   rt_gbuffer   the first-hit G-buffer on the render's walks: quads over the search BVH, octets over the octree behind them
#   rt_bloom     bloom: the energy above a threshold spread by a Gaussian pyramid (reduce, expand, composite) and added back
#   rt_dof       depth of field: a gather over each pixel's circle of confusion, from the first-hit distance of the guides
#   rt_motion    motion vectors from the guides and the previous camera, and motion blur: a gather along each 16 x 16 tile's line
# (the host forms of the last seven stage through a DevBuf of Backend each, rt_backend_hip.h, as rt_display does)
# the backend-independent C ABI, in both libraries: contexts, scene, renders, queries, progressions
# (rt_capi_host) and the frame stages with their shared argument rules (rt_capi_stages, rt_stage_args.h)
CAPI_OBJS := $(OBJ)/rt_capi_host.host.o $(OBJ)/rt_capi_stages.host.o
HIP_UNITS := rt_render rt_wave_run rt_probe rt_denoise rt_query rt_display rt_noise rt_adapt rt_dnv rt_temporal rt_firefly \
             rt_meter rt_upscale rt_gbuffer rt_bloom rt_dof rt_motion
$(HIP_UNITS:%=$(OBJ)/%.o): $(OBJ)/%.o: $(SRC)/%.hip $(HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the kernel-free half of the backend: contexts, uploads, the drivers over run_wave, rt_build_id
$(OBJ)/rt_backend.o: $(SRC)/rt_backend.hip $(HDRS) $(ALL_SRC)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRT_BUILD_SRC='"$(SRC_HASH)"' -c $< -o $@

$(LIB)/librt_hip.so: $(HIP_UNITS:%=$(OBJ)/%.o) $(OBJ)/rt_backend.o $(OBJ)/rt_scene.host.o $(OBJ)/rt_imageio.host.o $(CAPI_OBJS)
	@mkdir -p $(LIB)
	$(HIPCC) -shared --offload-arch=$(ARCH) -fPIC $^ -o $@

# BUILD_COMMIT: "<commit>[-dirty] src=<hash of the kernel sources>", rewritten by every `make`
# (the sources' hash names the build whatever was committed since; bench.py reports it)
stamp: $(LIB)/librt_hip.so
	@c=$$(git rev-parse --short HEAD 2>/dev/null || echo unknown); \
	  git diff --quiet HEAD -- $(SRC) include 2>/dev/null || c="$$c-dirty"; \
	  h=$$(cat $(SRC)/* include/*.h | sha256sum | cut -c1-12); echo "$$c src=$$h" > BUILD_COMMIT

$(LIB)/librt_hostsim.so: $(OBJ)/rt_hostsim.o $(OBJ)/rt_scene.host.o $(OBJ)/rt_imageio.host.o $(CAPI_OBJS)
	@mkdir -p $(LIB)
	$(CXX) -shared -fopenmp $^ -o $@

oracle/liboracle.so: oracle/cpu_oracle.cpp
	$(MAKE) -C oracle liboracle.so

build/libm_check: tests/native/libm_check.cpp $(SRC)/rt_libm.h $(SRC)/rt_fp.h $(SRC)/rt_digest.h
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -fopenmp -ffp-contract=off -I$(SRC) $< -o $@ -lm

build/cdf_check: tests/native/cdf_check.cpp $(OBJ)/rt_scene.host.o $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -I$(SRC) $< $(OBJ)/rt_scene.host.o -o $@

# the wavefront plan (rt_plan.h wave_plan) against a table worked out from the expressions it replaced
build/plan_check: tests/native/plan_check.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -I$(SRC) $< -o $@

# CPU replay of logged rays over search-BVH variants (tools/probe/walk_probe.cpp; study tool)
build/walk_probe: tools/probe/walk_probe.cpp $(OBJ)/rt_scene.host.o $(HDRS)
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -fopenmp -ffp-contract=off -I$(SRC) $< $(OBJ)/rt_scene.host.o -o $@ -lpthread

# CPU trip counts of stackless occlusion walks vs the short stack (tools/probe/stackless_probe.cpp; study tool)
build/stackless_probe: tools/probe/stackless_probe.cpp $(OBJ)/rt_scene.host.o $(HDRS)
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -fopenmp -ffp-contract=off -I$(SRC) $< $(OBJ)/rt_scene.host.o -o $@ -lpthread

# A host-only change leaves the kernels alone: make device-diff PARENT=<checkout of the commit before it>
# compiles the device side of every unit that has one (rt_wave_run and rt_backend have none) from both
# trees and fails on any differing assembly line besides the one naming the unit's __hip_cuid_ symbol.
# A unit the parent does not have (a new translation unit) is left out of the comparison and named.
DEV_UNITS := $(foreach u,$(filter-out rt_wave_run,$(HIP_UNITS)),$(if $(wildcard $(PARENT)/$(SRC)/$(u).hip),$(u)))
NEW_UNITS := $(filter-out rt_wave_run $(DEV_UNITS),$(HIP_UNITS))
build/devasm/%.s: $(SRC)/%.hip $(HDRS)
	@mkdir -p build/devasm
	$(HIPCC) $(HIPFLAGS) --cuda-device-only -S $< -o $@
build/devasm/%.parent.s: $(PARENT)/$(SRC)/%.hip
	@mkdir -p build/devasm
	$(HIPCC) $(HIPFLAGS) --cuda-device-only -S $< -o $@
device-diff: $(DEV_UNITS:%=build/devasm/%.s) $(DEV_UNITS:%=build/devasm/%.parent.s)
	@for u in $(DEV_UNITS); do \
	  n=$$(diff build/devasm/$$u.parent.s build/devasm/$$u.s | grep '^[<>]' | grep -vc __hip_cuid_); \
	  echo "$$u: $$(grep -c . build/devasm/$$u.s) lines, $$n differ besides __hip_cuid_"; [ $$n -eq 0 ] || exit 1; done
	@for u in $(NEW_UNITS); do echo "$$u: not in the parent"; done
.PHONY: device-diff

# the reference build (container only; needs /root/reference)
ref:
	$(MAKE) -C oracle/ref OPT=-O2

clean:
	rm -rf $(OBJ) $(LIB) build/libm_check oracle/liboracle.so

.PHONY: all ref clean stamp

# experiment builds: make variant V=name DEFS="-DRT_TAIL_OCC=2" -> lib/librt_hip_name.so (RT_HIP_LIB=...)
variant: $(OBJ)/rt_scene.host.o $(OBJ)/rt_imageio.host.o $(CAPI_OBJS)
	@mkdir -p $(LIB)
	for u in $(HIP_UNITS); do $(HIPCC) $(HIPFLAGS) $(DEFS) -c $(SRC)/$$u.hip -o $(OBJ)/$${u}_$(V).o || exit 1; done
	$(HIPCC) $(HIPFLAGS) $(DEFS) -DRT_BUILD_SRC='"$(SRC_HASH)"' -DRT_BUILD_DEFS='"$(DEFS)"' -c $(SRC)/rt_backend.hip -o $(OBJ)/rt_backend_$(V).o
	$(HIPCC) -shared --offload-arch=$(ARCH) -fPIC $(HIP_UNITS:%=$(OBJ)/%_$(V).o) $(OBJ)/rt_backend_$(V).o $^ -o $(LIB)/librt_hip_$(V).so

# the same for the hostsim build: make hostsim-variant V=name DEFS="-DRT_SLABS=0" ->
# lib/librt_hostsim_name.so (RT_HOSTSIM_LIB=...; study probes such as tools/far_probe.py)
hostsim-variant: $(OBJ)/rt_imageio.host.o
	@mkdir -p $(LIB)
	$(CXX) $(CXXFLAGS) -fopenmp $(DEFS) -DRT_BUILD_SRC='"$(SRC_HASH)"' -DRT_BUILD_DEFS='"$(DEFS)"' -c $(SRC)/rt_hostsim.cpp -o $(OBJ)/rt_hostsim_$(V).o
	$(CXX) $(CXXFLAGS) $(DEFS) -c $(SRC)/rt_scene.cpp -o $(OBJ)/rt_scene_$(V).o
	$(CXX) $(CXXFLAGS) $(DEFS) -c $(SRC)/rt_capi_host.cpp -o $(OBJ)/rt_capi_host_$(V).o
	$(CXX) $(CXXFLAGS) $(DEFS) -c $(SRC)/rt_capi_stages.cpp -o $(OBJ)/rt_capi_stages_$(V).o
	$(CXX) -shared -fopenmp $(OBJ)/rt_hostsim_$(V).o $(OBJ)/rt_scene_$(V).o $(OBJ)/rt_capi_host_$(V).o $(OBJ)/rt_capi_stages_$(V).o $(OBJ)/rt_imageio.host.o -o $(LIB)/librt_hostsim_$(V).so

# C++ drop-in checks (container only): include/render_kernel_hip.h against the reference's headers and objects
# (oracle/_ref, `make ref`). Every program in SHIM_PROGS is tests/native/<p>.cpp over tests/native/shim_common.h,
# linked to the hostsim build of the C ABI (build/<p>) and to the product library (build/<p>_hip: built here by
# `make shims-hip`, run on the GPU box, which has no reference tree; the binary carries what it needs).
# tests/test_shims.py holds the invocations and runs both forms; each program's head says what it checks.
SHIM_PROGS := shim_test $(addsuffix _shim_test,denoise query progress display noise adaptive dnv temporal firefly meter upscale gbuffer bloom dof motion)
shims: $(SHIM_PROGS:%=build/%)
shims-hip: $(SHIM_PROGS:%=build/%_hip)
.PHONY: shims shims-hip
REFDIR ?= /root/reference
REFOBJ := oracle/_ref/objO2
REFOBJS := $(REFOBJ)/bvh.o $(REFOBJ)/flattened_bvh.o $(REFOBJ)/triangle.o $(REFOBJ)/vec.o $(REFOBJ)/color.o \
  $(REFOBJ)/mat.o $(REFOBJ)/camera.o $(REFOBJ)/ray.o $(REFOBJ)/utils.o
build/%_test: tests/native/%_test.cpp tests/native/shim_common.h include/render_kernel_hip.h include/rt_hip.h $(LIB)/librt_hostsim.so
	@mkdir -p build
	$(CXX) -std=gnu++20 -O2 -fopenmp -Iinclude -I$(REFDIR)/include -I$(REFDIR)/rapidobj -I$(REFDIR) $< \
	  $(REFOBJS) -Wl,--gc-sections \
	  -L$(LIB) -lrt_hostsim -Wl,-rpath,'$$ORIGIN/../$(LIB)' -o $@

build/%_test_hip: tests/native/%_test.cpp tests/native/shim_common.h include/render_kernel_hip.h include/rt_hip.h $(LIB)/librt_hip.so
	@mkdir -p build
	$(CXX) -std=gnu++20 -O2 -fopenmp -Iinclude -I$(REFDIR)/include -I$(REFDIR)/rapidobj -I$(REFDIR) $< \
	  $(REFOBJS) -Wl,--gc-sections \
	  -L$(LIB) -lrt_hip -Wl,-rpath,'$$ORIGIN/../$(LIB)' -o $@

# Host sanitizers: the hostsim build of the render path + the CPU oracle +
# tests/native/sanitize_driver.cpp in one executable per sanitizer.
#   make sanitize  -> build/sanitize_asan (ASan + UBSan) and build/sanitize_tsan (TSan), run
#                     both; logs in profiles/r04_sanitize_{asan,tsan}.log
# TSan: libgomp is not TSan-instrumented (its barriers would be reported as races), so the
# TSan run uses one OpenMP thread per region; what it checks is the std::thread layer of the
# multi-device driver (rt_for_devices, rt_render_variants) and the shared context state.
SAN_SRCS := $(SRC)/rt_hostsim.cpp $(SRC)/rt_scene.cpp $(SRC)/rt_imageio.cpp $(SRC)/rt_capi_host.cpp $(SRC)/rt_capi_stages.cpp
SAN_NUM := -ffp-contract=off -fno-fast-math -fno-omit-frame-pointer -g -O1 -fopenmp
ASAN := -fsanitize=address,undefined -fno-sanitize-recover=undefined
TSAN := -fsanitize=thread

build/san_%/driver: tests/native/sanitize_driver.cpp oracle/cpu_oracle.cpp $(SAN_SRCS) $(HDRS)
	@mkdir -p build/san_$*
	for f in $(SAN_SRCS); do $(CXX) -std=c++17 $(SAN_NUM) $($(shell echo $* | tr a-z A-Z)) -c $$f -o build/san_$*/$$(basename $$f .cpp).o || exit 1; done
	$(CXX) -std=gnu++20 $(SAN_NUM) $($(shell echo $* | tr a-z A-Z)) -c oracle/cpu_oracle.cpp -o build/san_$*/cpu_oracle.o
	$(CXX) -std=c++17 $(SAN_NUM) $($(shell echo $* | tr a-z A-Z)) tests/native/sanitize_driver.cpp build/san_$*/*.o -o $@

sanitize: build/san_asan/driver build/san_tsan/driver
	ASAN_OPTIONS=halt_on_error=1:detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
	  OMP_NUM_THREADS=4 build/san_asan/driver scenes asan 2>&1 | tee profiles/r04_sanitize_asan.log
	TSAN_OPTIONS=halt_on_error=1:second_deadlock_stack=1 OMP_NUM_THREADS=1 \
	  build/san_tsan/driver scenes tsan 2>&1 | tee profiles/r04_sanitize_tsan.log

.PHONY: sanitize

# A drop-in's program under ASan + UBSan: make sanitize-X builds tests/native/X_shim_test.cpp with the hostsim
# sources of build/san_asan in one stand-alone executable, a host program with its own main (container only: the
# reference's objects), and runs it on the small Cornell scene under the flat sky: at 33 x 21, but for the layouts
# that differ and for adaptive, whose every-tile-takes-every-pass check does not hold at that size under that sky.
SAN_ARGS = - 33 21 3
sanitize-adaptive: SAN_ARGS = - 40 30 4
sanitize-denoise: SAN_ARGS = - 33 21 2 3
sanitize-query: SAN_ARGS = 33 21
sanitize-display: SAN_ARGS = - 33 21 3 build/san_asan/display.hdr
build/san_asan/%_shim_test: tests/native/%_shim_test.cpp tests/native/shim_common.h include/render_kernel_hip.h build/san_asan/driver
	$(CXX) -std=gnu++20 $(SAN_NUM) $(ASAN) -Iinclude -I$(REFDIR)/include -I$(REFDIR)/rapidobj -I$(REFDIR) $< \
	  $(SAN_SRCS:$(SRC)/%.cpp=build/san_asan/%.o) $(REFOBJS) -Wl,--gc-sections -o $@
.PRECIOUS: build/san_asan/%_shim_test
sanitize-%: build/san_asan/%_shim_test
	ASAN_OPTIONS=halt_on_error=1:detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 OMP_NUM_THREADS=4 \
	  $< scenes/cornell_pbr.obj $(SAN_ARGS)
