# Build of the three native pieces (no cmake needed):
#   hijiki_amd/lib/libhijiki_host.so  — C++ host: Scene / compile / BVH / block generator   (g++)
#   hijiki_amd/lib/libhijiki_hip.so   — HIP kernels + C ABI for gfx950                      (hipcc)
#   oracle/_build/libhj_oracle.so     — CPU restatement, test infrastructure only           (gcc)
ROCM ?= /opt/rocm
HIPCC ?= $(ROCM)/bin/hipcc
CXX ?= g++
CC ?= gcc
ARCH ?= gfx950

FP_STRICT = -ffp-contract=off -fno-fast-math
HOST_SRC = hijiki_amd/csrc/host/scene.cpp hijiki_amd/csrc/host/tree_opt.cpp hijiki_amd/csrc/host/synth.cpp hijiki_amd/csrc/host/blockgen.cpp \
           hijiki_amd/csrc/host/obj_loader.cpp hijiki_amd/csrc/host/image_io.cpp hijiki_amd/csrc/host/host_api.cpp
HOST_HDR = hijiki_amd/csrc/host/scene.hpp hijiki_amd/csrc/host/blockgen.hpp include/hijiki_hip.h include/hijiki_host.h
# libhijiki_hip.so: its translation units (hijiki_amd/csrc/api/hj_internal.h lists them); render.hip, scene_relayout.hip,
# scene_update.hip, lbvh_build.hip, tree_vote.hip, texture.hip, environment.hip, step_probe.hip, ray_query.hip, path_query.hip, path_adaptive.hip, gather_query.hip, probe_volume.hip, probe_visibility.hip, probe_update.hip, probe_place.hip, closest_query.hip, multi_hit.hip, aov.hip, follow.hip, probe_lit.hip, direct_lit.hip, denoise.hip, denoise_temporal.hip, motion.hip, motion_follow.hip, gather_adaptive.hip, lightmap_filter.hip, lightmap.hip and tree_reinsert.hip hold device code.  The register / scratch / LDS report of the path kernels: hijiki_amd/lib/resource_usage.txt
# (render.hip's kernels, then behind the line '# gather_query.hip' the gather query's, behind '# probe_volume.hip' the probe volumes', behind '# gather_adaptive.hip' the adaptive gather's, behind '# lightmap_filter.hip' the light-map filter's, then behind '# lightmap.hip' the light-map kernels': report_unit below).
# HIP_HDR: every unit is rebuilt when a header changes; kernels/*.h by wildcard, so a new kernel header (hj_compact.h, hj_lightmap_filter.h, hj_probe_vis.h, hj_probe_update.h, hj_probe_place.h, hj_closest.h, hj_multihit.h, hj_aov.h, hj_denoise.h, hj_denoise_temporal.h, hj_motion.h, hj_follow.h, hj_motion_follow.h, hj_chain.h, hj_walk_segment.h, hj_probe_lit.h, hj_direct_lit.h) needs no line here.  probe_visibility.hip, probe_update.hip, probe_place.hip, closest_query.hip, multi_hit.hip, aov.hip, follow.hip, probe_lit.hip, direct_lit.hip, denoise.hip, denoise_temporal.hip, motion.hip and motion_follow.hip have no section in the report: their own tests compile them for one.
HIP_UNITS = context scene_upload scene_relayout scene_update render render_calls comm lbvh_build tree_vote texture environment step_probe ray_query path_query path_adaptive gather_query probe_volume probe_visibility probe_update probe_place closest_query multi_hit aov follow probe_lit direct_lit denoise denoise_temporal motion motion_follow gather_adaptive lightmap_filter lightmap tree_reinsert
HIP_OBJ = $(HIP_UNITS:%=build/obj/%.o) build/obj/blockgen.o build/obj/light_grid.o
HIP_HDR = $(wildcard hijiki_amd/csrc/kernels/*.h) hijiki_amd/csrc/api/hj_internal.h hijiki_amd/csrc/api/hj_tuning.h hijiki_amd/csrc/api/light_grid.hpp hijiki_amd/csrc/api/scene_relayout.hpp hijiki_amd/csrc/api/refit_pass.hpp hijiki_amd/csrc/api/guard_box.hpp hijiki_amd/csrc/api/tree_vote.hpp hijiki_amd/csrc/api/tree_reinsert.h hijiki_amd/csrc/api/query_round.h hijiki_amd/csrc/api/query_round_loop.h hijiki_amd/csrc/api/chain_rounds.h hijiki_amd/csrc/api/probe_lit_volume.h hijiki_amd/csrc/api/adaptive_stop.h include/hijiki_hip.h hijiki_amd/csrc/host/blockgen.hpp
HIP_FLAGS = --offload-arch=$(ARCH) -std=c++17 -O3 -fPIC $(FP_STRICT) -fhip-fp32-correctly-rounded-divide-sqrt -fvisibility=hidden \
            -Wall -Wno-unused-function $(HIP_EXTRA)

all: host hip oracle cli
host: hijiki_amd/lib/libhijiki_host.so
hip: hijiki_amd/lib/libhijiki_hip.so
oracle: oracle/_build/libhj_oracle.so
cli: hijiki_amd/bin/hijiki-hip

hijiki_amd/lib/libhijiki_host.so: $(HOST_SRC) $(HOST_HDR)
	@mkdir -p hijiki_amd/lib
	$(CXX) -std=c++17 -O2 -g0 -fPIC -shared -Wall -Wextra $(FP_STRICT) -fvisibility=hidden \
	  -DHJ_BUILDING -pthread -o $@ $(HOST_SRC)

# $(call report_unit,UNIT,PREDECESSOR): UNIT.o compiled with the compiler's resource report, which replaces resource_usage.txt from the
# line '# UNIT.hip' on.  It stands behind PREDECESSOR.o, whose rule cuts the report from its own line on, so a rebuild of a unit
# rebuilds the sections behind it and a rebuild of the last unit alone replaces its section.  No predecessor: the unit starts the
# report, without a marker line.
define report_unit
build/obj/$(1).o: hijiki_amd/csrc/api/$(1).hip $$(HIP_HDR) $(2:%=build/obj/%.o)
	@mkdir -p build/obj hijiki_amd/lib
	$$(HIPCC) $$(HIP_FLAGS) -c $$< -o $$@ -Rpass-analysis=kernel-resource-usage 2> build/obj/$(1).report \
	  || (cat build/obj/$(1).report; false)
	@($(if $(2),sed '/^# $(1).hip$$$$/$(comma)$$$$d' hijiki_amd/lib/resource_usage.txt; echo '# $(1).hip';) cat build/obj/$(1).report) \
	  > build/obj/resource_usage.tmp && mv build/obj/resource_usage.tmp hijiki_amd/lib/resource_usage.txt
endef
comma := ,
$(eval $(call report_unit,render,))
$(eval $(call report_unit,gather_query,render))
$(eval $(call report_unit,probe_volume,gather_query))
$(eval $(call report_unit,gather_adaptive,probe_volume))
$(eval $(call report_unit,lightmap_filter,gather_adaptive))
$(eval $(call report_unit,lightmap,lightmap_filter))

build/obj/%.o: hijiki_amd/csrc/api/%.hip $(HIP_HDR)
	@mkdir -p build/obj
	$(HIPCC) $(HIP_FLAGS) -c $< -o $@

build/obj/light_grid.o: hijiki_amd/csrc/api/light_grid.cpp hijiki_amd/csrc/api/light_grid.hpp hijiki_amd/csrc/api/hj_tuning.h include/hijiki_hip.h
	@mkdir -p build/obj
	$(CXX) -std=c++17 -O2 -fPIC -pthread -Wall -Wextra $(FP_STRICT) -fvisibility=hidden -c $< -o $@

build/obj/blockgen.o: hijiki_amd/csrc/host/blockgen.cpp hijiki_amd/csrc/host/blockgen.hpp include/hijiki_hip.h
	@mkdir -p build/obj
	$(CXX) -std=c++17 -O2 -fPIC $(FP_STRICT) -fvisibility=hidden -c $< -o $@

hijiki_amd/lib/libhijiki_hip.so: $(HIP_OBJ)
	@mkdir -p hijiki_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(HIP_OBJ) -ldl -o $@
	@strings $@ | grep -q 'amdgcn-amd-amdhsa--$(ARCH)' || (echo 'ERROR: no $(ARCH) code object in $@'; rm -f $@; false)
	@python3 tools/build_stamp.py

oracle/_build/libhj_oracle.so: oracle/hj_oracle.c include/hijiki_hip.h
	@mkdir -p oracle/_build
	$(CC) -std=c11 -O2 -fPIC -shared -Wall -Wextra $(FP_STRICT) -mfma -fvisibility=hidden -o $@ oracle/hj_oracle.c -lm -lpthread

CLI_SRC = hijiki_amd/csrc/cli/main.cpp hijiki_amd/csrc/host/scene.cpp hijiki_amd/csrc/host/tree_opt.cpp hijiki_amd/csrc/host/synth.cpp \
          hijiki_amd/csrc/host/obj_loader.cpp hijiki_amd/csrc/host/image_io.cpp
hijiki_amd/bin/hijiki-hip: $(CLI_SRC) $(HOST_HDR) hijiki_amd/lib/libhijiki_hip.so
	@mkdir -p hijiki_amd/bin
	$(CXX) -std=c++17 -O2 -pthread -Wall -Wextra $(FP_STRICT) -o $@ $(CLI_SRC) -Lhijiki_amd/lib -lhijiki_hip \
	  -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,$(ROCM)/lib -L$(ROCM)/lib -lamdhip64

clean:
	rm -rf hijiki_amd/lib hijiki_amd/bin oracle/_build build/obj

.PHONY: all host hip oracle cli clean
