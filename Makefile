# Builds the MI355X engine: hand-written HIP kernels + C-ABI -> icp_amd/libicp_amd.so (gfx950 only).
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
# -ffp-contract=off: the canonical arithmetic has no fused multiply-add
# EXTRA: -D switches of an A/B build; BUILD: its object directory — e.g. `make BUILD=build/ol32 LIB=build/libicp_ol32.so EXTRA=-DICP_OL_BOXED_MIN=32 build/libicp_ol32.so`
EXTRA    ?=
BUILD    ?= build
HIPFLAGS ?= $(EXTRA) -O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=$(ARCH) -ffp-contract=off -fno-fast-math -Wall -Wno-unused-result -pthread -mllvm -amdgpu-kernarg-preload-count=14
SRC      := icp_amd/csrc/icp_kernels.hip icp_amd/csrc/icp_search_dense.hip icp_amd/csrc/icp_search_rej.hip icp_amd/csrc/icp_trim.hip icp_amd/csrc/icp_p2pl.hip icp_amd/csrc/icp_robust.hip icp_amd/csrc/icp_gicp.hip icp_amd/csrc/icp_symmetric.hip icp_amd/csrc/icp_unique.hip icp_amd/csrc/icp_median.hip icp_amd/csrc/icp_adaptive_trim.hip icp_amd/csrc/icp_pair_filter.hip icp_amd/csrc/icp_reciprocal.hip icp_amd/csrc/icp_projective.hip icp_amd/csrc/icp_quality.hip icp_amd/csrc/icp_pairs.hip icp_amd/csrc/icp_build.hip icp_amd/csrc/icp_capi.hip icp_amd/csrc/icp_run.hip icp_amd/csrc/icp_track.hip icp_amd/csrc/icp_reduce_scan.hip icp_amd/csrc/icp_standalone.hip icp_amd/csrc/icp_synth.cpp icp_amd/csrc/icp_batch.cpp icp_amd/csrc/icp_pyramid.hip icp_amd/csrc/icp_rgbd.hip icp_amd/csrc/icp_tsdf.hip icp_amd/csrc/icp_tsdf_surface.hip icp_amd/csrc/icp_tsdf_register.hip icp_amd/csrc/icp_tsdf_shift.hip
HDR      := icp_amd/csrc/icp_device.h icp_amd/csrc/icp_kernels.h icp_amd/csrc/icp_rbc_set.h icp_amd/csrc/icp_search.h icp_amd/csrc/icp_search_select.h icp_amd/csrc/icp_host.h icp_amd/csrc/icp_cguard.h icp_amd/csrc/icp_trim_apply.h icp_amd/csrc/icp_select.h icp_amd/csrc/icp_plane_moments.h icp_amd/csrc/icp_pair_rule.h icp_amd/csrc/icp_normal_rule.h icp_amd/csrc/icp_rgbd.h icp_amd/csrc/icp_tsdf.h icp_amd/csrc/icp_ldlt.h include/icp_amd.h
LIB      ?= icp_amd/libicp_amd.so
OBJ      := $(patsubst icp_amd/csrc/%,$(BUILD)/%.o,$(SRC))

all: $(LIB) oracle

# one object per source (the two k_search translation units are the long ones: `make` builds them side by side)
$(BUILD)/%.o: icp_amd/csrc/% $(HDR)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(LIB): $(OBJ)
	$(HIPCC) -fPIC --offload-arch=$(ARCH) -pthread -shared -o $@ $(OBJ)

oracle:
	$(MAKE) -C oracle

facade_test: $(LIB) tests/cpp/facade_test.cpp include/ICP/algorithms.hpp
	g++ -O2 -std=c++17 -Iinclude -o tests/cpp/facade_test tests/cpp/facade_test.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../../icp_amd'

pyramid_facade_test: $(LIB) tests/cpp/pyramid_facade_test.cpp include/ICP/algorithms.hpp
	g++ -O2 -std=c++17 -Wall -Iinclude -o tests/cpp/pyramid_facade_test tests/cpp/pyramid_facade_test.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../../icp_amd'

pairs_facade_test: $(LIB) tests/cpp/pairs_facade_test.cpp include/ICP/algorithms.hpp
	g++ -O2 -std=c++17 -Wall -Iinclude -o tests/cpp/pairs_facade_test tests/cpp/pairs_facade_test.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../../icp_amd'

rgbd_facade_test: $(LIB) tests/cpp/rgbd_facade_test.cpp include/ICP/algorithms.hpp
	g++ -O2 -std=c++17 -Wall -ffp-contract=off -Iinclude -o tests/cpp/rgbd_facade_test tests/cpp/rgbd_facade_test.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../../icp_amd'

tsdf_facade_test: $(LIB) tests/cpp/tsdf_facade_test.cpp include/ICP/algorithms.hpp
	g++ -O2 -std=c++17 -Wall -ffp-contract=off -Iinclude -o tests/cpp/tsdf_facade_test tests/cpp/tsdf_facade_test.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../../icp_amd'

tsdf_surface_facade_test: $(LIB) tests/cpp/tsdf_surface_facade_test.cpp include/ICP/algorithms.hpp
	g++ -O2 -std=c++17 -Wall -ffp-contract=off -Iinclude -o tests/cpp/tsdf_surface_facade_test tests/cpp/tsdf_surface_facade_test.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../../icp_amd'

tsdf_mesh_facade_test: $(LIB) tests/cpp/tsdf_mesh_facade_test.cpp include/ICP/algorithms.hpp
	g++ -O2 -std=c++17 -Wall -ffp-contract=off -Iinclude -o tests/cpp/tsdf_mesh_facade_test tests/cpp/tsdf_mesh_facade_test.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../../icp_amd'

tsdf_register_facade_test: $(LIB) tests/cpp/tsdf_register_facade_test.cpp include/ICP/algorithms.hpp
	g++ -O2 -std=c++17 -Wall -ffp-contract=off -Iinclude -o tests/cpp/tsdf_register_facade_test tests/cpp/tsdf_register_facade_test.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../../icp_amd'

tsdf_shift_facade_test: $(LIB) tests/cpp/tsdf_shift_facade_test.cpp include/ICP/algorithms.hpp
	g++ -O2 -std=c++17 -Wall -ffp-contract=off -Iinclude -o tests/cpp/tsdf_shift_facade_test tests/cpp/tsdf_shift_facade_test.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../../icp_amd'

icpreg_test: $(LIB) tests/cpp/icpreg_test.cpp include/ocl_icp_reg.hpp include/ocl_icp_sbs.hpp include/ICP/algorithms.hpp
	g++ -O2 -std=c++17 -Iinclude -o tests/cpp/icpreg_test tests/cpp/icpreg_test.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../../icp_amd'

# the reference's two example programs as command-line programs (examples/registration.cpp, examples/step_by_step.cpp)
examples: $(LIB) examples/registration.cpp examples/step_by_step.cpp include/ocl_icp_reg.hpp include/ocl_icp_sbs.hpp include/ICP/algorithms.hpp
	g++ -O2 -std=c++17 -Wall -Iinclude -o examples/registration examples/registration.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../icp_amd'
	g++ -O2 -std=c++17 -Wall -Iinclude -o examples/step_by_step examples/step_by_step.cpp -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../icp_amd'

# measurement: SIMD cycles per wave64 vector instruction by class (bench.py prices SQ_INSTS_VALU with the result: profiles/valu_issue.json)
valu_issue_probe: tests/cpp/valu_issue_probe.hip
	$(HIPCC) --offload-arch=$(ARCH) -O2 -o tests/cpp/valu_issue_probe tests/cpp/valu_issue_probe.hip

capi_example: $(LIB) tests/cpp/capi_example.c include/icp_amd.h
	gcc -O2 -std=c99 -Wall -Iinclude -o tests/cpp/capi_example tests/cpp/capi_example.c -Licp_amd -licp_amd -Wl,-rpath,'$$ORIGIN/../../icp_amd'

# Host-side sanitizer build (GPU ASan is not available on this pool): the CPU oracle, the synthetic
# generator and a driver over every oracle entry point at small / ragged / degenerate sizes, AddressSanitizer + UBSan.
# No OpenMP (its runtime is not instrumented).  `make asan` builds and runs it; tests/test_oracle_golden.py does too.
ASANFLAGS := -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -ffp-contract=off -fno-fast-math -mfma -Wall -Wno-unknown-pragmas
tests/cpp/asan_host: tests/cpp/asan_host.cpp oracle/icp_oracle.c oracle/icp_oracle.h icp_amd/csrc/icp_synth.cpp include/icp_amd.h
	gcc $(ASANFLAGS) -std=gnu11 -c oracle/icp_oracle.c -o tests/cpp/asan_oracle.o
	g++ $(ASANFLAGS) -std=c++17 -o $@ tests/cpp/asan_host.cpp icp_amd/csrc/icp_synth.cpp tests/cpp/asan_oracle.o -lm

# the selection of the dense search kernel against its rule as a table (host only: icp_search_select.h); tests/test_search_select_cpu.py runs it
tests/cpp/search_select_test: tests/cpp/search_select_test.cpp icp_amd/csrc/icp_search_select.h
	g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tests/cpp/search_select_test.cpp

search_select_test: tests/cpp/search_select_test
	tests/cpp/search_select_test

# the table of an RBC set against its sizes written out by hand (host only: icp_rbc_set.h, which needs HIP's vector types — the host half
# of a hipcc compilation, sanitized); tests/test_rbc_set_cpu.py runs it
tests/cpp/rbc_set_test: tests/cpp/rbc_set_test.cpp icp_amd/csrc/icp_rbc_set.h icp_amd/csrc/icp_kernels.h icp_amd/csrc/icp_device.h icp_amd/csrc/icp_search_select.h
	$(HIPCC) --cuda-host-only -O1 -g -std=c++17 -Wall -Werror -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -o $@ tests/cpp/rbc_set_test.cpp

rbc_set_test: tests/cpp/rbc_set_test
	tests/cpp/rbc_set_test

# the word areas behind the moments against offsets written out by hand (host only: icp_kernels.h, built like rbc_set_test);
# tests/test_mom_layout_cpu.py runs it
tests/cpp/mom_layout_test: tests/cpp/mom_layout_test.cpp icp_amd/csrc/icp_kernels.h icp_amd/csrc/icp_device.h icp_amd/csrc/icp_search_select.h
	$(HIPCC) --cuda-host-only -O1 -g -std=c++17 -Wall -Werror -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -o $@ tests/cpp/mom_layout_test.cpp

mom_layout_test: tests/cpp/mom_layout_test
	tests/cpp/mom_layout_test

asan: tests/cpp/asan_host
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 UBSAN_OPTIONS=print_stacktrace=1 tests/cpp/asan_host

clean:
	rm -rf build; rm -f $(LIB) examples/registration examples/step_by_step tests/cpp/facade_test tests/cpp/pyramid_facade_test tests/cpp/pairs_facade_test tests/cpp/rgbd_facade_test tests/cpp/tsdf_facade_test tests/cpp/tsdf_surface_facade_test tests/cpp/tsdf_mesh_facade_test tests/cpp/tsdf_register_facade_test tests/cpp/tsdf_shift_facade_test tests/cpp/capi_example tests/cpp/icpreg_test tests/cpp/asan_host tests/cpp/asan_oracle.o tests/cpp/search_select_test tests/cpp/rbc_set_test tests/cpp/mom_layout_test
	$(MAKE) -C oracle clean

.PHONY: all oracle clean asan examples search_select_test rbc_set_test mom_layout_test
