# Builds libmygram_gpu.so (HIP kernels for gfx950 + host C ABI) and the CPU oracle.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := mygram-db_amd/csrc
LIB := mygram-db_amd/libmygram_gpu.so
# -ffp-contract=off: BM25 arithmetic must round exactly like the reference's fp64 expression (no fused multiply-add)
CXXFLAGS := -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter -Iinclude
HIPFLAGS := --offload-arch=$(ARCH) $(CXXFLAGS)

OBJS := $(CSRC)/mgx_kernels.o $(CSRC)/mgx_highlight.o $(CSRC)/mgx_colsort.o $(CSRC)/mgx_facet.o $(CSRC)/mgx_documents.o $(CSRC)/mgx_build.o $(CSRC)/mgx_api.o $(CSRC)/mgx_compile.o $(CSRC)/mgx_columns.o $(CSRC)/mgx_tools.o

SHIM := mygram-db_amd/libmygram_shim.so

all: $(LIB) $(SHIM) oracle

$(CSRC)/mgx_kernels.o: $(CSRC)/mgx_kernels.hip $(CSRC)/mgx_internal.hpp $(CSRC)/mgx_launch.hpp $(CSRC)/mgx_fuzzy.hpp $(CSRC)/mgx_text.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# the HIGHLIGHT kernel is a translation unit of its own: the code of every other kernel is compiled from unchanged input
$(CSRC)/mgx_highlight.o: $(CSRC)/mgx_highlight.hip $(CSRC)/mgx_highlight.hpp $(CSRC)/mgx_internal.hpp $(CSRC)/mgx_launch.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# SORT <filter column>: its kernels too are a unit of their own (it restates the comparator it shares with the others)
$(CSRC)/mgx_colsort.o: $(CSRC)/mgx_colsort.hip $(CSRC)/mgx_colsort.hpp $(CSRC)/mgx_pkey.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# FACET in a batch: one more unit of its own (mgx_facet.hpp also holds the host-side plan, which compiles without HIP)
$(CSRC)/mgx_facet.o: $(CSRC)/mgx_facet.hip $(CSRC)/mgx_facet.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# page documents: the gather kernel, again a unit of its own (mgx_documents.hpp also holds the host-side record and arena
# plan, which compiles without HIP)
$(CSRC)/mgx_documents.o: $(CSRC)/mgx_documents.hip $(CSRC)/mgx_documents.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# the device column builder: a unit of its own as well (mgx_build.hpp also holds the key packing and the storage plan,
# which compile without HIP)
$(CSRC)/mgx_build.o: $(CSRC)/mgx_build.hip $(CSRC)/mgx_build.hpp $(CSRC)/mgx_internal.hpp $(CSRC)/mgx_text.hpp include/mygram_gpu.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/mgx_api.o: $(CSRC)/mgx_api.cpp $(CSRC)/mgx_build.hpp $(CSRC)/mgx_colsort.hpp $(CSRC)/mgx_pkey.hpp $(CSRC)/mgx_pages.hpp $(CSRC)/mgx_facet.hpp $(CSRC)/mgx_documents.hpp $(CSRC)/mgx_compile.hpp $(CSRC)/mgx_internal.hpp $(CSRC)/mgx_launch.hpp $(CSRC)/mgx_host.hpp $(CSRC)/mgx_highlight.hpp $(CSRC)/mgx_text.hpp include/mygram_gpu.h
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@
$(CSRC)/mgx_compile.o: $(CSRC)/mgx_compile.cpp $(CSRC)/mgx_compile.hpp $(CSRC)/mgx_internal.hpp $(CSRC)/mgx_host.hpp include/mygram_gpu.h
	g++ $(CXXFLAGS) -c $< -o $@
$(CSRC)/mgx_columns.o: $(CSRC)/mgx_columns.cpp $(CSRC)/mgx_build.hpp $(CSRC)/mgx_host.hpp $(CSRC)/mgx_text.hpp include/mygram_gpu.h
	g++ $(CXXFLAGS) -pthread -c $< -o $@
$(CSRC)/mgx_tools.o: $(CSRC)/mgx_tools.cpp include/mygram_tools.h $(CSRC)/mgx_fuzzy.hpp $(CSRC)/mgx_highlight.hpp $(CSRC)/mgx_text.hpp
	g++ $(CXXFLAGS) -pthread -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -pthread

# host C++17 layer (reference-signature classes, ExecuteBatch, BatchExecutor) + its C face for ctypes / cgo / JNI callers
# ICU (NormalizeText: NFKC / width / lower) when the system has it, like the reference's USE_ICU; MGX_NO_ICU=1 forces
# the ASCII fallback. mgxs_normalize_uses_icu() / NormalizeTextUsesIcu() report which branch was built.
ICU_OK := $(if $(MGX_NO_ICU),,$(shell printf '\043include <unicode/unorm2.h>\nint main(){return 0;}' | g++ -x c++ - -licuuc -licui18n -o /dev/null 2>/dev/null && echo 1))
ICU_FLAGS := $(if $(ICU_OK),-DMGX_USE_ICU,)
ICU_LIBS := $(if $(ICU_OK),-licui18n -licuuc,)
SHIM_SRC := $(CSRC)/shim/mygram_shim.cpp $(CSRC)/shim/shim_capi.cpp $(CSRC)/shim/normalize.cpp
$(SHIM): $(CSRC)/mgx_text.hpp $(CSRC)/mgx_highlight.hpp $(SHIM_SRC) $(CSRC)/shim/mygram_shim.hpp include/mygram_shim_c.h include/mygram_gpu.h $(LIB)
	g++ $(CXXFLAGS) $(ICU_FLAGS) -shared -o $@ $(SHIM_SRC) -Lmygram-db_amd -lmygram_gpu $(ICU_LIBS) -Wl,-rpath,'$$ORIGIN' -pthread

oracle:
	$(MAKE) -s -C oracle

# timing-ablation build of the library (tools only: MGX_DEBUG_SKIP then skips kernel phases; never shipped as the product)
ablation:
	$(HIPCC) $(HIPFLAGS) -DMGX_ABLATION -c $(CSRC)/mgx_kernels.hip -o /tmp/mgx_kernels_abl.o
	$(HIPCC) $(HIPFLAGS) -DMGX_ABLATION -x hip -c $(CSRC)/mgx_api.cpp -o /tmp/mgx_api_abl.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o mygram-db_amd/libmygram_gpu_ablation.so /tmp/mgx_kernels_abl.o $(CSRC)/mgx_highlight.o $(CSRC)/mgx_colsort.o $(CSRC)/mgx_facet.o $(CSRC)/mgx_documents.o $(CSRC)/mgx_build.o /tmp/mgx_api_abl.o $(CSRC)/mgx_compile.o $(CSRC)/mgx_columns.o $(CSRC)/mgx_tools.o -pthread

# the host pieces of mgx_colsort.hpp (key transform, collision scan) under the sanitizers: a stand-alone program, no GPU
colsort-host-asan:
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o colsort_host_check_asan tests/cpp/colsort_host_check.cpp
	python3 tests/test_column_sort_cpu.py > colsort_host_check_lines.txt
	./colsort_host_check_asan colsort_host_check_lines.txt

# the host side of mgx_pkey.hpp (key derivation, the key column, the comparator key_merge_kernel runs) likewise
pksort-host-asan:
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o pksort_host_check_asan tests/cpp/pksort_host_check.cpp
	python3 tests/test_primary_key_sort_cpu.py > pksort_host_check_lines.txt
	./pksort_host_check_asan pksort_host_check_lines.txt > /dev/null

# the original-text path of mgx_highlight.hpp (translation, pending-range filter, code point -> byte walk) likewise
highlight-original-host-asan:
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o highlight_original_host_check_asan tests/cpp/highlight_original_host_check.cpp
	python3 tests/test_highlight_original_cpu.py > highlight_original_host_check_lines.txt
	./highlight_original_host_check_asan highlight_original_host_check_lines.txt

# the host side of mgx_documents.hpp (record and arena plan, the restated gather) likewise
documents-host-asan:
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o documents_plan_check_asan tests/cpp/documents_plan_check.cpp
	./documents_plan_check_asan

# mgx_pages.hpp (the page plan of the bitmap group's fetch: pages, runs, top-k jobs, scratch layout) likewise
pages-host-asan:
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o pages_plan_check_asan tests/cpp/pages_plan_check.cpp
	./pages_plan_check_asan

# the host side of mgx_build.hpp (key packing, storage plan) and the decode rule of mgx_build.hip likewise
build-host-asan:
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o build_host_check_asan tests/cpp/build_host_check.cpp
	./build_host_check_asan

# the resident ending of mgx_build.hpp (mgx_index_build_device: allocation sizes, the lanes of resident_rows_kernel) likewise
resident-host-asan:
	g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o resident_plan_check_asan tests/cpp/resident_plan_check.cpp
	./resident_plan_check_asan

clean:
	rm -f $(OBJS) $(LIB) $(SHIM) build_host_check_asan resident_plan_check_asan colsort_host_check_asan colsort_host_check_lines.txt pksort_host_check_asan pksort_host_check_lines.txt highlight_original_host_check_asan highlight_original_host_check_lines.txt documents_plan_check_asan pages_plan_check_asan
	$(MAKE) -C oracle clean
.PHONY: all oracle clean ablation colsort-host-asan pksort-host-asan highlight-original-host-asan documents-host-asan pages-host-asan build-host-asan resident-host-asan
