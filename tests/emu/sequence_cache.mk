# TEST INFRASTRUCTURE — the sorting side of a fsdp_plan_sequence_cached pass (emu_sequence_cache.cpp) under the host SIMT emulator, as libraries of their own
# next to libfsdp_emu.so / libfsdp_emu_wide.so (Makefile), whose parameters they share by linking against them:
#     make -C tests/emu -f sequence_cache.mk
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -pthread -Wall -Wno-unused-variable -Wno-unused-but-set-variable -Wno-unknown-pragmas -Wno-sign-compare -Wno-attributes
CSRC = ../../ft-fsd-path-planning_amd/csrc
DEPS = emu_sequence_cache.cpp hip_emu.h emu_shared.h $(wildcard $(CSRC)/*.h) ../../include/fsdp.h
all: libfsdp_emu_sequence_cache.so libfsdp_emu_sequence_cache_wide.so
# (the libraries they link against come from the main Makefile; no -j here: one sub-make at a time)
libfsdp_emu.so libfsdp_emu_wide.so:
	$(MAKE) -s -f Makefile
libfsdp_emu_sequence_cache.so: $(DEPS) libfsdp_emu.so
	$(CXX) $(CXXFLAGS) -shared emu_sequence_cache.cpp -o $@ -L. -l:libfsdp_emu.so '-Wl,-rpath,$$ORIGIN'
libfsdp_emu_sequence_cache_wide.so: $(DEPS) libfsdp_emu_wide.so
	$(CXX) $(CXXFLAGS) -DFSDP_WIDE_SHAPES -shared emu_sequence_cache.cpp -o $@ -L. -l:libfsdp_emu_wide.so '-Wl,-rpath,$$ORIGIN'
clean:
	rm -f libfsdp_emu_sequence_cache.so libfsdp_emu_sequence_cache_wide.so
