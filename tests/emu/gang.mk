# TEST INFRASTRUCTURE — the gang twins of the plain sorting kernels (csrc/sort_kernel.h StageGang) under the host SIMT emulator: a
# library of its own next to libfsdp_emu.so (make -f gang.mk), built on demand by tests/test_gang_emu.py and by
# __graft_entry__.build().  emu_kernels.cpp comes along for the parameters.  Standard shapes only: the twins add a prologue in
# front of frame code that the wide emulator libraries already cover.
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -fno-gnu-unique -ffp-contract=off -fno-fast-math -pthread -Wall -Wno-unused-variable -Wno-unused-but-set-variable -Wno-unknown-pragmas -Wno-sign-compare -Wno-attributes
CSRC = ../../ft-fsd-path-planning_amd/csrc
MAKEFLAGS += -j2
DEPS = hip_emu.h emu_shared.h $(wildcard $(CSRC)/*.h) ../../include/fsdp.h
all: libfsdp_emu_gang.so
# (object files under names of their own: tests/emu/Makefile builds emu_kernels.o side by side with these)
libfsdp_emu_gang.so: gang_emu_kernels.o gang_emu_gang.o
	$(CXX) $(CXXFLAGS) -shared $^ -o $@
gang_%.o: %.cpp $(DEPS)
	$(CXX) $(CXXFLAGS) -c $< -o $@
.SECONDARY:
clean:
	rm -f gang_*.o libfsdp_emu_gang.so
