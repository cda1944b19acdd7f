# TEST INFRASTRUCTURE — the TABLE twins of the path stage's wrappers (csrc/gpath_table_kernel.h: per-frame global paths) under the
# host SIMT emulator: a library of its own next to libfsdp_emu.so (make -f gpath_table.mk), built on demand by
# tests/gpath_table_support.py and by __graft_entry__.build().  emu_kernels.cpp comes along for the parameters and the default path.
# Standard shapes only: the twins add a lookup in front of frame code that the wide emulator libraries already cover.
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -fno-gnu-unique -ffp-contract=off -fno-fast-math -pthread -Wall -Wno-unused-variable -Wno-unused-but-set-variable -Wno-unknown-pragmas -Wno-sign-compare -Wno-attributes
CSRC = ../../ft-fsd-path-planning_amd/csrc
MAKEFLAGS += -j2
DEPS = hip_emu.h emu_shared.h $(wildcard $(CSRC)/*.h) ../../include/fsdp.h
all: libfsdp_emu_gpath_table.so
# (object files under names of their own: tests/emu/Makefile builds emu_kernels.o side by side with these)
libfsdp_emu_gpath_table.so: gpt_emu_kernels.o gpt_emu_gpath_table.o
	$(CXX) $(CXXFLAGS) -shared $^ -o $@
gpt_%.o: %.cpp $(DEPS)
	$(CXX) $(CXXFLAGS) -c $< -o $@
.SECONDARY:
clean:
	rm -f gpt_*.o libfsdp_emu_gpath_table.so
