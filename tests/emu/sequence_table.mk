# TEST INFRASTRUCTURE — the chain kernel of a sequence pass with per-frame global paths (csrc/sequence_table_kernel.h) under the host
# SIMT emulator: a library of its own next to libfsdp_emu.so (make -f sequence_table.mk), built on demand by
# tests/sequence_table_support.py and by __graft_entry__.build().  emu_kernels.cpp comes along for the parameters and the default
# path, emu_gpath_table.cpp for the speculative pass with ids.  Standard shapes only, like gpath_table.mk.
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -fno-gnu-unique -ffp-contract=off -fno-fast-math -pthread -Wall -Wno-unused-variable -Wno-unused-but-set-variable -Wno-unknown-pragmas -Wno-sign-compare -Wno-attributes
CSRC = ../../ft-fsd-path-planning_amd/csrc
MAKEFLAGS += -j3
DEPS = hip_emu.h emu_shared.h $(wildcard $(CSRC)/*.h) ../../include/fsdp.h
all: libfsdp_emu_sequence_table.so
# (object files under names of their own: the other makefiles build the same sources side by side with these)
libfsdp_emu_sequence_table.so: seqt_emu_kernels.o seqt_emu_gpath_table.o seqt_emu_sequence_table.o
	$(CXX) $(CXXFLAGS) -shared $^ -o $@
seqt_%.o: %.cpp $(DEPS)
	$(CXX) $(CXXFLAGS) -c $< -o $@
.SECONDARY:
clean:
	rm -f seqt_*.o libfsdp_emu_sequence_table.so
