# TEST INFRASTRUCTURE — the history instantiations of the sorting kernels (csrc/sort_history_kernels.h) under the host SIMT emulator:
# libraries of their own next to libfsdp_emu[_wide].so (make -f history.mk), built on demand by tests/emu_history_lib.py and by
# __graft_entry__.build().  emu_kernels.cpp comes along for the parameters, the no_sort128 switch and the filter.
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -fno-gnu-unique -ffp-contract=off -fno-fast-math -pthread -Wall -Wno-unused-variable -Wno-unused-but-set-variable -Wno-unknown-pragmas -Wno-sign-compare -Wno-attributes
CSRC = ../../ft-fsd-path-planning_amd/csrc
MAKEFLAGS += -j4
DEPS = hip_emu.h emu_shared.h $(wildcard $(CSRC)/*.h) ../../include/fsdp.h
all: libfsdp_emu_history.so libfsdp_emu_history_wide.so
# (object files under names of their own: tests/emu/Makefile builds emu_kernels.o side by side with these)
libfsdp_emu_history.so: hist_emu_kernels.o hist_emu_history.o
libfsdp_emu_history_wide.so: hist_emu_kernels_wide.o hist_emu_history_wide.o
%.so:
	$(CXX) $(CXXFLAGS) -shared $^ -o $@
hist_%_wide.o: %.cpp $(DEPS)
	$(CXX) $(CXXFLAGS) -DFSDP_WIDE_SHAPES -c $< -o $@
hist_%.o: %.cpp $(DEPS)
	$(CXX) $(CXXFLAGS) -c $< -o $@
# the capacity cases under AddressSanitizer and UBSan: a stand-alone program (make -f history.mk history_cap_probe &&
# ./history_cap_probe), nothing of it is loaded into Python
SAN = -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
history_cap_probe: history_cap_probe.cpp emu_history.cpp emu_kernels.cpp $(DEPS)
	$(CXX) $(filter-out -O2 -fPIC,$(CXXFLAGS)) $(SAN) history_cap_probe.cpp emu_history.cpp emu_kernels.cpp -o $@
.SECONDARY:
clean:
	rm -f hist_*.o libfsdp_emu_history.so libfsdp_emu_history_wide.so history_cap_probe
