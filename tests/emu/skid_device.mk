# TEST INFRASTRUCTURE — the kernels of a skidpad device ticket (csrc/skid_device_kernel.h) under the host SIMT emulator: libraries
# of their own next to libfsdp_emu_device_io[_wide].so (make -f skid_device.mk), built on demand by tests/skid_device_support.py and
# by __graft_entry__.build()
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -fno-gnu-unique -ffp-contract=off -fno-fast-math -pthread -Wall -Wno-unused-variable -Wno-unused-but-set-variable -Wno-unknown-pragmas -Wno-sign-compare -Wno-attributes
CSRC = ../../ft-fsd-path-planning_amd/csrc
DEPS = hip_emu.h $(CSRC)/skid_device_kernel.h $(CSRC)/skid_state.h $(CSRC)/device_io_kernel.h $(CSRC)/fsdp_device.h $(CSRC)/device_prims.h ../../include/fsdp.h
all: libfsdp_emu_skid_device.so libfsdp_emu_skid_device_wide.so
libfsdp_emu_skid_device.so: emu_skid_device.cpp $(DEPS)
	$(CXX) $(CXXFLAGS) -shared $< -o $@
# the same kernel sources with the wide build's shapes (include/fsdp.h FSDP_WIDE_SHAPES)
libfsdp_emu_skid_device_wide.so: emu_skid_device.cpp $(DEPS)
	$(CXX) $(CXXFLAGS) -DFSDP_WIDE_SHAPES -shared $< -o $@
clean:
	rm -f libfsdp_emu_skid_device.so libfsdp_emu_skid_device_wide.so
