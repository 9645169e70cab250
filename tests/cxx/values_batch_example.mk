# Compiles values_batch_example.cpp against the in-tree library and the HIP runtime (it copies device results to the host
# itself; compile/link check, run on a GPU box):
#   make -C tests/cxx -f values_batch_example.mk
ROOT := ../..
ROCM ?= /opt/rocm
all: values_batch_example
values_batch_example: values_batch_example.cpp $(ROOT)/include/simd_minimizers_amd.hpp $(ROOT)/include/simd_minimizers_amd.h
	g++ -std=c++17 -O2 -D__HIP_PLATFORM_AMD__ -I$(ROOT)/include -I$(ROCM)/include -o $@ values_batch_example.cpp -L$(ROOT)/simd-minimizers_amd -lsimd_minimizers_amd -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../simd-minimizers_amd' -Wl,-rpath,$(ROCM)/lib
clean:
	rm -f values_batch_example
