# Compiles bgzf_crc_example.cpp against the in-tree library (compile/link check; run on a GPU box):
#   make -C tests/cxx -f bgzf_crc_example.mk
ROOT := ../..
ROCM ?= /opt/rocm
all: bgzf_crc_example
bgzf_crc_example: bgzf_crc_example.cpp $(ROOT)/include/simd_minimizers_amd.hpp $(ROOT)/include/simd_minimizers_amd.h
	g++ -std=c++17 -O2 -Wall -Wextra -I$(ROOT)/include -o $@ bgzf_crc_example.cpp -L$(ROOT)/simd-minimizers_amd -lsimd_minimizers_amd -Wl,-rpath,'$$ORIGIN/../../simd-minimizers_amd' -Wl,-rpath,$(ROCM)/lib
clean:
	rm -f bgzf_crc_example
