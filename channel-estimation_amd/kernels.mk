# The kernel translation units of libdsce.so (csrc/<name>.hip -> build/<name>.o)
# and the headers every object depends on: one list each for Makefile and
# asan.mk.  Each .hip is its own code object (no -fgpu-rdc).
KERNELS := kernels_mc kernels_setup kernels_export kernels_llr kernels_viterbi kernels_ldpc kernels_ldpc_layered kernels_ldpc_fixed
KERNEL_OBJ := $(KERNELS:%=$(ROOT)/build/%.o)
HDR := $(ROOT)/csrc/dsce_common.h $(ROOT)/csrc/dsce_kernels.h $(ROOT)/csrc/dsce_dispatch.h $(ROOT)/csrc/bm_tables.h $(ROOT)/csrc/stage_kernels.inc $(ROOT)/../include/dsce.h
