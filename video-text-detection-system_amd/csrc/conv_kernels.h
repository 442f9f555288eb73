// Host entries of the convolution kernels that kernel selection (conv_select.cpp) chooses among: launchers and their "supported"
// predicates.  Included by the .hip file that defines each of them, so the compiler sees declaration and definition together.
#pragma once
#include "vtd_common.h"

// conv_igemm.hip: the implicit-GEMM tile configurations, ids [0, vtd_conv_num_configs())
int vtd_launch_conv(const ConvParams& p, int cfg, hipStream_t stream);
int vtd_conv_num_configs();
bool vtd_conv_config_valid(const ConvParams& p, int cfg);
const char* vtd_conv_config_name(int cfg);  // "<rows>,<columns>,s<stages>[,...]" as the profile prints it; "default" outside the list
// conv_halo.hip
bool vtd_conv_halo_supported(const ConvParams& c, int* bn_out, int* tw_out);
bool vtd_conv_halo_c64_supported(const ConvParams& c, int tw);
int vtd_launch_conv_halo(const ConvParams& c, int bn, int tw, hipStream_t stream);
bool vtd_conv_halo_small_supported(const ConvParams& c);
int vtd_launch_conv_halo_small(const ConvParams& c, hipStream_t stream);
// pointwise.hip
bool vtd_pointwise128_supported(const ConvParams& c);
int vtd_launch_pointwise128(const ConvParams& c, hipStream_t stream);
// head_entry_halo.hip
extern "C" int vtd_head_entry_halo_steps(int py, int px, int nch1, int* out);
int vtd_launch_head_entry_halo(const ConvParams& c, const int* steps_dev, int nsteps, int big_tiles, hipStream_t stream);
#ifdef VTD_EXPERIMENTAL_CANDIDATES
// csrc/experimental/: measured, parity-green, LOSING candidates of the composed head entry.  They are not part of the
// product library: only an instrumented build (VTD_LIB_VARIANT=<tag> VTD_EXTRA_HIPCC_FLAGS=-DVTD_EXPERIMENTAL_CANDIDATES) carries them.
extern "C" int vtd_head_entry_half_schedule(const int* steps, int nsteps, int* out);
int vtd_launch_head_entry_half(const ConvParams& c, const int* sched_dev, int nsteps, hipStream_t stream);
int vtd_head_entry_pair_tables(int py, int px, int c2ch, int* half_steps, int* plan);
int vtd_launch_head_entry_pair(const ConvParams& c, const int* half_steps_dev, const int* plan_dev, int nh, hipStream_t stream);
#endif
