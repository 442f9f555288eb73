// Kernel selection for one convolution launch slot (conv_select.cpp): the slot's description (ConvOp), the table of kernel candidates
// beside the implicit-GEMM tile shapes, the timing contest and the tuning table.  For vtd_api.cpp and the trocr_graph.inc it includes.
#pragma once
#include <map>
#include <string>
#include "conv_kernels.h"

namespace vtd {
enum : int {  // include/vtd.h: vtd_strerror
    ERR_ARG = -1100, ERR_UNKNOWN_KEY = -1101, ERR_SHAPE = -1102, ERR_MISSING_KEY = -1103,
    ERR_NOT_FINALIZED = -1104, ERR_BATCH = -1105, ERR_GEOMETRY = -1106, ERR_CAPACITY = -1107,
};

struct ConvOp {
    TensorDesc in, out, res;
    bool has_res = false;
    half_t* w = nullptr;
    half_t* w_panel = nullptr;   // the same weights K-panel-major, [K / 32][cout_pad][32] (dense_gemm.hip; dense layers of the Transformer encoder only)
    float* bias = nullptr;
    int k_hi_step = 32, cin_steps = 1, kw = 1, s_step = 0, r_step = 0;  // scalar K walk (ConvParams)
    int K = 0, cout = 0, cout_pad = 0, stride = 1, in_y0 = 0, in_x0 = 0, flags = 0, ps_cout = 0, res_shift = 0;
    int ho = 0, wo = 0;           // GEMM row decomposition (input-pixel grid for transposed conv)
    int64_t macs_per_image = 0;
    void* out_f32 = nullptr;      // EPI_OUT_F32 destination
    int ldc = 0;
    int seg_cols = 0;             // EPI_OUT_F16 in column segments (ConvParams::seg_cols)
    void* seg_out[3] = {nullptr, nullptr, nullptr};
    int seg_ldc[3] = {0, 0, 0};
    const float* head_w = nullptr;  // EPI_HEAD_FINAL
    float head_b = 0.f;
    // classed dual-source mode (fused FPN top + head entry)
    const uint32_t* plist = nullptr;
    const int* tile_combo = nullptr;
    const uint32_t* plist_b = nullptr;  // 256-row cut of the pixel lists
    const int* tile_combo_border = nullptr;  // the 12 border classes only (interior classes run on head_entry_halo.hip)
    int tiles_border = 0;
    const int* he_steps = nullptr;  // step tables of the four interior classes
    int he_nsteps = 0;
    const int* hh_sched = nullptr;  // head_entry_half.hip: half-step schedules of the four interior classes
    const int* hp_half_steps = nullptr;  // head_entry_pair.hip: half-step tables and halo prefetch plans of the four interior classes
    const int* hp_plan = nullptr;
    int hp_nh = 0;
    const int* tile_combo_b = nullptr;
    int tiles_per_img_b = 0;
    int tiles_per_img = 0, seg1_steps = 0, cin_steps2 = 0, kw2 = 0, s_step2 = 0, r_step2 = 0, img_h = 0, img_w = 0;
    TensorDesc in2;
    const float* bias_tab = nullptr;
    // second K segment of a plain conv (conv_igemm.hip DUAL): a 1x1 window of `in2` at (oy * in2_mul >> in2_shr, ox * in2_mul >> in2_shr)
    bool dual = false;
    int in2_mul = 1, in2_shr = 0;
    int pool_pw = 0;   // 2 x pool_pw max-pool behind the ReLU fused into the epilogue (`out` = the pooled tensor); 0 = none
};

// Configuration ids: [0, vtd_conv_num_configs()) are the implicit-GEMM tile shapes (conv_igemm.hip), the ids below name the
// other kernels.  What the host knows about each of them is its row of the candidate table in conv_select.cpp.
static const int kHaloCfg = 100;  // the halo-tile kernel (conv_halo.hip) instead of an implicit-GEMM tile shape
static const int kHaloC64Cfg = 101;  // persistent resident-weight variant for 64 -> 64 channels
static const int kHeadEntryHaloCfg = 102;  // composed head entry: interior classes on head_entry_halo.hip, border classes on cfg 8
static const int kHeadEntryHalo256Cfg = 103;  // same, 16x16 pixel blocks with 64x64 register tiles (hand-pipelined)
static const int kHalo64Cfg = 104;  // second-generation halo kernel: 64 output channels per workgroup, hand-pipelined
static const int kHeadEntryPairCfg = 105;  // two 16x16 blocks per workgroup on one weight ring, 32-channel halos prefetched two groups ahead
static const int kPointwiseCfg = 106;  // streaming 1x1 convolution 128 -> 256 with the top-down add (pointwise.hip): the C3 lateral
static const int kHeadEntryHalfCfg = 107;  // 16x16 blocks on 32-channel half halos fetched two K-steps ahead (head_entry_half.hip): no exposed halo switch
static const int kHaloSmallCfg = 108;  // small-footprint halo kernel: 8x16 pixel blocks x 64 output channels, three workgroups per CU

// One kernel candidate beside the implicit-GEMM tile shapes.  Adding a kernel = adding its row (and its id above).
struct ConvCandidate {
    int id;
    const char* name;  // the stem of the slot's label in vtd_detector_get_profile
    bool (*valid)(const ConvOp&, const ConvParams&);
    int (*launch)(const ConvOp&, const ConvParams&, hipStream_t);
    bool needs_border;  // does the interior classes of the composed head entry only: the BORDER slot behind it must run, and the contest times the two together
    bool halo_switch;   // VTD_HALO_CONV=0 keeps it out of the contest
    char force_halo;    // the VTD_FORCE_HALO digit that pins it in the contest (0: none)
    int reps, rounds;   // contest: best of `rounds` rounds of `reps` launches
};
const ConvCandidate* find_conv_candidate(int id);  // nullptr: not a row (an implicit-GEMM id, or a kernel this build does not carry)
int launch_conv_op(const ConvOp& c, int n, hipStream_t s, int cfg = -1, float* prob_out = nullptr);
int launch_border_tiles(const ConvOp& c, int n, hipStream_t s);

// Kernel-selection table: "<op signature>|n<batch bucket>" -> configuration id.  Filled from vtd_*_set_tuning (a table
// shipped with the package / broadcast by rank 0) and by the timing contest for shapes the table does not hold;
// vtd_*_get_tuning serialises it.  With a complete table kernel choice -- hence fp32 summation order -- is the same in
// every process and on every rank.
struct TuningTable {
    std::map<std::string, int> tuning;
    bool tuning_measured = false;  // at least one entry came from this process's own timing contest
};
int choose_config(TuningTable* m, const ConvOp& c, int n, hipStream_t s, int* cfg);
int set_tuning_text(TuningTable* m, const char* text);
int64_t get_tuning_text(const TuningTable* m, char* buf, int64_t cap);
int batch_bucket(int n, int cap);
}  // namespace vtd
