// Kernel selection for the convolution launch slots of the detector, the CRNN and the Transformer recogniser: the table of kernel
// candidates beside the implicit-GEMM tile shapes, the launch by configuration id, the timing contest and the tuning table.
// A new kernel candidate is ONE row of kCandidates below (plus its id in conv_select.h and its prototypes in conv_kernels.h).
#include "conv_select.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace vtd {
static void fill_conv_params(const ConvOp& c, int n, ConvParams& p) {
    std::memset(&p, 0, sizeof(p));
    p.in = c.in.ptr; p.wgt = c.w; p.k_hi_step = c.k_hi_step; p.cin_steps = c.cin_steps; p.kw = c.kw; p.s_step = c.s_step; p.r_step = c.r_step; p.bias = c.bias;
    p.res = c.has_res ? c.res.ptr : nullptr;
    p.out = (c.flags & (EPI_OUT_F32 | EPI_OUT_F16)) ? c.out_f32 : (void*)c.out.ptr;
    p.M = n * c.ho * c.wo; p.K = c.K; p.cout = c.cout; p.cout_pad = c.cout_pad;
    p.ho = c.ho; p.wo = c.wo;
    p.in_hp = c.in.hp; p.in_wp = c.in.wp; p.in_c = c.in.c; p.in_y0 = c.in_y0; p.in_x0 = c.in_x0; p.stride = c.stride;
    p.out_hp = c.out.hp; p.out_wp = c.out.wp; p.out_c = c.out.c; p.out_ring = c.out.ring;
    p.res_hp = c.res.hp; p.res_wp = c.res.wp; p.res_ring = c.res.ring; p.res_shift = c.res_shift;
    p.ps_cout = c.ps_cout; p.flags = c.flags; p.ldc = c.ldc;
    p.seg_cols = c.seg_cols;
    for (int i = 0; i < 3; ++i) { p.seg_out[i] = c.seg_out[i]; p.seg_ldc[i] = c.seg_ldc[i]; }
    p.head_w = c.head_w; p.head_b = c.head_b; p.prob_out = (float*)c.out_f32;
    if (c.plist) {
        p.plist = c.plist; p.tile_combo = c.tile_combo; p.tiles_per_img = c.tiles_per_img;
        p.plist_b = c.plist_b; p.tile_combo_b = c.tile_combo_b; p.tiles_per_img_b = c.tiles_per_img_b;
        p.in2 = c.in2.ptr; p.in2_hp = c.in2.hp; p.in2_wp = c.in2.wp; p.in2_c = c.in2.c; p.in2_ring = c.in2.ring;
        p.seg1_steps = c.seg1_steps; p.cin_steps2 = c.cin_steps2; p.kw2 = c.kw2; p.s_step2 = c.s_step2; p.r_step2 = c.r_step2;
        p.bias_tab = c.bias_tab; p.img_h = c.img_h; p.img_w = c.img_w;
        p.M = n * c.tiles_per_img * 128;
    }
    p.pool_pw = c.pool_pw;
    if (c.dual) {
        p.in2 = c.in2.ptr; p.in2_hp = c.in2.hp; p.in2_wp = c.in2.wp; p.in2_c = c.in2.c; p.in2_ring = c.in2.ring;
        p.in2_mul = c.in2_mul; p.in2_shr = c.in2_shr;
        p.seg1_steps = c.seg1_steps; p.cin_steps2 = c.cin_steps2; p.kw2 = 1; p.s_step2 = 0; p.r_step2 = 0;
    }
}

static bool env_is(const char* name, char v) { const char* e = std::getenv(name); return e && e[0] == v; }
static bool halo_enabled() { return !env_is("VTD_HALO_CONV", '0'); }
static bool autotune_enabled() { return !env_is("VTD_AUTOTUNE", '0'); }

static bool halo_valid(const ConvParams& p, bool c64) {
    int bn = 0, tw = 0;
    return vtd_conv_halo_supported(p, &bn, &tw) && (!c64 || vtd_conv_halo_c64_supported(p, tw));
}
// bn: 0 = the channel-block width vtd_conv_halo_supported picks, 1 = the persistent 64 -> 64 variant, 2 = conv_halo64
static int launch_halo(const ConvParams& p, int bn, hipStream_t s) {
    int hbn = 0, tw = 0;
    return vtd_conv_halo_supported(p, &hbn, &tw) ? vtd_launch_conv_halo(p, bn ? bn : hbn, tw, s) : ERR_GEOMETRY;
}
static bool head_entry_valid(const ConvOp& c, const ConvParams& p) { return p.plist && c.he_steps && c.tile_combo_border; }

// The kernel candidates beside the implicit-GEMM tile shapes, in the order the contest tries them:
// {id, name, valid, launch, needs_border, halo_switch, force_halo, reps, rounds}
static const ConvCandidate kCandidates[] = {
    // composed head entry, interior classes only (border tiles = the next graph slot).  The variants are within ~5 %: best of two rounds of four
    {kHeadEntryHaloCfg, "head_entry_halo", head_entry_valid,
     [](const ConvOp& c, const ConvParams& p, hipStream_t s) { return vtd_launch_head_entry_halo(p, c.he_steps, c.he_nsteps, 0, s); }, true, true, 0, 4, 2},
    {kHeadEntryHalo256Cfg, "head_entry_halo256", head_entry_valid,
     [](const ConvOp& c, const ConvParams& p, hipStream_t s) { return vtd_launch_head_entry_halo(p, c.he_steps, c.he_nsteps, 1, s); }, true, true, 0, 4, 2},
#ifdef VTD_EXPERIMENTAL_CANDIDATES  // candidates of the instrumented build only
    {kHeadEntryPairCfg, "head_entry_pair", [](const ConvOp& c, const ConvParams& p) { return head_entry_valid(c, p) && c.hp_half_steps; },
     [](const ConvOp& c, const ConvParams& p, hipStream_t s) { return vtd_launch_head_entry_pair(p, c.hp_half_steps, c.hp_plan, c.hp_nh, s); }, true, true, 0, 4, 2},
    {kHeadEntryHalfCfg, "head_entry_half", [](const ConvOp& c, const ConvParams& p) { return head_entry_valid(c, p) && c.hh_sched; },
     [](const ConvOp& c, const ConvParams& p, hipStream_t s) { return vtd_launch_head_entry_half(p, c.hh_sched, c.he_nsteps, s); }, true, true, 0, 4, 2},
#endif
    {kPointwiseCfg, "pointwise128", [](const ConvOp&, const ConvParams& p) { return vtd_pointwise128_supported(p); },
     [](const ConvOp&, const ConvParams& p, hipStream_t s) { return vtd_launch_pointwise128(p, s); }, false, false, 0, 3, 1},
    {kHaloCfg, "conv_halo", [](const ConvOp&, const ConvParams& p) { return halo_valid(p, false); },
     [](const ConvOp&, const ConvParams& p, hipStream_t s) { return launch_halo(p, 0, s); }, false, true, 0, 3, 1},
    {kHaloC64Cfg, "conv_halo_c64_persistent", [](const ConvOp&, const ConvParams& p) { return halo_valid(p, true); },
     [](const ConvOp&, const ConvParams& p, hipStream_t s) { return launch_halo(p, 1, s); }, false, true, '2', 3, 1},
    {kHalo64Cfg, "conv_halo64", [](const ConvOp&, const ConvParams& p) { return halo_valid(p, false); },
     [](const ConvOp&, const ConvParams& p, hipStream_t s) { return launch_halo(p, 2, s); }, false, true, '3', 3, 1},
    {kHaloSmallCfg, "conv_halo_small", [](const ConvOp&, const ConvParams& p) { return vtd_conv_halo_small_supported(p); },
     [](const ConvOp&, const ConvParams& p, hipStream_t s) { return vtd_launch_conv_halo_small(p, s); }, false, true, '4', 3, 1},
};

const ConvCandidate* find_conv_candidate(int id) {
    for (const ConvCandidate& row : kCandidates)
        if (row.id == id) return &row;
    return nullptr;
}

// Configurations 0 / 12 / 13 / 14 / 15 are one kernel family (128 or 256 channels wide, 3- or 2-stage ring) at tile heights 256 / 208 /
// 272 rows, on 8 or 16 waves.  Which is cheapest depends on how the launch's tile count falls on the 256 CUs (one workgroup each), i.e.
// on the ACTUAL row count, which a per-bucket table cannot know (272 crops and 512 crops share a bucket; the table's entry was timed at
// 512): rounds x time per tile.  Time per tile = rows x columns / relative efficiency of the shape, measured on layer 2-4 and on the
// CRNN at 272 and 301 crops with every convolution forced onto each shape in turn (tools/gpu_rec_cfgs.sh, round 4): 4 x 2 waves of
// 64 x 64 (cfg 0) 1.0, the same tile on 16 waves (14) 1.04, 2 x 4 waves of 9+8 fragments x 32 (13: 272 rows) 0.92, 7+6 x 32 (12: 208 rows)
// 0.80, the 256 x 256 tile (15) 1.07.  What that buys at 272 crops: conv5 (34 816 rows x 512 channels; the table's 256 x 256 tile makes
// 272 tiles = two rounds for 1.06) 130 -> 85 us on 272-row tiles (512 tiles = two full rounds), conv3 / conv4 / conv6 58 / 99 / 177 ->
// 52 / 87 / 152 us; at 301 crops the 16-wave 256-row tile wins instead and conv5 takes 99 us.  The table's entry is tried first and
// keeps the slot unless another shape is cheaper by more than 6 % (short-K launches have per-tile overheads the model does not see).
// A pure function of the shape, and the tile shape never changes a bit of the result
// (tests/test_gpu_detector.py: test_implicit_gemm_tile_heights_bit_identical).
static int pick_tile_height(const ConvParams& p, int table_cfg) {
    if (const char* e = std::getenv("VTD_TILE_HEIGHT_MODEL"); e && e[0] == '0') return table_cfg;
    if (std::getenv("VTD_FORCE_CONV_CFG")) return table_cfg;  // tests pin one configuration
    static const struct { int cfg, bm, bn; double eff; } family[5] = {{0, 256, 128, 1.0}, {14, 256, 128, 1.04}, {13, 272, 128, 0.92}, {12, 208, 128, 0.80},
                                                                      {15, 256, 256, 1.07}};
    auto cost_of = [&](int cfg) -> double {
        for (const auto& k : family)
            if (k.cfg == cfg) {
                if (!vtd_conv_config_valid(p, k.cfg)) return 0.0;
                const int64_t tiles = (int64_t)((p.M + k.bm - 1) / k.bm) * (p.cout_pad / k.bn);
                return (double)((tiles + 255) / 256) * k.bm * k.bn / k.eff;
            }
        return 0.0;
    };
    const double table_cost = cost_of(table_cfg);
    if (table_cost == 0.0) return table_cfg;
    int best = table_cfg;
    double other_cost = table_cost * 0.94;   // another shape must beat the table's by more than 6 %
    for (const auto& k : family) {
        if (k.cfg == table_cfg) continue;
        const double c = cost_of(k.cfg);
        if (c > 0.0 && c < other_cost) { other_cost = c; best = k.cfg; }
    }
    return best;
}

int launch_conv_op(const ConvOp& c, int n, hipStream_t s, int cfg, float* prob_out) {
    ConvParams p;
    fill_conv_params(c, n, p);
    if (prob_out) p.prob_out = prob_out;
    if (const ConvCandidate* row = find_conv_candidate(cfg)) return row->valid(c, p) ? row->launch(c, p, s) : ERR_GEOMETRY;
    if (cfg >= vtd_conv_num_configs()) return ERR_GEOMETRY;  // a kernel this build does not carry
    if (!c.plist && (cfg == 0 || cfg == 12 || cfg == 13 || cfg == 14 || cfg == 15)) cfg = pick_tile_height(p, cfg);
    return vtd_launch_conv(p, cfg, s);
}

// Border pixels of the composed head entry: the same op restricted to the border classes' 128-row tiles.
int launch_border_tiles(const ConvOp& c, int n, hipStream_t s) {
    if (!c.tile_combo_border || c.tiles_border <= 0) return ERR_GEOMETRY;
    ConvParams pb;
    fill_conv_params(c, n, pb);
    pb.tile_combo = c.tile_combo_border; pb.tiles_per_img = c.tiles_border; pb.M = n * c.tiles_border * 128;
    pb.plist_b = nullptr; pb.tile_combo_b = nullptr; pb.tiles_per_img_b = 0;
    // 384 tiles on 256 CUs: one latency-bound round, so the 3-stage ring (two K-steps of loads in flight) beats the 2-stage one
    // that wins when several workgroups share a CU (41 vs 53 us)
    return vtd_launch_conv(pb, 9, s);
}

static bool config_valid_for(const ConvOp& c, int n, int cfg) {
    ConvParams p;
    fill_conv_params(c, n, p);
    if (const ConvCandidate* row = find_conv_candidate(cfg)) return row->valid(c, p);
    return cfg >= 0 && cfg < vtd_conv_num_configs() && vtd_conv_config_valid(p, cfg);
}

// One warm-up launch (it also sets the kernel's LDS attribute), then the best of `rounds` rounds of `reps` launches between two
// events on `s`, scaled to the 3 launches every candidate is compared on.
template <class F>
static int time_launches(F&& launch, int reps, int rounds, hipEvent_t e0, hipEvent_t e1, hipStream_t s, float* ms) {
    int rc = launch();
    *ms = 1e30f;
    for (int round = 0; round < rounds && !rc; ++round) {
        (void)hipEventRecord(e0, s);
        for (int rep = 0; rep < reps && !rc; ++rep) rc = launch();
        (void)hipEventRecord(e1, s);
        if (hipEventSynchronize(e1) != hipSuccess) rc = ERR_ARG;
        float t = 0.f;
        (void)hipEventElapsedTime(&t, e0, e1);
        *ms = std::min(*ms, t * (3.f / reps));
    }
    return rc;
}

// Times every valid tile configuration of one convolution at batch n and returns the fastest (HIP events on `s`).
// The launch writes the op's real output buffer; the graph recomputes it on the next forward anyway.
static int autotune_conv(const ConvOp& c, int n, hipStream_t s, int* best_cfg) {
    ConvParams p;
    fill_conv_params(c, n, p);
    // tests: pin the composed conv to one tile configuration (8..11) or head-entry kernel
    if (const char* fc = std::getenv("VTD_FORCE_CLASSED_CFG"); fc && p.plist && config_valid_for(c, n, std::atoi(fc))) {
        *best_cfg = std::atoi(fc);
        return 0;
    }
    hipEvent_t e0, e1;
    VTD_HIP_CHECK(hipEventCreate(&e0));
    VTD_HIP_CHECK(hipEventCreate(&e1));
    const bool verbose = env_is("VTD_AUTOTUNE_VERBOSE", '1');
    float best = 1e30f, ms = 0.f;
    int best_id = -1, rc = 0;
    for (int cfg = 0; cfg < vtd_conv_num_configs() && !rc; ++cfg) {
        if (!vtd_conv_config_valid(p, cfg)) continue;
        rc = time_launches([&] { return vtd_launch_conv(p, cfg, s); }, 3, 1, e0, e1, s, &ms);
        if (!rc && ms < best) { best = ms; best_id = cfg; }
    }
    // Plain timing, no hand-set handicaps: this back-to-back contest only serves shapes the shipped table
    // (vtd_amd/tuning/gfx950.txt, chosen by in-situ measurement of the whole pipeline: tools/tune_table.py) lacks.
    const char* force = std::getenv("VTD_FORCE_HALO");  // tests: 1 = take the halo kernel wherever it applies, 2 = and its persistent 64->64
    const char digit = force ? force[0] : 0;            // variant, 3 = the hand-pipelined 64-channel kernel, 4 = the small-footprint kernel
    bool pinned = false;  // the row VTD_FORCE_HALO names was taken: no later row may win on time
    for (const ConvCandidate& row : kCandidates) {
        if (rc) break;
        if ((row.halo_switch && !halo_enabled()) || !row.valid(c, p)) continue;
        if (row.id == kHaloCfg && digit >= '1' && digit <= '3') best = 1e30f;  // whatever ran before the halo kernels is out of the contest
        rc = time_launches([&] { int r = row.launch(c, p, s); return !r && row.needs_border ? launch_border_tiles(c, n, s) : r; }, row.reps, row.rounds,
                           e0, e1, s, &ms);
        if (verbose && row.needs_border)
            std::fprintf(stderr, "[autotune] head entry variant %d: %.1f us per launch incl. border tiles (best so far %.1f, cfg %d)\n", row.id,
                         ms / 3.f * 1e3f, best / 3.f * 1e3f, best_id);
        const bool pin = row.force_halo && row.force_halo == digit;
        if (!rc && !pinned && (ms < best || pin)) { best = ms; best_id = row.id; pinned = pin; }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *best_cfg = best_id;
    if (verbose)
        std::fprintf(stderr, "[autotune] M=%d N=%d K=%d%s -> cfg %d (%.1f us per launch)\n", p.M, p.cout, p.K, p.plist ? " classed" : "", best_id,
                     best / 3.f * 1e3f);
    return rc;
}

// Signature of one convolution launch slot: everything kernel choice may depend on except the batch.
static std::string conv_signature(const ConvOp& c) {
    char buf[192];
    int len = std::snprintf(buf, sizeof buf, "conv|in%dx%dx%d|out%dx%d|co%d|K%d|s%d|f%x|r%d|c%d", c.in.h, c.in.w, c.in.c, c.ho, c.wo, c.cout, c.K,
                            c.stride, (unsigned)c.flags, c.has_res ? 1 + c.res_shift : 0, c.plist ? 1 : 0);
    if (c.dual) len += std::snprintf(buf + len, sizeof buf - len, "|x%dm%ds%d", c.in2.c, c.in2_mul, c.in2_shr);  // second K segment (entries of plain convs keep their keys)
    if (c.pool_pw) std::snprintf(buf + len, sizeof buf - len, "|p2x%d", c.pool_pw);  // max-pool fused into the epilogue
    return buf;
}

// Configuration of one launch slot at batch bucket n: the table's entry when it has a valid one, else the timing contest
// (whose result joins the table), else -1 (built-in heuristic).
int choose_config(TuningTable* m, const ConvOp& c, int n, hipStream_t s, int* cfg) {
    const std::string key = conv_signature(c) + "|n" + std::to_string(n);
    auto it = m->tuning.find(key);
    // test switches that pin a kernel variant (VTD_FORCE_CLASSED_CFG, VTD_FORCE_HALO) are honoured by the contest: they outrank the table
    const bool forced = std::getenv("VTD_FORCE_CLASSED_CFG") || std::getenv("VTD_FORCE_HALO");
    if (const char* fc = std::getenv("VTD_FORCE_CONV_CFG"); fc && !c.plist && config_valid_for(c, n, std::atoi(fc))) {
        *cfg = std::atoi(fc);  // tests: one implicit-GEMM tile configuration wherever it is valid, every other slot as usual
        return 0;
    }
    if (const char* fp = std::getenv("VTD_FORCE_POINTWISE"); fp && fp[0] == '1' && config_valid_for(c, n, kPointwiseCfg)) {
        *cfg = kPointwiseCfg;  // tests: the streaming 1x1 kernel wherever it applies, every other slot as usual
        return 0;
    }
    if (!forced && it != m->tuning.end() && config_valid_for(c, n, it->second)) {
        *cfg = it->second;
        return 0;
    }
    *cfg = -1;
    if (!autotune_enabled()) return 0;
    int rc = autotune_conv(c, n, s, cfg);
    if (!rc && *cfg >= 0) {
        m->tuning[key] = *cfg;
        m->tuning_measured = true;
    }
    return rc;
}

int set_tuning_text(TuningTable* m, const char* text) {
    if (!m || !text) return ERR_ARG;
    const char* p = text;
    while (*p) {
        const char* eol = std::strchr(p, '\n');
        std::string line = eol ? std::string(p, eol) : std::string(p);
        p = eol ? eol + 1 : p + line.size();
        if (line.empty() || line[0] == '#') continue;
        const size_t sp = line.find_last_of(" \t");
        if (sp == std::string::npos || sp + 1 >= line.size()) return ERR_ARG;
        char* end = nullptr;
        const long v = std::strtol(line.c_str() + sp + 1, &end, 10);
        if (!end || *end != 0) return ERR_ARG;
        size_t ke = sp;
        while (ke > 0 && (line[ke - 1] == ' ' || line[ke - 1] == '\t')) --ke;
        m->tuning[line.substr(0, ke)] = (int)v;
    }
    return 0;
}

int64_t get_tuning_text(const TuningTable* m, char* buf, int64_t cap) {
    if (!m) return ERR_ARG;
    std::string out;
    for (const auto& kv : m->tuning) out += kv.first + " " + std::to_string(kv.second) + "\n";
    if (buf && cap > 0) {
        const size_t ncopy = std::min((size_t)cap - 1, out.size());
        std::memcpy(buf, out.data(), ncopy);
        buf[ncopy] = 0;
    }
    return (int64_t)out.size() + 1;
}

int batch_bucket(int n, int cap) {
    int b = 1;
    while (b < n) b <<= 1;
    return std::min(b, cap);
}

// The candidate table, readable without a GPU (tests/test_conv_candidates.py; internal, not in include/vtd.h): row `index`.
// Returns the number of rows, or a negative value on a bad argument.
extern "C" int vtd_conv_candidate_at(int index, int* id, int* needs_border, int* force_halo_digit, char* name, int name_cap) {
    const int rows = (int)(sizeof kCandidates / sizeof *kCandidates);
    if (index < 0 || index >= rows || !id || !needs_border || !force_halo_digit || !name || name_cap <= 0) return ERR_ARG;
    const ConvCandidate& row = kCandidates[index];
    *id = row.id; *needs_border = row.needs_border; *force_halo_digit = row.force_halo;
    std::snprintf(name, name_cap, "%s", row.name);
    return rows;
}
extern "C" int vtd_conv_igemm_config_count(void) { return vtd_conv_num_configs(); }

}  // namespace vtd
