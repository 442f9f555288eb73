// Host side of libvtd_hip.so: handles, checkpoint ingest (BatchNorm folding + fp16 repack), network
// graphs, workspace provisioning and the extern "C" entry points declared in include/vtd.h.
// Compiled with hipcc for gfx950; launches the kernels in conv_igemm.hip / detector_misc.hip / ...
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vtd.h"
#include "vtd_common.h"
#include "conv_select.h"  // ConvOp, kernel choice per launch slot; with conv_kernels.h, the convolution launchers it chooses among

// the other kernel launchers (defined in the .hip files)
int vtd_launch_preprocess(const uint8_t* frames, int n, int H, int W, half_t* out, const int* xb, const int* xk, int ksx,
                          const int* yb, const int* yk, int ksy, int max_rows, hipStream_t stream);
int vtd_preprocess_max_rows(const int* yb);
int vtd_preprocess_path(int W, int ksx, int ksy, int max_rows, int* lds_bytes);
int vtd_launch_nchw_to_input(const float* x, half_t* out, int n, hipStream_t stream);
int vtd_launch_maxpool(const TensorDesc& in, const TensorDesc& out, int n, int kh, int kw, int sh, int sw, int pad_h, int pad_w,
                       hipStream_t stream);
void vtd_stem_pool_pack_weights(const float* w_folded, half_t* packed);
int vtd_launch_stem_pool(const TensorDesc& in, const TensorDesc& out, const half_t* w_packed, const float* bias, int n, hipStream_t stream);
void vtd_head_tail_pack_w1(const half_t* w1_gemm, half_t* packed);
void vtd_head_tail_pack_w2(const float* w2, half_t* packed);
int vtd_launch_head_tail(const TensorDesc& in, const half_t* w1, const float* bias1, const half_t* w2, float b2, float* out, int n,
                         hipStream_t stream);

int vtd_launch_crop_resize(const uint8_t* frames, int nframes, int H, int W, const int32_t* boxes, int ncrops, uint8_t* out, hipStream_t s);
int vtd_launch_crnn_conv1(const uint8_t* in_u8, const float* in_f32, const half_t* w, const float* bias, half_t* out, int n, hipStream_t s);
int vtd_launch_lstm(const half_t* xs, const half_t* whh, half_t* hout, int D, int T, hipStream_t s);
int vtd_launch_ctc_greedy(const float* logits, int n, int T, int V, int ld, const int32_t* id2char, int blank, int apply_softmax,
                          int32_t* out, hipStream_t s);
int vtd_launch_compact_rows(const float* in, float* out, int64_t rows, int V, int ld, hipStream_t s);
int vtd_dbloss_ws_bytes();
int vtd_launch_dbloss(const float* prob, const float* thresh, const float* prob_t, const float* thresh_t, int64_t n, float smooth, double* workspace,
                      float* out4, double* sums5, hipStream_t stream);
int vtd_launch_dbloss_backward(const float* prob, const float* thresh, const float* prob_t, const float* thresh_t, int64_t n, float smooth,
                               const double* sums5, const float* grad_out4, float* grad_prob, float* grad_thresh, hipStream_t stream);
int vtd_launch_binary_counts(const float* pred, const float* target, int64_t n, float threshold, int64_t* counts4, hipStream_t stream);
int vtd_launch_adamw(const vtd_adamw_tensor* tensors, int count, const vtd_adamw_hyper* hyper, hipStream_t stream);
int64_t vtd_dbhead_ws_bytes(int n, int H, int W, int backward);
int vtd_launch_dbhead_pack(const void* x, int dtype, int n, int H, int W, void* feats, hipStream_t s);
int vtd_launch_dbhead_forward(const void* feats, int n, int H, int W, const vtd_dbhead_params* params, int training, float momentum, float eps,
                              void* ws, float* prob, float* thresh, float* stats_out, hipStream_t s);
int vtd_launch_dbhead_backward_input(int n, int H, int W, const vtd_dbhead_params* params, void* scratch, float* dfeats, float* dscale, hipStream_t s);
int vtd_launch_dbhead_unpack_input_grad(const float* dfeats, const float* dscale, int n, int H, int W, float* out, hipStream_t s);
int64_t vtd_fpn_ws_bytes(int n, int h5, int w5, int c5, int mode);
int vtd_launch_fpn_pack_tap(const void* x, int dtype, int n, int channels, int H, int W, void* out, hipStream_t s);
int vtd_launch_fpn_unpack_p2(const void* p2, int n, int H, int W, float* out, hipStream_t s);
int vtd_launch_fpn_pack_grad(const float* g, int n, int H, int W, float* out, hipStream_t s);
int vtd_launch_fpn_forward(const void* const* taps, int n, int h5, int w5, int c5, const vtd_fpn_params* params, void* ws, void* p2_out, hipStream_t s);
int vtd_launch_fpn_backward(const void* const* taps, int n, int h5, int w5, int c5, const vtd_fpn_params* params, const void* ws, const float* dp2,
                            const float* dscale, const vtd_fpn_params* grads, void* scratch, hipStream_t s);
int64_t vtd_fpn_input_ws_bytes(int n, int h5, int w5, int c5);
int vtd_launch_fpn_backward_input(int n, int h5, int w5, int c5, const vtd_fpn_params* params, void* scratch, int mask, float* const* dtaps,
                                  float* dscale, hipStream_t s);
int64_t vtd_basicblock_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_basicblock_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                  void* ws, void* y, hipStream_t s);
int vtd_launch_basicblock_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                   const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch,
                                   float* dx, float* dxscale, hipStream_t s);
int64_t vtd_resblock_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int64_t vtd_block64_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_block64_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps, void* ws,
                               void* y, hipStream_t s);
int vtd_launch_block64_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch,
                                float* dx, float* dxscale, hipStream_t s);
int vtd_launch_resblock_combine(float* a, const float* asc, const float* b, const float* bsc, int64_t numel, float* osc, hipStream_t s);
int64_t vtd_resblock_bn_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_resblock_bn_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                   float momentum, float eps, void* ws, void* y, float* stats, hipStream_t s);
int vtd_launch_resblock_bn_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                    float eps, const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp,
                                    void* scratch, float* dx, float* dxscale, hipStream_t s);
int64_t vtd_block_bn_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_block_bn_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                float momentum, float eps, void* ws, void* y, float* stats, hipStream_t s);
int vtd_launch_block_bn_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                 float eps, const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp,
                                 void* scratch, float* dx, float* dxscale, hipStream_t s);
int64_t vtd_trunk_bn_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_trunk_bn_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                float momentum, float eps, void* ws, void* y, float* stats, hipStream_t s);
int vtd_launch_trunk_bn_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                 float eps, const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp,
                                 void* scratch, float* dx, float* dxscale, hipStream_t s);
int vtd_launch_stem_pack_input(const void* x, int dtype, int n, int H, int W, void* tap, hipStream_t s);
int64_t vtd_stem_ws_bytes(int n, int H, int W, int mode);
int vtd_launch_stem_forward(const void* x, int n, int H, int W, const vtd_stem_params* P, float eps, void* ws, void* pool, void* idx, hipStream_t s);
int vtd_launch_stem_backward(const void* x, int n, int H, int W, const vtd_stem_params* P, float eps, const void* ws, const void* pool, const void* idx,
                             const float* dpool, const float* dscale, const vtd_stem_params* Gp, void* scratch, hipStream_t s);
int64_t vtd_stem_bn_ws_bytes(int n, int H, int W, int mode);
int vtd_launch_stem_bn_forward(const void* x, int n, int H, int W, const vtd_stem_params* P, int training, float momentum, float eps, void* ws, void* pool,
                               void* idx, float* stats, hipStream_t s);
int vtd_launch_stem_bn_backward(const void* x, int n, int H, int W, const vtd_stem_params* P, int training, float eps, const void* ws, const void* pool,
                                const void* idx, const float* dpool, const float* dscale, const vtd_stem_params* Gp, void* scratch, hipStream_t s);
int vtd_launch_resblock_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps, void* ws,
                                void* y, hipStream_t s);
int vtd_launch_resblock_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                 const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch,
                                 float* dx, float* dxscale, hipStream_t s);
int64_t vtd_bottleneck_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_bottleneck_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps, void* ws,
                                  void* y, hipStream_t s);
int vtd_launch_bottleneck_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                   const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp, void* scratch,
                                   float* dx, float* dxscale, hipStream_t s);
int64_t vtd_bottleneck_bn_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_bottleneck_bn_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, int training,
                                     float momentum, float eps, void* ws, void* y, float* stats, hipStream_t s);
int vtd_launch_bottleneck_bn_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, int training,
                                      float eps, const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp,
                                      void* scratch, float* dx, float* dxscale, hipStream_t s);
int64_t vtd_bottleneck256_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_bottleneck256_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                     void* ws, void* y, hipStream_t s);
int vtd_launch_bottleneck256_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                      const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp, void* scratch,
                                      float* dx, float* dxscale, hipStream_t s);
int64_t vtd_bottleneck128_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_bottleneck128_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                     void* ws, void* y, hipStream_t s);
int vtd_launch_bottleneck128_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                      const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp, void* scratch,
                                      float* dx, float* dxscale, hipStream_t s);
int64_t vtd_bottleneck64_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_bottleneck64_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                    void* ws, void* y, hipStream_t s);
int vtd_launch_bottleneck64_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                     const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp, void* scratch,
                                     float* dx, float* dxscale, hipStream_t s);
int vtd_launch_fpn_unpack_tap_grad(const float* g, const float* sc, int n, int channels, int H, int W, float* out, hipStream_t s);
int vtd_launch_dbhead_backward(const void* feats, int n, int H, int W, const vtd_dbhead_params* params, int training, const void* ws,
                               const float* prob, const float* thresh, const float* gprob, const float* gthresh, const vtd_dbhead_params* grads,
                               void* scratch, hipStream_t s);

namespace vtd {

using StateDict = std::map<std::string, std::vector<float>>;

struct DeviceArena {
    std::vector<void*> blocks;
    size_t total = 0;
    int alloc(void** out, size_t bytes, bool zero) {
        void* p = nullptr;
        bytes = (bytes + 255) & ~size_t(255);
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return -(int)e;
        if (zero) {
            e = hipMemset(p, 0, bytes);
            if (e != hipSuccess) return -(int)e;
        }
        blocks.push_back(p);
        total += bytes;
        *out = p;
        return 0;
    }
    ~DeviceArena() {
        for (void* p : blocks) (void)hipFree(p);
    }
};

static TensorDesc make_desc(int n, int h, int w, int c, int ring, int ring_br) {
    TensorDesc t;
    t.ptr = nullptr;
    t.n = n; t.h = h; t.w = w; t.c = c; t.ring = ring;
    t.hp = h + ring + ring_br;
    t.wp = w + ring + ring_br;
    return t;
}

struct Op {
    enum Kind { CONV, POOL, FINAL, STEMPOOL, HEADTAIL, BORDER } kind;  // BORDER: border-class tiles of the composed head entry in the slot before it, run iff that slot took the halo-plane kernel
    ConvOp conv;
    TensorDesc pin, pout;
    int pk[6] = {0, 0, 0, 0, 0, 0};  // kh,kw,sh,sw,ph,pw
    const float* fw = nullptr;
    float fbias = 0.f;
    int final_slot = 0;  // 0 = probability, 1 = threshold
    const half_t* spw = nullptr;  // STEMPOOL: fragment-ordered folded stem weights, bias
    const float* spb = nullptr;
    const half_t* htw1 = nullptr;  // HEADTAIL: fragment-ordered ConvT1 / ConvT2 weights
    const half_t* htw2 = nullptr;
};

// ---- Pillow resample coefficient tables (8-bit path, bilinear filter with antialias support scaling)
struct ResampleAxis {
    int ksize = 0;
    std::vector<int> bounds, kk;
};
static ResampleAxis pillow_axis(int in_size, int out_size) {
    ResampleAxis a;
    const double scale = (double)in_size / out_size;
    const double fscale = scale < 1.0 ? 1.0 : scale;
    const double support = fscale;  // bilinear support 1.0 * filterscale
    a.ksize = (int)std::ceil(support) * 2 + 1;
    a.bounds.assign(2 * (size_t)out_size, 0);
    a.kk.assign((size_t)out_size * a.ksize, 0);
    std::vector<double> pre(a.ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale, ss = 1.0 / fscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0) t = -t;
            const double wv = t < 1.0 ? 1.0 - t : 0.0;
            pre[x] = wv;
            ww += wv;
        }
        for (int x = 0; x < xmax; ++x) {
            const double v = ww != 0.0 ? pre[x] / ww : pre[x];
            a.kk[(size_t)xx * a.ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << 22)) : (int)(0.5 + v * (1 << 22));
        }
        a.bounds[2 * xx] = xmin;
        a.bounds[2 * xx + 1] = xmax;
    }
    return a;
}

struct PreTables {
    int *xb = nullptr, *xk = nullptr, *yb = nullptr, *yk = nullptr;
    int ksx = 0, ksy = 0, max_rows = 0;
};

// what both model handles share: the ingested state dict, the device arena and the kernel-selection table (conv_select.h)
struct ModelBase : TuningTable {
    StateDict sd;
    DeviceArena arena;
    int alloc_tensor(TensorDesc& t) {
        void* p = nullptr;
        int rc = arena.alloc(&p, (size_t)tensor_elems(t) * sizeof(half_t), true);
        t.ptr = (half_t*)p;
        return rc;
    }
    const std::vector<float>* get(const std::string& k, size_t numel) const {
        auto it = sd.find(k);
        if (it == sd.end() || it->second.size() != numel) return nullptr;
        return &it->second;
    }
};

}  // namespace vtd

using namespace vtd;

struct vtd_detector : vtd::ModelBase {
    std::string backbone;
    int max_batch = 0;
    bool finalized = false;
    std::vector<Op> ops;
    TensorDesc input;
    std::map<std::string, TensorDesc> taps;
    std::map<std::pair<int, int>, PreTables> pre;
    int64_t macs = 0;
    float* final_out[2] = {nullptr, nullptr};
    std::map<int, std::vector<int>> tuned;  // batch size -> tile config per op (-1 = heuristic)
    bool head_tail_kernel = true;  // dedicated persistent kernel for ConvT+BN+ReLU+ConvT+sigmoid (0: generic conv, 64x256 tile)
    bool fuse_stem_pool = true;  // conv7x7/s2 + BN + ReLU + maxpool3x3/s2 in one kernel (the 320x320x64 map is never written)
    bool fuse_fpn_head = true;  // compose FPN lateral(C2) + top-down add + P2 smooth + head conv into one classed conv
    bool fuse_downsample = true;  // a downsample block's 1x1 projection rides in the block's last conv as extra K-steps (attach_second_segment)
    size_t pool_ops = 0;  // ops up to and including the one that writes the pooled stem output (vtd_detector_forward_pool)
    size_t c2_ops = 0;  // ops up to and including the one that writes C2, the first residual stage's output (vtd_detector_forward_c2)
    size_t trunk_ops = 0;  // ops up to and including the last residual stage (vtd_detector_forward_trunk)
    size_t p2_ops = 0;  // unfused graph: ops up to and including the one that writes P2 (vtd_detector_forward_features)
    // optional per-op HIP-event timing (bench / roofline accounting)
    bool profiling = false;
    int prof_only = -1;  // >= 0: only this launch slot is bracketed with events
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev_spans;  // op index -> (start, stop)
    std::vector<double> prof_ms;
    std::vector<int64_t> prof_calls;
    std::vector<double> prof_macs;  // algorithmic MACs issued per op (accumulated)
    hipEvent_t take_event() {
        if (ev_used == ev_pool.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            ev_pool.push_back(e);
        }
        return ev_pool[ev_used++];
    }
    ~vtd_detector() {
        for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    }
};


struct vtd_recognizer : vtd::ModelBase {
    int vocab = 0, max_crops = 0;
    bool finalized = false;
    bool fuse_pools = true;       // the max-pools behind conv2 / conv4 / conv6 ride in those convolutions' epilogues (0: maxpool_kernel launches)
    uint8_t* resized = nullptr;   // [D,32,128,3] K6 output
    half_t* w1 = nullptr;         // conv1 fp16 [64][32] (K = 27 padded)
    float* b1 = nullptr;          // [64]
    TensorDesc t1;
    std::vector<Op> ops;          // conv2 .. conv7 with their pools
    TensorDesc t7, h0, h1;
    ConvOp xs_gemm[2], cls_gemm;
    half_t* whh[2] = {nullptr, nullptr};
    half_t* xs = nullptr;         // [D*31, 2048] fp16 gate pre-activations x W_ih^T + b
    float* logits_pad = nullptr;  // [D*31, 128]
    std::map<std::string, TensorDesc> taps;
    int64_t macs = 0;
    std::map<int, std::vector<int>> tuned;  // crop count bucket -> config per conv launch (ops..., xs0, xs1, cls)
};

namespace vtd {

struct Fold {
    std::vector<double> scale, shift;  // y = conv*scale + shift
};

// fp16 weight of a folded double product: rounded to float, then to half, as the fused stem+pool packing (which goes
// through a float array) and the test references do.  The float is materialised on purpose: written as one expression,
// the x86 backend may fold the two conversions into a single double -> half rounding, which differs from the two-step
// one whenever the float lands exactly halfway between two fp16 values (one stem weight of a calibrated checkpoint did).
static inline half_t half_of(double v) {
    volatile float f = (float)v;
    return (half_t)f;
}

// BatchNorm (eval) folded with an optional conv bias: y = (conv + b - mean) * g/sqrt(var+eps) + beta
static int fold_bn(const ModelBase* d, const std::string& bn, const std::string& bias_key, int cout, Fold& f) {
    f.scale.assign(cout, 1.0);
    f.shift.assign(cout, 0.0);
    const std::vector<float>* b = nullptr;
    if (!bias_key.empty()) {
        b = d->get(bias_key, cout);
        if (!b) return ERR_MISSING_KEY;
    }
    if (!bn.empty()) {
        auto g = d->get(bn + ".weight", cout), be = d->get(bn + ".bias", cout), mu = d->get(bn + ".running_mean", cout),
             var = d->get(bn + ".running_var", cout);
        if (!g || !be || !mu || !var) return ERR_MISSING_KEY;
        for (int c = 0; c < cout; ++c) {
            const double s = (double)(*g)[c] / std::sqrt((double)(*var)[c] + 1e-5);
            f.scale[c] = s;
            f.shift[c] = (double)(*be)[c] + ((b ? (double)(*b)[c] : 0.0) - (double)(*mu)[c]) * s;
        }
    } else if (b) {
        for (int c = 0; c < cout; ++c) f.shift[c] = (*b)[c];
    }
    return 0;
}

static int upload(DeviceArena& arena, const void* host, size_t bytes, void** dev) {
    int rc = arena.alloc(dev, bytes, false);
    if (rc) return rc;
    hipError_t e = hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : -(int)e;
}

// Host copy of a packed conv (build_conv with `keep`): what attach_second_segment concatenates.
struct HostConv {
    std::vector<half_t> w;     // [cout_pad][K]
    std::vector<float> bias;   // [cout_pad]
    int K = 0, cout_pad = 0;
    bool host_only = false;    // in: do not upload (the op only exists as a second K segment of another one)
};

// Generic conv: weights [cout, cin, kh, kw]; K order (r, s, c) over the input's channel stride.
static int build_conv(ModelBase* d, ConvOp& op, const TensorDesc& in, TensorDesc& out, const std::string& wkey,
                      const Fold& f, int cin, int cout, int kh, int kw, int stride, int pad, int flags, HostConv* keep = nullptr) {
    auto w = d->get(wkey, (size_t)cout * cin * kh * kw);
    if (!w) return ERR_MISSING_KEY;
    if (in.c != cin || (cin & 63) || in.ring < pad) return ERR_GEOMETRY;
    const int ho = (in.h + 2 * pad - kh) / stride + 1, wo = (in.w + 2 * pad - kw) / stride + 1;
    if (out.h != ho || out.w != wo || out.c != cout) return ERR_GEOMETRY;
    const int K = kh * kw * cin;
    const int cout_pad = (cout + 63) / 64 * 64;
    std::vector<half_t> wp((size_t)cout_pad * K, (half_t)0.f);
    for (int co = 0; co < cout; ++co)
        for (int c = 0; c < cin; ++c)
            for (int r = 0; r < kh; ++r)
                for (int s = 0; s < kw; ++s)
                    wp[(size_t)co * K + (size_t)(r * kw + s) * cin + c] =
                        half_of((double)(*w)[(((size_t)co * cin + c) * kh + r) * kw + s] * f.scale[co]);
    std::vector<float> bias(cout_pad, 0.f);
    for (int co = 0; co < cout; ++co) bias[co] = (float)f.shift[co];
    // cin % 64 == 0: a K-step never straddles two taps
    op.cin_steps = cin / 64; op.kw = kw; op.s_step = in.c; op.r_step = in.wp * in.c; op.k_hi_step = 32;
    int rc;
    if (!keep || !keep->host_only) {
        if ((rc = upload(d->arena, wp.data(), wp.size() * sizeof(half_t), (void**)&op.w))) return rc;
        if ((rc = upload(d->arena, bias.data(), bias.size() * sizeof(float), (void**)&op.bias))) return rc;
    }
    if (keep) { keep->w = wp; keep->bias = bias; keep->K = K; keep->cout_pad = cout_pad; }
    op.in = in; op.out = out; op.K = K; op.cout = cout; op.cout_pad = cout_pad; op.stride = stride;
    op.in_y0 = in.ring - pad; op.in_x0 = in.ring - pad; op.flags = flags; op.ho = ho; op.wo = wo;
    op.macs_per_image = (int64_t)ho * wo * cout * K;
    // last tap of the last output pixel must be inside the padded input
    if ((ho - 1) * stride + op.in_y0 + kh - 1 >= in.hp || (wo - 1) * stride + op.in_x0 + kw - 1 >= in.wp) return ERR_GEOMETRY;
    return 0;
}

// Folds a 1x1 convolution of a second tensor into `op` as extra K-steps (conv_igemm.hip DUAL):
//     op(in) + second(in2)  =  [W_op | W_second] * [im2col(in) ; in2 at (oy * mul >> shr, ox * mul >> shr)],   bias = b_op + b_second
// -- the residual branch's projection of a ResNet downsample block (text_detector.py:17-19 -> torchvision BasicBlock / Bottleneck
// `downsample`: 1x1 conv stride s + BN, added before the block's last ReLU; mul = s) or a coarser pyramid level's lateral (nearest-2x
// up-sampling = shr 1).  One launch less, and the projected map is never written or read back; the sum is formed in the fp32
// accumulators, i.e. WITHOUT the fp16 rounding of the projected map the two-launch path has (closer to the fp32 reference).
static int attach_second_segment(ModelBase* d, ConvOp& op, const HostConv& first, const ConvOp& sec_op, const HostConv& second,
                                 int mul, int shr) {
    if (first.cout_pad != second.cout_pad || first.K != op.K || second.K != sec_op.K || sec_op.kw != 1 || sec_op.K != sec_op.cin_steps * 64 ||
        sec_op.cout != op.cout || sec_op.ho != op.ho || sec_op.wo != op.wo || (first.K & 63) || (second.K & 63))
        return ERR_GEOMETRY;
    if (((op.ho - 1) * mul >> shr) >= sec_op.in.h || ((op.wo - 1) * mul >> shr) >= sec_op.in.w) return ERR_GEOMETRY;
    const int K = first.K + second.K;
    std::vector<half_t> wp((size_t)first.cout_pad * K);
    std::vector<float> bias(first.cout_pad);
    for (int co = 0; co < first.cout_pad; ++co) {
        std::memcpy(&wp[(size_t)co * K], &first.w[(size_t)co * first.K], (size_t)first.K * sizeof(half_t));
        std::memcpy(&wp[(size_t)co * K + first.K], &second.w[(size_t)co * second.K], (size_t)second.K * sizeof(half_t));
        bias[co] = (float)((double)first.bias[co] + (double)second.bias[co]);
    }
    int rc;
    if ((rc = upload(d->arena, wp.data(), wp.size() * sizeof(half_t), (void**)&op.w))) return rc;
    if ((rc = upload(d->arena, bias.data(), bias.size() * sizeof(float), (void**)&op.bias))) return rc;
    op.dual = true;
    op.in2 = sec_op.in; op.in2_mul = mul; op.in2_shr = shr;
    op.seg1_steps = first.K / 64; op.cin_steps2 = second.K / 64;
    op.K = K;
    op.macs_per_image += sec_op.macs_per_image;
    return 0;
}

// Stem: conv 7x7/s2/p3 on the ring-3 NHWC4 input.  K is laid out as 8 kernel rows x (8 taps x 4 ch):
// one kernel row = 64 contiguous bytes of the input, rows 7 / taps 7 / channel 3 carry zero weights.
static int build_stem(ModelBase* d, ConvOp& op, const TensorDesc& in, TensorDesc& out, const std::string& wkey, const Fold& f) {
    auto w = d->get(wkey, (size_t)64 * 3 * 7 * 7);
    if (!w) return ERR_MISSING_KEY;
    if (in.c != 4 || in.ring != 3 || in.hp != in.h + 6 || in.wp != in.w + 6 || out.h != in.h / 2 || out.w != in.w / 2 || out.c != 64)
        return ERR_GEOMETRY;
    const int K = 256;
    std::vector<half_t> wp((size_t)64 * K, (half_t)0.f);
    for (int co = 0; co < 64; ++co)
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 7; ++r)
                for (int s = 0; s < 7; ++s)
                    wp[(size_t)co * K + r * 32 + s * 4 + c] = half_of((double)(*w)[(((size_t)co * 3 + c) * 7 + r) * 7 + s] * f.scale[co]);
    std::vector<float> bias(64);
    for (int co = 0; co < 64; ++co) bias[co] = (float)f.shift[co];
    // one K-step = two kernel rows of 32 elements (8 taps x 4 ch): chunks 4-7 sit one input row below chunks 0-3
    op.cin_steps = 1; op.kw = 1; op.s_step = 0; op.r_step = 2 * in.wp * 4; op.k_hi_step = in.wp * 4;
    int rc;
    if ((rc = upload(d->arena, wp.data(), wp.size() * sizeof(half_t), (void**)&op.w))) return rc;
    if ((rc = upload(d->arena, bias.data(), bias.size() * sizeof(float), (void**)&op.bias))) return rc;
    op.in = in; op.out = out; op.K = K; op.cout = 64; op.cout_pad = 64; op.stride = 2;
    op.in_y0 = 0; op.in_x0 = 0; op.flags = EPI_RELU; op.ho = out.h; op.wo = out.w;
    op.macs_per_image = (int64_t)out.h * out.w * 64 * 147;
    if ((out.h - 1) * 2 + 7 >= in.hp || (out.w - 1) * 2 + 7 >= in.wp) return ERR_GEOMETRY;
    return 0;
}

// ConvTranspose2d(cin -> cout, k=2, s=2), weights [cin, cout, 2, 2]: GEMM with N = 4*cout and a pixel-shuffle store.
static int build_convt(ModelBase* d, ConvOp& op, const TensorDesc& in, TensorDesc& out, const std::string& wkey, const Fold& f,
                       int cin, int cout, int flags, std::vector<half_t>* host_w = nullptr) {
    auto w = d->get(wkey, (size_t)cin * cout * 4);
    if (!w) return ERR_MISSING_KEY;
    if (in.c != cin || (cin & 63) || out.h != 2 * in.h || out.w != 2 * in.w || out.c != cout || (cout & 15)) return ERR_GEOMETRY;
    const int K = cin, N = 4 * cout, cout_pad = (N + 63) / 64 * 64;
    std::vector<half_t> wp((size_t)cout_pad * K, (half_t)0.f);
    std::vector<float> bias(cout_pad, 0.f);
    for (int blk = 0; blk < 4; ++blk)
        for (int co = 0; co < cout; ++co) {
            const int nrow = blk * cout + co;
            bias[nrow] = (float)f.shift[co];
            for (int ci = 0; ci < cin; ++ci)
                wp[(size_t)nrow * K + ci] = half_of((double)(*w)[((size_t)ci * cout + co) * 4 + blk] * f.scale[co]);
        }
    op.cin_steps = K / 64; op.kw = 1; op.s_step = 0; op.r_step = 0; op.k_hi_step = 32;
    int rc;
    if ((rc = upload(d->arena, wp.data(), wp.size() * sizeof(half_t), (void**)&op.w))) return rc;
    if ((rc = upload(d->arena, bias.data(), bias.size() * sizeof(float), (void**)&op.bias))) return rc;
    if (host_w) *host_w = wp;
    op.in = in; op.out = out; op.K = K; op.cout = N; op.cout_pad = cout_pad; op.stride = 1;
    op.in_y0 = in.ring; op.in_x0 = in.ring; op.flags = flags | EPI_PIXEL_SHUFFLE; op.ps_cout = cout;
    op.ho = in.h; op.wo = in.w;
    op.macs_per_image = (int64_t)in.h * in.w * N * K;
    return 0;
}


// ------------------------------------------------------------------------------------------------
// Algebraic fusion of the FPN top and the DB-head entry.  Between C2 / L3 and the head's BatchNorm+ReLU the reference
// graph is linear:   L2 = Wl*C2 + bl + up2(L3);  P2 = smooth3x3(L2) + bs;  h = head3x3(P2) + bh   (zero padding at each conv)
// so   h[p] = bias(p) + sum_{u in 5x5} (Wc[u] Wl) C2[p+u] + sum_{u in 5x5} Wc[u] up2(L3)[p+u],   Wc[u] = sum_{t+s=u} Wh[t] Ws[s].
// The up-sampled term collapses onto the 3x3 neighbourhood of L3 around (y>>1, x>>1) with weights that depend on the
// pixel's parity; the zero padding of P2 makes Wc (and the bias) depend on which head taps are inside the image.  That
// gives 16 weight classes (4 row kinds x 4 column kinds) and 25 bias classes; tiles are built from a per-image pixel list so
// that every tile is of one class.  K = 25*Cin(C2) + 9*256 and N = 64: for R18 3904*64 MACs per pixel instead of
// 64*256 + 2304*256 + 2304*64 -- the 256-wide P2 map is never formed.
struct ComposedHeadEntry {
    std::vector<half_t> w;      // [16][64][K]
    std::vector<float> bias;    // [25][64]
    int K = 0;
};

static int compose_head_entry(const ModelBase* d, const std::string& hp, int c2ch, ComposedHeadEntry& out) {
    auto Wl = d->get("fpn.inner_blocks.3.weight", (size_t)256 * c2ch), bl = d->get("fpn.inner_blocks.3.bias", 256);
    auto Ws = d->get("fpn.layer_blocks.3.weight", (size_t)256 * 256 * 9), bs = d->get("fpn.layer_blocks.3.bias", 256);
    auto Wh = d->get(hp + "0.weight", (size_t)64 * 256 * 9), bh = d->get(hp + "0.bias", 64);
    if (!Wl || !bl || !Ws || !bs || !Wh || !bh) return ERR_MISSING_KEY;
    Fold f;
    int rc = fold_bn(d, hp + "1", "", 64, f);  // BN only: the conv bias is part of the composed bias below
    if (rc) return rc;
    const int K = 25 * c2ch + 9 * 256;
    out.K = K;
    // G[t][s] = Wh[t] * Ws[s]   (64 x 256), t,s in 3x3
    std::vector<float> WsT((size_t)9 * 256 * 256), WhT((size_t)9 * 64 * 256);
    for (int m = 0; m < 256; ++m)
        for (int c = 0; c < 256; ++c)
            for (int sI = 0; sI < 9; ++sI) WsT[((size_t)sI * 256 + m) * 256 + c] = (*Ws)[((size_t)m * 256 + c) * 9 + sI];
    for (int o = 0; o < 64; ++o)
        for (int m = 0; m < 256; ++m)
            for (int tI = 0; tI < 9; ++tI) WhT[((size_t)tI * 64 + o) * 256 + m] = (*Wh)[((size_t)o * 256 + m) * 9 + tI];
    std::vector<float> G((size_t)81 * 64 * 256);
    std::vector<double> row(256);
    for (int tI = 0; tI < 9; ++tI)
        for (int sI = 0; sI < 9; ++sI)
            for (int o = 0; o < 64; ++o) {
                std::fill(row.begin(), row.end(), 0.0);
                const float* wh = &WhT[((size_t)tI * 64 + o) * 256];
                for (int m = 0; m < 256; ++m) {
                    const double a = wh[m];
                    const float* ws = &WsT[((size_t)sI * 256 + m) * 256];
                    for (int c = 0; c < 256; ++c) row[c] += a * ws[c];
                }
                float* g = &G[(((size_t)tI * 9 + sI) * 64 + o) * 256];
                for (int c = 0; c < 256; ++c) g[c] = (float)row[c];
            }
    // hb[t][o] = Wh[t] * bs
    std::vector<double> hb(9 * 64, 0.0);
    for (int tI = 0; tI < 9; ++tI)
        for (int o = 0; o < 64; ++o) {
            double a = 0;
            for (int m = 0; m < 256; ++m) a += (double)WhT[((size_t)tI * 64 + o) * 256 + m] * (*bs)[m];
            hb[tI * 64 + o] = a;
        }
    auto tvalid = [](int cls, int t) { return cls == 0 ? t >= 0 : cls == 2 ? t <= 0 : true; };  // cls: 0 first row/col, 1 middle, 2 last
    out.w.assign((size_t)16 * 64 * K, (half_t)0.f);
    out.bias.assign(25 * 64, 0.f);
    std::vector<float> Wc((size_t)25 * 64 * 256);
    std::vector<double> wb((size_t)9 * 25 * 64, 0.0);  // [class][u][o] = Wc_class[u] * bl
    for (int cy = 0; cy < 3; ++cy)
        for (int cx = 0; cx < 3; ++cx) {
            std::fill(Wc.begin(), Wc.end(), 0.f);
            for (int ty = -1; ty <= 1; ++ty)
                for (int tx = -1; tx <= 1; ++tx) {
                    if (!tvalid(cy, ty) || !tvalid(cx, tx)) continue;
                    for (int sy = -1; sy <= 1; ++sy)
                        for (int sx = -1; sx <= 1; ++sx) {
                            const int u = (ty + sy + 2) * 5 + (tx + sx + 2);
                            const float* g = &G[((size_t)((ty + 1) * 3 + tx + 1) * 9 + (sy + 1) * 3 + sx + 1) * 64 * 256];
                            float* wc = &Wc[(size_t)u * 64 * 256];
                            for (size_t i = 0; i < (size_t)64 * 256; ++i) wc[i] += g[i];
                        }
                }
            const int cls = cy * 3 + cx;
            for (int u = 0; u < 25; ++u)
                for (int o = 0; o < 64; ++o) {
                    double a = 0;
                    const float* wc = &Wc[((size_t)u * 64 + o) * 256];
                    for (int c = 0; c < 256; ++c) a += (double)wc[c] * (*bl)[c];
                    wb[((size_t)cls * 25 + u) * 64 + o] = a;
                }
            // C2 part of this class: Wc[u] * Wl  -> [25][64][c2ch]
            std::vector<float> wc2((size_t)25 * 64 * c2ch);
            std::vector<double> r2(c2ch);
            for (int u = 0; u < 25; ++u)
                for (int o = 0; o < 64; ++o) {
                    std::fill(r2.begin(), r2.end(), 0.0);
                    const float* wc = &Wc[((size_t)u * 64 + o) * 256];
                    for (int c = 0; c < 256; ++c) {
                        const double a = wc[c];
                        const float* wl = &(*Wl)[(size_t)c * c2ch];
                        for (int k = 0; k < c2ch; ++k) r2[k] += a * wl[k];
                    }
                    for (int k = 0; k < c2ch; ++k) wc2[((size_t)u * 64 + o) * c2ch + k] = (float)r2[k];
                }
            // every (row kind, column kind) combo that uses this class: kinds 0:(first,even) 1:(mid,even) 2:(mid,odd) 3:(last,odd)
            for (int yk = 0; yk < 4; ++yk)
                for (int xk = 0; xk < 4; ++xk) {
                    const int ycls = yk == 0 ? 0 : yk == 3 ? 2 : 1, xcls = xk == 0 ? 0 : xk == 3 ? 2 : 1;
                    if (ycls != cy || xcls != cx) continue;
                    const int a = yk >= 2 ? 1 : 0, b = xk >= 2 ? 1 : 0;
                    half_t* dst = &out.w[(size_t)(yk * 4 + xk) * 64 * K];
                    for (int o = 0; o < 64; ++o) {
                        const double sc = f.scale[o];
                        for (int u = 0; u < 25; ++u)
                            for (int k = 0; k < c2ch; ++k)
                                dst[(size_t)o * K + (size_t)u * c2ch + k] = half_of(sc * wc2[((size_t)u * 64 + o) * c2ch + k]);
                        // L3 part: window offset uy lands on L3 row floor((a+uy)/2) (relative to y>>1), likewise columns
                        std::vector<double> acc((size_t)9 * 256, 0.0);
                        for (int uy = -2; uy <= 2; ++uy)
                            for (int ux = -2; ux <= 2; ++ux) {
                                const int i = (a + uy + 2) / 2 - 1 + 1, j = (b + ux + 2) / 2 - 1 + 1;  // floor((a+uy)/2) + 1 in 0..2
                                const float* wc = &Wc[((size_t)((uy + 2) * 5 + ux + 2) * 64 + o) * 256];
                                double* ac = &acc[(size_t)(i * 3 + j) * 256];
                                for (int c = 0; c < 256; ++c) ac[c] += wc[c];
                            }
                        for (int ij = 0; ij < 9; ++ij)
                            for (int c = 0; c < 256; ++c)
                                dst[(size_t)o * K + (size_t)25 * c2ch + (size_t)ij * 256 + c] = half_of(sc * acc[(size_t)ij * 256 + c]);
                    }
                }
        }
    // bias classes: y5/x5 in {0: first, 1: second, 2: interior, 3: second-to-last, 4: last}
    auto inside = [](int c5, int u) { return c5 == 0 ? u >= 0 : c5 == 1 ? u >= -1 : c5 == 3 ? u <= 1 : c5 == 4 ? u <= 0 : true; };
    for (int y5 = 0; y5 < 5; ++y5)
        for (int x5 = 0; x5 < 5; ++x5) {
            const int cy = y5 == 0 ? 0 : y5 == 4 ? 2 : 1, cx = x5 == 0 ? 0 : x5 == 4 ? 2 : 1;
            for (int o = 0; o < 64; ++o) {
                double a = (*bh)[o];
                for (int ty = -1; ty <= 1; ++ty)
                    for (int tx = -1; tx <= 1; ++tx)
                        if (tvalid(cy, ty) && tvalid(cx, tx)) a += hb[((ty + 1) * 3 + tx + 1) * 64 + o];
                for (int uy = -2; uy <= 2; ++uy)
                    for (int ux = -2; ux <= 2; ++ux)
                        if (inside(y5, uy) && inside(x5, ux)) a += wb[((size_t)(cy * 3 + cx) * 25 + (uy + 2) * 5 + ux + 2) * 64 + o];
                out.bias[(y5 * 5 + x5) * 64 + o] = (float)(f.scale[o] * a + f.shift[o]);
            }
        }
    return 0;
}

// per-image pixel list for the classed op: 16 (row kind x column kind) groups, each padded to whole 128-row tiles.
// `tile_combo` then lists the tiles in EXECUTION order as (weight class | pixel-list chunk << 8): the four parity classes
// of the image interior are interleaved chunk by chunk, so the tiles that gather the same rows of C2 / L3 run back to
// back on one XCD and its L2 serves the 4x overlap (class-major order re-streamed the whole image once per class).
static void build_pixel_list(int h, int w, int bm, std::vector<uint32_t>& plist, std::vector<int>& tile_combo) {
    auto kind_values = [](int n, int kind) {
        std::vector<int> v;
        if (kind == 0) v.push_back(0);
        else if (kind == 3) v.push_back(n - 1);
        else for (int i = (kind == 1 ? 2 : 1); i <= n - 2; i += 2) v.push_back(i);
        return v;
    };
    plist.clear();
    tile_combo.clear();
    std::vector<std::vector<int>> chunks(16);  // per combo: its pixel-list chunk indices, in raster order
    for (int yk = 0; yk < 4; ++yk)
        for (int xk = 0; xk < 4; ++xk) {
            const std::vector<int> ys = kind_values(h, yk), xs = kind_values(w, xk);
            size_t cnt = 0;
            const size_t first_chunk = plist.size() / bm;
            for (int y : ys)
                for (int x : xs) { plist.push_back((uint32_t)y | ((uint32_t)x << 16)); ++cnt; }
            while (cnt % bm) { plist.push_back(0xffffffffu); ++cnt; }
            for (size_t t = 0; t < cnt / bm; ++t) chunks[yk * 4 + xk].push_back((int)(first_chunk + t));
        }
    const int interior[4] = {1 * 4 + 1, 1 * 4 + 2, 2 * 4 + 1, 2 * 4 + 2};  // (mid even|odd rows) x (mid even|odd columns)
    size_t longest = 0;
    for (int c : interior) longest = std::max(longest, chunks[c].size());
    for (size_t t = 0; t < longest; ++t)
        for (int c : interior)
            if (t < chunks[c].size()) tile_combo.push_back(c | (chunks[c][t] << 8));
    for (int c = 0; c < 16; ++c) {
        bool is_interior = false;
        for (int q : interior) is_interior |= q == c;
        if (!is_interior)
            for (int ch : chunks[c]) tile_combo.push_back(c | (ch << 8));
    }
}

static int build_classed_head_entry(vtd_detector* d, ConvOp& op, const TensorDesc& c2, const TensorDesc& l3, TensorDesc& out,
                                    const std::string& hp) {
    if (c2.ring < 2 || l3.ring < 1 || (c2.c & 63) || l3.c != 256 || c2.h != 2 * l3.h || c2.w != 2 * l3.w || (c2.h & 1) || (c2.w & 1) ||
        out.h != c2.h || out.w != c2.w || out.c != 64)
        return ERR_GEOMETRY;
    ComposedHeadEntry ce;
    int rc = compose_head_entry(d, hp, c2.c, ce);
    if (rc) return rc;
    std::vector<uint32_t> plist;
    std::vector<int> tile_combo;
    build_pixel_list(c2.h, c2.w, 128, plist, tile_combo);
    std::vector<uint32_t> plist_b;
    std::vector<int> tile_combo_b;
    build_pixel_list(c2.h, c2.w, 256, plist_b, tile_combo_b);
    void *pl = nullptr, *tc = nullptr, *bt = nullptr, *plb = nullptr, *tcb = nullptr;
    if ((rc = upload(d->arena, plist_b.data(), plist_b.size() * sizeof(uint32_t), &plb))) return rc;
    if ((rc = upload(d->arena, tile_combo_b.data(), tile_combo_b.size() * sizeof(int), &tcb))) return rc;
    op.plist_b = (const uint32_t*)plb;
    op.tile_combo_b = (const int*)tcb;
    op.tiles_per_img_b = (int)tile_combo_b.size();
    if ((rc = upload(d->arena, ce.w.data(), ce.w.size() * sizeof(half_t), (void**)&op.w))) return rc;
    if ((rc = upload(d->arena, ce.bias.data(), ce.bias.size() * sizeof(float), &bt))) return rc;
    if ((rc = upload(d->arena, plist.data(), plist.size() * sizeof(uint32_t), &pl))) return rc;
    if ((rc = upload(d->arena, tile_combo.data(), tile_combo.size() * sizeof(int), &tc))) return rc;
    {   // interior classes on the halo-plane kernel: per-class step tables; border classes keep their 128-row tiles
        const int nch1 = c2.c / 64, nsteps = 25 * nch1 + 36;
        std::vector<int> steps((size_t)4 * nsteps * 2);
        for (int q = 0; q < 4; ++q)
            if (vtd_head_entry_halo_steps(q >> 1, q & 1, nch1, &steps[(size_t)q * nsteps * 2]) != nsteps) return ERR_GEOMETRY;
        std::vector<int> border;
        for (int e : tile_combo) {
            const int cl = e & 0xff;
            if (cl != 5 && cl != 6 && cl != 9 && cl != 10) border.push_back(e);
        }
        void *st = nullptr, *bd = nullptr;
        if ((rc = upload(d->arena, steps.data(), steps.size() * sizeof(int), &st))) return rc;
        if ((rc = upload(d->arena, border.data(), border.size() * sizeof(int), &bd))) return rc;
        op.he_steps = (const int*)st; op.he_nsteps = nsteps;
#ifdef VTD_EXPERIMENTAL_CANDIDATES
        if (25 * c2.c + 9 * 256 <= 0xffff) {  // half-halo kernel: schedules derived from the same step tables (16-bit weight column offsets)
            std::vector<int> sched((size_t)4 * nsteps * 4);
            bool ok = true;
            for (int q = 0; q < 4 && ok; ++q)
                ok = vtd_head_entry_half_schedule(&steps[(size_t)q * nsteps * 2], nsteps, &sched[(size_t)q * nsteps * 4]) == 0;
            void* sd = nullptr;
            if (ok) {
                if ((rc = upload(d->arena, sched.data(), sched.size() * sizeof(int), &sd))) return rc;
                op.hh_sched = (const int*)sd;
            }
        }
#endif
        op.tile_combo_border = (const int*)bd; op.tiles_border = (int)border.size();
#ifdef VTD_EXPERIMENTAL_CANDIDATES
        {   // pair kernel (head_entry_pair.hip): half-step tables + halo prefetch plans; only where its LDS budget holds (C2 of 64 channels)
            const int nh = 25 * (c2.c / 32) + 72;
            if (c2.c == 64) {
                std::vector<int> hs((size_t)4 * nh * 2), plan((size_t)4 * nh);
                bool ok = true;
                for (int q = 0; q < 4 && ok; ++q)
                    ok = vtd_head_entry_pair_tables(q >> 1, q & 1, c2.c, &hs[(size_t)q * nh * 2], &plan[(size_t)q * nh]) == nh;
                if (ok) {
                    void *hsd = nullptr, *pld = nullptr;
                    if ((rc = upload(d->arena, hs.data(), hs.size() * sizeof(int), &hsd))) return rc;
                    if ((rc = upload(d->arena, plan.data(), plan.size() * sizeof(int), &pld))) return rc;
                    op.hp_half_steps = (const int*)hsd; op.hp_plan = (const int*)pld; op.hp_nh = nh;
                }
            }
        }
#endif
    }
    op.bias = (float*)bt;  // first class doubles as the (unused) flat bias
    op.bias_tab = (const float*)bt;
    op.plist = (const uint32_t*)pl;
    op.tile_combo = (const int*)tc;
    op.tiles_per_img = (int)tile_combo.size();
    op.in = c2; op.in2 = l3; op.out = out;
    op.K = ce.K; op.cout = 64; op.cout_pad = 64; op.stride = 1;
    op.in_y0 = c2.ring - 2; op.in_x0 = c2.ring - 2;
    op.cin_steps = c2.c / 64; op.kw = 5; op.s_step = c2.c; op.r_step = c2.wp * c2.c; op.k_hi_step = 32;
    op.seg1_steps = 25 * (c2.c / 64);
    op.cin_steps2 = 4; op.kw2 = 3; op.s_step2 = 256; op.r_step2 = l3.wp * 256;
    op.flags = EPI_RELU; op.ho = c2.h; op.wo = c2.w; op.img_h = c2.h; op.img_w = c2.w;
    op.macs_per_image = (int64_t)c2.h * c2.w * 64 * ce.K;
    return 0;
}

static const int kStageWidth[4] = {64, 128, 256, 512};

static int build_detector_graph(vtd_detector* d) {
    const bool r50 = d->backbone == "resnet50";
    const int counts18[4] = {2, 2, 2, 2}, counts50[4] = {3, 4, 6, 3};
    const int* counts = r50 ? counts50 : counts18;
    const int B = d->max_batch;
    int rc;
    auto new_tensor = [&](int h, int w, int c, TensorDesc& t, int ring = 1) {
        t = make_desc(B, h, w, c, ring, ring);
        return d->alloc_tensor(t);
    };
    const bool fuse = d->fuse_fpn_head;
    auto push_conv = [&](const ConvOp& c) {
        Op o;
        o.kind = Op::CONV;
        o.conv = c;
        d->ops.push_back(o);
        d->macs += c.macs_per_image;
    };

    d->input = make_desc(B, 640, 640, 4, 3, 3);
    if ((rc = d->alloc_tensor(d->input))) return rc;
    d->taps["input"] = d->input;

    // stem + maxpool
    TensorDesc stem, x;
    if ((rc = new_tensor(160, 160, 64, x))) return rc;
    if (d->fuse_stem_pool) {
        Fold f;
        if ((rc = fold_bn(d, "backbone.1", "", 64, f))) return rc;
        auto w = d->get("backbone.0.weight", (size_t)64 * 3 * 7 * 7);
        if (!w) return ERR_MISSING_KEY;
        std::vector<float> wf(w->size());
        for (int co = 0; co < 64; ++co)
            for (int k = 0; k < 147; ++k) wf[(size_t)co * 147 + k] = (float)((double)(*w)[(size_t)co * 147 + k] * f.scale[co]);
        std::vector<half_t> packed((size_t)7 * 4 * 64 * 8);
        vtd_stem_pool_pack_weights(wf.data(), packed.data());
        std::vector<float> bias(64);
        for (int co = 0; co < 64; ++co) bias[co] = (float)f.shift[co];
        Op o;
        o.kind = Op::STEMPOOL;
        o.pin = d->input; o.pout = x;
        if ((rc = upload(d->arena, packed.data(), packed.size() * sizeof(half_t), (void**)&o.spw))) return rc;
        if ((rc = upload(d->arena, bias.data(), bias.size() * sizeof(float), (void**)&o.spb))) return rc;
        o.conv.macs_per_image = (int64_t)320 * 320 * 64 * 147;
        d->ops.push_back(o);
        d->macs += o.conv.macs_per_image;
    } else {
        if ((rc = new_tensor(320, 320, 64, stem))) return rc;
        Fold f;
        if ((rc = fold_bn(d, "backbone.1", "", 64, f))) return rc;
        ConvOp c;
        if ((rc = build_stem(d, c, d->input, stem, "backbone.0.weight", f))) return rc;
        push_conv(c);
        d->taps["stem"] = stem;
        Op o;
        o.kind = Op::POOL;
        o.pin = stem; o.pout = x;
        const int pk[6] = {3, 3, 2, 2, 1, 1};
        std::memcpy(o.pk, pk, sizeof(pk));
        d->ops.push_back(o);
    }
    d->taps["pool"] = x;
    d->pool_ops = d->ops.size();

    // residual stages
    TensorDesc tapsC[4];
    int cin = 64;
    for (int st = 0; st < 4; ++st) {
        const int width = kStageWidth[st];
        const int cout = r50 ? width * 4 : width;
        for (int b = 0; b < counts[st]; ++b) {
            const int stride = (b == 0 && st > 0) ? 2 : 1;
            const std::string pre = "backbone." + std::to_string(4 + st) + "." + std::to_string(b);
            const int hin = x.h, hout = hin / stride;
            TensorDesc idt = x;
            const bool project = stride != 1 || cin != cout;
            const bool fold_ds = project && d->fuse_downsample;   // the projection becomes extra K-steps of the block's last conv
            ConvOp ds_op;
            HostConv ds_host;
            if (project) {
                TensorDesc ds;
                if (fold_ds) ds = make_desc(B, hout, hout, cout, 1, 1);   // shape bookkeeping only: the projected map is never formed
                else if ((rc = new_tensor(hout, hout, cout, ds))) return rc;
                Fold f;
                if ((rc = fold_bn(d, pre + ".downsample.1", "", cout, f))) return rc;
                ds_host.host_only = fold_ds;
                if ((rc = build_conv(d, ds_op, x, ds, pre + ".downsample.0.weight", f, cin, cout, 1, 1, stride, 0, 0, &ds_host))) return rc;
                if (!fold_ds) {
                    push_conv(ds_op);
                    idt = ds;
                }
            }
            TensorDesc y;
            if (!r50) {
                TensorDesc t1;
                if ((rc = new_tensor(hout, hout, width, t1))) return rc;
                Fold f1, f2;
                if ((rc = fold_bn(d, pre + ".bn1", "", width, f1))) return rc;
                ConvOp c1;
                if ((rc = build_conv(d, c1, x, t1, pre + ".conv1.weight", f1, cin, width, 3, 3, stride, 1, EPI_RELU))) return rc;
                push_conv(c1);
                if ((rc = new_tensor(hout, hout, width, y, (fuse && st == 0 && b == counts[st] - 1) ? 2 : 1))) return rc;
                if ((rc = fold_bn(d, pre + ".bn2", "", width, f2))) return rc;
                ConvOp c2;
                HostConv h2;
                h2.host_only = fold_ds;
                if ((rc = build_conv(d, c2, t1, y, pre + ".conv2.weight", f2, width, width, 3, 3, 1, 1, fold_ds ? EPI_RELU : (EPI_RELU | EPI_RESIDUAL), &h2))) return rc;
                if (fold_ds) {
                    if ((rc = attach_second_segment(d, c2, h2, ds_op, ds_host, stride, 0))) return rc;
                } else {
                    c2.has_res = true; c2.res = idt; c2.res_shift = 0;
                }
                push_conv(c2);
            } else {
                TensorDesc t1, t2;
                if ((rc = new_tensor(hin, hin, width, t1))) return rc;
                Fold f1, f2, f3;
                if ((rc = fold_bn(d, pre + ".bn1", "", width, f1))) return rc;
                ConvOp c1;
                if ((rc = build_conv(d, c1, x, t1, pre + ".conv1.weight", f1, cin, width, 1, 1, 1, 0, EPI_RELU))) return rc;
                push_conv(c1);
                if ((rc = new_tensor(hout, hout, width, t2))) return rc;
                if ((rc = fold_bn(d, pre + ".bn2", "", width, f2))) return rc;
                ConvOp c2;
                if ((rc = build_conv(d, c2, t1, t2, pre + ".conv2.weight", f2, width, width, 3, 3, stride, 1, EPI_RELU))) return rc;
                push_conv(c2);
                if ((rc = new_tensor(hout, hout, cout, y, (fuse && st == 0 && b == counts[st] - 1) ? 2 : 1))) return rc;
                if ((rc = fold_bn(d, pre + ".bn3", "", cout, f3))) return rc;
                ConvOp c3;
                HostConv h3;
                h3.host_only = fold_ds;
                if ((rc = build_conv(d, c3, t2, y, pre + ".conv3.weight", f3, width, cout, 1, 1, 1, 0, fold_ds ? EPI_RELU : (EPI_RELU | EPI_RESIDUAL), &h3))) return rc;
                if (fold_ds) {
                    if ((rc = attach_second_segment(d, c3, h3, ds_op, ds_host, stride, 0))) return rc;
                } else {
                    c3.has_res = true; c3.res = idt; c3.res_shift = 0;
                }
                push_conv(c3);
            }
            x = y;
            cin = cout;
        }
        tapsC[st] = x;
        d->taps["c" + std::to_string(st + 2)] = x;
        if (st == 0) d->c2_ops = d->ops.size();
    }
    d->trunk_ops = d->ops.size();

    // FPN, intended wiring: inner[i] on C5,C4,C3,C2; top-down nearest-2x add fused in the epilogue
    TensorDesc last;
    for (int i = 0; i < (fuse ? 3 : 4); ++i) {
        const TensorDesc& feat = tapsC[3 - i];
        TensorDesc lat;
        if ((rc = new_tensor(feat.h, feat.w, 256, lat))) return rc;
        Fold f;
        const std::string k = "fpn.inner_blocks." + std::to_string(i);
        if ((rc = fold_bn(d, "", k + ".bias", 256, f))) return rc;
        ConvOp c;
        if ((rc = build_conv(d, c, feat, lat, k + ".weight", f, feat.c, 256, 1, 1, 1, 0, i ? EPI_RESIDUAL : 0))) return rc;
        if (i) { c.has_res = true; c.res = last; c.res_shift = 1; }
        push_conv(c);
        last = lat;
    }
    TensorDesc p2;
    if (!fuse) {
        if ((rc = new_tensor(160, 160, 256, p2))) return rc;
        Fold f;
        if ((rc = fold_bn(d, "", "fpn.layer_blocks.3.bias", 256, f))) return rc;
        ConvOp c;
        if ((rc = build_conv(d, c, last, p2, "fpn.layer_blocks.3.weight", f, 256, 256, 3, 3, 1, 1, 0))) return rc;
        push_conv(c);
        d->taps["p2"] = p2;
        d->p2_ops = d->ops.size();
    } else if (!d->get("fpn.inner_blocks.3.weight", (size_t)256 * tapsC[0].c) || !d->get("fpn.layer_blocks.3.weight", (size_t)256 * 256 * 9)) {
        return ERR_MISSING_KEY;
    }
    // layer_blocks.0..2 exist in checkpoints but their outputs are dead (text_detector.py:56); still validated
    for (int i = 0; i < 3; ++i) {
        const std::string k = "fpn.layer_blocks." + std::to_string(i);
        if (!d->get(k + ".weight", (size_t)256 * 256 * 9) || !d->get(k + ".bias", 256)) return ERR_MISSING_KEY;
    }

    // DB head branches (probability always; threshold provisioned, run on demand)
    const char* branch[2] = {"head.probability_head.", "head.threshold_head."};
    for (int br = 0; br < 2; ++br) {
        const std::string hp = branch[br];
        TensorDesc h1;
        if ((rc = new_tensor(160, 160, 64, h1))) return rc;
        Fold f1, f2;
        ConvOp c1;
        if (fuse) {
            // lateral(C2) + top-down add + P2 smooth + head conv + BN + ReLU as one classed dual-source conv on C2 and L3
            if ((rc = build_classed_head_entry(d, c1, tapsC[0], last, h1, hp))) return rc;
        } else {
            if ((rc = fold_bn(d, hp + "1", hp + "0.bias", 64, f1))) return rc;
            if ((rc = build_conv(d, c1, p2, h1, hp + "0.weight", f1, 256, 64, 3, 3, 1, 1, EPI_RELU))) return rc;
        }
        if ((rc = fold_bn(d, hp + "4", hp + "3.bias", 64, f2))) return rc;
        // ConvT(64->64)+BN+ReLU and ConvT(64->1)+sigmoid in one launch: the 64x320x320 intermediate never touches HBM
        ConvOp c2;
        TensorDesc h2 = make_desc(B, 320, 320, 64, 1, 1);  // shape bookkeeping only (no allocation)
        std::vector<half_t> w1_host;
        if ((rc = build_convt(d, c2, h1, h2, hp + "3.weight", f2, 64, 64, EPI_RELU, &w1_host))) return rc;
        auto w6 = d->get(hp + "6.weight", 64 * 4), b6 = d->get(hp + "6.bias", 1);
        if (!w6 || !b6) return ERR_MISSING_KEY;
        std::vector<float> wf(4 * 64);
        for (int blk = 0; blk < 4; ++blk)
            for (int ci = 0; ci < 64; ++ci) wf[blk * 64 + ci] = (*w6)[ci * 4 + blk];
        float* wdev = nullptr;
        if ((rc = upload(d->arena, wf.data(), wf.size() * sizeof(float), (void**)&wdev))) return rc;
        c2.flags = EPI_HEAD_FINAL;
        c2.head_w = wdev;
        c2.head_b = (*b6)[0];
        Op o1, o2;
        o1.kind = Op::CONV; o1.conv = c1; o1.final_slot = br;
        o2.kind = Op::FINAL; o2.conv = c2; o2.final_slot = br;
        if (d->head_tail_kernel) {
            std::vector<half_t> p1((size_t)4 * 4 * 2 * 64 * 8), p2((size_t)2 * 64 * 8);
            vtd_head_tail_pack_w1(w1_host.data(), p1.data());
            vtd_head_tail_pack_w2(wf.data(), p2.data());
            if ((rc = upload(d->arena, p1.data(), p1.size() * sizeof(half_t), (void**)&o2.htw1))) return rc;
            if ((rc = upload(d->arena, p2.data(), p2.size() * sizeof(half_t), (void**)&o2.htw2))) return rc;
            o2.kind = Op::HEADTAIL;
        }
        d->ops.push_back(o1);
        if (fuse) {
            Op ob;
            ob.kind = Op::BORDER; ob.conv = c1; ob.final_slot = br;
            ob.conv.macs_per_image = (int64_t)c1.tiles_border * 128 * 64 * c1.K;  // executed work of the border tiles
            d->ops.push_back(ob);
        }
        d->ops.push_back(o2);
        if (br == 0) {
            // macs_per_frame reports the ALGORITHMIC live work of the reference graph, whatever is fused:
            // lateral(C2) 1x1, P2 smooth 3x3 256->256 and head conv 3x3 256->64 count at their reference size
            const int64_t px = (int64_t)160 * 160;
            const int64_t ref_entry = fuse ? px * 256 * tapsC[0].c + px * 256 * 2304 + px * 64 * 2304 : c1.macs_per_image;
            d->macs += ref_entry + c2.macs_per_image + (int64_t)320 * 320 * 4 * 64;
            d->taps["head1"] = h1;
        }
    }
    return 0;
}

// dense NCHW float32 host copy of a ring-padded NHWC fp16 tensor (test taps)
static int read_tensor_nchw(const TensorDesc& t, int n, int creal, float* host_out, hipStream_t stream) {
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return -(int)e;
    std::vector<half_t> tmp((size_t)n * t.hp * t.wp * t.c);
    e = hipMemcpy(tmp.data(), t.ptr, tmp.size() * sizeof(half_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return -(int)e;
    for (int img = 0; img < n; ++img)
        for (int c = 0; c < creal; ++c)
            for (int y = 0; y < t.h; ++y)
                for (int x = 0; x < t.w; ++x)
                    host_out[(((size_t)img * creal + c) * t.h + y) * t.w + x] =
                        (float)tmp[(((size_t)img * t.hp + y + t.ring) * t.wp + x + t.ring) * t.c + c];
    return 0;
}

// Dense layer as a 1x1 convolution over a [rows,1,1,K]-shaped view: weights [N][K] (already in GEMM layout),
// float32 row-major output with leading dimension ldc (LSTM input projections, classifier).
static int build_linear(ModelBase* d, ConvOp& op, const TensorDesc& in, const std::vector<float>& W, const std::vector<float>& bias,
                        int N, int K, void* out_f32, int ldc, int out_flag = EPI_OUT_F32) {
    if (in.c != K || (K & 63) || (int)W.size() != N * K || (int)bias.size() != N || (ldc & 3) || ldc < N) return ERR_GEOMETRY;
    const int cout_pad = (N + 63) / 64 * 64;
    std::vector<half_t> wp((size_t)cout_pad * K, (half_t)0.f);
    for (size_t i = 0; i < (size_t)N * K; ++i) wp[i] = (half_t)W[i];
    std::vector<float> b(cout_pad, 0.f);
    for (int i = 0; i < N; ++i) b[i] = bias[i];
    op.cin_steps = K / 64; op.kw = 1; op.s_step = 0; op.r_step = 0; op.k_hi_step = 32;
    int rc;
    if ((rc = upload(d->arena, wp.data(), wp.size() * sizeof(half_t), (void**)&op.w))) return rc;
    if ((rc = upload(d->arena, b.data(), b.size() * sizeof(float), (void**)&op.bias))) return rc;
    op.in = in; op.out = in; op.K = K; op.cout = N; op.cout_pad = cout_pad; op.stride = 1;
    op.in_y0 = in.ring; op.in_x0 = in.ring; op.flags = out_flag; op.ho = in.h; op.wo = in.w;
    op.out_f32 = out_f32; op.ldc = ldc;
    op.macs_per_image = (int64_t)in.h * in.w * N * K;
    return 0;
}

static bool known_detector_key(const std::string& k) {
    return k.rfind("backbone.", 0) == 0 || k.rfind("fpn.", 0) == 0 || k.rfind("head.", 0) == 0;
}

static int get_pre_tables(vtd_detector* d, int H, int W, PreTables& out) {
    auto key = std::make_pair(H, W);
    auto it = d->pre.find(key);
    if (it != d->pre.end()) {
        out = it->second;
        return 0;
    }
    ResampleAxis ax = pillow_axis(W, 640), ay = pillow_axis(H, 640);
    PreTables t;
    t.ksx = ax.ksize; t.ksy = ay.ksize;
    t.max_rows = vtd_preprocess_max_rows(ay.bounds.data());
    int rc;
    if ((rc = upload(d->arena, ax.bounds.data(), ax.bounds.size() * sizeof(int), (void**)&t.xb))) return rc;
    if ((rc = upload(d->arena, ax.kk.data(), ax.kk.size() * sizeof(int), (void**)&t.xk))) return rc;
    if ((rc = upload(d->arena, ay.bounds.data(), ay.bounds.size() * sizeof(int), (void**)&t.yb))) return rc;
    if ((rc = upload(d->arena, ay.kk.data(), ay.kk.size() * sizeof(int), (void**)&t.yk))) return rc;
    d->pre[key] = t;
    out = t;
    return 0;
}

}  // namespace vtd

extern "C" {

const char* vtd_version(void) {
#ifdef VTD_EXPERIMENTAL_CANDIDATES
    return "vtd_hip 0.3 (gfx950) +experimental";
#else
    return "vtd_hip 0.3 (gfx950)";
#endif
}

const char* vtd_strerror(int code) {
    static thread_local char buf[128];
    switch (code) {
        case 0: return "ok";
        case ERR_ARG: return "invalid argument";
        case ERR_UNKNOWN_KEY: return "unknown state-dict key";
        case ERR_SHAPE: return "tensor has the wrong number of elements";
        case ERR_MISSING_KEY: return "state dict incomplete (missing or mis-sized key)";
        case ERR_NOT_FINALIZED: return "handle not finalized";
        case ERR_BATCH: return "batch exceeds the handle's max_batch";
        case ERR_GEOMETRY: return "layer geometry check failed";
        case ERR_CAPACITY: return "output capacity too small";
        case -2801: return "feature export needs a detector finalized with fuse_fpn_head=0 (the fused head entry never forms P2)";
        case -2802: return "DB head training: invalid argument or shape";
        case -2803: return "DB head training: misaligned buffer";
        case -2901: return "trunk export needs a detector finalized with fuse_fpn_head=0 (the fused graph pads C2 for the composed head entry)";
        case -2902: return "FPN training: invalid argument or shape";
        case -2903: return "FPN training: misaligned buffer";
        case -3001: return "BasicBlock training: invalid argument or unsupported geometry (built: 256 -> 512 stride 2 with even extents, 512 -> 512 stride 1)";
        case -3002: return "BasicBlock training: misaligned buffer";
        case -3003: return "BasicBlock training: the input gradient of the stride-2 block is not built (it needs a strided dgrad)";
        case -3101: return "ResNet block training: invalid argument or unsupported geometry (built: 128 -> 256 and 256 -> 512 stride 2 with even "
                           "extents, 256 -> 256 and 512 -> 512 stride 1)";
        case -3102: return "ResNet block training: misaligned buffer";
        case -3201: return "64-wide block training: invalid argument or unsupported geometry (built: 64 -> 64 stride 1, ResNet-18's layer1)";
        case -3202: return "64-wide block training: misaligned buffer";
        case -3401: return "BasicBlock batch-statistics training: invalid argument or unsupported geometry (built: 256 -> 512 stride 2 with even "
                           "extents, 512 -> 512 stride 1; training = 1 needs n h w >= 2)";
        case -3402: return "BasicBlock batch-statistics training: misaligned buffer";
        case -3403: return "BasicBlock batch-statistics training: the input gradient of the stride-2 block is not built";
        case -3501: return "ResNet block batch-statistics training: invalid argument or unsupported geometry (built: 128 -> 256 and 256 -> 512 "
                           "stride 2 with even extents, 256 -> 256 and 512 -> 512 stride 1; training = 1 needs n h w >= 2)";
        case -3502: return "ResNet block batch-statistics training: misaligned buffer";
        case -3701: return "trunk block batch-statistics training: invalid argument or unsupported geometry (built: 64 -> 128, 128 -> 256 and "
                           "256 -> 512 stride 2 with even extents, 128 -> 128, 256 -> 256 and 512 -> 512 stride 1; training = 1 needs n h w >= 2)";
        case -3702: return "trunk block batch-statistics training: misaligned buffer";
        case -3301: return "stem training: invalid argument or unsupported geometry (built: n >= 1, even image height and width >= 2)";
        case -3302: return "stem training: misaligned buffer";
        case -3801: return "stem batch-statistics training: invalid argument or unsupported geometry (built: n >= 1, even image height and width >= 2; "
                           "eps > 0, training 0 or 1, momentum in [0, 1]; training = 1 needs n hc wc >= 2 conv pixels)";
        case -3802: return "stem batch-statistics training: misaligned buffer";
        case -3901: return "Bottleneck training: invalid argument or unsupported geometry (built: width 512 with 1024 -> 2048 stride 2, even extents "
                           "and a downsample, or 2048 -> 2048 stride 1: ResNet-50's last stage)";
        case -3902: return "Bottleneck training: misaligned buffer";
        case -3903: return "256-wide Bottleneck training: invalid argument or unsupported geometry (built: width 256 with 512 -> 1024 stride 2, even "
                           "extents and a downsample, or 1024 -> 1024 stride 1: ResNet-50's res4)";
        case -3904: return "256-wide Bottleneck training: misaligned buffer";
        case -3905: return "128-wide Bottleneck training: invalid argument or unsupported geometry (built: width 128 with 256 -> 512 stride 2, even "
                           "extents and a downsample, or 512 -> 512 stride 1: ResNet-50's res3)";
        case -3906: return "128-wide Bottleneck training: misaligned buffer";
        case -3907: return "64-wide Bottleneck training: invalid argument or unsupported geometry (built: width 64 at stride 1 with 64 -> 256 and a "
                           "downsample, or 256 -> 256: ResNet-50's res2)";
        case -3908: return "64-wide Bottleneck training: misaligned buffer";
        case -4001: return "Bottleneck batch-statistics training: invalid argument or unsupported geometry (built: width 512 with 1024 -> 2048 stride 2 "
                           "or 2048 -> 2048 stride 1, width 256 with 512 -> 1024 stride 2 or 1024 -> 1024 stride 1, even extents at stride 2: "
                           "ResNet-50's res5 and res4; training 0 or 1, momentum in [0, 1]; training = 1 needs n h w >= 2)";
        case -4002: return "Bottleneck batch-statistics training: misaligned buffer";
        case -3601: return "AdamW step: invalid argument (null or not 4-byte aligned pointer, count < 0, n outside [0, 2^40), non-finite scalar, "
                           "bc2_sqrt <= 0)";
        default: break;
    }
    if (code <= -1000) {
        std::snprintf(buf, sizeof(buf), "vtd validation error %d", code);
        return buf;
    }
    if (code < 0) return hipGetErrorString((hipError_t)(-code));
    return "unknown";
}

// ---- training loss, forward (app/ml/training/trainer.py:48-56 / :66-71: BCELoss + BCELoss + DiceLoss on the detector's two maps)
int64_t vtd_dbloss_workspace_bytes(void) { return vtd_dbloss_ws_bytes(); }

int vtd_dbloss_forward(const float* prob_dev, const float* thresh_dev, const float* prob_target_dev, const float* thresh_target_dev, int64_t numel,
                       float smooth, void* workspace_dev, float* out4_dev, double* sums5_dev, vtd_stream stream) {
    if (!prob_dev || !prob_target_dev || !workspace_dev || !out4_dev || numel <= 0) return ERR_ARG;
    if ((thresh_dev == nullptr) != (thresh_target_dev == nullptr)) return ERR_ARG;
    return vtd_launch_dbloss(prob_dev, thresh_dev, prob_target_dev, thresh_target_dev, numel, smooth, (double*)workspace_dev, out4_dev, sums5_dev,
                             (hipStream_t)stream);
}

int vtd_dbloss_backward(const float* prob_dev, const float* thresh_dev, const float* prob_target_dev, const float* thresh_target_dev, int64_t numel,
                        float smooth, const double* sums5_dev, const float* grad_out4_dev, float* grad_prob_dev, float* grad_thresh_dev,
                        vtd_stream stream) {
    return vtd_launch_dbloss_backward(prob_dev, thresh_dev, prob_target_dev, thresh_target_dev, numel, smooth, sums5_dev, grad_out4_dev,
                                      grad_prob_dev, grad_thresh_dev, (hipStream_t)stream);
}

// ---- validation metrics (trainer.py:83-98): the three integer counts behind sklearn's binary precision / recall / F1
int vtd_binary_counts_accumulate(const float* pred_dev, const float* target_dev, int64_t numel, float threshold, int64_t* counts4_dev,
                                 vtd_stream stream) {
    return vtd_launch_binary_counts(pred_dev, target_dev, numel, threshold, counts4_dev, (hipStream_t)stream);
}

// ---- AdamW step (trainer.py:107-112; adamw.hip)
int vtd_adamw_step(const vtd_adamw_tensor* tensors, int count, const vtd_adamw_hyper* hyper, vtd_stream stream) {
    return vtd_launch_adamw(tensors, count, hyper, (hipStream_t)stream);
}

// ---- DB head training (dbhead_train.hip)
int vtd_dbhead_pack_features(const void* x_dev, int dtype, int n, int height, int width, void* feats_dev, vtd_stream stream) {
    return vtd_launch_dbhead_pack(x_dev, dtype, n, height, width, feats_dev, (hipStream_t)stream);
}

int64_t vtd_dbhead_train_workspace_bytes(int n, int height, int width, int backward) { return vtd_dbhead_ws_bytes(n, height, width, backward); }

int vtd_dbhead_train_forward(const void* feats_dev, int n, int height, int width, const vtd_dbhead_params* params, int training, float momentum,
                             float eps, void* workspace_dev, float* prob_dev, float* thresh_dev, float* stats_dev, vtd_stream stream) {
    return vtd_launch_dbhead_forward(feats_dev, n, height, width, params, training, momentum, eps, workspace_dev, prob_dev, thresh_dev, stats_dev,
                                     (hipStream_t)stream);
}

int vtd_dbhead_train_backward(const void* feats_dev, int n, int height, int width, const vtd_dbhead_params* params, int training,
                              const void* workspace_dev, const float* prob_dev, const float* thresh_dev, const float* grad_prob_dev,
                              const float* grad_thresh_dev, const vtd_dbhead_params* grads, void* scratch_dev, vtd_stream stream) {
    return vtd_launch_dbhead_backward(feats_dev, n, height, width, params, training, workspace_dev, prob_dev, thresh_dev, grad_prob_dev,
                                      grad_thresh_dev, grads, scratch_dev, (hipStream_t)stream);
}

int vtd_dbhead_train_backward_input(int n, int height, int width, const vtd_dbhead_params* params, void* scratch_dev, float* dfeats_dev,
                                    float* dscale_dev, vtd_stream stream) {
    return vtd_launch_dbhead_backward_input(n, height, width, params, scratch_dev, dfeats_dev, dscale_dev, (hipStream_t)stream);
}

// ---- FPN training (fpn_train.hip)
int vtd_fpn_train_pack_tap(const void* x_dev, int dtype, int n, int channels, int height, int width, void* tap_dev, vtd_stream stream) {
    return vtd_launch_fpn_pack_tap(x_dev, dtype, n, channels, height, width, tap_dev, (hipStream_t)stream);
}

int64_t vtd_fpn_train_workspace_bytes(int n, int h5, int w5, int c5_channels, int mode) { return vtd_fpn_ws_bytes(n, h5, w5, c5_channels, mode); }

int vtd_fpn_train_forward(const void* const* taps, int n, int h5, int w5, int c5_channels, const vtd_fpn_params* params, void* workspace_dev,
                          void* p2_dev, vtd_stream stream) {
    return vtd_launch_fpn_forward(taps, n, h5, w5, c5_channels, params, workspace_dev, p2_dev, (hipStream_t)stream);
}

int vtd_fpn_train_unpack_p2(const void* p2_dev, int n, int height, int width, float* p2_nchw_dev, vtd_stream stream) {
    return vtd_launch_fpn_unpack_p2(p2_dev, n, height, width, p2_nchw_dev, (hipStream_t)stream);
}

int vtd_fpn_train_pack_grad(const float* grad_nchw_dev, int n, int height, int width, float* dp2_dev, vtd_stream stream) {
    return vtd_launch_fpn_pack_grad(grad_nchw_dev, n, height, width, dp2_dev, (hipStream_t)stream);
}

int vtd_fpn_train_backward(const void* const* taps, int n, int h5, int w5, int c5_channels, const vtd_fpn_params* params, const void* workspace_dev,
                           const float* dp2_dev, const float* dscale_dev, const vtd_fpn_params* grads, void* scratch_dev, vtd_stream stream) {
    return vtd_launch_fpn_backward(taps, n, h5, w5, c5_channels, params, workspace_dev, dp2_dev, dscale_dev, grads, scratch_dev, (hipStream_t)stream);
}

// ---- BasicBlock training (resblock_train.hip)
int64_t vtd_basicblock_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode) {
    return vtd_basicblock_ws_bytes(n, h_in, w_in, cin, width, stride, mode);
}

int vtd_basicblock_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                 float eps, void* workspace_dev, void* y_dev, vtd_stream stream) {
    return vtd_launch_basicblock_forward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, (hipStream_t)stream);
}

int vtd_basicblock_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                  float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                  const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream) {
    return vtd_launch_basicblock_backward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, dy_dev, dscale_dev, grads,
                                          scratch_dev, dx_dev, dxscale_dev, (hipStream_t)stream);
}

// the six geometries of ResNet-18's layer2, layer3 and layer4, with the input gradient of the stride-2 blocks
int64_t vtd_resblock_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode) {
    return vtd_resblock_ws_bytes(n, h_in, w_in, cin, width, stride, mode);
}

int vtd_resblock_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                               float eps, void* workspace_dev, void* y_dev, vtd_stream stream) {
    return vtd_launch_resblock_forward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, (hipStream_t)stream);
}

int vtd_resblock_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream) {
    return vtd_launch_resblock_backward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, dy_dev, dscale_dev, grads,
                                        scratch_dev, dx_dev, dxscale_dev, (hipStream_t)stream);
}

int vtd_resblock_train_combine(float* a_dev, const float* ascale_dev, const float* b_dev, const float* bscale_dev, int64_t numel, float* outscale_dev,
                               vtd_stream stream) {
    return vtd_launch_resblock_combine(a_dev, ascale_dev, b_dev, bscale_dev, numel, outscale_dev, (hipStream_t)stream);
}

// ResNet-50's last stage: the two Bottleneck geometries of width 512
int64_t vtd_bottleneck_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode) {
    return vtd_bottleneck_ws_bytes(n, h_in, w_in, cin, width, stride, mode);
}

int vtd_bottleneck_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                 float eps, void* workspace_dev, void* y_dev, vtd_stream stream) {
    return vtd_launch_bottleneck_forward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, (hipStream_t)stream);
}

int vtd_bottleneck_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                  float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                  const vtd_bottleneck_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream) {
    return vtd_launch_bottleneck_backward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, dy_dev, dscale_dev, grads,
                                          scratch_dev, dx_dev, dxscale_dev, (hipStream_t)stream);
}

// ResNet-50's res4: the two Bottleneck geometries of width 256
int64_t vtd_bottleneck256_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode) {
    return vtd_bottleneck256_ws_bytes(n, h_in, w_in, cin, width, stride, mode);
}

int vtd_bottleneck256_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                    float eps, void* workspace_dev, void* y_dev, vtd_stream stream) {
    return vtd_launch_bottleneck256_forward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, (hipStream_t)stream);
}

int vtd_bottleneck256_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride,
                                     const vtd_bottleneck_params* params, float eps, const void* workspace_dev, const void* y_dev,
                                     const float* dy_dev, const float* dscale_dev, const vtd_bottleneck_params* grads, void* scratch_dev,
                                     float* dx_dev, float* dxscale_dev, vtd_stream stream) {
    return vtd_launch_bottleneck256_backward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, dy_dev, dscale_dev, grads,
                                             scratch_dev, dx_dev, dxscale_dev, (hipStream_t)stream);
}

// ResNet-50's res3: the two Bottleneck geometries of width 128
int64_t vtd_bottleneck128_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode) {
    return vtd_bottleneck128_ws_bytes(n, h_in, w_in, cin, width, stride, mode);
}

int vtd_bottleneck128_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                    float eps, void* workspace_dev, void* y_dev, vtd_stream stream) {
    return vtd_launch_bottleneck128_forward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, (hipStream_t)stream);
}

int vtd_bottleneck128_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride,
                                     const vtd_bottleneck_params* params, float eps, const void* workspace_dev, const void* y_dev,
                                     const float* dy_dev, const float* dscale_dev, const vtd_bottleneck_params* grads, void* scratch_dev,
                                     float* dx_dev, float* dxscale_dev, vtd_stream stream) {
    return vtd_launch_bottleneck128_backward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, dy_dev, dscale_dev, grads,
                                             scratch_dev, dx_dev, dxscale_dev, (hipStream_t)stream);
}

// ResNet-50's res2: the two Bottleneck geometries of width 64, both at stride 1
int64_t vtd_bottleneck64_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode) {
    return vtd_bottleneck64_ws_bytes(n, h_in, w_in, cin, width, stride, mode);
}

int vtd_bottleneck64_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                   float eps, void* workspace_dev, void* y_dev, vtd_stream stream) {
    return vtd_launch_bottleneck64_forward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, (hipStream_t)stream);
}

int vtd_bottleneck64_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride,
                                    const vtd_bottleneck_params* params, float eps, const void* workspace_dev, const void* y_dev,
                                    const float* dy_dev, const float* dscale_dev, const vtd_bottleneck_params* grads, void* scratch_dev,
                                    float* dx_dev, float* dxscale_dev, vtd_stream stream) {
    return vtd_launch_bottleneck64_backward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, dy_dev, dscale_dev, grads,
                                            scratch_dev, dx_dev, dxscale_dev, (hipStream_t)stream);
}

int64_t vtd_block64_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode) {
    return vtd_block64_ws_bytes(n, h_in, w_in, cin, width, stride, mode);
}

int vtd_block64_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                              float eps, void* workspace_dev, void* y_dev, vtd_stream stream) {
    return vtd_launch_block64_forward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, (hipStream_t)stream);
}

int vtd_block64_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                               float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                               const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream) {
    return vtd_launch_block64_backward(x_dev, n, h_in, w_in, cin, width, stride, params, eps, workspace_dev, y_dev, dy_dev, dscale_dev, grads,
                                       scratch_dev, dx_dev, dxscale_dev, (hipStream_t)stream);
}

// ---- BasicBlock training with batch-statistics BatchNorm (resblock_bn_train.hip)
int64_t vtd_resblock_bn_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode) {
    return vtd_resblock_bn_ws_bytes(n, h_in, w_in, cin, width, stride, mode);
}

int vtd_resblock_bn_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                  int training, float momentum, float eps, void* workspace_dev, void* y_dev, float* stats_dev, vtd_stream stream) {
    return vtd_launch_resblock_bn_forward(x_dev, n, h_in, w_in, cin, width, stride, params, training, momentum, eps, workspace_dev, y_dev, stats_dev,
                                          (hipStream_t)stream);
}

int vtd_resblock_bn_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                   int training, float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                   const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream) {
    return vtd_launch_resblock_bn_backward(x_dev, n, h_in, w_in, cin, width, stride, params, training, eps, workspace_dev, y_dev, dy_dev, dscale_dev,
                                           grads, scratch_dev, dx_dev, dxscale_dev, (hipStream_t)stream);
}

// the four geometries of layer3 and layer4, with the input gradient of the stride-2 blocks
int64_t vtd_block_bn_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode) {
    return vtd_block_bn_ws_bytes(n, h_in, w_in, cin, width, stride, mode);
}

int vtd_block_bn_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                               int training, float momentum, float eps, void* workspace_dev, void* y_dev, float* stats_dev, vtd_stream stream) {
    return vtd_launch_block_bn_forward(x_dev, n, h_in, w_in, cin, width, stride, params, training, momentum, eps, workspace_dev, y_dev, stats_dev,
                                       (hipStream_t)stream);
}

int vtd_block_bn_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                int training, float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream) {
    return vtd_launch_block_bn_backward(x_dev, n, h_in, w_in, cin, width, stride, params, training, eps, workspace_dev, y_dev, dy_dev, dscale_dev,
                                        grads, scratch_dev, dx_dev, dxscale_dev, (hipStream_t)stream);
}

// the six geometries of layer2, layer3 and layer4 and layer1's (64 -> 64, stride 1): the family that later stages join
int64_t vtd_trunk_bn_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode) {
    return vtd_trunk_bn_ws_bytes(n, h_in, w_in, cin, width, stride, mode);
}

int vtd_trunk_bn_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                               int training, float momentum, float eps, void* workspace_dev, void* y_dev, float* stats_dev, vtd_stream stream) {
    return vtd_launch_trunk_bn_forward(x_dev, n, h_in, w_in, cin, width, stride, params, training, momentum, eps, workspace_dev, y_dev, stats_dev,
                                       (hipStream_t)stream);
}

int vtd_trunk_bn_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                int training, float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream) {
    return vtd_launch_trunk_bn_backward(x_dev, n, h_in, w_in, cin, width, stride, params, training, eps, workspace_dev, y_dev, dy_dev, dscale_dev,
                                        grads, scratch_dev, dx_dev, dxscale_dev, (hipStream_t)stream);
}

// ResNet-50's res5 and res4 Bottlenecks with batch-statistics BatchNorm (csrc/bottleneck_bn_train.hip)
int64_t vtd_bottleneck_bn_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode) {
    return vtd_bottleneck_bn_ws_bytes(n, h_in, w_in, cin, width, stride, mode);
}

int vtd_bottleneck_bn_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                    int training, float momentum, float eps, void* workspace_dev, void* y_dev, float* stats_dev, vtd_stream stream) {
    return vtd_launch_bottleneck_bn_forward(x_dev, n, h_in, w_in, cin, width, stride, params, training, momentum, eps, workspace_dev, y_dev, stats_dev,
                                            (hipStream_t)stream);
}

int vtd_bottleneck_bn_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                     int training, float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev,
                                     const float* dscale_dev, const vtd_bottleneck_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev,
                                     vtd_stream stream) {
    return vtd_launch_bottleneck_bn_backward(x_dev, n, h_in, w_in, cin, width, stride, params, training, eps, workspace_dev, y_dev, dy_dev, dscale_dev,
                                             grads, scratch_dev, dx_dev, dxscale_dev, (hipStream_t)stream);
}

int vtd_stem_train_pack_input(const void* x_dev, int dtype, int n, int height, int width, void* tap_dev, vtd_stream stream) {
    return vtd_launch_stem_pack_input(x_dev, dtype, n, height, width, tap_dev, (hipStream_t)stream);
}

int64_t vtd_stem_train_workspace_bytes(int n, int height, int width, int mode) { return vtd_stem_ws_bytes(n, height, width, mode); }

int vtd_stem_train_forward(const void* x_tap_dev, int n, int height, int width, const vtd_stem_params* params, float eps, void* workspace_dev,
                           void* pool_tap_dev, void* idx_dev, vtd_stream stream) {
    return vtd_launch_stem_forward(x_tap_dev, n, height, width, params, eps, workspace_dev, pool_tap_dev, idx_dev, (hipStream_t)stream);
}

int vtd_stem_train_backward(const void* x_tap_dev, int n, int height, int width, const vtd_stem_params* params, float eps, const void* workspace_dev,
                            const void* pool_tap_dev, const void* idx_dev, const float* dpool_dev, const float* dscale_dev, const vtd_stem_params* grads,
                            void* scratch_dev, vtd_stream stream) {
    return vtd_launch_stem_backward(x_tap_dev, n, height, width, params, eps, workspace_dev, pool_tap_dev, idx_dev, dpool_dev, dscale_dev, grads,
                                    scratch_dev, (hipStream_t)stream);
}

int64_t vtd_stem_bn_train_workspace_bytes(int n, int height, int width, int mode) { return vtd_stem_bn_ws_bytes(n, height, width, mode); }

int vtd_stem_bn_train_forward(const void* x_tap_dev, int n, int height, int width, const vtd_stem_params* params, int training, float momentum, float eps,
                              void* workspace_dev, void* pool_tap_dev, void* idx_dev, float* stats_dev, vtd_stream stream) {
    return vtd_launch_stem_bn_forward(x_tap_dev, n, height, width, params, training, momentum, eps, workspace_dev, pool_tap_dev, idx_dev, stats_dev,
                                      (hipStream_t)stream);
}

int vtd_stem_bn_train_backward(const void* x_tap_dev, int n, int height, int width, const vtd_stem_params* params, int training, float eps,
                               const void* workspace_dev, const void* pool_tap_dev, const void* idx_dev, const float* dpool_dev, const float* dscale_dev,
                               const vtd_stem_params* grads, void* scratch_dev, vtd_stream stream) {
    return vtd_launch_stem_bn_backward(x_tap_dev, n, height, width, params, training, eps, workspace_dev, pool_tap_dev, idx_dev, dpool_dev, dscale_dev,
                                       grads, scratch_dev, (hipStream_t)stream);
}

int64_t vtd_fpn_train_input_workspace_bytes(int n, int h5, int w5, int c5_channels) { return vtd_fpn_input_ws_bytes(n, h5, w5, c5_channels); }

int vtd_fpn_train_backward_input(int n, int h5, int w5, int c5_channels, const vtd_fpn_params* params, void* scratch_dev, int level_mask,
                                 float* const* dtaps_dev, float* dscale_dev, vtd_stream stream) {
    return vtd_launch_fpn_backward_input(n, h5, w5, c5_channels, params, scratch_dev, level_mask, dtaps_dev, dscale_dev, (hipStream_t)stream);
}

int vtd_fpn_train_unpack_tap_grad(const float* dtap_dev, const float* dscale_dev, int n, int channels, int height, int width, float* grad_nchw_dev,
                                  vtd_stream stream) {
    return vtd_launch_fpn_unpack_tap_grad(dtap_dev, dscale_dev, n, channels, height, width, grad_nchw_dev, (hipStream_t)stream);
}

int vtd_dbhead_unpack_input_grad(const float* dfeats_dev, const float* dscale_dev, int n, int height, int width, float* grad_nchw_dev,
                                 vtd_stream stream) {
    return vtd_launch_dbhead_unpack_input_grad(dfeats_dev, dscale_dev, n, height, width, grad_nchw_dev, (hipStream_t)stream);
}

int vtd_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    return e == hipSuccess ? n : -(int)e;
}

int vtd_detector_create(const char* backbone, int max_batch, vtd_detector** out) {
    if (!backbone || !out || max_batch <= 0) return ERR_ARG;
    const std::string b = backbone;
    if (b != "resnet18" && b != "resnet50") return ERR_ARG;
    auto* d = new vtd_detector();
    d->backbone = b;
    d->max_batch = max_batch;
    *out = d;
    return 0;
}

void vtd_detector_destroy(vtd_detector* d) { delete d; }

int vtd_detector_set_tensor(vtd_detector* d, const char* key, const float* host_data, int64_t numel) {
    if (!d || !key || !host_data || numel < 0) return ERR_ARG;
    const std::string k = key;
    if (!known_detector_key(k)) return ERR_UNKNOWN_KEY;
    if (k.size() > 19 && k.compare(k.size() - 19, 19, "num_batches_tracked") == 0) return 0;
    d->sd[k].assign(host_data, host_data + numel);
    return 0;
}

int vtd_detector_set_option(vtd_detector* d, const char* name, int value) {
    if (!d || !name || d->finalized) return ERR_ARG;
    if (std::string(name) == "fuse_fpn_head") { d->fuse_fpn_head = value != 0; return 0; }
    if (std::string(name) == "fuse_stem_pool") { d->fuse_stem_pool = value != 0; return 0; }
    if (std::string(name) == "head_tail_kernel") { d->head_tail_kernel = value != 0; return 0; }
    if (std::string(name) == "fuse_downsample") { d->fuse_downsample = value != 0; return 0; }
    return ERR_UNKNOWN_KEY;
}

int vtd_detector_finalize(vtd_detector* d, vtd_stream stream) {
    if (!d) return ERR_ARG;
    if (d->finalized) return ERR_ARG;
    int rc = build_detector_graph(d);
    if (rc) return rc;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return -(int)e;
    d->sd.clear();
    d->finalized = true;
    return 0;
}

int vtd_detector_preprocess(vtd_detector* d, const uint8_t* frames_dev, int n, int height, int width, vtd_stream stream) {
    if (!d || !frames_dev || height <= 0 || width <= 0) return ERR_ARG;
    if (!d->finalized) return ERR_NOT_FINALIZED;
    if (n <= 0 || n > d->max_batch) return ERR_BATCH;
    PreTables t;
    int rc = get_pre_tables(d, height, width, t);
    if (rc) return rc;
    return vtd_launch_preprocess(frames_dev, n, height, width, d->input.ptr, t.xb, t.xk, t.ksx, t.yb, t.yk, t.ksy, t.max_rows,
                                 (hipStream_t)stream);
}

// The frame geometry of the pre-process, readable without a GPU (tests/test_frame_geometry.py; internal, not in include/vtd.h).
// vtd_preprocess_axis: the tables pillow_axis(in_size, out_size) builds -- *ksize taps per output, bounds [out_size][2] (first input,
// count), kk [out_size][*ksize] 22-bit coefficients (kk_cap: the ints kk holds).  0, or a negative value on a bad argument or a short
// buffer.  Sizes up to 65536, many times the largest frame any kernel takes.
int vtd_preprocess_axis(int in_size, int out_size, int* ksize, int* bounds, int* kk, int kk_cap) {
    if (in_size <= 0 || out_size <= 0 || in_size > 65536 || out_size > 65536 || !ksize || !bounds || !kk) return ERR_ARG;
    const ResampleAxis a = pillow_axis(in_size, out_size);
    if (kk_cap < 0 || (size_t)kk_cap < a.kk.size()) return ERR_CAPACITY;
    *ksize = a.ksize;
    std::copy(a.bounds.begin(), a.bounds.end(), bounds);
    std::copy(a.kk.begin(), a.kk.end(), kk);
    return 0;
}

// vtd_preprocess_plan: what vtd_detector_preprocess does with H x W frames -- tap counts, LDS rows per workgroup, the kernel
// (vtd_preprocess_path's numbering, detector_misc.hip) and its dynamic LDS bytes.  0, -1010 where the launcher refuses the size (the
// tap counts and rows are still written), or ERR_ARG.
int vtd_preprocess_plan(int H, int W, int* ksx, int* ksy, int* max_rows, int* path, int* lds_bytes) {
    if (H <= 0 || W <= 0 || H > 65536 || W > 65536 || !ksx || !ksy || !max_rows || !path || !lds_bytes) return ERR_ARG;
    const ResampleAxis ax = pillow_axis(W, 640), ay = pillow_axis(H, 640);
    *ksx = ax.ksize; *ksy = ay.ksize;
    *max_rows = vtd_preprocess_max_rows(ay.bounds.data());
    *path = -1; *lds_bytes = 0;
    const int rc = vtd_preprocess_path(W, *ksx, *ksy, *max_rows, lds_bytes);
    if (rc < 0) return rc;
    *path = rc;
    return 0;
}

int vtd_detector_set_input_nchw(vtd_detector* d, const float* x_dev, int n, vtd_stream stream) {
    if (!d || !x_dev) return ERR_ARG;
    if (!d->finalized) return ERR_NOT_FINALIZED;
    if (n <= 0 || n > d->max_batch) return ERR_BATCH;
    return vtd_launch_nchw_to_input(x_dev, d->input.ptr, n, (hipStream_t)stream);
}

// the graph's launches [0, op_end) for n frames of the current input
static int run_detector_ops(vtd_detector* d, int n, float* prob_dev, float* thresh_dev, hipStream_t s, size_t op_end) {
    float* outs[2] = {prob_dev, thresh_dev};
    // kernel choice per power-of-two batch bucket (1, 2, 4, ... max_batch), decided at the bucket's own size
    const int bucket = batch_bucket(n, d->max_batch);
    auto tit = d->tuned.find(bucket);
    if (tit == d->tuned.end()) {
        std::vector<int> cfgs(d->ops.size(), -1);
        for (size_t oi = 0; oi < d->ops.size(); ++oi)
            if (d->ops[oi].kind == Op::CONV) {
                int rc = choose_config(d, d->ops[oi].conv, bucket, s, &cfgs[oi]);
                if (rc) return rc;
            }
        tit = d->tuned.emplace(bucket, std::move(cfgs)).first;
    }
    const std::vector<int>& cfgs = tit->second;
    for (size_t oi = 0; oi < op_end; ++oi) {
        const Op& o = d->ops[oi];
        int rc = 0;
        if (o.final_slot == 1 && !thresh_dev) continue;
        if (o.kind == Op::BORDER) {
            const ConvCandidate* row = oi ? find_conv_candidate(cfgs[oi - 1]) : nullptr;
            if (!(row && row->needs_border)) continue;  // the gathered kernel did every class
        }
        hipEvent_t e0 = nullptr, e1 = nullptr;
        const bool prof = d->profiling && (d->prof_only < 0 || d->prof_only == (int)oi);
        if (prof) {
            e0 = d->take_event();
            e1 = d->take_event();
            if (!e0 || !e1) return ERR_ARG;
            VTD_HIP_CHECK(hipEventRecord(e0, s));
        }
        switch (o.kind) {
            case Op::CONV: rc = launch_conv_op(o.conv, n, s, cfgs[oi]); break;
            case Op::POOL: rc = vtd_launch_maxpool(o.pin, o.pout, n, o.pk[0], o.pk[1], o.pk[2], o.pk[3], o.pk[4], o.pk[5], s); break;
            case Op::FINAL: rc = launch_conv_op(o.conv, n, s, 7, outs[o.final_slot]); break;
            case Op::HEADTAIL:
                rc = vtd_launch_head_tail(o.conv.in, o.htw1, o.conv.bias, o.htw2, o.conv.head_b, outs[o.final_slot], n, s);
                break;
            case Op::BORDER: rc = launch_border_tiles(o.conv, n, s); break;
            case Op::STEMPOOL: rc = vtd_launch_stem_pool(o.pin, o.pout, o.spw, o.spb, n, s); break;
        }
        if (rc) return rc;
        if (prof) {
            VTD_HIP_CHECK(hipEventRecord(e1, s));
            d->ev_spans.push_back({(int)oi, {e0, e1}});
            d->prof_macs[oi] += (o.kind != Op::POOL) ? (double)o.conv.macs_per_image * n : 0.0;
        }
    }
    return 0;
}

int vtd_detector_forward(vtd_detector* d, int n, float* prob_dev, float* thresh_dev, vtd_stream stream) {
    if (!d || !prob_dev) return ERR_ARG;
    if (!d->finalized) return ERR_NOT_FINALIZED;
    if (n <= 0 || n > d->max_batch) return ERR_BATCH;
    return run_detector_ops(d, n, prob_dev, thresh_dev, (hipStream_t)stream, d->ops.size());
}

// trunk + FPN up to P2, then a copy of the n frames' ring-padded P2 into the caller's buffer (same layout: [n][162][162][256] fp16)
int vtd_detector_forward_features(vtd_detector* d, int n, void* feats_dev, vtd_stream stream) {
    if (!d || !feats_dev) return ERR_ARG;
    if (!d->finalized) return ERR_NOT_FINALIZED;
    if (n <= 0 || n > d->max_batch) return ERR_BATCH;
    if (d->fuse_fpn_head || !d->p2_ops || !d->taps.count("p2")) return -2801;
    if ((uintptr_t)feats_dev & 15) return -2803;
    hipStream_t s = (hipStream_t)stream;
    int rc = run_detector_ops(d, n, nullptr, nullptr, s, d->p2_ops);
    if (rc) return rc;
    const TensorDesc& p2 = d->taps["p2"];
    VTD_HIP_CHECK(hipMemcpyAsync(feats_dev, p2.ptr, (size_t)n * p2.hp * p2.wp * p2.c * sizeof(half_t), hipMemcpyDeviceToDevice, s));
    return 0;
}

// the trunk only, then a copy of the n frames' ring-padded taps C2..C5 into the caller's buffers (same layout: [n][h+2][w+2][c] fp16)
int vtd_detector_forward_trunk(vtd_detector* d, int n, void* c2_dev, void* c3_dev, void* c4_dev, void* c5_dev, vtd_stream stream) {
    void* dst[4] = {c2_dev, c3_dev, c4_dev, c5_dev};
    if (!d || !c2_dev || !c3_dev || !c4_dev || !c5_dev) return ERR_ARG;
    if (!d->finalized) return ERR_NOT_FINALIZED;
    if (n <= 0 || n > d->max_batch) return ERR_BATCH;
    if (d->fuse_fpn_head || !d->trunk_ops) return -2901;
    const char* names[4] = {"c2", "c3", "c4", "c5"};
    for (int i = 0; i < 4; ++i) {
        if ((uintptr_t)dst[i] & 15) return -2903;
        auto it = d->taps.find(names[i]);
        if (it == d->taps.end() || it->second.ring != 1) return -2901;
    }
    hipStream_t s = (hipStream_t)stream;
    int rc = run_detector_ops(d, n, nullptr, nullptr, s, d->trunk_ops);
    if (rc) return rc;
    for (int i = 0; i < 4; ++i) {
        const TensorDesc& t = d->taps[names[i]];
        VTD_HIP_CHECK(hipMemcpyAsync(dst[i], t.ptr, (size_t)n * t.hp * t.wp * t.c * sizeof(half_t), hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

// the stem and its max-pool only, then a copy of the n frames' ring-padded pooled map (what layer1 reads: [n][162][162][64] fp16)
int vtd_detector_forward_pool(vtd_detector* d, int n, void* pool_dev, vtd_stream stream) {
    if (!d || !pool_dev) return ERR_ARG;
    if (!d->finalized) return ERR_NOT_FINALIZED;
    if (n <= 0 || n > d->max_batch) return ERR_BATCH;
    auto it = d->taps.find("pool");
    if (!d->pool_ops || it == d->taps.end() || it->second.ring != 1) return -2901;
    if ((uintptr_t)pool_dev & 15) return -2903;
    hipStream_t s = (hipStream_t)stream;
    int rc = run_detector_ops(d, n, nullptr, nullptr, s, d->pool_ops);
    if (rc) return rc;
    const TensorDesc& t = it->second;
    VTD_HIP_CHECK(hipMemcpyAsync(pool_dev, t.ptr, (size_t)n * t.hp * t.wp * t.c * sizeof(half_t), hipMemcpyDeviceToDevice, s));
    return 0;
}

// the stem and the first residual stage only, then a copy of the n frames' ring-padded C2 ([n][162][162][c] fp16)
int vtd_detector_forward_c2(vtd_detector* d, int n, void* c2_dev, vtd_stream stream) {
    if (!d || !c2_dev) return ERR_ARG;
    if (!d->finalized) return ERR_NOT_FINALIZED;
    if (n <= 0 || n > d->max_batch) return ERR_BATCH;
    auto it = d->taps.find("c2");
    if (d->fuse_fpn_head || !d->c2_ops || it == d->taps.end() || it->second.ring != 1) return -2901;
    if ((uintptr_t)c2_dev & 15) return -2903;
    hipStream_t s = (hipStream_t)stream;
    int rc = run_detector_ops(d, n, nullptr, nullptr, s, d->c2_ops);
    if (rc) return rc;
    const TensorDesc& t = it->second;
    VTD_HIP_CHECK(hipMemcpyAsync(c2_dev, t.ptr, (size_t)n * t.hp * t.wp * t.c * sizeof(half_t), hipMemcpyDeviceToDevice, s));
    return 0;
}

int vtd_detector_set_profiling(vtd_detector* d, int enable) {
    if (!d || !d->finalized) return ERR_ARG;
    d->profiling = enable != 0;
    d->prof_only = enable >= 2 ? enable - 2 : -1;
    if (d->prof_only >= (int)d->ops.size()) return ERR_ARG;
    d->ev_spans.clear();
    d->ev_used = 0;
    d->prof_ms.assign(d->ops.size(), 0.0);
    d->prof_calls.assign(d->ops.size(), 0);
    d->prof_macs.assign(d->ops.size(), 0.0);
    return 0;
}

int vtd_detector_num_ops(const vtd_detector* d) { return d ? (int)d->ops.size() : 0; }

int vtd_detector_set_tuning(vtd_detector* d, const char* table_text) {
    if (!d) return ERR_ARG;
    int rc = set_tuning_text(d, table_text);
    if (!rc) d->tuned.clear();  // decisions already taken are re-taken against the new table
    return rc;
}

int64_t vtd_detector_get_tuning(const vtd_detector* d, char* buf, int64_t capacity) { return get_tuning_text(d, buf, capacity); }

int vtd_detector_tuning_measured(const vtd_detector* d) { return d && d->tuning_measured ? 1 : 0; }

int vtd_detector_get_profile(vtd_detector* d, int op_index, char* name, int name_cap, double* total_ms, int64_t* calls,
                             double* total_macs, vtd_stream stream) {
    if (!d || op_index < 0 || op_index >= (int)d->ops.size() || !name || name_cap < 32 || !total_ms || !calls || !total_macs)
        return ERR_ARG;
    if (!d->ev_spans.empty()) {  // resolve pending events once
        hipError_t e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) return -(int)e;
        for (auto& sp : d->ev_spans) {
            float ms = 0.f;
            e = hipEventElapsedTime(&ms, sp.second.first, sp.second.second);
            if (e != hipSuccess) return -(int)e;
            d->prof_ms[sp.first] += ms;
            d->prof_calls[sp.first] += 1;
        }
        d->ev_spans.clear();
        d->ev_used = 0;
    }
    const Op& o = d->ops[op_index];
    if (o.kind == Op::CONV) {
        const ConvOp& c = o.conv;
        int cfg = -1;
        if (!d->tuned.empty()) cfg = d->tuned.rbegin()->second[op_index];
        const ConvCandidate* row = find_conv_candidate(cfg);
        if (row && row->needs_border)
            std::snprintf(name, name_cap, "%s M/img=%d N=%d K=%d (lateral+smooth+head conv composed%s; border classes in the next slot)", row->name,
                          c.ho * c.wo, c.cout, c.K, cfg == kHeadEntryHalfCfg ? ", half halos two steps ahead" : "");
        else if (row && cfg == kPointwiseCfg)
            std::snprintf(name, name_cap, "%s 1x1%s streaming M/img=%d N=%d K=%d", row->name, c.has_res ? "+top-down add" : "", c.ho * c.wo, c.cout, c.K);
        else if (row)  // the conv_halo family
            std::snprintf(name, name_cap, "%s 3x3 M/img=%d N=%d K=%d", row->name, c.ho * c.wo, c.cout, c.K);
        else
            std::snprintf(name, name_cap, "conv_igemm<%s> M/img=%d N=%d K=%d%s", vtd_conv_config_name(cfg), c.ho * c.wo, c.cout, c.K,
                          c.plist ? " (lateral+smooth+head conv composed)" : "");
    } else if (o.kind == Op::POOL) {
        std::snprintf(name, name_cap, "maxpool %dx%d/s%d", o.pk[0], o.pk[1], o.pk[2]);
    } else if (o.kind == Op::BORDER) {
        std::snprintf(name, name_cap, "conv_igemm<128,64,s3,classed> border classes of the composed head entry (%d tiles/img)", o.conv.tiles_border);
    } else if (o.kind == Op::HEADTAIL) {
        std::snprintf(name, name_cap, "head_tail ConvT1+BN+ReLU+ConvT2+sigmoid fused M/img=%d N=256 K=64", o.conv.ho * o.conv.wo);
    } else if (o.kind == Op::STEMPOOL) {
        std::snprintf(name, name_cap, "stem_pool conv7x7/s2+BN+ReLU+maxpool3x3/s2 fused M/img=%d N=64 K=147", 320 * 320);
    } else {
        std::snprintf(name, name_cap, "conv_igemm<64,256,s2> ConvT1+ConvT2+sigmoid fused M/img=%d", o.conv.ho * o.conv.wo);
    }
    const bool have = d->prof_ms.size() == d->ops.size();  // set_profiling never called: names only
    *total_ms = have ? d->prof_ms[op_index] : 0.0;
    *calls = have ? d->prof_calls[op_index] : 0;
    *total_macs = have ? d->prof_macs[op_index] : 0.0;
    return 0;
}

int vtd_detector_read_tap(vtd_detector* d, const char* name, int n, float* host_out, int64_t capacity, vtd_stream stream) {
    if (!d || !name || !host_out) return ERR_ARG;
    if (!d->finalized) return ERR_NOT_FINALIZED;
    auto it = d->taps.find(name);
    if (it == d->taps.end()) return ERR_UNKNOWN_KEY;
    const TensorDesc& t = it->second;
    if (n <= 0 || n > t.n) return ERR_BATCH;
    const int creal = (std::string(name) == "input") ? 3 : t.c;
    if (capacity < (int64_t)n * creal * t.h * t.w) return ERR_CAPACITY;
    return read_tensor_nchw(t, n, creal, host_out, (hipStream_t)stream);
}

int64_t vtd_detector_macs_per_frame(const vtd_detector* d) { return d ? d->macs : 0; }

}  // extern "C"

// ================================================================================================ recognizer
namespace vtd {

static int build_recognizer_graph(vtd_recognizer* r) {
    const int D = r->max_crops;
    int rc;
    auto new_tensor = [&](int h, int w, int c, int ring, TensorDesc& t) {
        t = make_desc(D, h, w, c, ring, ring);
        return r->alloc_tensor(t);
    };
    void* p = nullptr;
    if ((rc = r->arena.alloc(&p, (size_t)D * 32 * 128 * 3, true))) return rc;
    r->resized = (uint8_t*)p;
    // conv1 (fp32 VALU kernel, pool fused)
    {
        Fold f;
        if ((rc = fold_bn(r, "cnn.1", "cnn.0.bias", 64, f))) return rc;
        auto w = r->get("cnn.0.weight", 64 * 3 * 3 * 3);
        if (!w) return ERR_MISSING_KEY;
        std::vector<half_t> wp(64 * 32, (half_t)0.f);
        std::vector<float> bp(64);
        for (int co = 0; co < 64; ++co) {
            bp[co] = (float)f.shift[co];
            for (int c = 0; c < 3; ++c)
                for (int rr = 0; rr < 3; ++rr)
                    for (int ss = 0; ss < 3; ++ss)
                        wp[co * 32 + (rr * 3 + ss) * 3 + c] = half_of((double)(*w)[((co * 3 + c) * 3 + rr) * 3 + ss] * f.scale[co]);
        }
        if ((rc = upload(r->arena, wp.data(), wp.size() * sizeof(half_t), (void**)&r->w1))) return rc;
        if ((rc = upload(r->arena, bp.data(), bp.size() * 4, (void**)&r->b1))) return rc;
        if ((rc = new_tensor(16, 64, 64, 1, r->t1))) return rc;
        r->taps["conv1"] = r->t1;
        r->macs += (int64_t)32 * 128 * 64 * 27;
    }
    struct Spec { int conv, bn, cin, cout, k, pad, ph, pw; };
    const Spec specs[6] = {{4, 5, 64, 128, 3, 1, 2, 2},  {8, 9, 128, 256, 3, 1, 0, 0},   {11, 12, 256, 256, 3, 1, 2, 1},
                           {15, 16, 256, 512, 3, 1, 0, 0}, {18, 19, 512, 512, 3, 1, 2, 1}, {22, 23, 512, 512, 2, 0, 0, 0}};
    TensorDesc x = r->t1;
    for (const Spec& sp : specs) {
        const int ho = x.h + 2 * sp.pad - sp.k + 1, wo = x.w + 2 * sp.pad - sp.k + 1;
        TensorDesc y;
        // MaxPool2d((2, pw)) behind the conv's ReLU (text_recognizer.py:17-22): taken in the convolution's register epilogue, the
        // un-pooled map (71 MB behind conv2 at 272 crops) is never written; bit-identical to the separate pool (conv_igemm.hip)
        const bool pooled = sp.ph == 2 && r->fuse_pools && !(ho & 1) && wo % sp.pw == 0;
        if (pooled) y = make_desc(D, ho, wo, sp.cout, 1, 1);   // shape bookkeeping only
        else if ((rc = new_tensor(ho, wo, sp.cout, 1, y))) return rc;
        Fold f;
        const std::string ck = "cnn." + std::to_string(sp.conv), bk = "cnn." + std::to_string(sp.bn);
        if ((rc = fold_bn(r, bk, ck + ".bias", sp.cout, f))) return rc;
        Op o;
        o.kind = Op::CONV;
        if ((rc = build_conv(r, o.conv, x, y, ck + ".weight", f, sp.cin, sp.cout, sp.k, sp.k, 1, sp.pad, EPI_RELU))) return rc;
        if (pooled) {
            TensorDesc z;
            if ((rc = new_tensor(ho / 2, wo / sp.pw, sp.cout, 1, z))) return rc;
            o.conv.out = z;
            o.conv.pool_pw = sp.pw;
            y = z;
        }
        r->ops.push_back(o);
        r->macs += o.conv.macs_per_image;
        x = y;
        if (sp.ph && !pooled) {
            TensorDesc z;
            if ((rc = new_tensor(x.h / sp.ph, x.w / sp.pw, x.c, 1, z))) return rc;
            Op po;
            po.kind = Op::POOL;
            po.pin = x; po.pout = z;
            const int pk[6] = {sp.ph, sp.pw, sp.ph, sp.pw, 0, 0};
            std::memcpy(po.pk, pk, sizeof(pk));
            r->ops.push_back(po);
            x = z;
        }
        // stage taps conv2..conv6: the layer's output behind its pool, whichever launch took the pool (conv7 is the `cnn` tap)
        if (&sp != &specs[5]) r->taps["conv" + std::to_string((int)(&sp - specs) + 2)] = x;
    }
    if (x.h != 1 || x.w != 31 || x.c != 512) return ERR_GEOMETRY;
    r->t7 = x;
    r->taps["cnn"] = x;
    const int T = 31;
    // LSTM: hoisted input projections (both directions stacked -> N = 2048) + recurrent weights
    if ((rc = r->arena.alloc(&p, (size_t)D * T * 2048 * sizeof(half_t), true))) return rc;
    r->xs = (half_t*)p;
    if ((rc = r->arena.alloc(&p, (size_t)D * T * 128 * 4, true))) return rc;
    r->logits_pad = (float*)p;
    r->h0 = make_desc(D, 1, T, 512, 0, 0);
    r->h1 = make_desc(D, 1, T, 512, 0, 0);
    if ((rc = r->alloc_tensor(r->h0)) || (rc = r->alloc_tensor(r->h1))) return rc;
    r->taps["h0"] = r->h0;
    r->taps["h1"] = r->h1;
    for (int layer = 0; layer < 2; ++layer) {
        std::vector<float> W((size_t)2048 * 512), B(2048);
        std::vector<half_t> whh((size_t)2 * 1024 * 256);
        for (int dir = 0; dir < 2; ++dir) {
            const std::string suf = "_l" + std::to_string(layer) + (dir ? "_reverse" : "");
            auto wih = r->get("rnn.weight_ih" + suf, (size_t)1024 * 512), wh = r->get("rnn.weight_hh" + suf, (size_t)1024 * 256);
            auto bih = r->get("rnn.bias_ih" + suf, 1024), bhh = r->get("rnn.bias_hh" + suf, 1024);
            if (!wih || !wh || !bih || !bhh) return ERR_MISSING_KEY;
            std::copy(wih->begin(), wih->end(), W.begin() + (size_t)dir * 1024 * 512);
            for (int i = 0; i < 1024; ++i) B[dir * 1024 + i] = (*bih)[i] + (*bhh)[i];
            for (size_t i = 0; i < (size_t)1024 * 256; ++i) whh[(size_t)dir * 1024 * 256 + i] = (half_t)(*wh)[i];
        }
        if ((rc = build_linear(r, r->xs_gemm[layer], layer ? r->h0 : r->t7, W, B, 2048, 512, r->xs, 2048, EPI_OUT_F16))) return rc;
        if ((rc = upload(r->arena, whh.data(), whh.size() * sizeof(half_t), (void**)&r->whh[layer]))) return rc;
        r->macs += r->xs_gemm[layer].macs_per_image + (int64_t)2 * T * 1024 * 256;
    }
    {
        auto w = r->get("classifier.weight", (size_t)r->vocab * 512), b = r->get("classifier.bias", r->vocab);
        if (!w || !b) return ERR_MISSING_KEY;
        if (r->vocab > 128) return ERR_GEOMETRY;
        if ((rc = build_linear(r, r->cls_gemm, r->h1, *w, *b, r->vocab, 512, r->logits_pad, 128))) return rc;
        r->macs += r->cls_gemm.macs_per_image;
    }
    return 0;
}

}  // namespace vtd

extern "C" {

int vtd_recognizer_create(int vocab_size, int max_crops, vtd_recognizer** out) {
    if (!out || vocab_size <= 0 || vocab_size > 128 || max_crops <= 0) return ERR_ARG;
    auto* r = new vtd_recognizer();
    r->vocab = vocab_size;
    r->max_crops = max_crops;
    *out = r;
    return 0;
}

void vtd_recognizer_destroy(vtd_recognizer* r) { delete r; }

int vtd_recognizer_set_tensor(vtd_recognizer* r, const char* key, const float* host_data, int64_t numel) {
    if (!r || !key || !host_data || numel < 0) return ERR_ARG;
    const std::string k = key;
    if (k.rfind("cnn.", 0) != 0 && k.rfind("rnn.", 0) != 0 && k.rfind("classifier.", 0) != 0) return ERR_UNKNOWN_KEY;
    if (k.size() > 19 && k.compare(k.size() - 19, 19, "num_batches_tracked") == 0) return 0;
    r->sd[k].assign(host_data, host_data + numel);
    return 0;
}

int vtd_recognizer_set_option(vtd_recognizer* r, const char* name, int value) {
    if (!r || !name || r->finalized) return ERR_ARG;
    if (std::string(name) == "fuse_pools") { r->fuse_pools = value != 0; return 0; }
    return ERR_UNKNOWN_KEY;
}

int vtd_recognizer_finalize(vtd_recognizer* r, vtd_stream stream) {
    if (!r || r->finalized) return ERR_ARG;
    int rc = build_recognizer_graph(r);
    if (rc) return rc;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return -(int)e;
    r->sd.clear();
    r->finalized = true;
    return 0;
}

int vtd_recognizer_crop_resize(vtd_recognizer* r, const uint8_t* frames_dev, int n_frames, int height, int width,
                               const int32_t* boxes_dev, int ncrops, vtd_stream stream) {
    if (!r || !frames_dev || !boxes_dev || n_frames <= 0 || height <= 0 || width <= 0) return ERR_ARG;
    if (!r->finalized) return ERR_NOT_FINALIZED;
    if (ncrops <= 0 || ncrops > r->max_crops) return ERR_BATCH;
    int rc = vtd_launch_crop_resize(frames_dev, n_frames, height, width, boxes_dev, ncrops, r->resized, (hipStream_t)stream);
    if (rc) return rc;
    return vtd_launch_crnn_conv1(r->resized, nullptr, r->w1, r->b1, r->t1.ptr, ncrops, (hipStream_t)stream);
}

int vtd_recognizer_set_input_nchw(vtd_recognizer* r, const float* x_dev, int ncrops, vtd_stream stream) {
    if (!r || !x_dev) return ERR_ARG;
    if (!r->finalized) return ERR_NOT_FINALIZED;
    if (ncrops <= 0 || ncrops > r->max_crops) return ERR_BATCH;
    return vtd_launch_crnn_conv1(nullptr, x_dev, r->w1, r->b1, r->t1.ptr, ncrops, (hipStream_t)stream);
}

int vtd_recognizer_forward(vtd_recognizer* r, int ncrops, float* logits_dev, vtd_stream stream) {
    if (!r || !logits_dev) return ERR_ARG;
    if (!r->finalized) return ERR_NOT_FINALIZED;
    if (ncrops <= 0 || ncrops > r->max_crops) return ERR_BATCH;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    // tile configs are tuned per power-of-two bucket of the crop count (the count changes from batch to batch)
    const int bucket = batch_bucket(ncrops, r->max_crops);
    auto tit = r->tuned.find(bucket);
    const size_t nops = r->ops.size();
    if (tit == r->tuned.end()) {
        std::vector<int> cfgs(nops + 3, -1);
        for (size_t oi = 0; oi < nops; ++oi)
            if (r->ops[oi].kind == Op::CONV && (rc = choose_config(r, r->ops[oi].conv, bucket, s, &cfgs[oi]))) return rc;
        for (int layer = 0; layer < 2; ++layer)
            if ((rc = choose_config(r, r->xs_gemm[layer], bucket, s, &cfgs[nops + layer]))) return rc;
        if ((rc = choose_config(r, r->cls_gemm, bucket, s, &cfgs[nops + 2]))) return rc;
        tit = r->tuned.emplace(bucket, std::move(cfgs)).first;
    }
    const std::vector<int>& cfgs = tit->second;
    for (size_t oi = 0; oi < nops; ++oi) {
        const Op& o = r->ops[oi];
        if (o.kind == Op::CONV) rc = launch_conv_op(o.conv, ncrops, s, cfgs[oi]);
        else rc = vtd_launch_maxpool(o.pin, o.pout, ncrops, o.pk[0], o.pk[1], o.pk[2], o.pk[3], o.pk[4], o.pk[5], s);
        if (rc) return rc;
    }
    half_t* hout[2] = {r->h0.ptr, r->h1.ptr};
    for (int layer = 0; layer < 2; ++layer) {
        if ((rc = launch_conv_op(r->xs_gemm[layer], ncrops, s, cfgs[nops + layer]))) return rc;
        if ((rc = vtd_launch_lstm(r->xs, r->whh[layer], hout[layer], ncrops, 31, s))) return rc;
    }
    if ((rc = launch_conv_op(r->cls_gemm, ncrops, s, cfgs[nops + 2]))) return rc;
    return vtd_launch_compact_rows(r->logits_pad, logits_dev, (int64_t)ncrops * 31, r->vocab, 128, s);
}

int vtd_recognizer_read_tap(vtd_recognizer* r, const char* name, int ncrops, float* host_out, int64_t capacity, vtd_stream stream) {
    if (!r || !name || !host_out) return ERR_ARG;
    if (!r->finalized) return ERR_NOT_FINALIZED;
    if (ncrops <= 0 || ncrops > r->max_crops) return ERR_BATCH;
    if (std::string(name) == "resized") {  // uint8 [n,32,128,3] widened to float
        if (capacity < (int64_t)ncrops * 32 * 128 * 3) return ERR_CAPACITY;
        hipError_t e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) return -(int)e;
        std::vector<uint8_t> tmp((size_t)ncrops * 32 * 128 * 3);
        e = hipMemcpy(tmp.data(), r->resized, tmp.size(), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return -(int)e;
        for (size_t i = 0; i < tmp.size(); ++i) host_out[i] = tmp[i];
        return 0;
    }
    auto it = r->taps.find(name);
    if (it == r->taps.end()) return ERR_UNKNOWN_KEY;
    const TensorDesc& t = it->second;
    if (capacity < (int64_t)ncrops * t.c * t.h * t.w) return ERR_CAPACITY;
    return read_tensor_nchw(t, ncrops, t.c, host_out, (hipStream_t)stream);
}

int64_t vtd_recognizer_macs_per_crop(const vtd_recognizer* r) { return r ? r->macs : 0; }

int vtd_recognizer_set_tuning(vtd_recognizer* r, const char* table_text) {
    if (!r) return ERR_ARG;
    int rc = set_tuning_text(r, table_text);
    if (!rc) r->tuned.clear();
    return rc;
}

int64_t vtd_recognizer_get_tuning(const vtd_recognizer* r, char* buf, int64_t capacity) { return get_tuning_text(r, buf, capacity); }

int vtd_recognizer_tuning_measured(const vtd_recognizer* r) { return r && r->tuning_measured ? 1 : 0; }

int vtd_ctc_greedy_decode(const float* logits_dev, int n, int T, int V, const int32_t* id2char_dev, int blank_id, int apply_softmax,
                          int32_t* out_dev, vtd_stream stream) {
    if (!logits_dev || !id2char_dev || !out_dev || n <= 0) return ERR_ARG;
    return vtd_launch_ctc_greedy(logits_dev, n, T, V, V, id2char_dev, blank_id, apply_softmax, out_dev, (hipStream_t)stream);
}

}  // extern "C"

#include "trocr_graph.inc"
