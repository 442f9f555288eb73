// ResNet BasicBlock training with batch-statistics BatchNorm (torch's train() mode: the statistics of the batch normalise, the running
// statistics are updated in place), forward and backward, for the blocks of ResNet-18's layer1, layer2, layer3 and layer4: (64 -> 64,
// stride 1), (64 -> 128, stride 2, downsample), (128 -> 128, stride 1), (128 -> 256, stride 2, downsample), (256 -> 256, stride 1),
// (256 -> 512, stride 2, downsample) and (512 -> 512, stride 1).  W below is the block's width (64, 128, 256 or 512), a template argument
// of every kernel.  Three entry families share the launch functions, told apart by their error base as in resblock_train.hip:
// vtd_resblock_bn_train_* (-3400: layer4's two geometries, no input gradient of the stride-2 block, -3403), vtd_block_bn_train_* (-3500:
// layer3's and layer4's four geometries, the input gradient of either stride) and vtd_trunk_bn_train_* (-3700: the seven geometries, layer1's
// (64 -> 64, stride 1) and layer2's two under this base alone, the input gradient of either stride; the family that the stem joins later).
// With training = 0 the entries hand the call to the frozen-statistics path (resblock_train.hip) unchanged: the first family to
// vtd_basicblock_train_*, the other two to vtd_resblock_train_*, and the 64-wide geometry to vtd_block64_train_*.
// Tensors are padded taps (ring-padded NHWC fp16, ring 1).  y = relu(bn2(conv2(relu(bn1(conv1(x))))) + id), id = x or ds_bn(ds(x)).
//
// Forward, per convolution + BatchNorm pair (conv1 / bn1, the downsample, conv2 / bn2):
//   pack             the raw weights -> fp16 GEMM panel [W][ksz^2 cin] (k = tap * cin + ci); no fold: gamma rstd is not known yet
//   conv             conv_igemm.hip with EPI_OUT_F32 and a zero bias: z [M][W] fp32, kept in the workspace for the backward
//   stats partial    workgroup g owns rows g per .. g per + per - 1 (per = ceil(M / G), G = min(256, ceil(M / 256))).  W / 4 threads cover the
//                    width, 4 channels each with 16-byte loads, so the 256 threads are P = 1024 / W parts of the workgroup's r rows: part k
//                    sums rows ceil(k r / P) .. ceil((k + 1) r / P) - 1 in row order, sums of z and z^2 in fp64.
//                    W = 512: two halves, lower + upper.  W = 256: four quarters, (q0 + q1) + (q2 + q3) -- the rule of rb_reduce64_kernel.
//                    W = 128: eight eighths, ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7)).  W = 64: sixteen parts of 16 lanes, the
//                    eight-part order on each half, then lower + upper: (((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7))) +
//                    (((q8 + q9) + (q10 + q11)) + ((q12 + q13) + (q14 + q15))).  A part without rows (r < P) adds exact zeros.
//                    Then (count, mean, M2) per channel
//   stats finish     one thread per channel: Chan's combination of the partials in workgroup order (fp64) -> mu, biased sigma^2; the running
//                    values mean <- (1 - m) mean + m mu, var <- (1 - m) var + m sigma^2 M / (M - 1); table {mu, rstd, gamma, beta} [4][W]
//   apply            relu(((z - mu) rstd) gamma + beta [+ id]) -> ring-padded fp16 tap; the downsample's has no ReLU.  One thread = 8 channels
// Backward from dy (NHWC fp32 times a power of two):
//   mask             g2 = dy (y > 0): the gradient at bn2's output, of the downsample's BatchNorm output, and of an identity input
//   reduce           per pair, g the gradient at the BatchNorm output, xh = (z - mu) rstd from the saved z: s1 = sum g, s2 = sum g xh in fp64,
//                    max |g| and max |xh| per channel; rows and threads as in `stats partial`
//   finish           partials in workgroup order; dbeta = s1, dgamma = s2 (scale undone); the table {gamma rstd, s1 / M, s2 / M}; the
//                    power-of-two multiplier from max_c |gamma rstd| (max |g| + |s1| / M + max |xh| |s2| / M), which bounds |dz|
//   form             dz = gamma rstd (g - s1 / M - xh s2 / M) in fp32, times the multiplier, as fp16: flat [M][W] and ring-padded
//   wgrad<3>         G[c][k] = sum_m dz[m][c] x[m][k] on wgrad_mfma.h, min(8, ceil(M / 4096)) slabs; dW = the slabs summed in order in fp64
//                    with the scale undone: dz carries gamma rstd, no factor follows.  W = 128 has one column tile, so it takes the rule
//                    of resblock_train.hip's 128-wide blocks: wgrad<4> over layer2.0's 64-channel input (a tap per 64-column group), wgrad<3>
//                    otherwise, ceil(ksz^2 cin / 128) q-tiles and per launch min(ceil(512 / q-tiles), ceil(M / 1024)) slabs
//   wgrad<5>         W = 64 (layer1): the 64-row tile over dz [M][64] (lda = 64) and the 64-channel input, K = 576 = 5 q-tiles for conv2
//                    and conv1 alike, min(ceil(512 / 5), ceil(M / 1024)) slabs of [64][576] floats: the rule of resblock_train.hip's
//                    64-wide block
//   dgrad            da1 = conv2^T(dz2): conv_igemm.hip on the raw weights rotated by 180 degrees and transposed; g1 = da1 (a1 > 0)
//   dx (stride 1)    conv1^T(dz1) the same way, plus g2 brought to the same scale
//   dx (stride 2)    (vtd_block_bn_train_* and vtd_trunk_bn_train_*) the construction of resblock_train.hip on the batch-statistics
//                    quantities: dz1 goes to the even positions of a zeroed ring-padded plane of the input's 2h x 2w pixels (`form` with
//                    dil = 2), the stride-1 3x3 dgrad runs over that plane on the raw conv1 weights, rotated and transposed.  The
//                    downsample's transpose is a 1x1 GEMM of dz_d, the downsample BatchNorm's own dz (not g2, not dz2: each pair has
//                    its own statistics), on the transposed raw downsample weights; it runs right after the downsample pair's `form`, into a buffer of its own, because the dz planes are reused
//                    by bn1.  dz_d carries its own power-of-two multiplier scd[2]; the product is added at the even (row, column) positions
//                    times sc2[2] sc1[2] / scd[2], which brings it to dz1's scale exactly
// Nothing divides by gamma or sigma.  No atomics, shape-only grids, fixed summation orders: bitwise repeatable.
// The bt_* kernels live in resblock_bn_common.h, unchanged, where bottleneck_bn_train.hip (ResNet-50's Bottlenecks) finds them too.
#include "resblock_bn_common.h"

#include "conv_kernels.h"
int64_t vtd_basicblock_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_basicblock_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                  void* ws, void* y, hipStream_t s);
int vtd_launch_basicblock_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                   const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch,
                                   float* dx, float* dxscale, hipStream_t s);

int64_t vtd_block64_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_block64_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps, void* ws,
                               void* y, hipStream_t s);
int vtd_launch_block64_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch,
                                float* dx, float* dxscale, hipStream_t s);

int64_t vtd_resblock_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_resblock_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps, void* ws,
                                void* y, hipStream_t s);
int vtd_launch_resblock_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                 const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch,
                                 float* dx, float* dxscale, hipStream_t s);

namespace {

// error bases: the vtd_resblock_bn_train_* entries (layer4's two geometries, no strided dx) answer -3401 / -3402 / -3403, the
// vtd_block_bn_train_* entries (four geometries) -3501 / -3502, the vtd_trunk_bn_train_* entries (seven geometries: layer2's 128-wide
// blocks and layer1's 64-wide block under this base alone) -3701 / -3702
constexpr int BT_LEGACY = -3400, BT_GENERAL = -3500, BT_TRUNK = -3700;

struct Geo {
    int n, hin, win, cin, width, stride, h, w;
    int64_t m;
    bool ds;
    int red;       // reduce workgroups
    int64_t per;   // rows of each
};

bool make_geo(int n, int hin, int win, int cin, int width, int stride, int base, Geo& g) {
    if (n <= 0 || hin <= 0 || win <= 0 || n > 65535 || hin > 4096 || win > 4096) return false;
    if (width == 64) {   // layer1's block alone, written out: the rule below would admit (32, 64, 2)
        if (base != BT_TRUNK || cin != 64 || stride != 1) return false;
    } else {
        if (width != 512 && (base == BT_LEGACY || width != 256) && (base != BT_TRUNK || width != 128)) return false;
        if (!((cin == width / 2 && stride == 2 && !(hin & 1) && !(win & 1)) || (cin == width && stride == 1))) return false;
    }
    g.n = n; g.hin = hin; g.win = win; g.cin = cin; g.width = width; g.stride = stride; g.h = hin / stride; g.w = win / stride;
    g.m = (int64_t)n * g.h * g.w;
    g.ds = stride == 2;
    int64_t r = (g.m + 255) / 256;
    g.red = (int)(r < 1 ? 1 : r > BT_MAX_RED ? BT_MAX_RED : r);
    g.per = (g.m + g.red - 1) / g.red;
    return (int64_t)n * (hin + 2) * (win + 2) * width < (1ll << 31);
}

// the workspace of a training = 1 forward.  tab: {mu, rstd, gamma, beta} [4][W] per pair (bn1, bn2, the downsample's)
struct FwdLayout { int64_t a1, id, z1, z2, zd, w1, w2, wd, zero, part, tab, total; };
struct BwdLayout { int64_t g2, g1, dzh, dzp, wt, zero, part, pmax, coef, sc, slab, zp, wdt, dst, total; };

FwdLayout fwd_layout(const Geo& g) {
    FwdLayout L;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    const int64_t W = g.width, pad = (int64_t)g.n * (g.h + 2) * (g.w + 2) * W * 2, zb = g.m * W * 4;
    L.a1 = take(pad); L.id = take(g.ds ? pad : 0);
    L.z1 = take(zb); L.z2 = take(zb); L.zd = take(g.ds ? zb : 0);
    L.w1 = take(W * 9 * g.cin * 2); L.w2 = take(W * 9 * W * 2); L.wd = take(g.ds ? W * g.cin * 2 : 0);
    L.zero = take(W * 4);
    L.part = take((int64_t)BT_MAX_RED * W * 3 * 8);
    L.tab = take(3 * 4 * W * 4);
    L.total = o;
    return L;
}

// `strided`: room for the stride-2 block's input gradient (the zero-inserted plane, the downsample's transposed panel and ds^T(dz_d)), at
// the end
BwdLayout bwd_layout(const Geo& g, bool strided) {
    BwdLayout L;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    const int64_t W = g.width, pad = (int64_t)g.n * (g.h + 2) * (g.w + 2) * W * 2;
    L.g2 = take(g.m * W * 4); L.g1 = take(g.m * W * 4);
    L.dzh = take(g.m * W * 2); L.dzp = take(pad);
    L.wt = take(W * 9 * W * 2);
    L.zero = take(W * 4);
    L.part = take((int64_t)BT_MAX_RED * 2 * W * 8); L.pmax = take((int64_t)BT_MAX_RED * 2 * W * 4);
    L.coef = take(3 * W * 4);
    L.sc = take(3 * 4 * 4);
    int64_t slab = (int64_t)wg_slabs(g.m) * W * 9 * W;
    if (W == 64) slab = (int64_t)wg_slabs128(g.m, wg_nqt(3, 64)) * 64 * 9 * 64;   // conv2 and conv1 alike: 5 q-tiles, slab [64][576]
    if (W == 128) {   // per launch (conv2, conv1, the downsample), as resblock_train.hip sizes it: the largest of the three
        slab = (int64_t)wg_slabs128(g.m, wg_nqt(3, 128)) * W * 9 * 128;
        const int64_t c1 = (int64_t)wg_slabs128(g.m, wg_nqt(3, g.cin)) * W * 9 * g.cin, dsl = g.ds ? (int64_t)wg_slabs128(g.m, wg_nqt(1, g.cin)) * W * g.cin : 0;
        slab = c1 > slab ? c1 : slab;
        slab = dsl > slab ? dsl : slab;
    }
    L.slab = take(slab * 4);
    L.zp = take(strided ? (int64_t)g.n * (g.hin + 2) * (g.win + 2) * W * 2 : 0);
    L.wdt = take(strided ? (int64_t)g.cin * W * 2 : 0);
    L.dst = take(strided ? g.m * g.cin * 4 : 0);
    L.total = o;
    return L;
}

int64_t ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode, int base) {
    Geo g;
    if (!make_geo(n, hin, win, cin, width, stride, base, g) || mode < 0 || mode > 1) return base - 1;
    const bool general = base != BT_LEGACY;
    // either mode of `training` runs in one allocation: the frozen path's layout starts at offset 0 too
    const int64_t frozen = width == 64 ? vtd_block64_ws_bytes(n, hin, win, cin, width, stride, mode)
                           : general   ? vtd_resblock_ws_bytes(n, hin, win, cin, width, stride, mode)
                                       : vtd_basicblock_ws_bytes(n, hin, win, cin, width, stride, mode);
    const int64_t own = mode ? bwd_layout(g, general && g.ds).total : fwd_layout(g).total;
    if (frozen < 0) return base - 1;
    return frozen > own ? frozen : own;
}

template <int W>
int forward_launches(const void* x, const Geo& g, const vtd_basicblock_params* P, float momentum, float eps, void* ws, void* y, float* stats,
                     hipStream_t s) {
    const FwdLayout L = fwd_layout(g);
    const int n = g.n, hin = g.hin, win = g.win, cin = g.cin, stride = g.stride;
    const int64_t M = g.m;
    char* w = (char*)ws;
    half_t *a1 = (half_t*)(w + L.a1), *id = (half_t*)(w + L.id), *w1 = (half_t*)(w + L.w1), *w2 = (half_t*)(w + L.w2), *wd = (half_t*)(w + L.wd);
    float *z1 = (float*)(w + L.z1), *z2 = (float*)(w + L.z2), *zd = (float*)(w + L.zd), *zero = (float*)(w + L.zero), *tab = (float*)(w + L.tab);
    double* part = (double*)(w + L.part);
    hipLaunchKernelGGL(bt_pack_kernel<W>, dim3(nblk((int64_t)W * 9 * cin + W)), dim3(BT_THREADS), 0, s, (const float*)P->conv1_w, cin, 9, w1, zero);
    hipLaunchKernelGGL(bt_pack_kernel<W>, dim3(nblk((int64_t)W * 9 * W)), dim3(BT_THREADS), 0, s, (const float*)P->conv2_w, W, 9, w2, (float*)nullptr);
    if (g.ds) hipLaunchKernelGGL(bt_pack_kernel<W>, dim3(nblk((int64_t)W * cin)), dim3(BT_THREADS), 0, s, (const float*)P->ds_w, cin, 1, wd, (float*)nullptr);
    const unsigned ring = nblk((int64_t)n * (2 * (g.w + 2) + 2 * g.h) * (W / 8));
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring), dim3(RB_THREADS), 0, s, a1, n, g.h, g.w, W);
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring), dim3(RB_THREADS), 0, s, (half_t*)y, n, g.h, g.w, W);
    if (g.ds) hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring), dim3(RB_THREADS), 0, s, id, n, g.h, g.w, W);
    VTD_HIP_CHECK(hipGetLastError());

    // a convolution of a padded tap into z [M][W] fp32: zero bias, no activation
    auto conv_f32 = [&](const half_t* in, int ic, int hi, int wi, int ksz, int st, const half_t* wp, float* z) {
        ConvParams c = conv_of(n, g.h, g.w, W, in, ic, hi, wi, ksz, st, wp, zero);
        c.out = z; c.ldc = W; c.flags = EPI_OUT_F32;
        return vtd_launch_conv(c, -1, s);
    };
    // one pair: conv -> z, the batch statistics (and the running update), the normalised tap
    auto pair = [&](const half_t* in, int ic, int hi, int wi, int ksz, int st, const half_t* wp, float* z, int row, const float* gam, const float* bet,
                    float* rmean, float* rvar, const half_t* res, int relu, half_t* out) {
        const int rc = conv_f32(in, ic, hi, wi, ksz, st, wp, z);
        if (rc) return rc;
        hipLaunchKernelGGL(bt_stats_partial_kernel<W>, dim3(g.red), dim3(BT_THREADS), 0, s, (const float*)z, M, g.per, part);
        hipLaunchKernelGGL(bt_stats_finish_kernel<W>, dim3((W + BT_THREADS - 1) / BT_THREADS), dim3(BT_THREADS), 0, s, (const double*)part, g.red, gam, bet, rmean, rvar, momentum,
                           eps, tab + row * 4 * W, stats ? stats + row * 2 * W : (float*)nullptr);
        hipLaunchKernelGGL(bt_apply_kernel<W>, dim3(nblk(M * (W / 8))), dim3(BT_THREADS), 0, s, (const float*)z, M, (const float*)(tab + row * 4 * W), res,
                           relu, g.h, g.w, out);
        return -(int)hipGetLastError();
    };
    int rc;
    if ((rc = pair((const half_t*)x, cin, hin, win, 3, stride, w1, z1, 0, P->bn1_w, P->bn1_b, P->bn1_mean, P->bn1_var, nullptr, 1, a1))) return rc;
    if (g.ds && (rc = pair((const half_t*)x, cin, hin, win, 1, 2, wd, zd, 2, P->ds_bn_w, P->ds_bn_b, P->ds_bn_mean, P->ds_bn_var, nullptr, 0, id))) return rc;
    return pair(a1, W, g.h, g.w, 3, 1, w2, z2, 1, P->bn2_w, P->bn2_b, P->bn2_mean, P->bn2_var, g.ds ? id : (const half_t*)x, 1, (half_t*)y);
}

int launch_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training, float momentum,
                   float eps, void* ws, void* y, float* stats, hipStream_t s, int base) {
    Geo g;
    if (!x || !ws || !y || !make_geo(n, hin, win, cin, width, stride, base, g) || !params_ok(P, g.ds) || !(eps > 0.f) || (training != 0 && training != 1))
        return base - 1;
    if (training && (g.m < 2 || !(momentum >= 0.f && momentum <= 1.f))) return base - 1;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)ws & 255) || ((uintptr_t)stats & 3)) return base - 2;
    if (!training && width == 64) return vtd_launch_block64_forward(x, n, hin, win, cin, width, stride, P, eps, ws, y, s);
    if (!training)
        return base == BT_LEGACY ? vtd_launch_basicblock_forward(x, n, hin, win, cin, width, stride, P, eps, ws, y, s)
                                 : vtd_launch_resblock_forward(x, n, hin, win, cin, width, stride, P, eps, ws, y, s);
    if (width == 64) return forward_launches<64>(x, g, P, momentum, eps, ws, y, stats, s);
    if (width == 128) return forward_launches<128>(x, g, P, momentum, eps, ws, y, stats, s);
    return width == 256 ? forward_launches<256>(x, g, P, momentum, eps, ws, y, stats, s) : forward_launches<512>(x, g, P, momentum, eps, ws, y, stats, s);
}

template <int W>
int backward_launches(const void* x, const Geo& g, const vtd_basicblock_params* P, const void* ws, const void* y, const float* dy, const float* dscale,
                      const vtd_basicblock_params* Gp, void* scratch, float* dx, float* dxscale, hipStream_t s, bool general) {
    const FwdLayout L = fwd_layout(g);
    const BwdLayout B = bwd_layout(g, general && g.ds);
    const int n = g.n, hin = g.hin, win = g.win, cin = g.cin, stride = g.stride;
    const int64_t M = g.m;
    const char* w = (const char*)ws;
    char* q = (char*)scratch;
    const half_t* a1 = (const half_t*)(w + L.a1);
    const float *z1 = (const float*)(w + L.z1), *z2 = (const float*)(w + L.z2), *zd = (const float*)(w + L.zd), *tab = (const float*)(w + L.tab);
    float *g2 = (float*)(q + B.g2), *g1 = (float*)(q + B.g1), *zero = (float*)(q + B.zero), *pmax = (float*)(q + B.pmax), *coef = (float*)(q + B.coef),
          *sc = (float*)(q + B.sc), *slab = (float*)(q + B.slab);
    half_t *dzh = (half_t*)(q + B.dzh), *dzp = (half_t*)(q + B.dzp), *wt = (half_t*)(q + B.wt);
    double* part = (double*)(q + B.part);
    float *sc2 = sc, *scd = sc + 4, *sc1 = sc + 8;
    const unsigned ring = nblk((int64_t)n * (2 * (g.w + 2) + 2 * g.h) * (W / 8));
    const int S = wg_slabs(M);
    const double inv_m = 1.0 / (double)M;
    const bool strided_dx = dx && g.ds;      // the general entries only: the others refused it

    // one pair's BatchNorm backward: the two channel sums, dgamma / dbeta, the scale, dz as the fp16 operands: flat, and (when `plane` is given)
    // the interior of the ring-padded dzp (dil = 1) or the even positions of the zeroed plane of the input's extent (dil = 2)
    auto bn_back = [&](const float* gr, const float* z, int row, const float* in_sc, float* out_sc, float* dgam, float* dbet, half_t* plane, int dil) {
        const float* t = tab + row * 4 * W;
        hipLaunchKernelGGL(bt_bwd_reduce_kernel<W>, dim3(g.red), dim3(BT_THREADS), 0, s, gr, z, t, M, g.per, part, pmax);
        hipLaunchKernelGGL(bt_bwd_finish_kernel<W>, dim3(1), dim3(W), 0, s, (const double*)part, (const float*)pmax, g.red, inv_m, t, in_sc, coef, dgam, dbet,
                           out_sc);
        if (plane && dil == 1) hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring), dim3(RB_THREADS), 0, s, plane, n, g.h, g.w, W);
        hipLaunchKernelGGL(bt_form_kernel<W>, dim3(nblk(M * (W / 8))), dim3(BT_THREADS), 0, s, gr, z, t, (const float*)coef, (const float*)out_sc, M, g.h, g.w,
                           dil, dzh, plane);
    };
    auto wgrad = [&](const half_t* xin, int xc, int hi, int wi, int ksz, int st, const float* scl, float* dw) {
        WgArgs wa;
        wa.a = dzh; wa.lda = W; wa.x = xin; wa.xc = xc; wa.n = n; wa.H = g.h; wa.W = g.w; wa.rows = M; wa.slab = slab;
        // W <= 128: one column tile, so the slabs of each launch by its own q-tiles (the rule of resblock_train.hip's 128- and 64-wide blocks)
        const int nqt = W <= 128 ? wg_nqt(ksz, xc) : ksz * ksz * xc / 128, Sl = W <= 128 ? wg_slabs128(M, nqt) : S;
        wa.slab_len = slab_rows(M, Sl); wa.ksz = ksz; wa.stride = st; wa.Hin = hi; wa.Win = wi;
        if (W == 64)   // layer1: the 64-row tile, one column tile, slab [64][576]
            hipLaunchKernelGGL(dbhead_train_wgrad_kernel<5>, dim3(nqt * Sl, 1), dim3(WG_THREADS), 0, s, wa);
        else if (xc & 127)   // layer2.0's 64-channel input: a tap per 64-column group
            hipLaunchKernelGGL(dbhead_train_wgrad_kernel<4>, dim3(nqt * Sl, W / 128), dim3(WG_THREADS), 0, s, wa);
        else
            hipLaunchKernelGGL(dbhead_train_wgrad_kernel<3>, dim3(nqt * Sl, W / 128), dim3(WG_THREADS), 0, s, wa);
        hipLaunchKernelGGL(bt_dw_kernel, dim3(W), dim3(BT_THREADS), 0, s, (const float*)slab, Sl, xc, ksz * ksz, scl, dw);
    };
    // conv^T of a padded dz plane of hp x wp pixels (W channels) into [n hp wp][rows] fp32: the raw weights of a conv with `rows` input
    // channels, rotated and transposed into `panel`
    auto dgrad = [&](const half_t* gp, int hp, int wp, const float* wsrc, int rows, int ksz, half_t* panel, float* out) {
        hipLaunchKernelGGL(bt_pack_dgrad_kernel<W>, dim3(nblk((int64_t)rows * ksz * ksz * W + W)), dim3(BT_THREADS), 0, s, wsrc, rows, ksz * ksz, panel, zero);
        ConvParams c = conv_of(n, hp, wp, rows, gp, W, hp, wp, ksz, 1, panel, zero);
        c.out = out; c.ldc = rows; c.flags = EPI_OUT_F32;
        return vtd_launch_conv(c, -1, s);
    };

    int rc;
    hipLaunchKernelGGL(rb_mask_kernel, dim3(nblk(M * (W / 4))), dim3(RB_THREADS), 0, s, dy, (const half_t*)y, M, g.h, g.w, W, g2);
    bn_back(g2, z2, 1, dscale, sc2, Gp->bn2_w, Gp->bn2_b, dzp, 1);
    wgrad(a1, W, g.h, g.w, 3, 1, sc2, Gp->conv2_w);
    VTD_HIP_CHECK(hipGetLastError());
    // da1 = conv2^T(dz2) into the g1 buffer, masked in place by a1 > 0
    if ((rc = dgrad(dzp, g.h, g.w, (const float*)P->conv2_w, W, 3, wt, g1))) return rc;
    if (g.ds) {   // the downsample pair: its upstream gradient is g2
        bn_back(g2, zd, 2, dscale, scd, Gp->ds_bn_w, Gp->ds_bn_b, strided_dx ? dzp : (half_t*)nullptr, 1);
        wgrad((const half_t*)x, cin, hin, win, 1, 2, scd, Gp->ds_w);
        // ds^T(dz_d) at dz_d's scale into a buffer of its own, now: bn1's pair takes the dz operands next
        if (strided_dx && (rc = dgrad(dzp, g.h, g.w, (const float*)P->ds_w, cin, 1, (half_t*)(q + B.wdt), (float*)(q + B.dst)))) return rc;
    }
    hipLaunchKernelGGL(rb_mask_kernel, dim3(nblk(M * (W / 4))), dim3(RB_THREADS), 0, s, (const float*)g1, a1, M, g.h, g.w, W, g1);
    if (strided_dx) VTD_HIP_CHECK(hipMemsetAsync(q + B.zp, 0, (size_t)n * (hin + 2) * (win + 2) * W * 2, s));
    bn_back(g1, z1, 0, sc2, sc1, Gp->bn1_w, Gp->bn1_b, strided_dx ? (half_t*)(q + B.zp) : dx ? dzp : (half_t*)nullptr, strided_dx ? 2 : 1);
    wgrad((const half_t*)x, cin, hin, win, 3, stride, sc1, Gp->conv1_w);
    VTD_HIP_CHECK(hipGetLastError());
    if (dx && !g.ds) {
        if ((rc = dgrad(dzp, g.h, g.w, (const float*)P->conv1_w, W, 3, wt, dx))) return rc;
        hipLaunchKernelGGL(rb_add_identity_kernel, dim3(nblk(M * (W / 4))), dim3(RB_THREADS), 0, s, dx, (const float*)g2, M * (W / 4), (const float*)sc2,
                           (const float*)sc1);
        hipLaunchKernelGGL(rb_copy_scale_kernel, dim3(1), dim3(64), 0, s, (const float*)sc1, dxscale);
    } else if (dx) {
        // dz1 sits at the even positions of the zeroed plane of the input's size: the stride-1 path over it, see the head of this file
        if ((rc = dgrad((const half_t*)(q + B.zp), hin, win, (const float*)P->conv1_w, cin, 3, wt, dx))) return rc;
        hipLaunchKernelGGL(bt_add_downsample_kernel, dim3(nblk(M * (cin / 4))), dim3(BT_THREADS), 0, s, dx, (const float*)(q + B.dst), M, g.h, g.w, cin,
                           (const float*)sc2, (const float*)sc1, (const float*)scd);
        hipLaunchKernelGGL(rb_copy_scale_kernel, dim3(1), dim3(64), 0, s, (const float*)sc1, dxscale);
    }
    return -(int)hipGetLastError();
}

int launch_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training, float eps,
                    const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch, float* dx,
                    float* dxscale, hipStream_t s, int base) {
    Geo g;
    const bool legacy = base == BT_LEGACY;
    if (!x || !ws || !y || !dy || !dscale || !scratch || !make_geo(n, hin, win, cin, width, stride, base, g) || !params_ok(P, g.ds) || !grads_ok(Gp, g.ds) ||
        !(eps > 0.f) || (dx && !dxscale) || (training != 0 && training != 1) || (training && g.m < 2))
        return base - 1;
    if (legacy && dx && g.stride != 1) return base - 3;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)ws & 255) || ((uintptr_t)scratch & 255) || ((uintptr_t)dy & 15) || ((uintptr_t)dscale & 7) ||
        ((uintptr_t)dx & 15) || ((uintptr_t)dxscale & 7))
        return base - 2;
    if (!training && width == 64) return vtd_launch_block64_backward(x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s);
    if (!training)
        return legacy ? vtd_launch_basicblock_backward(x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s)
                      : vtd_launch_resblock_backward(x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s);
    if (width == 64) return backward_launches<64>(x, g, P, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s, !legacy);
    if (width == 128) return backward_launches<128>(x, g, P, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s, !legacy);
    return width == 256 ? backward_launches<256>(x, g, P, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s, !legacy)
                        : backward_launches<512>(x, g, P, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s, !legacy);
}

}  // namespace

int64_t vtd_resblock_bn_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    return ws_bytes(n, hin, win, cin, width, stride, mode, BT_LEGACY);
}

int vtd_launch_resblock_bn_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                   float momentum, float eps, void* ws, void* y, float* stats, hipStream_t s) {
    return launch_forward(x, n, hin, win, cin, width, stride, P, training, momentum, eps, ws, y, stats, s, BT_LEGACY);
}

int vtd_launch_resblock_bn_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                    float eps, const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp,
                                    void* scratch, float* dx, float* dxscale, hipStream_t s) {
    return launch_backward(x, n, hin, win, cin, width, stride, P, training, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s, BT_LEGACY);
}

// the four geometries of layer3 and layer4, with the input gradient of the stride-2 blocks
int64_t vtd_block_bn_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    return ws_bytes(n, hin, win, cin, width, stride, mode, BT_GENERAL);
}

int vtd_launch_block_bn_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                float momentum, float eps, void* ws, void* y, float* stats, hipStream_t s) {
    return launch_forward(x, n, hin, win, cin, width, stride, P, training, momentum, eps, ws, y, stats, s, BT_GENERAL);
}

int vtd_launch_block_bn_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                 float eps, const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp,
                                 void* scratch, float* dx, float* dxscale, hipStream_t s) {
    return launch_backward(x, n, hin, win, cin, width, stride, P, training, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s, BT_GENERAL);
}

// the seven geometries of layer1, layer2, layer3 and layer4, with the input gradient of the stride-2 blocks: the family that the stem joins
int64_t vtd_trunk_bn_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    return ws_bytes(n, hin, win, cin, width, stride, mode, BT_TRUNK);
}

int vtd_launch_trunk_bn_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                float momentum, float eps, void* ws, void* y, float* stats, hipStream_t s) {
    return launch_forward(x, n, hin, win, cin, width, stride, P, training, momentum, eps, ws, y, stats, s, BT_TRUNK);
}

int vtd_launch_trunk_bn_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                 float eps, const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp,
                                 void* scratch, float* dx, float* dxscale, hipStream_t s) {
    return launch_backward(x, n, hin, win, cin, width, stride, P, training, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s, BT_TRUNK);
}
