// ResNet BasicBlock training with frozen-statistics BatchNorm (the running statistics normalise and are never written; gamma and beta
// learn), forward and backward, for the blocks of ResNet-18's layer2, layer3 and layer4: (64 -> 128, stride 2, downsample), (128 -> 128,
// stride 1), (128 -> 256, stride 2, downsample), (256 -> 256, stride 1), (256 -> 512, stride 2, downsample) and (512 -> 512, stride 1);
// and for layer1's (64 -> 64, stride 1) behind entries of its own (vtd_block64_train_*).  W below is the block's width (64, 128, 256 or
// 512), a launch argument.
// Tensors are padded taps (ring-padded NHWC fp16, ring 1).  y = relu(bn2(conv2(relu(bn1(conv1(x))))) + id), id = x or ds_bn(ds(x)).
//
// Forward:
//   fold             per convolution: w gamma rstd -> fp16 GEMM panel [W][ksz^2 cin] (k = tap * cin + ci), bias = beta - mean gamma rstd;
//                    on the device, every call
//   conv x 2 or 3    conv_igemm.hip: conv1 (3x3, stride s, ReLU) -> padded a1; downsample (1x1, stride 2) -> padded id; conv2 (3x3,
//                    EPI_RESIDUAL from id or x, ReLU) -> padded y.  a1 and id stay in the workspace
// Backward from dy (NHWC fp32 times a power of two):
//   mask             g2 = dy (y > 0) in fp32: the gradient at bn2's output and of the identity path
//   reduce / finish  per-channel fp64 sums s_c in a fixed order, max |.|, a power-of-two scale; form: the fp16 operands (flat and ring-padded).
//                    W = 128: the 256 threads of a workgroup are two halves of 128 channels; the lower half sums the first ceil(r / 2) of
//                    the workgroup's r rows in row order, the upper half the rest, and the partial is lower + upper
//                    W = 64: four quarters of 64 channels; quarter k sums rows ceil(k r / 4) .. ceil((k + 1) r / 4) - 1 of the workgroup's r
//                    rows in row order, and the partial is (q0 + q1) + (q2 + q3)
//   wgrad<3>         G[c][k] = sum_m g[m][c] x[m][k] on wgrad_mfma.h (W / 128 128-column tiles; 3x3 / 1x1 gather at stride 1 / 2), slabs.
//   wgrad<4>         the same over layer2.0's 64-channel input (conv1: K = 576, the downsample: K = 64): a 64-column group per tap.
//                    Slabs: W = 256 and 512 cut the rows into min(8, ceil(rows / 4096)) slabs for every launch of a block.  W = 128 has
//                    one column tile, so each launch takes min(ceil(512 / q-tiles), ceil(rows / 1024)) slabs: two workgroups per CU of
//                    the 256 when the rows allow slabs of 1024 (conv2 and layer2.1's conv1, 9 q-tiles: 57; layer2.0's conv1, 5: 103; its
//                    downsample, 1: 512)
//   wgrad<5>         W = 64 (layer1): the 64-row tile over the 64-channel input, K = 576 = 5 q-tiles (the last half empty), slab
//                    [64][576]; slabs by the 128-wide rule: min(ceil(512 / 5), ceil(rows / 1024)) = min(103, .)
//   param            slabs summed in order in fp64; dW = gamma rstd G, dbeta = s, dgamma = rstd (sum_k w G - mean s): no division by gamma
//   dgrad            da1 = conv2^T(g2): conv_igemm.hip on the folded weights rotated by 180 degrees and transposed; g1 = da1 (a1 > 0)
//   dx (stride 1)    conv1^T(g1) the same way, plus g2 brought to the same scale
//   dx (stride 2)    at the input's 2h x 2w: input row i receives tap t of output row o where 2 o + t - 1 = i.  g1 is written into a zeroed
//                    ring-padded plane Z of 2h x 2w pixels at the even positions (Z[2o][2p] = g1[o][p]); then dx[i] = sum_t' Z[i + t' - 1]
//                    w[2 - t'], the stride-1 3x3 path on the rotated, transposed folded weights: even rows meet a non-zero Z at the
//                    centre tap only, odd rows at the two outer taps, and row 2h - 1 reads the ring (zero) for o = h.  The downsample's
//                    transpose is a 1x1 GEMM of g2 on the transposed folded weights, added at the even (row, column) positions after
//                    the power-of-two multiplier that brings it to g1's scale.  (The new entries only: vtd_resblock_train_*.)
// No atomics, shape-only grids, fixed summation orders: bitwise repeatable.
// The ring, mask and identity-add kernels, the argument checks and the convolution descriptor are in resblock_common.h, shared with
// resblock_bn_train.hip; so are the kernels that take every width from their launch (fold, the 256 / 512-wide reduce, finish, form, the
// dgrad panel, param), which bottleneck_train.hip runs too.
#include "resblock_common.h"

#include <cstring>

#include "conv_kernels.h"

namespace {

constexpr int RB_MAX_RED = 256;
// error bases: the vtd_basicblock_train_* entries (layer4's two geometries, no strided dgrad) answer -3001 / -3002 / -3003, the
// vtd_resblock_train_* entries (six geometries) -3101 / -3102, the vtd_block64_train_* entries (layer1's 64 -> 64 stride 1 alone)
// -3201 / -3202
constexpr int RB_LEGACY = -3000, RB_GENERAL = -3100, RB_NARROW = -3200;

struct Geo {
    int n, hin, win, cin, width, stride, h, w;
    int64_t m;
    bool ds;
};

bool make_geo(int n, int hin, int win, int cin, int width, int stride, int base, Geo& g) {
    const bool legacy = base == RB_LEGACY;
    if (n <= 0 || hin <= 0 || win <= 0 || n > 65535 || hin > 4096 || win > 4096) return false;
    if (base == RB_NARROW) {   // layer1's block and nothing else; width 64 under no other base
        if (width != 64 || cin != 64 || stride != 1) return false;
    } else if (width != 512 && (legacy || (width != 256 && width != 128))) {
        return false;
    }
    if (!((cin == width / 2 && stride == 2 && !(hin & 1) && !(win & 1)) || (cin == width && stride == 1))) return false;
    g.n = n; g.hin = hin; g.win = win; g.cin = cin; g.width = width; g.stride = stride; g.h = hin / stride; g.w = win / stride;
    g.m = (int64_t)n * g.h * g.w;
    g.ds = stride == 2;
    return (int64_t)n * (hin + 2) * (win + 2) * width < (1ll << 31);
}

struct FwdLayout { int64_t a1, id, w1, w2, wd, bias, total; };
struct BwdLayout { int64_t g2, g1, g2h, g1h, g2p, g1p, wt, zero, part, pmax, sum2, sum1, sc, slab, zp, wdt, total; };

FwdLayout fwd_layout(const Geo& g) {
    FwdLayout L;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    const int64_t W = g.width, pad = (int64_t)g.n * (g.h + 2) * (g.w + 2) * W * 2;
    L.a1 = take(pad); L.id = take(g.ds ? pad : 0);
    L.w1 = take(W * 9 * g.cin * 2); L.w2 = take(W * 9 * W * 2); L.wd = take(g.ds ? W * g.cin * 2 : 0);
    L.bias = take(3 * W * 4);
    L.total = o;
    return L;
}

// `strided`: room for the stride-2 block's input gradient (the zero-inserted plane and the downsample's transposed panel), at the end
BwdLayout bwd_layout(const Geo& g, bool strided) {
    BwdLayout L;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    const int64_t W = g.width, pad = (int64_t)g.n * (g.h + 2) * (g.w + 2) * W * 2;
    L.g2 = take(g.m * W * 4); L.g1 = take(g.m * W * 4);
    L.g2h = take(g.m * W * 2); L.g1h = take(g.m * W * 2);
    L.g2p = take(pad); L.g1p = take(pad);
    L.wt = take(W * 9 * W * 2);
    L.zero = take(W * 4);
    L.part = take((int64_t)RB_MAX_RED * W * 8); L.pmax = take(RB_MAX_RED * 4);
    L.sum2 = take(W * 8); L.sum1 = take(W * 8);
    L.sc = take(2 * 4 * 4);
    int64_t slab = (int64_t)wg_slabs(g.m) * W * 9 * W;
    if (W == 64) slab = (int64_t)wg_slabs128(g.m, wg_nqt(3, 64)) * 64 * 9 * 64;   // conv2 and conv1 alike: 5 q-tiles, slab [64][576]
    if (W == 128) {   // per launch: conv2, conv1, the downsample
        slab = (int64_t)wg_slabs128(g.m, wg_nqt(3, 128)) * W * 9 * 128;
        const int64_t c1 = (int64_t)wg_slabs128(g.m, wg_nqt(3, g.cin)) * W * 9 * g.cin, dsl = g.ds ? (int64_t)wg_slabs128(g.m, wg_nqt(1, g.cin)) * W * g.cin : 0;
        slab = c1 > slab ? c1 : slab;
        slab = dsl > slab ? dsl : slab;
    }
    L.slab = take(slab * 4);
    L.zp = take(strided ? (int64_t)g.n * (g.hin + 2) * (g.win + 2) * W * 2 : 0);
    L.wdt = take(strided ? (int64_t)g.cin * W * 2 : 0);
    L.total = o;
    return L;
}

// ---- backward: what is specific to the BasicBlock's widths -------------------------------------------------------------------------------
// the stride-2 block: dx [n][2H][2Wd][cin] (at g1's total scale) += ds^T(g2) [n][H][Wd][cin] (at g2's total scale) times g1's own
// multiplier, a power of two, at the even (row, column) positions: the 1x1 stride-2 convolution reads no other.  One thread = 4 channels.
__global__ __launch_bounds__(RB_THREADS) void rb_add_downsample_kernel(float* dx, const float* t, int64_t rows, int H, int Wd, int cin, const float* sc1) {
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    const int C4 = cin >> 2;
    if (i >= rows * C4) return;
    const int cq = (int)(i % C4);
    const int64_t m = i / C4;
    const int HW = H * Wd, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    float* d = dx + (((int64_t)img * 2 * H + 2 * y) * 2 * Wd + 2 * x) * cin + 4 * cq;
    const float mul = sc1[2];
    floatx4 a = *(floatx4*)d;
    const floatx4 b = *(const floatx4*)(t + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += b[e] * mul;
    *(floatx4*)d = a;
}

// a [items] (times asc[0]) <- a + b (times bsc[0]) with both brought to the smaller of the two scales: every multiplier is a power of two.
// osc = {that scale, 1 / it}.  One thread = 4 values.
__global__ __launch_bounds__(RB_THREADS) void rb_combine_kernel(float* a, const float* asc, const float* b, const float* bsc, int64_t items4, float* osc) {
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    const bool first = asc[0] <= bsc[0];
    const float so = first ? asc[0] : bsc[0], ma = so * asc[1], mb = so * bsc[1];
    if (i == 0) { osc[0] = so; osc[1] = first ? asc[1] : bsc[1]; }
    if (i >= items4) return;
    const floatx4 x = *(const floatx4*)(a + i * 4), y = *(const floatx4*)(b + i * 4);
    floatx4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = x[e] * ma + y[e] * mb;
    *(floatx4*)(a + i * 4) = o;
}

void to_padded(ConvParams& c, const Geo& g, half_t* out) {
    c.out = out; c.out_hp = g.h + 2; c.out_wp = g.w + 2; c.out_c = g.width; c.out_ring = 1;
}

int64_t ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode, int base) {
    Geo g;
    if (!make_geo(n, hin, win, cin, width, stride, base, g) || mode < 0 || mode > 1) return base - 1;
    return mode ? bwd_layout(g, base != RB_LEGACY && g.ds).total : fwd_layout(g).total;
}

int launch_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps, void* ws, void* y,
                   hipStream_t s, int base) {
    Geo g;
    if (!x || !ws || !y || !make_geo(n, hin, win, cin, width, stride, base, g) || !params_ok(P, g.ds) || !(eps > 0.f)) return base - 1;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)ws & 255)) return base - 2;
    const FwdLayout L = fwd_layout(g);
    const int W = width;
    char* w = (char*)ws;
    half_t *a1 = (half_t*)(w + L.a1), *id = (half_t*)(w + L.id), *w1 = (half_t*)(w + L.w1), *w2 = (half_t*)(w + L.w2), *wd = (half_t*)(w + L.wd);
    float* bias = (float*)(w + L.bias);
    hipLaunchKernelGGL(rb_fold_kernel, dim3(nblk((int64_t)W * 9 * cin + W)), dim3(RB_THREADS), 0, s, (const float*)P->conv1_w, (const float*)P->bn1_w,
                       (const float*)P->bn1_b, (const float*)P->bn1_mean, (const float*)P->bn1_var, eps, W, cin, 9, w1, bias);
    hipLaunchKernelGGL(rb_fold_kernel, dim3(nblk((int64_t)W * 9 * W + W)), dim3(RB_THREADS), 0, s, (const float*)P->conv2_w, (const float*)P->bn2_w,
                       (const float*)P->bn2_b, (const float*)P->bn2_mean, (const float*)P->bn2_var, eps, W, W, 9, w2, bias + W);
    if (g.ds)
        hipLaunchKernelGGL(rb_fold_kernel, dim3(nblk((int64_t)W * cin + W)), dim3(RB_THREADS), 0, s, (const float*)P->ds_w, (const float*)P->ds_bn_w,
                           (const float*)P->ds_bn_b, (const float*)P->ds_bn_mean, (const float*)P->ds_bn_var, eps, W, cin, 1, wd, bias + 2 * W);
    const unsigned ring = nblk((int64_t)n * (2 * (g.w + 2) + 2 * g.h) * (W / 8));
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring), dim3(RB_THREADS), 0, s, a1, n, g.h, g.w, W);
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring), dim3(RB_THREADS), 0, s, (half_t*)y, n, g.h, g.w, W);
    VTD_HIP_CHECK(hipGetLastError());
    int rc;
    ConvParams c = conv_of(n, g.h, g.w, W, (const half_t*)x, cin, hin, win, 3, stride, w1, bias);
    c.flags = EPI_RELU;
    to_padded(c, g, a1);
    if ((rc = vtd_launch_conv(c, -1, s))) return rc;
    if (g.ds) {
        ConvParams d = conv_of(n, g.h, g.w, W, (const half_t*)x, cin, hin, win, 1, 2, wd, bias + 2 * W);
        to_padded(d, g, id);
        if ((rc = vtd_launch_conv(d, -1, s))) return rc;
    }
    ConvParams e = conv_of(n, g.h, g.w, W, a1, W, g.h, g.w, 3, 1, w2, bias + W);
    e.flags = EPI_RELU | EPI_RESIDUAL;
    e.res = g.ds ? id : (const half_t*)x; e.res_hp = g.h + 2; e.res_wp = g.w + 2; e.res_ring = 1; e.res_shift = 0;
    to_padded(e, g, (half_t*)y);
    return vtd_launch_conv(e, -1, s);
}

int launch_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps, const void* ws,
                    const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch, float* dx, float* dxscale,
                    hipStream_t s, int base) {
    Geo g;
    const bool legacy = base == RB_LEGACY;
    if (!x || !ws || !y || !dy || !dscale || !scratch || !make_geo(n, hin, win, cin, width, stride, base, g) || !params_ok(P, g.ds) || !grads_ok(Gp, g.ds) ||
        !(eps > 0.f) || (dx && !dxscale))
        return base - 1;
    if (legacy && dx && g.stride != 1) return base - 3;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)ws & 255) || ((uintptr_t)scratch & 255) || ((uintptr_t)dy & 15) || ((uintptr_t)dscale & 7) ||
        ((uintptr_t)dx & 15) || ((uintptr_t)dxscale & 7))
        return base - 2;
    const FwdLayout L = fwd_layout(g);
    const BwdLayout B = bwd_layout(g, !legacy && g.ds);
    const int W = width;
    char* q = (char*)scratch;
    const half_t* a1 = (const half_t*)((const char*)ws + L.a1);
    float *g2 = (float*)(q + B.g2), *g1 = (float*)(q + B.g1), *zero = (float*)(q + B.zero), *pmax = (float*)(q + B.pmax), *sc = (float*)(q + B.sc),
          *slab = (float*)(q + B.slab);
    half_t *g2h = (half_t*)(q + B.g2h), *g1h = (half_t*)(q + B.g1h), *g2p = (half_t*)(q + B.g2p), *g1p = (half_t*)(q + B.g1p), *wt = (half_t*)(q + B.wt);
    double *part = (double*)(q + B.part), *sum2 = (double*)(q + B.sum2), *sum1 = (double*)(q + B.sum1);
    float *sc2 = sc, *sc1 = sc + 4;
    const int64_t M = g.m;
    int Gr = (int)((M + 255) / 256);
    Gr = Gr < 1 ? 1 : Gr > RB_MAX_RED ? RB_MAX_RED : Gr;
    const int64_t per = (M + Gr - 1) / Gr;
    const unsigned ring = nblk((int64_t)n * (2 * (g.w + 2) + 2 * g.h) * (W / 8));
    const int S = wg_slabs(M);
    int rc;

    auto stage = [&](const float* v, const half_t* act, float* gout, const float* in_sc, double* sum, float* out_sc, half_t* flat, half_t* padded) {
        hipLaunchKernelGGL(rb_mask_kernel, dim3(nblk(M * (W / 4))), dim3(RB_THREADS), 0, s, v, act, M, g.h, g.w, W, gout);
        if (W == 64)
            hipLaunchKernelGGL(rb_reduce64_kernel, dim3(Gr), dim3(RB_THREADS), 0, s, (const float*)gout, M, per, part, pmax);
        else if (W == 128)
            hipLaunchKernelGGL(rb_reduce128_kernel, dim3(Gr), dim3(RB_THREADS), 0, s, (const float*)gout, M, per, part, pmax);
        else
            hipLaunchKernelGGL(rb_reduce_kernel, dim3(Gr), dim3(RB_THREADS), 0, s, (const float*)gout, M, per, W, part, pmax);
        hipLaunchKernelGGL(rb_finish_kernel, dim3(1), dim3(RB_THREADS), 0, s, (const double*)part, (const float*)pmax, Gr, W, in_sc, sum, out_sc);
        hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring), dim3(RB_THREADS), 0, s, padded, n, g.h, g.w, W);
        hipLaunchKernelGGL(rb_form_kernel, dim3(nblk(M * (W / 8))), dim3(RB_THREADS), 0, s, (const float*)gout, M, (const float*)out_sc, g.h, g.w, W, 1, flat,
                           padded);
    };
    auto wgrad = [&](const half_t* a, const half_t* xin, int xc, int hi, int wi, int ksz, int st, const float* scl, const double* sum, const float* w,
                     const float* gam, const float* mean, const float* var, float* dw, float* dgam, float* dbet) {
        WgArgs wa;
        wa.a = a; wa.lda = W; wa.x = xin; wa.xc = xc; wa.n = n; wa.H = g.h; wa.W = g.w; wa.rows = M; wa.slab = slab;
        const int nqt = wg_nqt(ksz, xc), Sl = W <= 128 ? wg_slabs128(M, nqt) : S;
        wa.slab_len = slab_rows(M, Sl); wa.ksz = ksz; wa.stride = st; wa.Hin = hi; wa.Win = wi;
        if (W == 64)   // layer1: the 64-row tile, one column tile, slab [64][576]
            hipLaunchKernelGGL(dbhead_train_wgrad_kernel<5>, dim3(nqt * Sl, 1), dim3(WG_THREADS), 0, s, wa);
        else if (xc & 127)   // layer2.0's 64-channel input: a tap per 64-column group
            hipLaunchKernelGGL(dbhead_train_wgrad_kernel<4>, dim3(nqt * Sl, W / 128), dim3(WG_THREADS), 0, s, wa);
        else
            hipLaunchKernelGGL(dbhead_train_wgrad_kernel<3>, dim3(nqt * Sl, W / 128), dim3(WG_THREADS), 0, s, wa);
        hipLaunchKernelGGL(rb_param_kernel, dim3(W), dim3(RB_THREADS), 0, s, (const float*)slab, Sl, xc, ksz * ksz, scl, sum, w, gam, mean, var, eps, dw, dgam,
                           dbet);
    };
    // conv^T of a padded gradient plane of hp x wp pixels (W channels) into [n hp wp][rows] fp32: the folded weights of a conv with `rows`
    // input channels, rotated and transposed into `panel`
    auto dgrad = [&](const half_t* gp, int hp, int wp, const float* w, const float* gam, const float* var, int rows, int ksz, half_t* panel, float* out) {
        hipLaunchKernelGGL(rb_pack_dgrad_kernel, dim3(nblk(rows * ksz * ksz * W + W)), dim3(RB_THREADS), 0, s, w, gam, var, eps, W, rows, ksz * ksz, panel,
                           zero);
        ConvParams c = conv_of(n, hp, wp, rows, gp, W, hp, wp, ksz, 1, panel, zero);
        c.out = out; c.ldc = rows; c.flags = EPI_OUT_F32;
        return vtd_launch_conv(c, -1, s);
    };

    // g2 = dy (y > 0): the gradient at bn2's output, of the downsample's BatchNorm output, and of an identity input
    stage(dy, (const half_t*)y, g2, dscale, sum2, sc2, g2h, g2p);
    VTD_HIP_CHECK(hipGetLastError());
    wgrad(g2h, a1, W, g.h, g.w, 3, 1, sc2, sum2, (const float*)P->conv2_w, (const float*)P->bn2_w, (const float*)P->bn2_mean, (const float*)P->bn2_var,
          Gp->conv2_w, Gp->bn2_w, Gp->bn2_b);
    if (g.ds)
        wgrad(g2h, (const half_t*)x, cin, hin, win, 1, 2, sc2, sum2, (const float*)P->ds_w, (const float*)P->ds_bn_w, (const float*)P->ds_bn_mean,
              (const float*)P->ds_bn_var, Gp->ds_w, Gp->ds_bn_w, Gp->ds_bn_b);
    VTD_HIP_CHECK(hipGetLastError());
    // da1 = conv2^T(g2) into the g1 buffer, masked in place by a1 > 0
    if ((rc = dgrad(g2p, g.h, g.w, (const float*)P->conv2_w, (const float*)P->bn2_w, (const float*)P->bn2_var, W, 3, wt, g1))) return rc;
    stage(g1, a1, g1, sc2, sum1, sc1, g1h, g1p);
    wgrad(g1h, (const half_t*)x, cin, hin, win, 3, stride, sc1, sum1, (const float*)P->conv1_w, (const float*)P->bn1_w, (const float*)P->bn1_mean,
          (const float*)P->bn1_var, Gp->conv1_w, Gp->bn1_w, Gp->bn1_b);
    VTD_HIP_CHECK(hipGetLastError());
    if (dx && !g.ds) {
        if ((rc = dgrad(g1p, g.h, g.w, (const float*)P->conv1_w, (const float*)P->bn1_w, (const float*)P->bn1_var, W, 3, wt, dx))) return rc;
        hipLaunchKernelGGL(rb_add_identity_kernel, dim3(nblk(M * (W / 4))), dim3(RB_THREADS), 0, s, dx, (const float*)g2, M * (W / 4), (const float*)sc2,
                           (const float*)sc1);
        hipLaunchKernelGGL(rb_copy_scale_kernel, dim3(1), dim3(64), 0, s, (const float*)sc1, dxscale);
    } else if (dx) {
        // g1 at the even positions of a zeroed plane of the input's size, then the stride-1 path: see the head of this file
        half_t *zp = (half_t*)(q + B.zp), *wdt = (half_t*)(q + B.wdt);
        VTD_HIP_CHECK(hipMemsetAsync(zp, 0, (size_t)n * (hin + 2) * (win + 2) * W * 2, s));
        hipLaunchKernelGGL(rb_form_kernel, dim3(nblk(M * (W / 8))), dim3(RB_THREADS), 0, s, (const float*)g1, M, (const float*)sc1, g.h, g.w, W, 2,
                           (half_t*)nullptr, zp);
        if ((rc = dgrad(zp, hin, win, (const float*)P->conv1_w, (const float*)P->bn1_w, (const float*)P->bn1_var, cin, 3, wt, dx))) return rc;
        // ds^T(g2) at g2's scale into the g1 buffer (its fp32 values are in the operands by now), then onto the even positions
        if ((rc = dgrad(g2p, g.h, g.w, (const float*)P->ds_w, (const float*)P->ds_bn_w, (const float*)P->ds_bn_var, cin, 1, wdt, g1))) return rc;
        hipLaunchKernelGGL(rb_add_downsample_kernel, dim3(nblk(M * (cin / 4))), dim3(RB_THREADS), 0, s, dx, (const float*)g1, M, g.h, g.w, cin,
                           (const float*)sc1);
        hipLaunchKernelGGL(rb_copy_scale_kernel, dim3(1), dim3(64), 0, s, (const float*)sc1, dxscale);
    }
    return -(int)hipGetLastError();
}

}  // namespace

int64_t vtd_basicblock_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    return ws_bytes(n, hin, win, cin, width, stride, mode, RB_LEGACY);
}

int vtd_launch_basicblock_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                  void* ws, void* y, hipStream_t s) {
    return launch_forward(x, n, hin, win, cin, width, stride, P, eps, ws, y, s, RB_LEGACY);
}

int vtd_launch_basicblock_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                   const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch,
                                   float* dx, float* dxscale, hipStream_t s) {
    return launch_backward(x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s, RB_LEGACY);
}

// the six geometries, with the input gradient of the stride-2 blocks
int64_t vtd_resblock_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    return ws_bytes(n, hin, win, cin, width, stride, mode, RB_GENERAL);
}

int vtd_launch_resblock_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps, void* ws,
                                void* y, hipStream_t s) {
    return launch_forward(x, n, hin, win, cin, width, stride, P, eps, ws, y, s, RB_GENERAL);
}

int vtd_launch_resblock_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                 const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch,
                                 float* dx, float* dxscale, hipStream_t s) {
    return launch_backward(x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s, RB_GENERAL);
}

// layer1's geometry alone: (64 -> 64, stride 1)
int64_t vtd_block64_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    return ws_bytes(n, hin, win, cin, width, stride, mode, RB_NARROW);
}

int vtd_launch_block64_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps, void* ws,
                               void* y, hipStream_t s) {
    return launch_forward(x, n, hin, win, cin, width, stride, P, eps, ws, y, s, RB_NARROW);
}

int vtd_launch_block64_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch,
                                float* dx, float* dxscale, hipStream_t s) {
    return launch_backward(x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s, RB_NARROW);
}

int vtd_launch_resblock_combine(float* a, const float* asc, const float* b, const float* bsc, int64_t numel, float* osc, hipStream_t s) {
    if (!a || !asc || !b || !bsc || !osc || numel <= 0 || (numel & 3) || numel >= (1ll << 40) || osc == asc || osc == bsc) return RB_GENERAL - 1;
    if ((((uintptr_t)a | (uintptr_t)b) & 15) || (((uintptr_t)asc | (uintptr_t)bsc | (uintptr_t)osc) & 7)) return RB_GENERAL - 2;
    hipLaunchKernelGGL(rb_combine_kernel, dim3(nblk(numel / 4)), dim3(RB_THREADS), 0, s, a, asc, b, bsc, numel / 4, osc);
    return -(int)hipGetLastError();
}
