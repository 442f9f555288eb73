// ResNet Bottleneck (v1.5: the stride sits on the 3x3) training with batch-statistics BatchNorm (torch's train() mode: the statistics of the
// batch normalise, the running statistics are updated in place), forward and backward, for the blocks of ResNet-50's two upper stages:
//   res5 (torchvision's layer4), W = 512: (1024 -> 512 -> 2048, stride 2, downsample) and (2048 -> 512 -> 2048, stride 1, identity)
//   res4 (torchvision's layer3), W = 256: (512 -> 256 -> 1024, stride 2, downsample) and (1024 -> 256 -> 1024, stride 1, identity)
// The host path is generic in the width W, as bottleneck_train.hip's; the entries (vtd_bottleneck_bn_train_*, -4001 / -4002) are gated to
// W = 512 and 256: res3 (128), res2 (64) and the stem follow later.  With training = 0 the entries hand the call to the frozen-statistics
// path (bottleneck_train.hip: vtd_bottleneck_train_* at W = 512, vtd_bottleneck256_train_* at W = 256) unchanged.
// Tensors are padded taps (ring-padded NHWC fp16, ring 1).  y = relu(bn3(conv3(a2)) + id), a2 = relu(bn2(conv2(a1))), a1 = relu(bn1(conv1(x))),
// id = x or ds_bn(ds(x)); conv1 1x1 cin -> W, conv2 3x3 at stride s, conv3 1x1 W -> 4 W, ds 1x1 cin = 2 W -> 4 W at stride s.
// The contract is the one resblock_bn_train.hip states at its head, on three or four convolution + BatchNorm pairs; the kernels of the
// W-wide pairs (bn1, bn2) are that file's, from resblock_bn_common.h, as they are.
//
// Forward, per convolution + BatchNorm pair (conv1 / bn1, conv2 / bn2, the downsample, conv3 / bn3):
//   pack             the raw weights -> fp16 GEMM panel [cout][ksz^2 cin] (k = tap * cin + ci); no fold: gamma rstd is not known yet
//   conv             conv_igemm.hip with EPI_OUT_F32 and a zero bias: z [rows][C] fp32, kept in the workspace for the backward.  conv1 is 1x1
//                    at the INPUT's extent: z1 has n h_in w_in rows and a1 is padded at the input's extent, as in the frozen path; the others
//                    have the output's n h w rows.  The statistics stay unfused from the convolution's epilogue, as at every other width: the
//                    epilogue would need a cross-tile fp64 combination in a fixed order, which is what the partial + finish pair is
//   stats partial    C = W (bn1, bn2): bt_stats_partial_kernel<W>, G = min(256, ceil(rows / 256)) workgroups, the parts and their order
//                    as resblock_bn_train.hip states them.  C = 4 W (bn3, the downsample's; 2048 or 1024): bw_stats_partial_kernel<C / 1024>,
//                    G = min(256, ceil(rows / 32)) workgroups of ceil(rows / G) consecutive rows each, in row order; thread t owns channels
//                    1024 j + 4 t .. 1024 j + 4 t + 3 for j < C / 1024 (bk_mask_reduce_kernel's ownership), so every wave load is 1 KiB of one
//                    row and a workgroup's loads are the whole row; sums of z and z^2 in fp64 in row order, one thread per channel group:
//                    no parts, no LDS join.  Then (count, mean, M2) per channel.  The reduce grid (workgroups, rows of each) is per pair:
//                    bn1's row count differs from the others' in the stride-2 block
//   stats finish     bt_stats_finish_kernel<C>, one thread per channel: Chan's combination of the partials in workgroup order (fp64) -> mu,
//                    biased sigma^2; the running values mean <- (1 - m) mean + m mu, var <- (1 - m) var + m sigma^2 M / (M - 1); table
//                    {mu, rstd, gamma, beta} [4][C]
//   apply            bt_apply_kernel<C>: relu(((z - mu) rstd) gamma + beta [+ id]) -> ring-padded fp16 tap; the downsample's has no ReLU.
//                    One thread = 8 channels
// Backward from dy (NHWC fp32 [n h w][4 W] times a power of two):
//   mask + reduce    bw_bwd_reduce_kernel<C / 1024, true>, ONE pass over the 4 W-wide gradient: reads dy, y and z3, writes g3 = dy (y > 0)
//                    (the gradient at bn3's output, of the downsample's BatchNorm output, and of an identity input) and, with xh =
//                    (z3 - mu) rstd from the saved z3, the per-channel partials s1 = sum g3, s2 = sum g3 xh in fp64, max |g3| and max |xh|;
//                    rows and threads as in the 4 W-wide `stats partial`.  The downsample's pair reduces the same g3 against its own z_d
//                    (bw_bwd_reduce_kernel<C / 1024, false>: no mask, nothing written but the partials)
//   finish           C = 4 W: bw_bwd_finish_kernel<C>, one workgroup of 1024 threads, thread t = channel t (and t + 1024 at C = 2048); the
//                    partials in workgroup order (fp64); dbeta = s1, dgamma = s2 (scale undone); the table {gamma rstd, s1 / M, s2 / M};
//                    the power-of-two multiplier from max_c |gamma rstd| (max |g| + |s1| / M + max |xh| |s2| / M), which bounds |dz|:
//                    bt_bwd_finish_kernel's rule.  C = W: bt_bwd_reduce_kernel<W> and bt_bwd_finish_kernel<W> as they are
//   form             bt_form_kernel<C>: dz = gamma rstd (g - s1 / M - xh s2 / M) in fp32, times the multiplier, as fp16: flat [rows][C]
//                    and ring-padded
//   wgrad<3>         G[c][k] = sum_m dz[m][c] x[m][k] on wgrad_mfma.h as it stands: conv3 (lda 4 W, xc W, 1x1), the downsample (lda 4 W, xc
//                    2 W, 1x1 at stride 2), conv2 (lda W, xc W, 3x3 at stride s over a1) and conv1 (lda W, xc = cin, 1x1, rows = n h_in
//                    w_in).  Slabs: bottleneck_train.hip's rule for these widths, min(8, ceil(rows / 4096)) of the LAUNCH's rows.  bt_dw_kernel:
//                    dW = the slabs summed in slab order in fp64 with the scale undone: dz carries gamma rstd, no factor follows
//   da2, da1         conv3^T(dz3) (a 1x1 GEMM 4 W -> W) and conv2^T(dz2) (3x3 at stride 1) on the raw weights, rotated by 180 degrees and
//                    transposed (bt_pack_dgrad_kernel); g2 = da2 (a2 > 0), g1 = da1 (a1 > 0).  Stride 2: dz2 goes to the even positions of
//                    a zeroed ring-padded plane of the input's extent (`form` with dil = 2) and the same stride-1 path runs over it
//   dx (optional)    conv1^T(dz1), a 1x1 GEMM W -> cin at dz1's total scale; plus, stride 1, g3 times the three pairs' power-of-two
//                    multipliers (one scale); or, stride 2, ds^T(dz_d) -- the downsample pair has its own statistics and its own dz_d,
//                    with its own multiplier scd[2] -- added at the even (row, column) positions times sc3[2] sc2[2] sc1[2] / scd[2], which
//                    brings it to dz1's scale exactly
// Nothing divides by gamma or sigma.  No atomics, shape-only grids, fixed summation orders: bitwise repeatable.
#include "resblock_bn_common.h"

#include "conv_kernels.h"

#include <type_traits>

int64_t vtd_bottleneck_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_bottleneck_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps, void* ws,
                                  void* y, hipStream_t s);
int vtd_launch_bottleneck_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                   const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp, void* scratch,
                                   float* dx, float* dxscale, hipStream_t s);
int64_t vtd_bottleneck256_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_bottleneck256_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                     void* ws, void* y, hipStream_t s);
int vtd_launch_bottleneck256_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                      const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp, void* scratch,
                                      float* dx, float* dxscale, hipStream_t s);

namespace {

constexpr int BW_ERR_ARG = -4001, BW_ERR_ALIGN = -4002;
constexpr int BW_FINISH_THREADS = 1024;

// a reduce grid: G workgroups of `per` consecutive rows
struct Red { int G; int64_t per; };

Red red_grid(int64_t rows, int per_wg) {
    int64_t G = (rows + per_wg - 1) / per_wg;
    G = G < 1 ? 1 : G > BT_MAX_RED ? BT_MAX_RED : G;
    return {(int)G, (rows + G - 1) / G};
}

struct Geo {
    int n, hin, win, cin, stride, h, w;
    int W, OUT;                  // the Bottleneck width and 4 W
    int64_t m, min, pin, pout;   // output rows, input rows, padded pixels of the input's and the output's extent
    bool ds;                     // the block has a downsample (1x1 at the block's stride): a stage's first block
    Red r1, r2, r3;              // the reduce grids: bn1 (W wide, the input's rows), bn2 (W wide), bn3 and the downsample's (4 W wide)
};

bool make_geo(int n, int hin, int win, int cin, int width, int stride, Geo& g) {
    if (n <= 0 || hin <= 0 || win <= 0 || n > 65535 || hin > 4096 || win > 4096) return false;
    if (width != 512 && width != 256) return false;   // the gate of this family: res3, res2 (128, 64) are not built
    const int W = width, OUT = 4 * W;
    const bool first = cin == 2 * W && stride == 2 && !(hin & 1) && !(win & 1);
    if (!(first || (cin == OUT && stride == 1))) return false;
    g.W = W; g.OUT = OUT;
    g.n = n; g.hin = hin; g.win = win; g.cin = cin; g.stride = stride; g.h = hin / stride; g.w = win / stride;
    g.m = (int64_t)n * g.h * g.w; g.min = (int64_t)n * hin * win;
    g.pin = (int64_t)n * (hin + 2) * (win + 2); g.pout = (int64_t)n * (g.h + 2) * (g.w + 2);
    g.ds = first;
    g.r1 = red_grid(g.min, 256); g.r2 = red_grid(g.m, 256); g.r3 = red_grid(g.m, 32);
    // every tensor the convolutions index: x, a1 and the planes of the input's extent, y and id
    return g.pin * (cin > W ? cin : W) < (1ll << 31) && g.pout * OUT < (1ll << 31);
}

// the workspace of a training = 1 forward.  tab: {mu, rstd, gamma, beta} [4][C] per pair, C the pair's width; st: {mu, sigma^2} [2][W] of a
// W-wide pair on its way to the caller's [2][4 W] row
struct FwdLayout { int64_t a1, a2, id, z1, z2, z3, zd, w1, w2, w3, wd, zero, part, tab1, tab2, tab3, tabd, st, total; };
struct BwdLayout { int64_t g3, g2, g1, dzh, dz3p, dz2p, dz1p, wt, zero, part, pmax, coef, sc, slab, total; };

FwdLayout fwd_layout(const Geo& g) {
    FwdLayout L;
    const int64_t W = g.W, OUT = g.OUT;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    L.a1 = take(g.pin * W * 2); L.a2 = take(g.pout * W * 2); L.id = take(g.ds ? g.pout * OUT * 2 : 0);
    L.z1 = take(g.min * W * 4); L.z2 = take(g.m * W * 4); L.z3 = take(g.m * OUT * 4); L.zd = take(g.ds ? g.m * OUT * 4 : 0);
    L.w1 = take(W * g.cin * 2); L.w2 = take(W * 9 * W * 2); L.w3 = take(OUT * W * 2); L.wd = take(g.ds ? OUT * g.cin * 2 : 0);
    L.zero = take(OUT * 4);
    L.part = take((int64_t)BT_MAX_RED * OUT * 3 * 8);
    L.tab1 = take(4 * W * 4); L.tab2 = take(4 * W * 4); L.tab3 = take(4 * OUT * 4); L.tabd = take(g.ds ? 4 * OUT * 4 : 0);
    L.st = take(2 * W * 4);
    L.total = o;
    return L;
}

BwdLayout bwd_layout(const Geo& g) {
    BwdLayout L;
    const int64_t W = g.W, OUT = g.OUT;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    L.g3 = take(g.m * OUT * 4); L.g2 = take(g.m * W * 4); L.g1 = take(g.min * W * 4);
    const int64_t f3 = g.m * OUT, f1 = g.min * W;
    L.dzh = take((f3 > f1 ? f3 : f1) * 2);   // the flat operands of one pair at a time
    L.dz3p = take(g.pout * OUT * 2);         // dz3, then dz_d, ring-padded
    L.dz2p = take(g.pin * W * 2);            // stride 1: dz2 ring-padded; stride 2: the zero-inserted plane.  Both of the input's extent
    L.dz1p = take(g.pin * W * 2);
    L.wt = take(W * 9 * W * 2);              // the largest transposed panel: conv2's 9 W^2 (the downsample's is 2 W x 4 W)
    L.zero = take(OUT * 4);
    L.part = take((int64_t)BT_MAX_RED * 2 * OUT * 8); L.pmax = take((int64_t)BT_MAX_RED * 2 * OUT * 4);
    L.coef = take(3 * OUT * 4);
    L.sc = take(4 * 4 * 4);
    // conv2's slab [W][9 W] is the largest of the launches over the output's rows (conv3 [4 W][W], the downsample [4 W][2 W]);
    // conv1's [W][cin] goes with the input's rows
    const int64_t so = (int64_t)wg_slabs(g.m) * W * 9 * W, si = (int64_t)wg_slabs(g.min) * W * g.cin;
    L.slab = take((so > si ? so : si) * 4);
    L.total = o;
    return L;
}

// ---- the 4 W-wide pairs (C = 1024 NJ: 2048 at res5, 1024 at res4) -------------------------------------------------------------------------
// z [rows][C] fp32 -> part[g][c] = {count, mean, M2} (fp64) over the workgroup's rows m0 .. m1 - 1 in row order.  Thread t owns channels
// 1024 j + 4 t .. 1024 j + 4 t + 3 for j < NJ: a wave's 16-byte loads cover 1 KiB of the row.  One thread per channel: no LDS join
template <int NJ>
__global__ __launch_bounds__(BT_THREADS) void bw_stats_partial_kernel(const float* z, int64_t rows, int64_t per, double* part) {
    constexpr int C = 1024 * NJ;
    const int t = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows, m1 = m0 + per < rows ? m0 + per : rows;
    double s[4 * NJ], q[4 * NJ];
#pragma unroll
    for (int k = 0; k < 4 * NJ; ++k) { s[k] = 0.0; q[k] = 0.0; }
#pragma unroll 4
    for (int64_t m = m0; m < m1; ++m) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const floatx4 v = *(const floatx4*)(z + m * C + j * 1024 + 4 * t);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const double a = (double)v[e]; s[4 * j + e] += a; q[4 * j + e] += a * a; }
        }
    }
    const double cnt = (double)(m1 - m0);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double S = s[4 * j + e], Q = q[4 * j + e];
            const double mean = cnt > 0 ? S / cnt : 0.0;
            double* o = part + ((int64_t)blockIdx.x * C + j * 1024 + 4 * t + e) * 3;
            o[0] = cnt; o[1] = mean; o[2] = cnt > 0 ? fmax(Q - S * mean, 0.0) : 0.0;
        }
}

// The backward's reduce of a 4 W-wide pair, rows and threads as bw_stats_partial_kernel.  MASK: v = dy [rows][C] fp32 and act = the
// ring-padded fp16 output y [n][H + 2][Wd + 2][C]; g = v where act > 0, else 0, is written to `out` -- mask and reduce in one pass.
// Otherwise g = v as it is (the downsample's pair: g3 against its own z) and nothing but the partials is written.
// part[blk][0][c] = sum g, part[blk][1][c] = sum g xh (fp64), pmax[blk][0][c] = max |g|, pmax[blk][1][c] = max |xh| (NaN kept),
// xh = (z - mu) rstd as the forward formed it: bt_bwd_reduce_kernel's outputs and layout
template <int NJ, bool MASK>
__global__ __launch_bounds__(BT_THREADS) void bw_bwd_reduce_kernel(const float* v, const half_t* act, const float* z, const float* tab, int64_t rows,
                                                                   int64_t per, int H, int Wd, float* out, double* part, float* pmax) {
    constexpr int C = 1024 * NJ;
    const int t = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows, m1 = m0 + per < rows ? m0 + per : rows;
    floatx4 mu[NJ], rs[NJ], mg[NJ], mx[NJ];
    double s1[4 * NJ], s2[4 * NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        mu[j] = *(const floatx4*)(tab + j * 1024 + 4 * t);
        rs[j] = *(const floatx4*)(tab + C + j * 1024 + 4 * t);
#pragma unroll
        for (int e = 0; e < 4; ++e) { mg[j][e] = 0.f; mx[j][e] = 0.f; s1[4 * j + e] = 0.0; s2[4 * j + e] = 0.0; }
    }
    const int HW = H * Wd;
    int img = (int)(m0 / HW), rem = (int)(m0 - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    for (int64_t m = m0; m < m1; ++m) {
        const half_t* a = MASK ? act + (((int64_t)img * (H + 2) + y + 1) * (Wd + 2) + x + 1) * C : nullptr;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = j * 1024 + 4 * t;
            floatx4 gv = *(const floatx4*)(v + m * C + c);
            const floatx4 zv = *(const floatx4*)(z + m * C + c);
            if constexpr (MASK) {
                const half4 hh = *(const half4*)(a + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) gv[e] = (float)hh[e] > 0.f ? gv[e] : 0.f;
                *(floatx4*)(out + m * C + c) = gv;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (zv[e] - mu[j][e]) * rs[j][e];
                s1[4 * j + e] += (double)gv[e];
                s2[4 * j + e] += (double)gv[e] * (double)xh;
                mg[j][e] = nmax(mg[j][e], fabsf(gv[e]));
                mx[j][e] = nmax(mx[j][e], fabsf(xh));
            }
        }
        if (MASK) { if (++x == Wd) { x = 0; if (++y == H) { y = 0; ++img; } } }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int64_t b = (int64_t)blockIdx.x * 2 * C + j * 1024 + 4 * t;
        doublex4 o1, o2;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o1[e] = s1[4 * j + e]; o2[e] = s2[4 * j + e]; }
        *(doublex4*)(part + b) = o1; *(doublex4*)(part + b + C) = o2;
        *(floatx4*)(pmax + b) = mg[j]; *(floatx4*)(pmax + b + C) = mx[j];
    }
}

// bt_bwd_finish_kernel for C = 1024 or 2048 in one workgroup of 1024 threads: thread t = channel t (and t + 1024 at C = 2048).  The
// partials in workgroup order (fp64).  dbeta = s1, dgamma = s2 with the incoming scale undone; coef = {gamma rstd, s1 / M, s2 / M} [3][C] at
// the incoming scale; out_sc = {total scale, 1 / total, this stage's multiplier, 0}: the multiplier is a power of two from the bound
// max_c |gamma rstd| (max |g| + |s1| / M + max |xh| |s2| / M) >= max |dz| (1 when that is zero or not finite)
template <int C>
__global__ __launch_bounds__(BW_FINISH_THREADS) void bw_bwd_finish_kernel(const double* part, const float* pmax, int G, double inv_m, const float* tab,
                                                                          const float* in_sc, float* coef, float* dgam, float* dbet, float* out_sc) {
    static_assert(C == 1024 || C == 2048, "one or two channels per thread");
    const int t = threadIdx.x;
    float bound = 0.f;
#pragma unroll
    for (int k = 0; k < C / BW_FINISH_THREADS; ++k) {
        const int c = t + k * BW_FINISH_THREADS;
        double s1 = 0.0, s2 = 0.0;
        float mg = 0.f, mx = 0.f;
        for (int g = 0; g < G; ++g) {
            const int64_t b = (int64_t)g * 2 * C + c;
            s1 += part[b]; s2 += part[b + C];
            mg = nmax(mg, pmax[b]); mx = nmax(mx, pmax[b + C]);
        }
        const float A = tab[2 * C + c] * tab[C + c], B = (float)(s1 * inv_m), Cf = (float)(s2 * inv_m);
        coef[c] = A; coef[C + c] = B; coef[2 * C + c] = Cf;
        dbet[c] = (float)(s1 * (double)in_sc[1]);
        dgam[c] = (float)(s2 * (double)in_sc[1]);
        bound = nmax(bound, (float)(fabs((double)A) * ((double)mg + fabs((double)B) + (double)mx * fabs((double)Cf))));
    }
    __shared__ float sh[BW_FINISH_THREADS];
    sh[t] = bound;
    __syncthreads();
    for (int o = BW_FINISH_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] = nmax(sh[t], sh[t + o]);
        __syncthreads();
    }
    if (t == 0) {
        const float bnd = sh[0];
        const double tin = (double)in_sc[0];
        int e = 0;
        if (bnd > 0.f && isfinite(bnd)) e = (int)floor(log2((double)RB_SCALE_TARGET / (double)bnd));
        const int ein = (tin > 0.0 && isfinite(tin)) ? ilogb(tin) : 0;
        int et = ein + e;
        et = et < -120 ? -120 : et > 120 ? 120 : et;
        e = et - ein;
        const double tot = tin * ldexp(1.0, e);
        out_sc[0] = (float)tot; out_sc[1] = (float)(1.0 / tot); out_sc[2] = ldexpf(1.0f, e); out_sc[3] = 0.f;
    }
}

// stride 1: dx [items4 x 4] (at dz1's total scale) += g3 (at the incoming scale) times the three pairs' multipliers, powers of two
__global__ __launch_bounds__(BT_THREADS) void bw_add_identity_kernel(float* dx, const float* g3, int64_t items4, const float* sc3, const float* sc2,
                                                                     const float* sc1) {
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (i >= items4) return;
    const float mul = sc3[2] * sc2[2] * sc1[2];
    floatx4 a = *(floatx4*)(dx + i * 4);
    const floatx4 b = *(const floatx4*)(g3 + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += b[e] * mul;
    *(floatx4*)(dx + i * 4) = a;
}

// stride 2: dx [n][2H][2Wd][cin] (at dz1's total scale, dscale sc3[2] sc2[2] sc1[2]) += t = ds^T(dz_d) [n][H][Wd][cin] (at dz_d's total
// scale, dscale scd[2]) times sc3[2] sc2[2] sc1[2] / scd[2], powers of two all four, at the even (row, column) positions: the 1x1 stride-2
// convolution reads no other.  One thread = 4 channels.
__global__ __launch_bounds__(BT_THREADS) void bw_add_downsample_kernel(float* dx, const float* t, int64_t rows, int H, int Wd, int cin, const float* sc3,
                                                                       const float* sc2, const float* sc1, const float* scd) {
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    const int C4 = cin >> 2;
    if (i >= rows * C4) return;
    const int cq = (int)(i % C4);
    const int64_t m = i / C4;
    const int HW = H * Wd, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    float* d = dx + (((int64_t)img * 2 * H + 2 * y) * 2 * Wd + 2 * x) * cin + 4 * cq;
    const float mul = sc3[2] * sc2[2] * sc1[2] / scd[2];
    floatx4 a = *(floatx4*)d;
    const floatx4 b = *(const floatx4*)(t + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += b[e] * mul;
    *(floatx4*)d = a;
}

// the tensors of one struct the block reads: params (five per pair) or grads (the three learnable fields per pair)
int struct_check(const vtd_bottleneck_params* p, bool ds, bool stats) {
    if (!p) return BW_ERR_ARG;
    const float* const f[4][5] = {{p->conv1_w, p->bn1_w, p->bn1_b, p->bn1_mean, p->bn1_var}, {p->conv2_w, p->bn2_w, p->bn2_b, p->bn2_mean, p->bn2_var},
                                  {p->conv3_w, p->bn3_w, p->bn3_b, p->bn3_mean, p->bn3_var}, {p->ds_w, p->ds_bn_w, p->ds_bn_b, p->ds_bn_mean, p->ds_bn_var}};
    uintptr_t bits = 0;
    for (int i = 0; i < (ds ? 4 : 3); ++i)
        for (int j = 0; j < (stats ? 5 : 3); ++j) {
            if (!f[i][j]) return BW_ERR_ARG;
            bits |= (uintptr_t)f[i][j];
        }
    return (bits & 3) ? BW_ERR_ALIGN : 0;
}

unsigned ring_blocks(int n, int h, int w, int ch) { return nblk((int64_t)n * (2 * (w + 2) + 2 * h) * (ch / 8)); }

int64_t ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    Geo g;
    if (!make_geo(n, hin, win, cin, width, stride, g) || mode < 0 || mode > 1) return BW_ERR_ARG;
    // either mode of `training` runs in one allocation: the frozen path's layout starts at offset 0 too
    const int64_t frozen = width == 512 ? vtd_bottleneck_ws_bytes(n, hin, win, cin, width, stride, mode)
                                        : vtd_bottleneck256_ws_bytes(n, hin, win, cin, width, stride, mode);
    const int64_t own = mode ? bwd_layout(g).total : fwd_layout(g).total;
    if (frozen < 0) return BW_ERR_ARG;
    return frozen > own ? frozen : own;
}

template <int W>
int forward_launches(const void* x, const Geo& g, const vtd_bottleneck_params* P, float momentum, float eps, void* ws, void* y, float* stats,
                     hipStream_t s) {
    constexpr int OUT = 4 * W, NJ = OUT / 1024;
    const FwdLayout L = fwd_layout(g);
    const int n = g.n, hin = g.hin, win = g.win, cin = g.cin, stride = g.stride;
    const int64_t M = g.m, Min = g.min;
    char* w = (char*)ws;
    half_t *a1 = (half_t*)(w + L.a1), *a2 = (half_t*)(w + L.a2), *id = (half_t*)(w + L.id), *w1 = (half_t*)(w + L.w1), *w2 = (half_t*)(w + L.w2),
           *w3 = (half_t*)(w + L.w3), *wd = (half_t*)(w + L.wd);
    float *z1 = (float*)(w + L.z1), *z2 = (float*)(w + L.z2), *z3 = (float*)(w + L.z3), *zd = (float*)(w + L.zd), *zero = (float*)(w + L.zero),
          *tab1 = (float*)(w + L.tab1), *tab2 = (float*)(w + L.tab2), *tab3 = (float*)(w + L.tab3), *tabd = (float*)(w + L.tabd), *st = (float*)(w + L.st);
    double* part = (double*)(w + L.part);
    VTD_HIP_CHECK(hipMemsetAsync(zero, 0, OUT * 4, s));   // the convolutions' bias row, up to 4 W outputs
    hipLaunchKernelGGL(bt_pack_kernel<W>, dim3(nblk((int64_t)W * cin)), dim3(BT_THREADS), 0, s, (const float*)P->conv1_w, cin, 1, w1, (float*)nullptr);
    hipLaunchKernelGGL(bt_pack_kernel<W>, dim3(nblk((int64_t)W * 9 * W)), dim3(BT_THREADS), 0, s, (const float*)P->conv2_w, W, 9, w2, (float*)nullptr);
    hipLaunchKernelGGL(bt_pack_kernel<OUT>, dim3(nblk((int64_t)OUT * W)), dim3(BT_THREADS), 0, s, (const float*)P->conv3_w, W, 1, w3, (float*)nullptr);
    if (g.ds)
        hipLaunchKernelGGL(bt_pack_kernel<OUT>, dim3(nblk((int64_t)OUT * cin)), dim3(BT_THREADS), 0, s, (const float*)P->ds_w, cin, 1, wd, (float*)nullptr);
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, hin, win, W)), dim3(RB_THREADS), 0, s, a1, n, hin, win, W);
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, g.h, g.w, W)), dim3(RB_THREADS), 0, s, a2, n, g.h, g.w, W);
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, g.h, g.w, OUT)), dim3(RB_THREADS), 0, s, (half_t*)y, n, g.h, g.w, OUT);
    if (g.ds) hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, g.h, g.w, OUT)), dim3(RB_THREADS), 0, s, id, n, g.h, g.w, OUT);
    VTD_HIP_CHECK(hipGetLastError());

    // a convolution of a padded tap of hi x wi pixels into z [n ho wo][cout] fp32: zero bias, no activation
    auto conv_f32 = [&](const half_t* in, int ic, int hi, int wi, int ho, int wo, int cout, int ksz, int st_, const half_t* wp, float* z) {
        ConvParams c = conv_of(n, ho, wo, cout, in, ic, hi, wi, ksz, st_, wp, zero);
        c.out = z; c.ldc = cout; c.flags = EPI_OUT_F32;
        return vtd_launch_conv(c, -1, s);
    };
    // a W-wide pair after its convolution: the batch statistics (and the running update), the normalised tap of ho x wo pixels.  The
    // reported statistics go through st [2][W] into the first W columns of the caller's [2][4 W] row
    auto narrow = [&](const float* z, int64_t rows, const Red& r, int row, float* tab, const float* gam, const float* bet, float* rmean, float* rvar, int ho,
                      int wo, half_t* out) {
        hipLaunchKernelGGL(bt_stats_partial_kernel<W>, dim3(r.G), dim3(BT_THREADS), 0, s, z, rows, r.per, part);
        hipLaunchKernelGGL(bt_stats_finish_kernel<W>, dim3((W + BT_THREADS - 1) / BT_THREADS), dim3(BT_THREADS), 0, s, (const double*)part, r.G, gam, bet, rmean,
                           rvar, momentum, eps, tab, stats ? st : (float*)nullptr);
        if (stats)
            VTD_HIP_CHECK(hipMemcpy2DAsync(stats + (int64_t)row * 2 * OUT, (size_t)OUT * 4, st, (size_t)W * 4, (size_t)W * 4, 2, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(bt_apply_kernel<W>, dim3(nblk(rows * (W / 8))), dim3(BT_THREADS), 0, s, z, rows, (const float*)tab, (const half_t*)nullptr, 1, ho, wo,
                           out);
        return -(int)hipGetLastError();
    };
    // a 4 W-wide pair over the output's rows
    auto wide = [&](const float* z, int row, float* tab, const float* gam, const float* bet, float* rmean, float* rvar, const half_t* res, int relu,
                    half_t* out) {
        hipLaunchKernelGGL(bw_stats_partial_kernel<NJ>, dim3(g.r3.G), dim3(BT_THREADS), 0, s, z, M, g.r3.per, part);
        hipLaunchKernelGGL(bt_stats_finish_kernel<OUT>, dim3(OUT / BT_THREADS), dim3(BT_THREADS), 0, s, (const double*)part, g.r3.G, gam, bet, rmean, rvar,
                           momentum, eps, tab, stats ? stats + (int64_t)row * 2 * OUT : (float*)nullptr);
        hipLaunchKernelGGL(bt_apply_kernel<OUT>, dim3(nblk(M * (OUT / 8))), dim3(BT_THREADS), 0, s, z, M, (const float*)tab, res, relu, g.h, g.w, out);
        return -(int)hipGetLastError();
    };
    int rc;
    if ((rc = conv_f32((const half_t*)x, cin, hin, win, hin, win, W, 1, 1, w1, z1))) return rc;
    if ((rc = narrow(z1, Min, g.r1, 0, tab1, P->bn1_w, P->bn1_b, P->bn1_mean, P->bn1_var, hin, win, a1))) return rc;
    if ((rc = conv_f32(a1, W, hin, win, g.h, g.w, W, 3, stride, w2, z2))) return rc;
    if ((rc = narrow(z2, M, g.r2, 1, tab2, P->bn2_w, P->bn2_b, P->bn2_mean, P->bn2_var, g.h, g.w, a2))) return rc;
    if (g.ds) {
        if ((rc = conv_f32((const half_t*)x, cin, hin, win, g.h, g.w, OUT, 1, stride, wd, zd))) return rc;
        if ((rc = wide(zd, 3, tabd, P->ds_bn_w, P->ds_bn_b, P->ds_bn_mean, P->ds_bn_var, nullptr, 0, id))) return rc;
    }
    if ((rc = conv_f32(a2, W, g.h, g.w, g.h, g.w, OUT, 1, 1, w3, z3))) return rc;
    return wide(z3, 2, tab3, P->bn3_w, P->bn3_b, P->bn3_mean, P->bn3_var, g.ds ? id : (const half_t*)x, 1, (half_t*)y);
}

template <int W>
int backward_launches(const void* x, const Geo& g, const vtd_bottleneck_params* P, const void* ws, const void* y, const float* dy, const float* dscale,
                      const vtd_bottleneck_params* Gp, void* scratch, float* dx, float* dxscale, hipStream_t s) {
    constexpr int OUT = 4 * W, NJ = OUT / 1024;
    const FwdLayout L = fwd_layout(g);
    const BwdLayout B = bwd_layout(g);
    const int n = g.n, hin = g.hin, win = g.win, cin = g.cin, stride = g.stride;
    const int64_t M = g.m, Min = g.min;
    const char* w = (const char*)ws;
    char* q = (char*)scratch;
    const half_t *a1 = (const half_t*)(w + L.a1), *a2 = (const half_t*)(w + L.a2);
    const float *z1 = (const float*)(w + L.z1), *z2 = (const float*)(w + L.z2), *z3 = (const float*)(w + L.z3), *zd = (const float*)(w + L.zd),
                *tab1 = (const float*)(w + L.tab1), *tab2 = (const float*)(w + L.tab2), *tab3 = (const float*)(w + L.tab3), *tabd = (const float*)(w + L.tabd);
    float *g3 = (float*)(q + B.g3), *g2 = (float*)(q + B.g2), *g1 = (float*)(q + B.g1), *zero = (float*)(q + B.zero), *pmax = (float*)(q + B.pmax),
          *coef = (float*)(q + B.coef), *sc = (float*)(q + B.sc), *slab = (float*)(q + B.slab);
    half_t *dzh = (half_t*)(q + B.dzh), *dz3p = (half_t*)(q + B.dz3p), *dz2p = (half_t*)(q + B.dz2p), *dz1p = (half_t*)(q + B.dz1p), *wt = (half_t*)(q + B.wt);
    double* part = (double*)(q + B.part);
    float *sc3 = sc, *scd = sc + 4, *sc2 = sc + 8, *sc1 = sc + 12;
    int rc;

    // the rest of a 4 W-wide pair's BatchNorm backward after its reduce: dgamma / dbeta, the scale, dz as the fp16 operands (flat, and the
    // interior of the ring-padded dz3p when `plane`)
    auto wide_finish_form = [&](const float* z, const float* tab, const float* in_sc, float* out_sc, float* dgam, float* dbet, bool plane) {
        hipLaunchKernelGGL(bw_bwd_finish_kernel<OUT>, dim3(1), dim3(BW_FINISH_THREADS), 0, s, (const double*)part, (const float*)pmax, g.r3.G, 1.0 / (double)M, tab,
                           in_sc, coef, dgam, dbet, out_sc);
        hipLaunchKernelGGL(bt_form_kernel<OUT>, dim3(nblk(M * (OUT / 8))), dim3(BT_THREADS), 0, s, (const float*)g3, z, tab, (const float*)coef,
                           (const float*)out_sc, M, g.h, g.w, 1, dzh, plane ? dz3p : (half_t*)nullptr);
    };
    // a W-wide pair: `gr` [rows][W] of ho x wo pixels masked in place by the padded activation, then the reduce, the finish and the operands
    // (`plane`: ring-padded at pixel (dil y, dil x), or none)
    auto narrow_back = [&](float* gr, const half_t* act, const float* z, const float* tab, int64_t rows, const Red& r, int ho, int wo, const float* in_sc,
                           float* out_sc, float* dgam, float* dbet, half_t* plane, int dil) {
        hipLaunchKernelGGL(rb_mask_kernel, dim3(nblk(rows * (W / 4))), dim3(RB_THREADS), 0, s, (const float*)gr, act, rows, ho, wo, W, gr);
        hipLaunchKernelGGL(bt_bwd_reduce_kernel<W>, dim3(r.G), dim3(BT_THREADS), 0, s, (const float*)gr, z, tab, rows, r.per, part, pmax);
        hipLaunchKernelGGL(bt_bwd_finish_kernel<W>, dim3(1), dim3(W), 0, s, (const double*)part, (const float*)pmax, r.G, 1.0 / (double)rows, tab, in_sc, coef,
                           dgam, dbet, out_sc);
        hipLaunchKernelGGL(bt_form_kernel<W>, dim3(nblk(rows * (W / 8))), dim3(BT_THREADS), 0, s, (const float*)gr, z, tab, (const float*)coef,
                           (const float*)out_sc, rows, ho, wo, dil, dzh, plane);
    };
    // dzh: [rows][lda] operands of a convolution of ksz x ksz at stride st over the padded input xin (xc channels, hi x wi pixels) whose output
    // has ho x wo pixels
    auto wgrad = [&](int lda, int64_t rows, int ho, int wo, const half_t* xin, int xc, int hi, int wi, int ksz, int st, const float* scl, float* dw) {
        WgArgs wa;
        wa.a = dzh; wa.lda = lda; wa.x = xin; wa.xc = xc; wa.n = n; wa.H = ho; wa.W = wo; wa.rows = rows; wa.slab = slab;
        const int nqt = wg_nqt(ksz, xc), Sl = wg_slabs(rows);
        wa.slab_len = slab_rows(rows, Sl); wa.ksz = ksz; wa.stride = st; wa.Hin = hi; wa.Win = wi;
        hipLaunchKernelGGL(dbhead_train_wgrad_kernel<3>, dim3(nqt * Sl, lda / 128), dim3(WG_THREADS), 0, s, wa);
        hipLaunchKernelGGL(bt_dw_kernel, dim3(lda), dim3(BT_THREADS), 0, s, (const float*)slab, Sl, xc, ksz * ksz, scl, dw);
    };
    // conv^T of a padded dz plane gp of hp x wp pixels into [n hp wp][rows] fp32: the raw weights of a convolution with `rows` input channels
    // and CO (the plane's) output channels, rotated and transposed into the panel `wt`
    auto dgrad = [&](auto co, const half_t* gp, int hp, int wp, const float* wsrc, int rows, int ksz, float* out) {
        constexpr int CO = decltype(co)::value;
        hipLaunchKernelGGL(bt_pack_dgrad_kernel<CO>, dim3(nblk((int64_t)rows * ksz * ksz * CO + CO)), dim3(BT_THREADS), 0, s, wsrc, rows, ksz * ksz, wt, zero);
        ConvParams c = conv_of(n, hp, wp, rows, gp, CO, hp, wp, ksz, 1, wt, zero);
        c.out = out; c.ldc = rows; c.flags = EPI_OUT_F32;
        return vtd_launch_conv(c, -1, s);
    };
    const std::integral_constant<int, W> narrow_c;
    const std::integral_constant<int, OUT> wide_c;

    // the zero bias row of the transposed convolutions: up to 4 W outputs (conv1^T of the identity block)
    VTD_HIP_CHECK(hipMemsetAsync(zero, 0, OUT * 4, s));
    // bn3: g3 = dy (y > 0) and its partials in one pass
    hipLaunchKernelGGL((bw_bwd_reduce_kernel<NJ, true>), dim3(g.r3.G), dim3(BT_THREADS), 0, s, dy, (const half_t*)y, z3, tab3, M, g.r3.per, g.h, g.w, g3, part,
                       pmax);
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, g.h, g.w, OUT)), dim3(RB_THREADS), 0, s, dz3p, n, g.h, g.w, OUT);
    wide_finish_form(z3, tab3, dscale, sc3, Gp->bn3_w, Gp->bn3_b, true);
    wgrad(OUT, M, g.h, g.w, a2, W, g.h, g.w, 1, 1, sc3, Gp->conv3_w);
    VTD_HIP_CHECK(hipGetLastError());
    // da2 = conv3^T(dz3) into the g2 buffer
    if ((rc = dgrad(wide_c, dz3p, g.h, g.w, (const float*)P->conv3_w, W, 1, g2))) return rc;
    if (g.ds) {   // the downsample pair: its upstream gradient is g3, its statistics and its dz_d are its own
        hipLaunchKernelGGL((bw_bwd_reduce_kernel<NJ, false>), dim3(g.r3.G), dim3(BT_THREADS), 0, s, (const float*)g3, (const half_t*)nullptr, zd, tabd, M,
                           g.r3.per, g.h, g.w, (float*)nullptr, part, pmax);
        wide_finish_form(zd, tabd, dscale, scd, Gp->ds_bn_w, Gp->ds_bn_b, dx != nullptr);   // dz3p's ring is zero already
        wgrad(OUT, M, g.h, g.w, (const half_t*)x, cin, hin, win, 1, stride, scd, Gp->ds_w);
        VTD_HIP_CHECK(hipGetLastError());
        // ds^T(dz_d) at dz_d's scale into the g3 buffer: its fp32 values are in the operands by now, and the identity add is the other block's
        if (dx && (rc = dgrad(wide_c, dz3p, g.h, g.w, (const float*)P->ds_w, cin, 1, g3))) return rc;
    }
    // bn2: dz2 ring-padded at the input's extent -- the interior for the stride-1 block, the even positions of a zeroed plane at stride 2
    if (stride == 2)
        VTD_HIP_CHECK(hipMemsetAsync(dz2p, 0, (size_t)g.pin * W * 2, s));
    else
        hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, g.h, g.w, W)), dim3(RB_THREADS), 0, s, dz2p, n, g.h, g.w, W);
    narrow_back(g2, a2, z2, tab2, M, g.r2, g.h, g.w, sc3, sc2, Gp->bn2_w, Gp->bn2_b, dz2p, stride);
    wgrad(W, M, g.h, g.w, a1, W, hin, win, 3, stride, sc2, Gp->conv2_w);
    VTD_HIP_CHECK(hipGetLastError());
    // da1 = conv2^T(dz2) at the input's extent into the g1 buffer
    if ((rc = dgrad(narrow_c, dz2p, hin, win, (const float*)P->conv2_w, W, 3, g1))) return rc;
    if (dx) hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, hin, win, W)), dim3(RB_THREADS), 0, s, dz1p, n, hin, win, W);
    narrow_back(g1, a1, z1, tab1, Min, g.r1, hin, win, sc2, sc1, Gp->bn1_w, Gp->bn1_b, dx ? dz1p : (half_t*)nullptr, 1);
    wgrad(W, Min, hin, win, (const half_t*)x, cin, hin, win, 1, 1, sc1, Gp->conv1_w);
    VTD_HIP_CHECK(hipGetLastError());
    if (dx) {
        if ((rc = dgrad(narrow_c, dz1p, hin, win, (const float*)P->conv1_w, cin, 1, dx))) return rc;
        if (!g.ds)
            hipLaunchKernelGGL(bw_add_identity_kernel, dim3(nblk(M * (OUT / 4))), dim3(BT_THREADS), 0, s, dx, (const float*)g3, M * (OUT / 4), (const float*)sc3,
                               (const float*)sc2, (const float*)sc1);
        else
            hipLaunchKernelGGL(bw_add_downsample_kernel, dim3(nblk(M * (cin / 4))), dim3(BT_THREADS), 0, s, dx, (const float*)g3, M, g.h, g.w, cin,
                               (const float*)sc3, (const float*)sc2, (const float*)sc1, (const float*)scd);
        hipLaunchKernelGGL(rb_copy_scale_kernel, dim3(1), dim3(64), 0, s, (const float*)sc1, dxscale);
    }
    return -(int)hipGetLastError();
}

}  // namespace

int64_t vtd_bottleneck_bn_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    return ws_bytes(n, hin, win, cin, width, stride, mode);
}

int vtd_launch_bottleneck_bn_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, int training,
                                     float momentum, float eps, void* ws, void* y, float* stats, hipStream_t s) {
    Geo g;
    if (!x || !ws || !y || !make_geo(n, hin, win, cin, width, stride, g) || !(eps > 0.f) || (training != 0 && training != 1)) return BW_ERR_ARG;
    const int pc = struct_check(P, g.ds, true);
    if (pc == BW_ERR_ARG) return pc;
    if (training && (g.m < 2 || !(momentum >= 0.f && momentum <= 1.f))) return BW_ERR_ARG;   // g.min >= g.m: every pair has two rows
    if (pc || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)ws & 255) || ((uintptr_t)stats & 3)) return BW_ERR_ALIGN;
    if (!training)
        return width == 512 ? vtd_launch_bottleneck_forward(x, n, hin, win, cin, width, stride, P, eps, ws, y, s)
                            : vtd_launch_bottleneck256_forward(x, n, hin, win, cin, width, stride, P, eps, ws, y, s);
    return width == 512 ? forward_launches<512>(x, g, P, momentum, eps, ws, y, stats, s) : forward_launches<256>(x, g, P, momentum, eps, ws, y, stats, s);
}

int vtd_launch_bottleneck_bn_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, int training,
                                      float eps, const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp,
                                      void* scratch, float* dx, float* dxscale, hipStream_t s) {
    Geo g;
    if (!x || !ws || !y || !dy || !dscale || !scratch || !make_geo(n, hin, win, cin, width, stride, g) || !(eps > 0.f) || (dx && !dxscale) ||
        (training != 0 && training != 1) || (training && g.m < 2))
        return BW_ERR_ARG;
    const int pc = struct_check(P, g.ds, true), gc = struct_check(Gp, g.ds, false);
    if (pc == BW_ERR_ARG || gc == BW_ERR_ARG) return BW_ERR_ARG;
    if (pc || gc || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)ws & 255) || ((uintptr_t)scratch & 255) || ((uintptr_t)dy & 15) ||
        ((uintptr_t)dscale & 7) || ((uintptr_t)dx & 15) || ((uintptr_t)dxscale & 7))
        return BW_ERR_ALIGN;
    if (!training)
        return width == 512 ? vtd_launch_bottleneck_backward(x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s)
                            : vtd_launch_bottleneck256_backward(x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s);
    return width == 512 ? backward_launches<512>(x, g, P, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s)
                        : backward_launches<256>(x, g, P, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s);
}
