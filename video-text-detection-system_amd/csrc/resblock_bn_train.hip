// ResNet BasicBlock training with batch-statistics BatchNorm (torch's train() mode: the statistics of the batch normalise, the running
// statistics are updated in place), forward and backward, for the two blocks of ResNet-18's layer4: (256 -> 512, stride 2, downsample) and
// (512 -> 512, stride 1).  W = 512 throughout.  With training = 0 the entries hand the call to the frozen-statistics path
// (resblock_train.hip, vtd_basicblock_train_*) unchanged.
// Tensors are padded taps (ring-padded NHWC fp16, ring 1).  y = relu(bn2(conv2(relu(bn1(conv1(x))))) + id), id = x or ds_bn(ds(x)).
//
// Forward, per convolution + BatchNorm pair (conv1 / bn1, the downsample, conv2 / bn2):
//   pack             the raw weights -> fp16 GEMM panel [W][ksz^2 cin] (k = tap * cin + ci); no fold: gamma rstd is not known yet
//   conv             conv_igemm.hip with EPI_OUT_F32 and a zero bias: z [M][W] fp32, kept in the workspace for the backward
//   stats partial    workgroup g owns rows g per .. g per + per - 1 (per = ceil(M / G), G = min(256, ceil(M / 256))).  Thread t owns channels
//                    4 (t % 128) .. + 3 with 16-byte loads; t < 128 sums the first ceil(r / 2) of the workgroup's r rows in row order, t >= 128
//                    the rest; sums of z and z^2 in fp64, lower + upper, then (count, mean, M2) per channel
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
//                    with the scale undone: dz carries gamma rstd, no factor follows
//   dgrad            da1 = conv2^T(dz2): conv_igemm.hip on the raw weights rotated by 180 degrees and transposed; g1 = da1 (a1 > 0)
//   dx (stride 1)    conv1^T(dz1) the same way, plus g2 brought to the same scale.  The stride-2 block forms no input gradient here
// Nothing divides by gamma or sigma.  No atomics, shape-only grids, fixed summation orders: bitwise repeatable.
#include "resblock_common.h"

int vtd_launch_conv(const ConvParams& p, int cfg, hipStream_t stream);
int64_t vtd_basicblock_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode);
int vtd_launch_basicblock_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                  void* ws, void* y, hipStream_t s);
int vtd_launch_basicblock_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, float eps,
                                   const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp, void* scratch,
                                   float* dx, float* dxscale, hipStream_t s);

namespace {

constexpr int BT_THREADS = RB_THREADS;
constexpr int BT_W = 512;          // the block's width: layer4's
constexpr int BT_MAX_RED = 256;
constexpr int BT_ERR = -3400;

typedef double doublex4 __attribute__((ext_vector_type(4)));

struct Geo {
    int n, hin, win, cin, stride, h, w;
    int64_t m;
    bool ds;
    int red;       // reduce workgroups
    int64_t per;   // rows of each
};

bool make_geo(int n, int hin, int win, int cin, int width, int stride, Geo& g) {
    if (n <= 0 || hin <= 0 || win <= 0 || n > 65535 || hin > 4096 || win > 4096 || width != BT_W) return false;
    if (!((cin == 256 && stride == 2 && !(hin & 1) && !(win & 1)) || (cin == 512 && stride == 1))) return false;
    g.n = n; g.hin = hin; g.win = win; g.cin = cin; g.stride = stride; g.h = hin / stride; g.w = win / stride;
    g.m = (int64_t)n * g.h * g.w;
    g.ds = stride == 2;
    int64_t r = (g.m + 255) / 256;
    g.red = (int)(r < 1 ? 1 : r > BT_MAX_RED ? BT_MAX_RED : r);
    g.per = (g.m + g.red - 1) / g.red;
    return (int64_t)n * (hin + 2) * (win + 2) * width < (1ll << 31);
}

// the workspace of a training = 1 forward.  tab: {mu, rstd, gamma, beta} [4][W] per pair (bn1, bn2, the downsample's)
struct FwdLayout { int64_t a1, id, z1, z2, zd, w1, w2, wd, zero, part, tab, total; };
struct BwdLayout { int64_t g2, g1, dzh, dzp, wt, zero, part, pmax, coef, sc, slab, total; };

FwdLayout fwd_layout(const Geo& g) {
    FwdLayout L;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    const int64_t W = BT_W, pad = (int64_t)g.n * (g.h + 2) * (g.w + 2) * W * 2, zb = g.m * W * 4;
    L.a1 = take(pad); L.id = take(g.ds ? pad : 0);
    L.z1 = take(zb); L.z2 = take(zb); L.zd = take(g.ds ? zb : 0);
    L.w1 = take(W * 9 * g.cin * 2); L.w2 = take(W * 9 * W * 2); L.wd = take(g.ds ? W * g.cin * 2 : 0);
    L.zero = take(W * 4);
    L.part = take((int64_t)BT_MAX_RED * W * 3 * 8);
    L.tab = take(3 * 4 * W * 4);
    L.total = o;
    return L;
}

BwdLayout bwd_layout(const Geo& g) {
    BwdLayout L;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    const int64_t W = BT_W, pad = (int64_t)g.n * (g.h + 2) * (g.w + 2) * W * 2;
    L.g2 = take(g.m * W * 4); L.g1 = take(g.m * W * 4);
    L.dzh = take(g.m * W * 2); L.dzp = take(pad);
    L.wt = take(W * 9 * W * 2);
    L.zero = take(W * 4);
    L.part = take((int64_t)BT_MAX_RED * 2 * W * 8); L.pmax = take((int64_t)BT_MAX_RED * 2 * W * 4);
    L.coef = take(3 * W * 4);
    L.sc = take(3 * 4 * 4);
    L.slab = take((int64_t)wg_slabs(g.m) * W * 9 * W * 4);
    L.total = o;
    return L;
}

// NaN-keeping maximum, as resblock_train.hip's reduce kernels take it
__device__ __forceinline__ float nmax(float m, float a) { return a > m || a != a ? a : m; }

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
// wp [W][taps cin], k = tap * cin + ci: half(w[co][ci][tap]); zero[W] = 0 (the convolutions' bias row)
__global__ __launch_bounds__(BT_THREADS) void bt_pack_kernel(const float* w, int cin, int taps, half_t* wp, float* zero) {
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    const int K = taps * cin;
    if (i < (int64_t)BT_W * K) {
        const int co = (int)(i / K), k = (int)(i - (int64_t)co * K), tap = k / cin, ci = k - tap * cin;
        wp[i] = (half_t)w[((int64_t)co * cin + ci) * taps + tap];
    } else if (zero && i < (int64_t)BT_W * K + BT_W) {
        zero[i - (int64_t)BT_W * K] = 0.f;
    }
}

// the rows [lo, hi) of thread t in workgroup `blk`: the lower half of the workgroup's rows for t < 128, the upper half for t >= 128
__device__ __forceinline__ void bt_rows(int64_t rows, int64_t per, int hf, int64_t& m0, int64_t& m1, int64_t& lo, int64_t& hi) {
    m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows;
    m1 = m0 + per < rows ? m0 + per : rows;
    const int64_t mid = m0 + (m1 - m0 + 1) / 2;
    lo = hf ? mid : m0;
    hi = hf ? m1 : mid;
}

// z [rows][W] fp32 -> part[g][c] = {count, mean, M2} (fp64).  LDS [value][thread]: consecutive lanes, consecutive doubles
__global__ __launch_bounds__(BT_THREADS) void bt_stats_partial_kernel(const float* z, int64_t rows, int64_t per, double* part) {
    const int t = threadIdx.x, j = t & 127, hf = t >> 7;
    int64_t m0, m1, lo, hi;
    bt_rows(rows, per, hf, m0, m1, lo, hi);
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int64_t m = lo; m < hi; ++m) {
        const floatx4 v = *(const floatx4*)(z + m * BT_W + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const double a = (double)v[e]; s[e] += a; q[e] += a * a; }
    }
    __shared__ double sh[8][128];
    if (hf) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { sh[e][j] = s[e]; sh[4 + e][j] = q[e]; }
    }
    __syncthreads();
    if (!hf) {
        const double cnt = (double)(m1 - m0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double S = s[e] + sh[e][j], Q = q[e] + sh[4 + e][j];
            const double mean = cnt > 0 ? S / cnt : 0.0;
            double* o = part + ((int64_t)blockIdx.x * BT_W + 4 * j + e) * 3;
            o[0] = cnt; o[1] = mean; o[2] = cnt > 0 ? fmax(Q - S * mean, 0.0) : 0.0;
        }
    }
}

// One thread per channel: Chan's combination of the partials in workgroup order (fp64), torch's running-statistics update, the table
// {mu, rstd, gamma, beta} and (optionally) stats_out = {mu, sigma^2} [2][W]
__global__ __launch_bounds__(BT_THREADS) void bt_stats_finish_kernel(const double* part, int G, const float* gam, const float* bet, float* rmean, float* rvar,
                                                                     float momentum, float eps, float* tab, float* stats_out) {
    const int c = blockIdx.x * BT_THREADS + threadIdx.x;
    double n = 0.0, mu = 0.0, m2 = 0.0;
    for (int g = 0; g < G; ++g) {
        const double* q = part + ((int64_t)g * BT_W + c) * 3;
        const double nb = q[0];
        if (nb <= 0.0) continue;
        const double tot = n + nb, d = q[1] - mu;
        mu += d * (nb / tot);
        m2 += q[2] + d * d * (n * nb / tot);
        n = tot;
    }
    const double var = m2 / n, unbiased = m2 / (n - 1.0);   // n >= 2: the entry refuses fewer rows
    rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * mu);
    rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * unbiased);
    tab[c] = (float)mu;
    tab[BT_W + c] = (float)(1.0 / sqrt(var + (double)eps));
    tab[2 * BT_W + c] = gam[c];
    tab[3 * BT_W + c] = bet[c];
    if (stats_out) {
        stats_out[c] = (float)mu;
        stats_out[BT_W + c] = (float)var;
    }
}

// out (padded tap) = [relu](((z - mu) rstd) gamma + beta [+ res]); res is a padded tap of the output's extents.  One thread = 8 channels
__global__ __launch_bounds__(BT_THREADS) void bt_apply_kernel(const float* z, int64_t rows, const float* tab, const half_t* res, int relu, int H, int Wd,
                                                              half_t* out) {
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (i >= rows * (BT_W / 8)) return;
    const int c0 = (int)(i & 63) * 8;
    const int64_t m = i >> 6;
    const int HW = H * Wd, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    const int64_t off = (((int64_t)img * (H + 2) + y + 1) * (Wd + 2) + x + 1) * BT_W + c0;
    half8 rv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (res) rv = *(const half8*)(res + off);
    half8 h;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const floatx4 v = *(const floatx4*)(z + i * 8 + 4 * k);
        const floatx4 mu = *(const floatx4*)(tab + c0 + 4 * k), rs = *(const floatx4*)(tab + BT_W + c0 + 4 * k);
        const floatx4 gm = *(const floatx4*)(tab + 2 * BT_W + c0 + 4 * k), bt = *(const floatx4*)(tab + 3 * BT_W + c0 + 4 * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = ((v[e] - mu[e]) * rs[e]) * gm[e] + bt[e];
            if (res) a += (float)rv[4 * k + e];
            if (relu) a = a > 0.f ? a : 0.f;
            h[4 * k + e] = (half_t)a;
        }
    }
    *(half8*)(out + off) = h;
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
// g, z [rows][W] fp32 -> part[blk][0][c] = sum g, part[blk][1][c] = sum g xh (fp64), pmax[blk][0][c] = max |g|, pmax[blk][1][c] = max |xh|,
// xh = (z - mu) rstd as the forward formed it.  Rows and threads as bt_stats_partial_kernel
__global__ __launch_bounds__(BT_THREADS) void bt_bwd_reduce_kernel(const float* g, const float* z, const float* tab, int64_t rows, int64_t per, double* part,
                                                                   float* pmax) {
    const int t = threadIdx.x, j = t & 127, hf = t >> 7;
    int64_t m0, m1, lo, hi;
    bt_rows(rows, per, hf, m0, m1, lo, hi);
    const floatx4 mu = *(const floatx4*)(tab + 4 * j), rs = *(const floatx4*)(tab + BT_W + 4 * j);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    floatx4 mg = {0.f, 0.f, 0.f, 0.f}, mx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int64_t m = lo; m < hi; ++m) {
        const floatx4 gv = *(const floatx4*)(g + m * BT_W + 4 * j), zv = *(const floatx4*)(z + m * BT_W + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (zv[e] - mu[e]) * rs[e];
            s1[e] += (double)gv[e];
            s2[e] += (double)gv[e] * (double)xh;
            mg[e] = nmax(mg[e], fabsf(gv[e]));
            mx[e] = nmax(mx[e], fabsf(xh));
        }
    }
    __shared__ double sh[8][128];
    __shared__ float shm[8][128];
    if (hf) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { sh[e][j] = s1[e]; sh[4 + e][j] = s2[e]; shm[e][j] = mg[e]; shm[4 + e][j] = mx[e]; }
    }
    __syncthreads();
    if (!hf) {
        doublex4 o1, o2;
        floatx4 p1, p2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o1[e] = s1[e] + sh[e][j]; o2[e] = s2[e] + sh[4 + e][j];
            p1[e] = nmax(mg[e], shm[e][j]); p2[e] = nmax(mx[e], shm[4 + e][j]);
        }
        const int64_t b = (int64_t)blockIdx.x * 2 * BT_W + 4 * j;
        *(doublex4*)(part + b) = o1; *(doublex4*)(part + b + BT_W) = o2;
        *(floatx4*)(pmax + b) = p1; *(floatx4*)(pmax + b + BT_W) = p2;
    }
}

// One workgroup of W threads, thread c = channel c.  The partials in workgroup order (fp64).  dbeta = s1, dgamma = s2 with the incoming scale
// undone; coef = {gamma rstd, s1 / M, s2 / M} [3][W] at the incoming scale; out_sc = {total scale, 1 / total, this stage's multiplier, 0}:
// the multiplier is a power of two from the bound max_c |gamma rstd| (max |g| + |s1| / M + max |xh| |s2| / M) >= max |dz| (1 when that is
// zero or not finite)
__global__ __launch_bounds__(BT_W) void bt_bwd_finish_kernel(const double* part, const float* pmax, int G, double inv_m, const float* tab, const float* in_sc,
                                                             float* coef, float* dgam, float* dbet, float* out_sc) {
    const int c = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    float mg = 0.f, mx = 0.f;
    for (int g = 0; g < G; ++g) {
        const int64_t b = (int64_t)g * 2 * BT_W + c;
        s1 += part[b]; s2 += part[b + BT_W];
        mg = nmax(mg, pmax[b]); mx = nmax(mx, pmax[b + BT_W]);
    }
    const float A = tab[2 * BT_W + c] * tab[BT_W + c], B = (float)(s1 * inv_m), C = (float)(s2 * inv_m);
    coef[c] = A; coef[BT_W + c] = B; coef[2 * BT_W + c] = C;
    dbet[c] = (float)(s1 * (double)in_sc[1]);
    dgam[c] = (float)(s2 * (double)in_sc[1]);
    __shared__ float sh[BT_W];
    sh[c] = (float)(fabs((double)A) * ((double)mg + fabs((double)B) + (double)mx * fabs((double)C)));
    __syncthreads();
    for (int o = BT_W / 2; o > 0; o >>= 1) {
        if (c < o) sh[c] = nmax(sh[c], sh[c + o]);
        __syncthreads();
    }
    if (c == 0) {
        const float bound = sh[0];
        const double tin = (double)in_sc[0];
        int e = 0;
        if (bound > 0.f && isfinite(bound)) e = (int)floor(log2((double)RB_SCALE_TARGET / (double)bound));
        const int ein = (tin > 0.0 && isfinite(tin)) ? ilogb(tin) : 0;
        int et = ein + e;
        et = et < -120 ? -120 : et > 120 ? 120 : et;
        e = et - ein;
        const double tot = tin * ldexp(1.0, e);
        out_sc[0] = (float)tot; out_sc[1] = (float)(1.0 / tot); out_sc[2] = ldexpf(1.0f, e); out_sc[3] = 0.f;
    }
}

// dz = gamma rstd (g - s1 / M - xh s2 / M) in fp32, times the multiplier, as fp16: flat [rows][W] and (when given) the interior of a
// ring-padded plane.  One thread = 8 channels.
__global__ __launch_bounds__(BT_THREADS) void bt_form_kernel(const float* g, const float* z, const float* tab, const float* coef, const float* sc,
                                                             int64_t rows, int H, int Wd, half_t* flat, half_t* padded) {
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (i >= rows * (BT_W / 8)) return;
    const int c0 = (int)(i & 63) * 8;
    const float mul = sc[2];
    half8 h;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const floatx4 gv = *(const floatx4*)(g + i * 8 + 4 * k), zv = *(const floatx4*)(z + i * 8 + 4 * k);
        const floatx4 mu = *(const floatx4*)(tab + c0 + 4 * k), rs = *(const floatx4*)(tab + BT_W + c0 + 4 * k);
        const floatx4 A = *(const floatx4*)(coef + c0 + 4 * k), B = *(const floatx4*)(coef + BT_W + c0 + 4 * k),
                      C = *(const floatx4*)(coef + 2 * BT_W + c0 + 4 * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (zv[e] - mu[e]) * rs[e];
            h[4 * k + e] = (half_t)(A[e] * (gv[e] - B[e] - xh * C[e]) * mul);
        }
    }
    *(half8*)(flat + i * 8) = h;
    if (padded) {
        const int64_t m = i >> 6;
        const int HW = H * Wd, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
        *(half8*)(padded + (((int64_t)img * (H + 2) + y + 1) * (Wd + 2) + x + 1) * BT_W + c0) = h;
    }
}

// wt [cin][taps * W]: row ci, k = tap' * W + co holds half(w[co][ci][taps - 1 - tap']) (the window rotated by 180 degrees, the raw weights
// transposed, rounded as the forward packs them); a zero bias row of W entries
__global__ __launch_bounds__(BT_THREADS) void bt_pack_dgrad_kernel(const float* w, int cin, int taps, half_t* wt, float* zero) {
    const int i = blockIdx.x * BT_THREADS + threadIdx.x;
    const int K = taps * BT_W;
    if (i < cin * K) {
        const int ci = i / K, k = i - ci * K, tap = k / BT_W, co = k - tap * BT_W;
        wt[i] = (half_t)w[((int64_t)co * cin + ci) * taps + (taps - 1 - tap)];
    } else if (i < cin * K + BT_W) {
        zero[i - cin * K] = 0.f;
    }
}

// One workgroup per output channel c: dW[c][ci][tap] = the slabs summed in slab order (fp64) with the scale undone, k = tap * cin + ci
__global__ __launch_bounds__(BT_THREADS) void bt_dw_kernel(const float* slab, int S, int cin, int taps, const float* sc, float* dw) {
    const int c = blockIdx.x, K = taps * cin;
    const double inv = (double)sc[1];
    const int64_t nel = (int64_t)gridDim.x * K;
    for (int k = threadIdx.x; k < K; k += BT_THREADS) {
        double G = 0.0;
        for (int s = 0; s < S; ++s) G += (double)slab[(int64_t)s * nel + (int64_t)c * K + k];
        const int tap = k / cin, ci = k - tap * cin;
        dw[((int64_t)c * cin + ci) * taps + tap] = (float)(G * inv);
    }
}

}  // namespace

int64_t vtd_resblock_bn_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    Geo g;
    if (!make_geo(n, hin, win, cin, width, stride, g) || mode < 0 || mode > 1) return BT_ERR - 1;
    // either mode of `training` runs in one allocation: the frozen path's layout starts at offset 0 too
    const int64_t frozen = vtd_basicblock_ws_bytes(n, hin, win, cin, width, stride, mode), own = mode ? bwd_layout(g).total : fwd_layout(g).total;
    if (frozen < 0) return BT_ERR - 1;
    return frozen > own ? frozen : own;
}

int vtd_launch_resblock_bn_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                   float momentum, float eps, void* ws, void* y, float* stats, hipStream_t s) {
    Geo g;
    if (!x || !ws || !y || !make_geo(n, hin, win, cin, width, stride, g) || !params_ok(P, g.ds) || !(eps > 0.f) || (training != 0 && training != 1))
        return BT_ERR - 1;
    if (training && (g.m < 2 || !(momentum >= 0.f && momentum <= 1.f))) return BT_ERR - 1;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)ws & 255) || ((uintptr_t)stats & 3)) return BT_ERR - 2;
    if (!training) return vtd_launch_basicblock_forward(x, n, hin, win, cin, width, stride, P, eps, ws, y, s);
    const FwdLayout L = fwd_layout(g);
    const int W = BT_W;
    const int64_t M = g.m;
    char* w = (char*)ws;
    half_t *a1 = (half_t*)(w + L.a1), *id = (half_t*)(w + L.id), *w1 = (half_t*)(w + L.w1), *w2 = (half_t*)(w + L.w2), *wd = (half_t*)(w + L.wd);
    float *z1 = (float*)(w + L.z1), *z2 = (float*)(w + L.z2), *zd = (float*)(w + L.zd), *zero = (float*)(w + L.zero), *tab = (float*)(w + L.tab);
    double* part = (double*)(w + L.part);
    hipLaunchKernelGGL(bt_pack_kernel, dim3(nblk((int64_t)W * 9 * cin + W)), dim3(BT_THREADS), 0, s, (const float*)P->conv1_w, cin, 9, w1, zero);
    hipLaunchKernelGGL(bt_pack_kernel, dim3(nblk((int64_t)W * 9 * W)), dim3(BT_THREADS), 0, s, (const float*)P->conv2_w, W, 9, w2, (float*)nullptr);
    if (g.ds) hipLaunchKernelGGL(bt_pack_kernel, dim3(nblk((int64_t)W * cin)), dim3(BT_THREADS), 0, s, (const float*)P->ds_w, cin, 1, wd, (float*)nullptr);
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
        hipLaunchKernelGGL(bt_stats_partial_kernel, dim3(g.red), dim3(BT_THREADS), 0, s, (const float*)z, M, g.per, part);
        hipLaunchKernelGGL(bt_stats_finish_kernel, dim3(W / BT_THREADS), dim3(BT_THREADS), 0, s, (const double*)part, g.red, gam, bet, rmean, rvar, momentum,
                           eps, tab + row * 4 * W, stats ? stats + row * 2 * W : (float*)nullptr);
        hipLaunchKernelGGL(bt_apply_kernel, dim3(nblk(M * (W / 8))), dim3(BT_THREADS), 0, s, (const float*)z, M, (const float*)(tab + row * 4 * W), res, relu,
                           g.h, g.w, out);
        return -(int)hipGetLastError();
    };
    int rc;
    if ((rc = pair((const half_t*)x, cin, hin, win, 3, stride, w1, z1, 0, P->bn1_w, P->bn1_b, P->bn1_mean, P->bn1_var, nullptr, 1, a1))) return rc;
    if (g.ds && (rc = pair((const half_t*)x, cin, hin, win, 1, 2, wd, zd, 2, P->ds_bn_w, P->ds_bn_b, P->ds_bn_mean, P->ds_bn_var, nullptr, 0, id))) return rc;
    return pair(a1, W, g.h, g.w, 3, 1, w2, z2, 1, P->bn2_w, P->bn2_b, P->bn2_mean, P->bn2_var, g.ds ? id : (const half_t*)x, 1, (half_t*)y);
}

int vtd_launch_resblock_bn_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_basicblock_params* P, int training,
                                    float eps, const void* ws, const void* y, const float* dy, const float* dscale, const vtd_basicblock_params* Gp,
                                    void* scratch, float* dx, float* dxscale, hipStream_t s) {
    Geo g;
    if (!x || !ws || !y || !dy || !dscale || !scratch || !make_geo(n, hin, win, cin, width, stride, g) || !params_ok(P, g.ds) || !grads_ok(Gp, g.ds) ||
        !(eps > 0.f) || (dx && !dxscale) || (training != 0 && training != 1) || (training && g.m < 2))
        return BT_ERR - 1;
    if (dx && g.stride != 1) return BT_ERR - 3;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)ws & 255) || ((uintptr_t)scratch & 255) || ((uintptr_t)dy & 15) || ((uintptr_t)dscale & 7) ||
        ((uintptr_t)dx & 15) || ((uintptr_t)dxscale & 7))
        return BT_ERR - 2;
    if (!training) return vtd_launch_basicblock_backward(x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s);
    const FwdLayout L = fwd_layout(g);
    const BwdLayout B = bwd_layout(g);
    const int W = BT_W;
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

    // one pair's BatchNorm backward: the two channel sums, dgamma / dbeta, the scale, dz as the fp16 operands
    auto bn_back = [&](const float* gr, const float* z, int row, const float* in_sc, float* out_sc, float* dgam, float* dbet, bool want_padded) {
        const float* t = tab + row * 4 * W;
        hipLaunchKernelGGL(bt_bwd_reduce_kernel, dim3(g.red), dim3(BT_THREADS), 0, s, gr, z, t, M, g.per, part, pmax);
        hipLaunchKernelGGL(bt_bwd_finish_kernel, dim3(1), dim3(BT_W), 0, s, (const double*)part, (const float*)pmax, g.red, inv_m, t, in_sc, coef, dgam, dbet,
                           out_sc);
        if (want_padded) hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring), dim3(RB_THREADS), 0, s, dzp, n, g.h, g.w, W);
        hipLaunchKernelGGL(bt_form_kernel, dim3(nblk(M * (W / 8))), dim3(BT_THREADS), 0, s, gr, z, t, (const float*)coef, (const float*)out_sc, M, g.h, g.w,
                           dzh, want_padded ? dzp : (half_t*)nullptr);
    };
    auto wgrad = [&](const half_t* xin, int xc, int hi, int wi, int ksz, int st, const float* scl, float* dw) {
        WgArgs wa;
        wa.a = dzh; wa.lda = W; wa.x = xin; wa.xc = xc; wa.n = n; wa.H = g.h; wa.W = g.w; wa.rows = M; wa.slab = slab;
        wa.slab_len = slab_rows(M, S); wa.ksz = ksz; wa.stride = st; wa.Hin = hi; wa.Win = wi;
        hipLaunchKernelGGL(dbhead_train_wgrad_kernel<3>, dim3(ksz * ksz * xc / 128 * S, W / 128), dim3(WG_THREADS), 0, s, wa);
        hipLaunchKernelGGL(bt_dw_kernel, dim3(W), dim3(BT_THREADS), 0, s, (const float*)slab, S, xc, ksz * ksz, scl, dw);
    };
    // conv^T of the padded dz plane into [M][W] fp32: the raw weights of a 3x3 conv with W input channels, rotated and transposed
    auto dgrad = [&](const float* wsrc, float* out) {
        hipLaunchKernelGGL(bt_pack_dgrad_kernel, dim3(nblk((int64_t)W * 9 * W + W)), dim3(BT_THREADS), 0, s, wsrc, W, 9, wt, zero);
        ConvParams c = conv_of(n, g.h, g.w, W, dzp, W, g.h, g.w, 3, 1, wt, zero);
        c.out = out; c.ldc = W; c.flags = EPI_OUT_F32;
        return vtd_launch_conv(c, -1, s);
    };

    int rc;
    hipLaunchKernelGGL(rb_mask_kernel, dim3(nblk(M * (W / 4))), dim3(RB_THREADS), 0, s, dy, (const half_t*)y, M, g.h, g.w, W, g2);
    bn_back(g2, z2, 1, dscale, sc2, Gp->bn2_w, Gp->bn2_b, true);
    wgrad(a1, W, g.h, g.w, 3, 1, sc2, Gp->conv2_w);
    VTD_HIP_CHECK(hipGetLastError());
    // da1 = conv2^T(dz2) into the g1 buffer, masked in place by a1 > 0
    if ((rc = dgrad((const float*)P->conv2_w, g1))) return rc;
    if (g.ds) {   // the downsample pair: its upstream gradient is g2
        bn_back(g2, zd, 2, dscale, scd, Gp->ds_bn_w, Gp->ds_bn_b, false);
        wgrad((const half_t*)x, cin, hin, win, 1, 2, scd, Gp->ds_w);
    }
    hipLaunchKernelGGL(rb_mask_kernel, dim3(nblk(M * (W / 4))), dim3(RB_THREADS), 0, s, (const float*)g1, a1, M, g.h, g.w, W, g1);
    bn_back(g1, z1, 0, sc2, sc1, Gp->bn1_w, Gp->bn1_b, dx != nullptr);
    wgrad((const half_t*)x, cin, hin, win, 3, stride, sc1, Gp->conv1_w);
    VTD_HIP_CHECK(hipGetLastError());
    if (dx) {
        if ((rc = dgrad((const float*)P->conv1_w, dx))) return rc;
        hipLaunchKernelGGL(rb_add_identity_kernel, dim3(nblk(M * (W / 4))), dim3(RB_THREADS), 0, s, dx, (const float*)g2, M * (W / 4), (const float*)sc2,
                           (const float*)sc1);
        hipLaunchKernelGGL(rb_copy_scale_kernel, dim3(1), dim3(64), 0, s, (const float*)sc1, dxscale);
    }
    return -(int)hipGetLastError();
}
