// What the two batch-statistics BatchNorm training files share (resblock_bn_train.hip: ResNet-18's BasicBlocks; bottleneck_bn_train.hip:
// ResNet-50's Bottlenecks): the kernels of one convolution + BatchNorm pair in train() mode, moved here unchanged from
// resblock_bn_train.hip, whose head states their contract and their fixed summation orders.  Every kernel is a template of the pair's
// channel count W or takes it from its launch; the per-channel reduces (stats partial, backward reduce, backward finish) put W / 4 lanes
// across the width and stop at W = 512 -- bottleneck_bn_train.hip has its own for the 1024- and 2048-wide pairs.
#ifndef VTD_RESBLOCK_BN_COMMON_H
#define VTD_RESBLOCK_BN_COMMON_H
#include "resblock_common.h"

namespace {   // per translation unit, as every kernel of this library

constexpr int BT_THREADS = RB_THREADS;
constexpr int BT_MAX_RED = 256;

typedef double doublex4 __attribute__((ext_vector_type(4)));

// NaN-keeping maximum, as resblock_train.hip's reduce kernels take it
__device__ __forceinline__ float nmax(float m, float a) { return a > m || a != a ? a : m; }

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
// wp [W][taps cin], k = tap * cin + ci: half(w[co][ci][tap]); zero[W] = 0 (the convolutions' bias row)
template <int W>
__global__ __launch_bounds__(BT_THREADS) void bt_pack_kernel(const float* w, int cin, int taps, half_t* wp, float* zero) {
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    const int K = taps * cin;
    if (i < (int64_t)W * K) {
        const int co = (int)(i / K), k = (int)(i - (int64_t)co * K), tap = k / cin, ci = k - tap * cin;
        wp[i] = (half_t)w[((int64_t)co * cin + ci) * taps + tap];
    } else if (zero && i < (int64_t)W * K + W) {
        zero[i - (int64_t)W * K] = 0.f;
    }
}

// the rows [lo, hi) of part `grp` of the P = 1024 / W parts of workgroup `blk`'s r rows: ceil(grp r / P) .. ceil((grp + 1) r / P) - 1.  W = 512:
// the lower half (the first ceil(r / 2) rows) and the upper; W = 256: four quarters; W = 128: eight eighths; W = 64: sixteen parts
template <int W>
__device__ __forceinline__ void bt_rows(int64_t rows, int64_t per, int grp, int64_t& m0, int64_t& m1, int64_t& lo, int64_t& hi) {
    constexpr int P = 4 * BT_THREADS / W;
    m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows;
    m1 = m0 + per < rows ? m0 + per : rows;
    const int64_t r = m1 - m0;
    lo = m0 + (grp * r + P - 1) / P;
    hi = m0 + ((grp + 1) * r + P - 1) / P;
}

// the parts of one workgroup, part 0 in registers and the others in LDS [part - 1][value][lane]: lower + upper for two parts,
// (q0 + q1) + (q2 + q3) for four, ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7)) for eight; for sixteen the eight-part order on
// q0 .. q7 and on q8 .. q15, then lower + upper
template <int P, int L>
__device__ __forceinline__ double bt_join(double own, double (*sh)[8][L], int v, int j) {
    static_assert(P == 2 || P == 4 || P == 8 || P == 16, "a fixed order is written out for two, four, eight and sixteen parts");
    if constexpr (P == 2) return own + sh[0][v][j];
    else if constexpr (P == 4) return (own + sh[0][v][j]) + (sh[1][v][j] + sh[2][v][j]);
    else if constexpr (P == 8)
        return ((own + sh[0][v][j]) + (sh[1][v][j] + sh[2][v][j])) + ((sh[3][v][j] + sh[4][v][j]) + (sh[5][v][j] + sh[6][v][j]));
    else {
        const double lower = ((own + sh[0][v][j]) + (sh[1][v][j] + sh[2][v][j])) + ((sh[3][v][j] + sh[4][v][j]) + (sh[5][v][j] + sh[6][v][j]));
        const double upper = ((sh[7][v][j] + sh[8][v][j]) + (sh[9][v][j] + sh[10][v][j])) + ((sh[11][v][j] + sh[12][v][j]) + (sh[13][v][j] + sh[14][v][j]));
        return lower + upper;
    }
}

// z [rows][W] fp32 -> part[g][c] = {count, mean, M2} (fp64).  LDS [part][value][lane]: consecutive lanes, consecutive doubles
template <int W>
__global__ __launch_bounds__(BT_THREADS) void bt_stats_partial_kernel(const float* z, int64_t rows, int64_t per, double* part) {
    constexpr int L = W / 4, P = BT_THREADS / L;
    const int t = threadIdx.x, j = t % L, grp = t / L;
    int64_t m0, m1, lo, hi;
    bt_rows<W>(rows, per, grp, m0, m1, lo, hi);
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int64_t m = lo; m < hi; ++m) {
        const floatx4 v = *(const floatx4*)(z + m * W + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const double a = (double)v[e]; s[e] += a; q[e] += a * a; }
    }
    __shared__ double sh[P - 1][8][L];
    if (grp) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { sh[grp - 1][e][j] = s[e]; sh[grp - 1][4 + e][j] = q[e]; }
    }
    __syncthreads();
    if (!grp) {
        const double cnt = (double)(m1 - m0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double S = bt_join<P, L>(s[e], sh, e, j), Q = bt_join<P, L>(q[e], sh, 4 + e, j);
            const double mean = cnt > 0 ? S / cnt : 0.0;
            double* o = part + ((int64_t)blockIdx.x * W + 4 * j + e) * 3;
            o[0] = cnt; o[1] = mean; o[2] = cnt > 0 ? fmax(Q - S * mean, 0.0) : 0.0;
        }
    }
}

// One thread per channel: Chan's combination of the partials in workgroup order (fp64), torch's running-statistics update, the table
// {mu, rstd, gamma, beta} and (optionally) stats_out = {mu, sigma^2} [2][W]
template <int W>
__global__ __launch_bounds__(BT_THREADS) void bt_stats_finish_kernel(const double* part, int G, const float* gam, const float* bet, float* rmean, float* rvar,
                                                                     float momentum, float eps, float* tab, float* stats_out) {
    const int c = blockIdx.x * BT_THREADS + threadIdx.x;
    if (c >= W) return;      // W = 128: half of the one workgroup, W = 64: a quarter
    double n = 0.0, mu = 0.0, m2 = 0.0;
    for (int g = 0; g < G; ++g) {
        const double* q = part + ((int64_t)g * W + c) * 3;
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
    tab[W + c] = (float)(1.0 / sqrt(var + (double)eps));
    tab[2 * W + c] = gam[c];
    tab[3 * W + c] = bet[c];
    if (stats_out) {
        stats_out[c] = (float)mu;
        stats_out[W + c] = (float)var;
    }
}

// out (padded tap) = [relu](((z - mu) rstd) gamma + beta [+ res]); res is a padded tap of the output's extents.  One thread = 8 channels
template <int W>
__global__ __launch_bounds__(BT_THREADS) void bt_apply_kernel(const float* z, int64_t rows, const float* tab, const half_t* res, int relu, int H, int Wd,
                                                              half_t* out) {
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (i >= rows * (W / 8)) return;
    const int c0 = (int)(i % (W / 8)) * 8;
    const int64_t m = i / (W / 8);
    const int HW = H * Wd, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    const int64_t off = (((int64_t)img * (H + 2) + y + 1) * (Wd + 2) + x + 1) * W + c0;
    half8 rv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (res) rv = *(const half8*)(res + off);
    half8 h;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const floatx4 v = *(const floatx4*)(z + i * 8 + 4 * k);
        const floatx4 mu = *(const floatx4*)(tab + c0 + 4 * k), rs = *(const floatx4*)(tab + W + c0 + 4 * k);
        const floatx4 gm = *(const floatx4*)(tab + 2 * W + c0 + 4 * k), bt = *(const floatx4*)(tab + 3 * W + c0 + 4 * k);
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
// xh = (z - mu) rstd as the forward formed it.  Rows, threads and the order of the parts as bt_stats_partial_kernel
template <int W>
__global__ __launch_bounds__(BT_THREADS) void bt_bwd_reduce_kernel(const float* g, const float* z, const float* tab, int64_t rows, int64_t per, double* part,
                                                                   float* pmax) {
    constexpr int L = W / 4, P = BT_THREADS / L;
    const int t = threadIdx.x, j = t % L, grp = t / L;
    int64_t m0, m1, lo, hi;
    bt_rows<W>(rows, per, grp, m0, m1, lo, hi);
    const floatx4 mu = *(const floatx4*)(tab + 4 * j), rs = *(const floatx4*)(tab + W + 4 * j);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    floatx4 mg = {0.f, 0.f, 0.f, 0.f}, mx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int64_t m = lo; m < hi; ++m) {
        const floatx4 gv = *(const floatx4*)(g + m * W + 4 * j), zv = *(const floatx4*)(z + m * W + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (zv[e] - mu[e]) * rs[e];
            s1[e] += (double)gv[e];
            s2[e] += (double)gv[e] * (double)xh;
            mg[e] = nmax(mg[e], fabsf(gv[e]));
            mx[e] = nmax(mx[e], fabsf(xh));
        }
    }
    __shared__ double sh[P - 1][8][L];
    __shared__ float shm[P - 1][8][L];
    if (grp) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sh[grp - 1][e][j] = s1[e]; sh[grp - 1][4 + e][j] = s2[e];
            shm[grp - 1][e][j] = mg[e]; shm[grp - 1][4 + e][j] = mx[e];
        }
    }
    __syncthreads();
    if (!grp) {
        doublex4 o1, o2;
        floatx4 p1, p2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o1[e] = bt_join<P, L>(s1[e], sh, e, j); o2[e] = bt_join<P, L>(s2[e], sh, 4 + e, j);
            p1[e] = mg[e]; p2[e] = mx[e];
#pragma unroll
            for (int k = 0; k < P - 1; ++k) { p1[e] = nmax(p1[e], shm[k][e][j]); p2[e] = nmax(p2[e], shm[k][4 + e][j]); }
        }
        const int64_t b = (int64_t)blockIdx.x * 2 * W + 4 * j;
        *(doublex4*)(part + b) = o1; *(doublex4*)(part + b + W) = o2;
        *(floatx4*)(pmax + b) = p1; *(floatx4*)(pmax + b + W) = p2;
    }
}

// One workgroup of W threads, thread c = channel c.  The partials in workgroup order (fp64).  dbeta = s1, dgamma = s2 with the incoming scale
// undone; coef = {gamma rstd, s1 / M, s2 / M} [3][W] at the incoming scale; out_sc = {total scale, 1 / total, this stage's multiplier, 0}:
// the multiplier is a power of two from the bound max_c |gamma rstd| (max |g| + |s1| / M + max |xh| |s2| / M) >= max |dz| (1 when that is
// zero or not finite)
template <int W>
__global__ __launch_bounds__(W) void bt_bwd_finish_kernel(const double* part, const float* pmax, int G, double inv_m, const float* tab, const float* in_sc,
                                                          float* coef, float* dgam, float* dbet, float* out_sc) {
    const int c = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    float mg = 0.f, mx = 0.f;
    for (int g = 0; g < G; ++g) {
        const int64_t b = (int64_t)g * 2 * W + c;
        s1 += part[b]; s2 += part[b + W];
        mg = nmax(mg, pmax[b]); mx = nmax(mx, pmax[b + W]);
    }
    const float A = tab[2 * W + c] * tab[W + c], B = (float)(s1 * inv_m), C = (float)(s2 * inv_m);
    coef[c] = A; coef[W + c] = B; coef[2 * W + c] = C;
    dbet[c] = (float)(s1 * (double)in_sc[1]);
    dgam[c] = (float)(s2 * (double)in_sc[1]);
    __shared__ float sh[W];
    sh[c] = (float)(fabs((double)A) * ((double)mg + fabs((double)B) + (double)mx * fabs((double)C)));
    __syncthreads();
    for (int o = W / 2; o > 0; o >>= 1) {
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

// dz = gamma rstd (g - s1 / M - xh s2 / M) in fp32, times the multiplier, as fp16: flat [rows][W] and (when given) a ring-padded plane
// [n][dil H + 2][dil Wd + 2][W] at pixel (dil y, dil x): dil = 1 fills the interior, dil = 2 the even positions of the stride-2 dgrad's
// zero-inserted plane.  One thread = 8 channels.
template <int W>
__global__ __launch_bounds__(BT_THREADS) void bt_form_kernel(const float* g, const float* z, const float* tab, const float* coef, const float* sc,
                                                             int64_t rows, int H, int Wd, int dil, half_t* flat, half_t* padded) {
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (i >= rows * (W / 8)) return;
    const int c0 = (int)(i % (W / 8)) * 8;
    const float mul = sc[2];
    half8 h;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const floatx4 gv = *(const floatx4*)(g + i * 8 + 4 * k), zv = *(const floatx4*)(z + i * 8 + 4 * k);
        const floatx4 mu = *(const floatx4*)(tab + c0 + 4 * k), rs = *(const floatx4*)(tab + W + c0 + 4 * k);
        const floatx4 A = *(const floatx4*)(coef + c0 + 4 * k), B = *(const floatx4*)(coef + W + c0 + 4 * k),
                      C = *(const floatx4*)(coef + 2 * W + c0 + 4 * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (zv[e] - mu[e]) * rs[e];
            h[4 * k + e] = (half_t)(A[e] * (gv[e] - B[e] - xh * C[e]) * mul);
        }
    }
    *(half8*)(flat + i * 8) = h;
    if (padded) {
        const int64_t m = i / (W / 8);
        const int HW = H * Wd, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
        *(half8*)(padded + (((int64_t)img * (dil * H + 2) + dil * y + 1) * (dil * Wd + 2) + dil * x + 1) * W + c0) = h;
    }
}

// wt [cin][taps * W]: row ci, k = tap' * W + co holds half(w[co][ci][taps - 1 - tap']) (the window rotated by 180 degrees, the raw weights
// transposed, rounded as the forward packs them); a zero bias row of W entries
template <int W>
__global__ __launch_bounds__(BT_THREADS) void bt_pack_dgrad_kernel(const float* w, int cin, int taps, half_t* wt, float* zero) {
    const int i = blockIdx.x * BT_THREADS + threadIdx.x;
    const int K = taps * W;
    if (i < cin * K) {
        const int ci = i / K, k = i - ci * K, tap = k / W, co = k - tap * W;
        wt[i] = (half_t)w[((int64_t)co * cin + ci) * taps + (taps - 1 - tap)];
    } else if (i < cin * K + W) {
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

// the stride-2 block: dx [n][2H][2Wd][cin] (at dz1's total scale, dscale sc2[2] sc1[2]) += t = ds^T(dz_d) [n][H][Wd][cin] (at dz_d's total
// scale, dscale scd[2]) times sc2[2] sc1[2] / scd[2], powers of two all three, at the even (row, column) positions: the 1x1 stride-2
// convolution reads no other.  One thread = 4 channels.
__global__ __launch_bounds__(BT_THREADS) void bt_add_downsample_kernel(float* dx, const float* t, int64_t rows, int H, int Wd, int cin, const float* sc2,
                                                                       const float* sc1, const float* scd) {
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    const int C4 = cin >> 2;
    if (i >= rows * C4) return;
    const int cq = (int)(i % C4);
    const int64_t m = i / C4;
    const int HW = H * Wd, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    float* d = dx + (((int64_t)img * 2 * H + 2 * y) * 2 * Wd + 2 * x) * cin + 4 * cq;
    const float mul = sc2[2] * sc1[2] / scd[2];
    floatx4 a = *(floatx4*)d;
    const floatx4 b = *(const floatx4*)(t + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += b[e] * mul;
    *(floatx4*)d = a;
}

}  // namespace

#endif  // VTD_RESBLOCK_BN_COMMON_H
